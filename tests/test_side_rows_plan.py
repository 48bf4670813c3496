"""Side rows of the long-row batch-major form (tunable "batch_major_side_rows") on the CPU: the host-side planner
alfd_host_stream_plan_side takes the rows beyond 384 entries out of the row blocks, lists them longest first, and plans
everything else as alfd_host_stream_plan does; the blocks decode back, the side list's compact CSR reproduces its rows,
and every row is in exactly one of the two (all counted into decode_mismatches).  The variant is not used without a long
row (then every field is alfd_host_stream_plan's) and refused when the long rows hold more than 1/8 of the entries.

No GPU here, and a context cannot be created without one: that the tunable defaults to 0 and refuses 2 is asserted in
tests/test_gpu_side_rows.py; here the header's word on both, the symbols and a null context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import launch_shape_cases as lc
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 384                                            # kVsMaxLen: the longest row a row block takes


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def _long(m):
    """Rows beyond the limit, longest first, ties by row number."""
    ln = np.diff(np.asarray(m.row_ptr))
    rows = np.flatnonzero(ln > LIMIT)
    return rows[np.lexsort((rows, -ln[rows]))], ln


def _grown(m, row, length):
    """A copy of m whose row `row` holds `length` entries: its own, then the nearest unused columns, sorted; the new
    entries take values the row already has (no new dictionary entries)."""
    rp, col, val = np.asarray(m.row_ptr), np.asarray(m.col), np.asarray(m.val)
    c, v = col[rp[row]:rp[row + 1]], val[rp[row]:rp[row + 1]]
    assert 0 < c.size <= length
    spare = np.setdiff1d(np.arange(m.ncols), c)
    spare = spare[np.argsort(np.abs(spare - row), kind="stable")][:length - c.size]
    nc = np.concatenate([c, spare])
    nv = np.concatenate([v, np.resize(v, spare.size)])
    order = np.argsort(nc, kind="stable")
    ln = np.diff(rp).copy()
    ln[row] = length
    nrp = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    return problems.Csr(m.nrows, m.ncols, nrp,
                        np.concatenate([col[:rp[row]], nc[order], col[rp[row + 1]:]]).astype(np.int32),
                        np.concatenate([val[:rp[row]], nv[order], val[rp[row + 1]:]]))


def test_planted_long_rows_go_to_the_side_list():
    m = lc.long_rows(3365, "few")
    want, ln = _long(m)
    assert [int(ln[r]) for r in want] == [1025, 1024, 1023, 513, 512, 511]
    assert not solver.host_stream_plan(m)["ok"]                       # what the form does with them today
    info = solver.host_stream_plan(m, side_rows=True)
    assert info["ok"] == 1
    assert info["side_rows"].tolist() == want.tolist()
    assert info["side_nnz"] == 4608
    assert info["rows_covered"] == 3359
    assert info["decode_mismatches"] == 0


def test_without_a_long_row_the_plan_is_the_plain_one():
    m = lc.long_rows(3365, "few", 384)
    plain = solver.host_stream_plan(m)
    info = solver.host_stream_plan(m, side_rows=True)
    assert plain["ok"] == 1 and info["side_rows"].size == 0 and info["side_nnz"] == 0
    for k, v in plain.items():
        assert info[k] == v, k
    assert info["rows_covered"] == m.nrows and info["decode_mismatches"] == 0


def test_the_limit_is_384_entries():
    base = lc.long_rows(3365, "few", 384)
    ln = np.diff(np.asarray(base.row_ptr))
    at384 = np.flatnonzero(ln == 384)
    assert at384.size >= 1
    row = int(np.flatnonzero((ln > 100) & (ln < 384))[7])            # any ordinary row
    m = _grown(base, row, 385)
    assert int(np.diff(m.row_ptr)[row]) == 385 and _long(m)[0].tolist() == [row]
    info = solver.host_stream_plan(m, side_rows=True)
    assert info["ok"] == 1 and info["decode_mismatches"] == 0
    assert info["side_rows"].tolist() == [row] and info["side_nnz"] == 385      # 385 entries: the side list
    assert info["rows_covered"] == m.nrows - 1                                  # 384 entries: still a row of the blocks
    at = _grown(base, row, 384)
    info = solver.host_stream_plan(at, side_rows=True)
    assert info["ok"] == 1 and info["side_rows"].size == 0 and info["rows_covered"] == at.nrows
    assert info["decode_mismatches"] == 0


@pytest.fixture(scope="module")
def refined12():
    return problems.stokes3d_sphere(12, 2, assembly="cellwise", local_refine=1)


@pytest.mark.parametrize("blocks", ["runs_of_96", "bricks"])
def test_refined_mesh_plans_with_its_long_rows_aside(refined12, blocks):
    A = refined12.mats["A"]
    want, ln = _long(A)
    assert A.nrows == 61503 and want.size == 654
    bl = None
    if blocks == "bricks":
        bl = solver.brick_blocks_from_points(problems.row_support_points(refined12), (16, 4, 1))
    assert not solver.host_stream_plan(A, row_block=96, blocks=bl)["ok"]
    info = solver.host_stream_plan(A, row_block=96, blocks=bl, side_rows=True)
    print("refined (12, 2)", blocks, {k: v for k, v in info.items() if k != "side_rows"},
          "B/nnz %.2f" % (info["stream_bytes"] / A.nnz), "side share %.4f" % (info["side_nnz"] / A.nnz))
    assert info["ok"] == 1
    assert info["side_rows"].size == 654 and info["side_rows"].tolist() == want.tolist()
    assert info["side_nnz"] == int(ln[want].sum()) and 8 * info["side_nnz"] <= A.nnz
    assert info["rows_covered"] == A.nrows - 654
    assert info["decode_mismatches"] == 0


def test_a_matrix_of_long_rows_is_refused():
    """Every row holds 400 entries: all of them are long, far more than 1/8 of the entries."""
    n = 1200
    rng = np.random.default_rng(5)
    pool = rng.uniform(-1.0, 1.0, 30)
    cols = [np.sort((i - 200 + np.arange(400)) % n) for i in range(n)]
    rp = (400 * np.arange(n + 1)).astype(np.int64)
    col = np.concatenate(cols).astype(np.int32)
    m = problems.Csr(n, n, rp, col, pool[rng.integers(0, 30, col.size)])
    info = solver.host_stream_plan(m, side_rows=True)
    assert info["ok"] == 0 and info["side_rows"].size == 0 and info["side_nnz"] == 0


def test_symbols_mirror_and_null_arguments():
    lib = solver.load_library()
    for name in ("alfd_host_stream_plan_side", "alfd_get_side_rows"):
        assert hasattr(lib, name) and name in solver.ABI_SYMBOLS
    assert hasattr(solver.Context, "side_rows")
    info = _abi.SideRowsInfo()
    assert lib.alfd_get_side_rows(None, _abi.A, C.byref(info)) == _abi.E_INVALID
    assert lib.alfd_set_tunable(None, b"batch_major_side_rows", 1) == _abi.E_INVALID
    m = lc.long_rows(480, "few", 384)
    rp, col, val = (np.ascontiguousarray(a) for a in (m.row_ptr, m.col, m.val))
    plan, n = _abi.StreamPlanInfo(), C.c_int64()
    assert lib.alfd_host_stream_plan_side(m.nrows, rp.ctypes.data, col.ctypes.data, val.ctypes.data, 96, 0, None, None,
                                          None, None, C.byref(n), C.byref(plan)) == _abi.E_INVALID


def test_struct_mirrors_the_header_and_the_tunable_is_documented():
    hdr = open(os.path.join(ROOT, "include", "alfd", "alfd.h")).read()
    body = re.search(r"typedef struct alfd_side_rows_info \{(.*?)\} alfd_side_rows_info;", hdr, re.S).group(1)
    assert re.sub(r"\s", "", body) == "int64_trows,nnz,longest,interior_rows,grid;"
    assert [k for k, _ in _abi.SideRowsInfo._fields_] == ["rows", "nnz", "longest", "interior_rows", "grid"]
    assert C.sizeof(_abi.SideRowsInfo) == 5 * 8
    at = hdr.index('"batch_major_side_rows" (0/1')
    doc = hdr[at:hdr.index('"nested_mp_host_stepped"', at)]
    assert "default 0" in doc and "refused with ALFD_E_INVALID" in doc
    assert "#define ALFD_ABI_VERSION 12" in hdr
