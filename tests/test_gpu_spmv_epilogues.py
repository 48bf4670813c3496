"""The diagonal-scaled SpMV epilogues on every storage form (alfd_spmv_scaled: the solver's own spmv() dispatch).

Every SpMV kernel family is compiled with four epilogues: 0 y = s, 1 y = fma(alpha, s, y), 2 y = d .* s,
3 y = s and y2 = d .* s.  Epilogues 2 and 3 carry the augmented-Lagrangian term t = W^-1 .* (C x) and the nested
grad-div term q = Mp_lumped^-1 .* (B u) of the solver; tests/test_gpu_parity.py reaches 0 and 1 only.  Here every
storage form runs 2 and 3 (and 0 out of a NaN-prefilled y), each case after asserting through alfd_get_matrix_info that
the form under test is the one the slot holds.

Two references per case, neither involving the code under test:
  * bitwise: s = the oracle's canonical sum (mode 0); epilogue 2 must give y == d * s, epilogue 3 y == s and
    y2 == d * s -- one IEEE multiply in NumPy is the exact reference;
  * independent: ref = d .* (A x) in np.longdouble from the CSR arrays, with the derived row-wise bound
    |y2_r - ref_r| <= (len_r + 2) 2^-53 |d_r| (|A||x|)_r (len_r - 1 additions and len_r products / fma of the row sum
    in any order, one multiply by d_r, second-order terms in the slack), should oracle and library ever share an error.

d_r = +-uniform(0.5, 2) 2^k with k in -20..20 per row, every factor distinct (a d indexed by the block-local row, the
list position or the batch row shows), about 1 % exact zeros.  y and y2 go in as NaN: a row neither the kernel nor the
sparse-row memset writes comes back NaN.

Sizes are the smallest that reach each form under default thresholds: long rows need 96 * 256 = 24 576 rows (N = 10
vector Q2: 27 783), short rows min(512, 96 * 2 * 64 / L) * 256: 98 304 for L = 32 and 131 072 for L = 16 / 8 (Q2 2-D
N = 181 and Q1 2-D N = 362: 131 769 rows).  The 27-point stencil passes the row threshold of L = 32 at N = 46, but
its single-entry boundary rows keep the mean row length at or below 24 (16 lanes) up to N = 66: N = 67, 314 432 rows,
is the smallest Q1 3-D operator on 32 lanes."""
import numpy as np
import pytest

from fictitious_domain_al_preconditioners_amd import _abi, problems, solver
from spmv_reference import Case

pytestmark = pytest.mark.gpu
LONG_GEN = dict(dim=3, degree=2, ncomp=3, stokes=False, grad_div=True, gamma_grad_div=10.0, radius=0.1, immersed_refine=0)


def _form(info, **want):
    got = {k: info[k] for k in want}
    assert got == want, info


@pytest.fixture
def ctx(built):
    c = solver.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def long_problem():
    """Vector Q2 with grad-div at the smallest size that takes the long-row window / batch-major forms."""
    for n in (10, 20):
        pb = problems.generate(n_cells=n, **LONG_GEN)
        if pb.mats["A"].nrows >= 96 * 256:
            return pb
    raise AssertionError("no size reaches 256 row blocks")


@pytest.fixture(scope="module")
def long_case(long_problem):
    return Case(long_problem.mats["A"], 31)


def _scaled_values(a, factors, rng):
    v = np.array(a.val) * (1.0 + rng.integers(0, factors, a.nnz) / float(factors))
    return problems.Csr(a.nrows, a.ncols, np.array(a.row_ptr), np.array(a.col), v)


@pytest.mark.parametrize("avg,lanes", [(3, 4), (7, 8), (14, 16), (30, 32), (70, 64), (200, 64)])
def test_plain_csr_scaled_epilogues_bitwise(ctx, avg, lanes):
    """spmv_kernel<L, EPI, false> for L = 4 .. 64 and, for rows beyond 48 entries, the streaming kernel: 3001 rows
    (odd: the last wave holds a partially filled set of row groups), far below every window threshold."""
    import scipy.sparse as sp
    a = sp.random(3001, 2500, density=avg / 2500.0, random_state=int(avg), format="csr")
    a.data[:] = np.random.default_rng(5).uniform(-1, 1, a.nnz)
    case = Case(problems.Csr.from_scipy(a), 100 + avg)
    ctx.set_matrix(_abi.A, case.m)
    _form(ctx.matrix_info(_abi.A), lanes=lanes, windowed=0, batch_major=0, value_indexed=0)
    case.check(ctx, f"rand{avg}", mode1=True)


def test_sparse_row_scaled_epilogues_bitwise(ctx):
    """The sparse-row form (spmv_kernel<L, EPI, true> on the list of non-empty rows; less than half of the rows hold an
    entry): rows outside the list come back exactly 0 in y AND in y2 out of NaN-prefilled buffers -- the memsets of
    spmv_m -- and a matrix without any entry (n_list == 0) is all zeros without a launch."""
    import scipy.sparse as sp
    a = sp.random(5000, 400, density=0.05, random_state=1, format="lil")
    a[10:4900, :] = 0
    case = Case(problems.Csr.from_scipy(a.tocsr()), 7)
    empty = np.diff(case.m.row_ptr) == 0
    assert empty[10:4900].all() and 2 * int((~empty).sum()) < case.m.nrows
    assert not np.any(case.s[empty]) and not np.any(case.ds[empty])       # what the references ask of those rows
    ctx.set_matrix(_abi.A, case.m)
    _form(ctx.matrix_info(_abi.A), lanes=16, windowed=0, batch_major=0)
    case.check(ctx, "sparse_rows", mode1=True)
    nan = np.full(case.m.nrows, np.nan)
    y, y2 = ctx.spmv_scaled(_abi.A, case.x, case.d, nan, nan)
    assert not np.any(y[empty]) and not np.any(y2[empty])
    assert not np.any(ctx.spmv_scaled(_abi.A, case.x, case.d, nan)[empty])
    none = Case(problems.Csr(700, 300, np.zeros(701, np.int64), np.zeros(0, np.int32), np.zeros(0)), 8)
    ctx.set_matrix(_abi.A, none.m)
    assert ctx.matrix_info(_abi.A)["nnz"] == 0
    none.check(ctx, "no entries")
    y, y2 = ctx.spmv_scaled(_abi.A, none.x, none.d, np.full(700, np.nan), np.full(700, np.nan))
    assert not np.any(y) and not np.any(y2)


def test_argument_validation_on_a_live_context(ctx):
    """ALFD_E_INVALID for a null x, d or y, an unset slot, a slot out of range and y2 == y; nothing is written."""
    m = problems.Csr(3, 3, np.array([0, 1, 2, 3], np.int64), np.array([0, 1, 2], np.int32), np.ones(3))
    ctx.set_matrix(_abi.A, m)
    v, y = np.ones(3), np.full(3, np.nan)
    p, q = v.ctypes.data, y.ctypes.data
    lib, h = ctx._lib, ctx._h
    for args in ((None, p, q, None), (p, None, q, None), (p, p, None, None), (p, p, q, q)):
        assert lib.alfd_spmv_scaled(h, _abi.A, *args) == _abi.E_INVALID, args
    for slot in (_abi.B, -1, 99):
        assert lib.alfd_spmv_scaled(h, slot, p, p, q, None) == _abi.E_INVALID, slot
    assert np.isnan(y).all()
    with pytest.raises(ValueError):
        ctx.spmv_scaled(_abi.A, v, np.ones(2), y)
    y2 = np.full(3, np.nan)
    assert lib.alfd_spmv_scaled(h, _abi.A, p, p, q, y2.ctypes.data) == _abi.OK
    assert np.array_equal(y, v) and np.array_equal(y2, v)


@pytest.mark.parametrize("blocks", ["runs", "bricks", "noshare", "waves2", "waves8_xcd"])
def test_batch_major_long_rows_scaled_epilogues_bitwise(ctx, long_problem, long_case, blocks):
    """spmv_vs_kernel: row blocks as runs of the numbering and as mesh bricks, plain 4-row batches only
    (batch_major_share = 0), 2 and 8 waves per block, the XCD-contiguous block order."""
    m = long_case.m
    if blocks == "noshare":
        ctx.set_tunable("batch_major_share", 0)
    if blocks != "runs":
        ctx.set_row_blocks(_abi.A, *problems.brick_row_blocks(long_problem.params, (8, 2, 2)))
    ctx.set_matrix(_abi.A, m)
    info = ctx.matrix_info(_abi.A)
    _form(info, lanes=64, windowed=1, value_indexed=1, batch_major=1 if blocks == "runs" else 2, batch_major_wide=0)
    assert info["batch_major_blocks"] >= 256
    assert (info["shared_nnz"] == 0) == (blocks == "noshare"), info
    if blocks == "waves2":
        ctx.set_tunable("batch_major_waves", 2)
    if blocks == "waves8_xcd":
        ctx.set_tunable("batch_major_waves", 8)
        ctx.set_tunable("batch_major_xcd", 1)
    long_case.check(ctx, blocks)
    if blocks == "runs":                      # the XCD order on runs of the numbering too (4 waves)
        ctx.set_tunable("batch_major_xcd", 1)
        long_case.check(ctx, "runs, xcd order")


def test_batch_major_wide_codes_scaled_epilogues_bitwise(ctx, long_problem):
    """spmv_vs_kernel<EPI, 0, 4, 1>: 10-bit dictionary codes / 11-bit window columns, for blocks with more than 512
    distinct values (every value multiplied by one of 16 factors)."""
    case = Case(_scaled_values(long_problem.mats["A"], 16, np.random.default_rng(7)), 32)
    ctx.set_matrix(_abi.A, case.m)
    _form(ctx.matrix_info(_abi.A), lanes=64, windowed=1, batch_major=1, batch_major_wide=1)
    case.check(ctx, "wide codes")


def test_batch_major_edge_rows_scaled_epilogues_bitwise(ctx, long_problem):
    """spmv_vs_kernel on structurally empty rows (class 0 batches: every epilogue still has to write them), single-entry
    rows and perturbed rows that are no translate of anything, on mesh bricks."""
    a = long_problem.mats["A"].to_scipy().tolil()
    rng = np.random.default_rng(5)
    for r in range(0, a.shape[0], 97):
        a.rows[r], a.data[r] = [], []
    for r in range(50, a.shape[0], 1013):
        a.rows[r], a.data[r] = a.rows[r][:1], a.data[r][:1]
    a = a.tocsr()
    for r in range(31, a.shape[0], 211):
        a.data[a.indptr[r]:a.indptr[r + 1]] *= 1.0 + 0.25 * rng.integers(1, 4)
    case = Case(problems.Csr.from_scipy(a), 33)
    ctx.set_row_blocks(_abi.A, *problems.brick_row_blocks(long_problem.params, (8, 4, 2)))
    ctx.set_matrix(_abi.A, case.m)
    _form(ctx.matrix_info(_abi.A), lanes=64, windowed=1, batch_major=2)
    case.check(ctx, "edge rows")
    empty = np.diff(case.m.row_ptr) == 0
    y, y2 = ctx.spmv_scaled(_abi.A, case.x, case.d, np.full(empty.size, np.nan), np.full(empty.size, np.nan))
    assert empty.sum() > 200 and not np.any(y[empty]) and not np.any(y2[empty])


@pytest.mark.parametrize("form", ["dict8", "wide16", "rawblocks", "nodict", "value_index_off"])
def test_window_forms_scaled_epilogues_bitwise(ctx, long_problem, long_case, form):
    """The round-1 window kernels on long rows (batch_major = 0): the 8-bit dictionary (spmv_window_vib_kernel), 16-bit
    codes and raw blocks, no dictionary at all (spmv_window_kernel), and a dictionary-coded matrix run through the
    general kernel (value_index = 0)."""
    a = long_problem.mats["A"]
    rng = np.random.default_rng(11)
    case = long_case
    if form == "wide16":                                    # every value scaled by one of 9 factors
        v = np.array(a.val) * (1.0 + 0.125 * rng.integers(0, 9, a.nnz))
    elif form in ("rawblocks", "nodict"):                   # random values in the first 30 % of the rows / everywhere
        v = np.array(a.val, copy=True)
        pick = rng.random(v.size) < (0.4 if form == "rawblocks" else 1.0)
        if form == "rawblocks":
            pick[int(a.row_ptr[int(0.3 * a.nrows)]):] = False
        v[pick] = rng.uniform(-1, 1, int(pick.sum()))
    if form in ("wide16", "rawblocks", "nodict"):
        case = Case(problems.Csr(a.nrows, a.ncols, np.array(a.row_ptr), np.array(a.col), v), 34)
    m = case.m
    ctx.set_tunable("batch_major", 0)
    ctx.set_matrix(_abi.A, m)
    info = ctx.matrix_info(_abi.A)
    _form(info, lanes=64, windowed=1, batch_major=0)
    assert info["window_blocks"] >= 256
    if form in ("dict8", "value_index_off"):
        assert info["value_indexed"] and info["value_wide_nnz"] == 0 and info["value_indexed_nnz"] == m.nnz, info
    elif form == "wide16":
        assert info["value_indexed"] and info["value_wide_nnz"] > m.nnz // 2, info
    elif form == "rawblocks":
        assert info["value_indexed"] and 0 < info["value_indexed_blocks"] < info["window_blocks"], info
    else:
        assert not info["value_indexed"], info
    if form == "value_index_off":
        ctx.set_tunable("value_index", 0)
    case.check(ctx, form)


SHORT = {"q1_3d_L32": (dict(dim=3, degree=1, ncomp=1, n_cells=67), 32),
         "q2_2d_L16": (dict(dim=2, degree=2, ncomp=1, n_cells=181), 16),
         "q1_2d_L8": (dict(dim=2, degree=1, ncomp=1, n_cells=362), 8)}


@pytest.mark.parametrize("kind", list(SHORT))
def test_short_rows_scaled_epilogues_bitwise(ctx, kind):
    """spmv_vss_kernel (batch-major short rows: one stored template row per batch of translate rows, L = 32 / 16 / 8)
    and, with batch_major = 0 on the same slot, spmv_window_group_kernel; the same with every 7th row perturbed (rows
    without a translate partner are batches of one)."""
    gen, lanes = SHORT[kind]
    m = problems.generate(radius=0.1, **gen).mats["A"]
    assert m.nrows >= min(512, 96 * 2 * 64 // lanes) * 256
    v = np.array(m.val, copy=True)
    for r in range(3, m.nrows, 7):
        v[m.row_ptr[r]:m.row_ptr[r + 1]] *= 1.0 + 0.125 * (r % 5)
    perturbed = problems.Csr(m.nrows, m.ncols, np.array(m.row_ptr), np.array(m.col), v)
    for tag, case in ((kind, Case(m, 35)), (kind + " perturbed", Case(perturbed, 36))):
        ctx.set_tunable("batch_major", 1)
        ctx.set_matrix(_abi.A, case.m)
        info = ctx.matrix_info(_abi.A)
        _form(info, lanes=lanes, windowed=1, batch_major=1)
        assert info["shared_nnz"] > 0.5 * case.m.nnz, info
        case.check(ctx, tag + ", batch-major")
        ctx.set_tunable("batch_major", 0)           # the L-lane window kernel on the same slot
        _form(ctx.matrix_info(_abi.A), lanes=lanes, windowed=1, batch_major=0)
        case.check(ctx, tag + ", window groups")


def test_ragged_short_rows_scaled_epilogues_bitwise(ctx):
    """spmv_window_group_kernel on a ragged banded matrix (0 .. 20 entries per row, empty rows) with a few far-away
    columns, just above the 131 072-row threshold of L = 8.  Far-away columns alone become window segments of their
    own; every 32nd block of 512 rows therefore has its columns scattered over the whole matrix, so that its window
    does not fit and the block falls back to global x.  (No two rows are translates: the batch-major short-row form
    refuses this matrix.)"""
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    n = 132000
    cnt = rng.integers(0, 21, n)
    rows = np.repeat(np.arange(n), cnt)
    cols = np.clip(rows + rng.integers(-400, 401, rows.size), 0, n - 1)
    far = rng.integers(0, rows.size, 200)
    cols[far] = rng.integers(0, n, 200)
    scattered = (rows // 512) % 32 == 5
    cols[scattered] = rng.integers(0, n, int(scattered.sum()))
    a = sp.csr_matrix((rng.uniform(-1, 1, rows.size), (rows, cols)), shape=(n, n))
    a.sum_duplicates()
    case = Case(problems.Csr.from_scipy(a), 37)
    empty = np.diff(case.m.row_ptr) == 0
    assert empty.sum() > 1000
    ctx.set_tunable("batch_major", 0)
    ctx.set_matrix(_abi.A, case.m)
    info = ctx.matrix_info(_abi.A)
    _form(info, lanes=8, windowed=1, batch_major=0)
    assert 0 < info["window_fallback_blocks"] < info["window_blocks"], info
    case.check(ctx, "ragged, window groups")
    y, y2 = ctx.spmv_scaled(_abi.A, case.x, case.d, np.full(n, np.nan), np.full(n, np.nan))
    assert not np.any(y[empty]) and not np.any(y2[empty])


def test_divergence_block_scaled_by_the_lumped_pressure_mass_bitwise(ctx):
    """A production operand: q = Mp_lumped^-1 .* (B u) of the nested grad-div term, B of the Taylor-Hood pair at
    N = 36 (50 653 pressure rows; batch-major with blocks split for their x windows), d = 1 / rowsum(Mp)."""
    pb = problems.stokes3d_sphere(n_cells=36, immersed_refine=2)
    mp = pb.mats["Mp"]
    d = 1.0 / np.add.reduceat(np.asarray(mp.val), np.asarray(mp.row_ptr[:-1], np.int64))
    assert np.diff(mp.row_ptr).min() > 0 and np.all(d > 0)
    case = Case(pb.mats["B"], 38, d=d)
    ctx.set_matrix(_abi.B, case.m)
    info = ctx.matrix_info(_abi.B)
    _form(info, batch_major=1, windowed=1)
    assert info["streamed_bytes"] < 2.5 * case.m.nnz, info
    case.check(ctx, "B", slot=_abi.B)
    generic = Case(case.m, 39)                   # and with the distinct, signed, partly zero scale of the other cases
    generic.check(ctx, "B, generic d", slot=_abi.B)
