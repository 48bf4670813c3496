"""The element-wise tails of the fused smoother steps at the block end of the batch-major A launch (tunable
"ml_tail_in_spmv") against the separate tail launch.  Everything is compared bit for bit: the
arithmetic of an element is the same expression under the same compiler flags, only the launch it runs in differs.

  * whole solves on ONE context with the tunable 1, 0, 1: solution blocks, residual history, iteration counts; the
    counter of fused launches (alfd_get_fused_tail_launches) says that the path ran, or did not;
  * the kernel through alfd_spmv_tail_step at shapes no solver case reaches: form 0 (A launch with the epilogue, then
    the rows party of the tail) against form 1 (y = A x, then the whole tail), every mode the kernel instantiates, on
    the planted operators of launch_shape_cases.py (480 .. 3 365 rows) with the rows of Ct -- the rows the epilogue
    must leave to the tail launch -- placed where a block begins and ends;
  * the tail launch itself, aug_tail_kernel<L, MODE> at every lane count and mode, against the oracle and the header
    comment of the kernel (form 1 alone: no other test chooses which of the 30 instantiations runs);
  * an output vector at the address of x is refused before anything is launched;
  * the epilogue together with the second party of a pair launch.

What form 0 leaves in y: A x on the rows of Ct and NOTHING on the others (alfd.h), so y is compared on the rows of Ct
and must keep its fill elsewhere."""
import numpy as np
import pytest

import cases
import launch_shape_cases as lc
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver

pytestmark = pytest.mark.gpu

SOLVES = ["stokes3d_gmg", "stokes3d_gmg_patch", "stokes3d_bench_settings", "stokes3d_multilevel",
          "stokes3d_gmg_deg1", "stokes3d_gmg_patch_deg1", "stokes3d_bench_settings_deg1", "stokes3d_multilevel_deg1",
          "stokes3d_gmg_deg2", "stokes3d_gmg_coarse5", "elliptic_modified_gmg_patch"]
MODES = [_abi.TAIL_STEP, _abi.TAIL_LAST, _abi.TAIL_LAST_ADD, _abi.TAIL_RES, _abi.TAIL_RES_INIT]
NT = 53                                    # multipliers that the planted Ct addresses
FILL = 1.0e3                               # outputs are pre-filled with FILL + row


def _case(name):
    if name.endswith("_deg1"):
        pb, cfg = cases.case(name[:-len("_deg1")])
        cfg.ml_smooth_degree = 1
        cfg.ml_smooth_degree_coarse = 0
        if cfg.ml_patch_degree > 0:
            cfg.ml_patch_degree = 1
        return pb, cfg
    if name.endswith("_deg2"):             # the only step of the sweep multiplies z and must deliver z: it falls back
        pb, cfg = cases.case(name[:-len("_deg2")])
        cfg.ml_smooth_degree = 2
        return pb, cfg
    if name.endswith("_coarse5"):
        pb, cfg = cases.case(name[:-len("_coarse5")])
        cfg.ml_smooth_degree_coarse = 5
        return pb, cfg
    return cases.case(name)


def _solve(ctx, rhs, on):
    ctx.set_tunable("ml_tail_in_spmv", on)
    before = ctx.fused_tail_launches()
    x, res = ctx.solve(rhs, raise_on_failure=False)
    return x, res, ctx.history().copy(), ctx.fused_tail_launches() - before


@pytest.mark.parametrize("name", SOLVES)
def test_solves_with_and_without_the_epilogue_bit_for_bit(built, monkeypatch, name):
    # read at alfd_create: operators of one row block and more take the window forms, so that these small cases run A
    # (and their level operators) on the batch-major kernel as the large ones do by themselves
    monkeypatch.setenv("ALFD_SPMV_WINDOW_MIN_BLOCKS", "1")
    pb, cfg = _case(name)
    levels = cases.aggregates_of(pb, cfg)
    osys = cases.oracle_system(pb, cfg)
    rhs = cases.prepared_rhs(osys, pb, cfg)
    ctx = solver.context_from_problem(pb, cfg, aggregates=levels)
    try:
        info = ctx.matrix_info(_abi.A)
        x1, r1, h1, n1 = _solve(ctx, rhs, 1)
        x0, r0, h0, n0 = _solve(ctx, rhs, 0)
        x2, r2, h2, n2 = _solve(ctx, rhs, 1)      # and back: the switch leaves no state behind
    finally:
        ctx.close()
    print(name, "outer", r1.outer_iterations, "inner", r1.inner_iterations, "mp", r1.mp_iterations, "status", r1.status,
          "batch_major", info["batch_major"], "lanes", info["lanes"], "fused launches on / off / on", n1, n0, n2)
    assert r1.outer_iterations > 0 and r1.inner_iterations > 0
    assert n0 == 0
    assert n1 == n2
    if name != "elliptic_modified_gmg_patch":     # that one may fall back on every level: whatever it does, same bits
        assert (n1 > 0) if info["batch_major"] else True, (info, n1)
    for xa, ra, ha in ((x1, r1, h1), (x2, r2, h2)):
        assert (ra.status, ra.outer_iterations, ra.inner_iterations, ra.mp_iterations, ra.inner_failures) == \
               (r0.status, r0.outer_iterations, r0.inner_iterations, r0.mp_iterations, r0.inner_failures)
        assert np.array_equal(ha, h0)
        assert len(xa) == len(x0)
        for a, b in zip(xa, x0):
            assert np.array_equal(a, b)


def test_tunable_and_environment_variable(built):
    """Values outside 0 / 1 are refused; ALFD_ML_TAIL_IN_SPMV is read at alfd_create (a fresh child process each)."""
    import os
    import subprocess
    import sys
    ctx = solver.Context(0)
    try:
        for v in (0, 1):
            ctx.set_tunable("ml_tail_in_spmv", v)
        for v in (-1, 2, 7):
            with pytest.raises(solver.AlfdError) as e:
                ctx.set_tunable("ml_tail_in_spmv", v)
            assert e.value.status == _abi.E_INVALID
    finally:
        ctx.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import cases\n"
            "from fictitious_domain_al_preconditioners_amd import solver\n"
            "pb, cfg = cases.case('stokes3d_gmg')\n"
            "osys = cases.oracle_system(pb, cfg)\n"
            "rhs = cases.prepared_rhs(osys, pb, cfg)\n"
            "ctx = solver.context_from_problem(pb, cfg, aggregates=cases.aggregates_of(pb, cfg))\n"
            "x, res = ctx.solve(rhs)\n"
            "print('FUSED', ctx.fused_tail_launches(), res.inner_iterations)\n"
            % (root, os.path.join(root, "tests")))
    counts = {}
    for v in ("0", "1"):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ALFD_ML_TAIL_IN_SPMV=v, ALFD_SPMV_WINDOW_MIN_BLOCKS="1"),
                             check=True,
                             capture_output=True, text=True, timeout=600).stdout
        line = [ln for ln in out.splitlines() if ln.startswith("FUSED")][-1].split()
        counts[v] = (int(line[1]), int(line[2]))
    print("fused launches, inner iterations: ALFD_ML_TAIL_IN_SPMV=0", counts["0"], "=1", counts["1"])
    assert counts["0"][0] == 0 and counts["1"][0] > 0 and counts["0"][1] == counts["1"][1]


# ------------------------------------------------------------------------------------------- the kernel, through the hook
class Step:
    """Inputs of one step on an n-row operator: computed once per (n, seed), read-only."""

    def __init__(self, n, seed, nt=NT):
        rng = np.random.default_rng(seed)
        self.n = n
        self.x = rng.uniform(-1.0, 1.0, n)
        self.t = rng.uniform(-1.0, 1.0, nt)
        self.dinv = rng.uniform(0.5, 2.0, n)
        self.rin, self.din, self.zin, self.zout = (rng.uniform(-1.0, 1.0, n) for _ in range(4))
        self.fill = FILL + np.arange(n, dtype=np.float64)
        for a in (self.x, self.t, self.dinv, self.rin, self.din, self.zin, self.zout, self.fill):
            a.setflags(write=False)


def _ct(n, rows, seed=5):
    """Ct with 1 .. 20 entries in each of `rows` (sorted, distinct), none elsewhere."""
    rng = np.random.default_rng(seed)
    cnt = np.zeros(n, np.int64)
    cnt[list(rows)] = rng.integers(1, 21, len(rows))
    rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(NT, int(k), replace=False)) for k in cnt if k] or [np.zeros(0)]).astype(np.int32)
    return rp, col, rng.uniform(-1.0, 1.0, col.size), NT


def _run(ctx, form, mode, st, ct, slot_c=-1, w=None, **over):
    kw = dict(gamma=3.5, c1=0.625, c2=-1.75, store_res=1, slot_c=slot_c, w=w, dinv=st.dinv, rin=st.rin, din=st.din,
              zin=st.zin, y=st.fill, res=st.fill + 0.25, d=st.fill + 0.5, z=st.fill + 0.75, zout=st.zout)
    kw.update(over)
    return ctx.spmv_tail_step(_abi.A, form, mode, ct, st.x, st.t if w is None else np.full(NT, np.nan), **kw)


def _compare(ctx, st, ct, tag, modes=MODES, **kw):
    listed = np.diff(ct[0]) > 0
    for mode in modes:
        for store_res in ((0, 1) if mode == _abi.TAIL_RES_INIT else (1,)):
            before = ctx.fused_tail_launches()
            a = _run(ctx, 0, mode, st, ct, store_res=store_res, **kw)
            assert ctx.fused_tail_launches() == before + 1, (tag, mode)
            b = _run(ctx, 1, mode, st, ct, store_res=store_res, **kw)
            assert ctx.fused_tail_launches() == before + 1, (tag, mode)
            stored = {_abi.TAIL_STEP: ("res", "d", "z"), _abi.TAIL_LAST: ("z",), _abi.TAIL_LAST_ADD: ("zout",),
                      _abi.TAIL_RES: ("res",), _abi.TAIL_RES_INIT: ("z", "res") if store_res else ("z",)}[mode]
            for k in ("res", "d", "z", "zout") + (("t",) if "t" in b else ()):
                bad = np.flatnonzero(~(a[k] == b[k]))
                assert bad.size == 0, (tag, mode, store_res, k, int(bad.size), int(bad[0]))
            for k, off in (("res", 0.25), ("d", 0.5), ("z", 0.75)):
                if k in stored:
                    assert not np.any(b[k] == st.fill + off), (tag, mode, k, "not stored")
                else:
                    assert np.array_equal(b[k], st.fill + off), (tag, mode, k, "stored")
            assert np.array_equal(b["zout"], st.zout) == ("zout" not in stored), (tag, mode)
            assert np.array_equal(a["y"][listed], b["y"][listed]), (tag, mode, "y on the rows of Ct")
            assert np.array_equal(a["y"][~listed], st.fill[~listed]), (tag, mode, "y stored outside Ct")


@pytest.fixture
def ctx(built, monkeypatch):
    monkeypatch.setenv("ALFD_SPMV_WINDOW_MIN_BLOCKS", "1")
    c = solver.Context(0)
    yield c
    c.close()


def _upload(ctx, m, rows=None, share=1, blocks=None, wide=0):
    if rows is not None:
        ctx.set_tunable("batch_major_rows", rows)
    ctx.set_tunable("batch_major_share", share)
    if blocks is not None:
        ctx.set_row_blocks(_abi.A, *blocks)
    ctx.set_matrix(_abi.A, m)
    info = ctx.matrix_info(_abi.A)
    assert info["batch_major"] in (1, 2) and info["lanes"] == 64 and info["batch_major_wide"] == wide, info
    return info


@pytest.mark.parametrize("n", lc.LONG_SIZES)
def test_rows_of_ct_at_the_block_edges(ctx, n):
    """96 rows per block.  (i) no row in Ct; (ii) every row of block 1 and none of blocks 0 and 2; (iii) the first and
    the last row of a block and the last row of the matrix."""
    m = lc.long_rows(n, "few", 384)
    info = _upload(ctx, m, rows=96)
    assert info["batch_major_blocks"] == -(-n // 96)
    st = Step(n, 60 + n)
    _compare(ctx, st, _ct(n, []), ("no row", n))
    _compare(ctx, st, _ct(n, range(96, 192)), ("one block", n))
    _compare(ctx, st, _ct(n, [96, 191, 192, n - 1]), ("edges", n))


def test_last_block_shorter_than_a_batch(ctx):
    """(iv) 3 365 rows in blocks of 96 and two last blocks of 3 and 2 rows; rows of Ct in both."""
    n = 3365
    m = lc.long_rows(n, "few", 384)
    ptr = np.r_[np.arange(0, 3361, 96), 3363, 3365].astype(np.int64)
    info = _upload(ctx, m, blocks=(ptr, np.arange(n, dtype=np.int32)))
    assert info["batch_major"] == 2 and info["batch_major_blocks"] == ptr.size - 1
    _compare(ctx, Step(n, 61), _ct(n, [5, 3361, 3364]), "short last blocks")


def test_plain_batches_only_and_most_batches_per_block(ctx):
    """Without sharing every batch is a plain one of four rows of one class: 96 ragged rows of up to six classes make
    the most batches per block the planner produces for this operator -- the row buffer's high-water mark."""
    n = 3072
    m = lc.long_rows(n, "few", 384)
    with_sharing = _upload(ctx, m, rows=96)["batch_major_batches"]
    info = _upload(ctx, m, rows=96, share=0)
    print("batches with / without sharing", with_sharing, info["batch_major_batches"], "blocks", info["batch_major_blocks"],
          "lds", info["batch_major_lds_bytes"])
    assert info["shared_nnz"] == 0 and info["batch_major_batches"] >= with_sharing, info
    assert info["batch_major_batches"] >= 24 * info["batch_major_blocks"]      # 96 rows: 24 batches and more
    _compare(ctx, Step(n, 62), _ct(n, [0, 95, 96, 1000, 3071]), "plain batches")


def test_shared_batches_of_every_size_in_mesh_bricks(ctx):
    """The planted operators hold no translates (no shared batch, asserted above through the batch counts): the edge
    rows of test_gpu_batch_loop.py in mesh bricks bring shared batches of 16, 8 and 4 rows beside plain ones, and empty
    rows."""
    from test_gpu_batch_loop import GEN, _edge_rows
    base = problems.generate(n_cells=6, **GEN)
    m = _edge_rows(base.mats["A"])
    info = _upload(ctx, m, rows=96, blocks=problems.brick_row_blocks(base.params, (4, 2, 2)))
    assert info["batch_major"] == 2 and 0 < info["shared_nnz"] < m.nnz, info
    n = m.nrows
    _compare(ctx, Step(n, 67), _ct(n, [0, 1, 97, 500, 501, 502, 5300, n - 1]), "bricks")


def test_wide_codes(ctx):
    """More than 512 distinct values in a block: the 10-bit codes, whose dictionary takes 8 KB of the LDS."""
    n = 3072
    a = lc.long_rows(n, "few", 384)
    v = np.array(a.val) * (1.0 + np.random.default_rng(7).integers(0, 32, a.nnz) / 32.0)
    m = problems.Csr(n, n, np.array(a.row_ptr), np.array(a.col), v)
    _upload(ctx, m, rows=48, wide=1)
    _compare(ctx, Step(n, 63), _ct(n, [47, 48, 2000]), "wide codes")


def test_an_output_at_the_address_of_x_is_refused(ctx):
    n = 480
    m = lc.long_rows(n, "few", 384)
    _upload(ctx, m, rows=96)
    st, ct = Step(n, 64), _ct(n, [7])
    for mode, name in ((_abi.TAIL_STEP, "z"), (_abi.TAIL_STEP, "d"), (_abi.TAIL_STEP, "res"), (_abi.TAIL_LAST, "z"),
                       (_abi.TAIL_LAST_ADD, "zout"), (_abi.TAIL_RES, "res"), (_abi.TAIL_RES_INIT, "z"), (_abi.TAIL_RES, "y")):
        before = ctx.fused_tail_launches()
        with pytest.raises(solver.AlfdError) as e:
            _run(ctx, 0, mode, st, ct, **{name: "x"})
        assert e.value.status == _abi.E_INVALID, (mode, name)
        assert ctx.fused_tail_launches() == before
    # an INPUT at the address of x is what the sweep does (its first direction is the iterate): accepted, same bits
    a = _run(ctx, 0, _abi.TAIL_STEP, st, ct, din="x", zin="x")
    b = _run(ctx, 1, _abi.TAIL_STEP, st, ct, din="x", zin="x")
    for k in ("res", "d", "z"):
        assert np.array_equal(a[k], b[k]), k
    # and in place, as the later steps of a sweep run: res over rin
    a = _run(ctx, 0, _abi.TAIL_STEP, st, ct, res="rin")
    b = _run(ctx, 1, _abi.TAIL_STEP, st, ct, res="rin")
    for k in ("res", "d", "z"):
        assert np.array_equal(a[k], b[k]), k


def test_mode_without_an_epilogue_and_operator_without_one(ctx):
    """TAIL_RES_INIT_ADD keeps the separate launch; so does an operator with half of its rows in Ct."""
    n = 480
    _upload(ctx, lc.long_rows(n, "few", 384), rows=96)
    st = Step(n, 65)
    for mode, ct in ((_abi.TAIL_RES_INIT_ADD, _ct(n, [7])), (_abi.TAIL_RES, _ct(n, range(0, n, 2)))):
        before = ctx.fused_tail_launches()
        with pytest.raises(solver.AlfdError) as e:
            _run(ctx, 0, mode, st, ct)
        assert e.value.status in (_abi.E_INVALID, _abi.E_UNSUPPORTED)
        assert ctx.fused_tail_launches() == before
        _run(ctx, 1, mode, st, ct)


# ---------------------------------------------------------------- the tail launch itself: aug_tail_kernel<L, MODE>
LANE_ROWS = {4: (1, 6), 8: (7, 12), 16: (13, 24), 32: (25, 48), 64: (49, 96)}   # lanes: row lengths of Ct, uniform
NT_LANES = 96
ALL_MODES = MODES + [_abi.TAIL_RES_INIT_ADD]


def _tail_reference(mode, store_res, y, st, c1, c2):
    """The vectors `mode` stores, from the header comment of aug_tail_kernel (kernels.hpp): res = rin - y;
    step modes d = fma(c1, din, c2 * (dinv .* res)), z = zin + d; init modes z = c1 * (dinv .* res);
    the ADD modes zout = fma(1, z, zout)."""
    from sparse_product_reference import fma
    res = st.rin - y
    out = {}
    if mode in (_abi.TAIL_STEP, _abi.TAIL_LAST, _abi.TAIL_LAST_ADD):
        prod = c2 * (st.dinv * res)
        d = np.array([fma(c1, float(a), float(b)) for a, b in zip(st.din, prod)])
        z = st.zin + d
    elif mode != _abi.TAIL_RES:
        z = c1 * (st.dinv * res)
    if mode in (_abi.TAIL_STEP, _abi.TAIL_RES) or (mode == _abi.TAIL_RES_INIT and store_res):
        out["res"] = res
    if mode == _abi.TAIL_STEP:
        out["d"] = d
    if mode in (_abi.TAIL_STEP, _abi.TAIL_LAST, _abi.TAIL_RES_INIT):
        out["z"] = z
    if mode in (_abi.TAIL_LAST_ADD, _abi.TAIL_RES_INIT_ADD):
        out["zout"] = np.array([fma(1.0, float(a), float(b)) for a, b in zip(z, st.zout)])
    return out


def test_tail_launch_every_lane_count_and_mode(built, monkeypatch):
    """aug_tail_kernel<L, MODE> for L = 4, 8, 16, 32, 64 and the six modes, Ct in full and in row-list form, through form 1
    of alfd_spmv_tail_step on 480 rows against the oracle, bit for bit: y = A x, y = fma(gamma, Ct t, y) at the lane
    count the row lengths of Ct give (asserted from the oracle's answer), then the element-wise expressions of the mode.
    A full-form Ct of 64-lane rows counts as plain CSR rows only where the stream kernel is off: ALFD_SPMV_STREAM_R = 0
    for this context (A then runs on spmv_kernel<64>; the canonical sums do not depend on that)."""
    from oracle import oracle
    monkeypatch.setenv("ALFD_SPMV_STREAM_R", "0")
    n, gamma, c1, c2 = 480, 3.5, 0.625, -1.75
    A = lc.long_rows(n, "few", 384)
    st = Step(n, 68, NT_LANES)
    ax, _ = oracle.spmv(A, st.x, None, mode=0)
    ctx = solver.Context(0)
    try:
        ctx.set_matrix(_abi.A, A)
        for L, (lo, hi) in LANE_ROWS.items():
            for form, rows in (("full", np.arange(n)), ("row list", np.arange(0, n, 4))):
                rng = np.random.default_rng(100 + L + len(rows))
                cnt = np.zeros(n, np.int64)
                cnt[rows] = rng.integers(lo, hi + 1, len(rows))
                rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
                col = np.concatenate([np.sort(rng.choice(NT_LANES, int(k), replace=False)) for k in cnt if k]).astype(np.int32)
                val = rng.uniform(-1.0, 1.0, col.size)
                y, used = oracle.spmv(problems.Csr(n, NT_LANES, rp, col, val), st.t, ax, mode=1, alpha=gamma, lanes=0)
                assert used == L, (L, form, used)
                assert not np.array_equal(y[rows], ax[rows])
                for mode in ALL_MODES:
                    for store_res in ((0, 1) if mode == _abi.TAIL_RES_INIT else (1,)):
                        tag = (L, form, mode, store_res)
                        got = _run(ctx, 1, mode, st, (rp, col, val, NT_LANES), store_res=store_res)
                        want = _tail_reference(mode, store_res, y, st, c1, c2)
                        assert np.array_equal(got["y"], ax), (tag, "y")     # the tail consumes y + gamma Ct t, stores it nowhere
                        for k, fill in (("res", st.fill + 0.25), ("d", st.fill + 0.5), ("z", st.fill + 0.75), ("zout", st.zout)):
                            bad = np.flatnonzero(~(got[k] == want.get(k, fill)))
                            assert bad.size == 0, (tag, k, "stored" if k in want else "kept", int(bad.size), int(bad[0]))
                            if k in want:
                                assert not np.any(got[k] == fill), (tag, k, "not stored")
    finally:
        ctx.close()


def test_epilogue_beside_the_second_party_of_a_pair_launch(ctx):
    """A level-1-like pair: C with NT rows rides behind A's workgroups, t = w .* (C x) feeds the rows party."""
    from test_gpu_pair_launch import _random_c
    n = 3365
    m = lc.long_rows(n, "few", 384)
    _upload(ctx, m, rows=96)
    ctx.set_matrix(_abi.C_, _random_c(NT, n, 32, 9))
    assert ctx.matrix_info(_abi.C_)["batch_major"] == 0
    w = np.random.default_rng(3).uniform(0.5, 2.0, NT)
    for fuse in (2, 3, 1):                  # slot A is a fine-level operator: the pair launch takes it from ml_fuse 3 on
        ctx.set_tunable("ml_fuse", fuse)
        _compare(ctx, Step(n, 66), _ct(n, [0, 100, 191, 3364]), ("pair", fuse), slot_c=_abi.C_, w=w)
