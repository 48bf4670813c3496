"""The pair launch of the factored operators (tunable "ml_fuse" >= 2, alfd_spmv_pair): t = d .* (C x) as extra workgroups
of the grid that computes y = A x.

Kernel level: alfd_spmv_pair against alfd_spmv (slot A) plus alfd_spmv_scaled (slot C) on the same context, bit for bit
out of NaN-prefilled outputs -- both first parties (the long-row batch-major kernel and the streaming kernel), the second
party with 16, 32 and 64 lanes per row, C with one row, with more and with fewer workgroups than A, the XCD-contiguous
block order (which must count A's workgroups, not the grid's).

Solve level: the same solve on ONE context with ml_fuse 3, 2, 1, 0 and 3 again gives the same bits, on the small cases
as they are (stream and plain forms) and with the window threshold lowered so that their patch and level operators are
batch-major with few blocks.

Launch counts: one application of the inner preconditioner at a size where the kernels of the bench run; every level of
ml_fuse removes timed launches, and a pair is ONE launch of A's timing class."""
import numpy as np
import pytest
import scipy.sparse as sp

import cases
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver
from test_gpu_spmv_epilogues import long_problem  # noqa: F401  (the long-row operator and its row blocks)

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx(built):
    c = solver.Context(0)
    yield c
    c.close()


def _random_c(nrows, ncols, lanes, seed):
    """Row lengths around `lanes` (Poisson-like, some beyond one pass of the lane group), every 11th row empty."""
    a = sp.random(nrows, ncols, density=(lanes - 2) / ncols, random_state=seed, format="lil")
    for r in range(5, nrows, 11):
        a.rows[r], a.data[r] = [], []
    a = a.tocsr()
    a.data[:] = np.random.default_rng(seed).uniform(-1, 1, a.nnz)
    return problems.Csr.from_scipy(a)


def _check_pair(ctx, nr_a, nr_c, x, tag):
    """slot A (nr_a rows) / slot C (nr_c rows) of ctx through the pair launch against the two separate launches."""
    d = np.random.default_rng(nr_c).uniform(0.5, 2.0, nr_c) * np.exp2(np.arange(nr_c) % 41 - 20.0)
    y_ref, _ = ctx.spmv(_abi.A, x, np.full(nr_a, np.nan), mode=0)
    t_ref = ctx.spmv_scaled(_abi.C_, x, d, np.full(nr_c, np.nan))
    y, t = ctx.spmv_pair(_abi.A, _abi.C_, x, d, np.full(nr_a, np.nan), np.full(nr_c, np.nan))
    assert not np.isnan(y_ref).any() and not np.isnan(t_ref).any(), tag
    assert np.array_equal(y, y_ref), (tag, "y", int(np.count_nonzero(y != y_ref)))
    assert np.array_equal(t, t_ref), (tag, "t", int(np.count_nonzero(t != t_ref)))


def _c_sizes(n_a, lanes):
    """Row counts of C: one row; fewer and more workgroups (256 / lanes rows each) than A's n_a; no multiple of a group."""
    rpb = 256 // lanes
    sizes = {"one row": 1, "fewer": 37 * rpb + 3, "more": (n_a + 40) * rpb + 3}
    assert sizes["fewer"] // rpb + 1 < n_a < sizes["more"] // rpb and n_a + 41 < 2048
    return sizes


def _run_c_sizes(ctx, nr_a, n_a, ncols, lanes, x, tag):
    for name, nrows in _c_sizes(n_a, lanes).items():
        c = _random_c(nrows, ncols, lanes, 100 + lanes) if nrows > 1 else \
            problems.Csr(1, ncols, np.array([0, lanes + 3], np.int64), np.arange(0, 5 * (lanes + 3), 5, dtype=np.int32),
                         np.linspace(-1.0, 1.0, lanes + 3))
        assert nrows % (256 // lanes) != 0
        ctx.set_matrix(_abi.C_, c)
        info = ctx.matrix_info(_abi.C_)
        assert (info["lanes"], info["windowed"], info["batch_major"]) == (lanes, 0, 0), info
        _check_pair(ctx, nr_a, nrows, x, (tag, lanes, name))
    return nrows


@pytest.mark.parametrize("lanes", [16, 32, 64])
def test_pair_on_the_batch_major_kernel_bitwise(ctx, long_problem, lanes):
    """spmv_vs_kernel<0, 0, 4, 0, true> on mesh bricks; the XCD order remaps by A's block count."""
    m = long_problem.mats["A"]
    ctx.set_row_blocks(_abi.A, *problems.brick_row_blocks(long_problem.params, (8, 2, 2)))
    ctx.set_matrix(_abi.A, m)
    info = ctx.matrix_info(_abi.A)
    assert info["batch_major"] == 2 and info["lanes"] == 64 and info["batch_major_wide"] == 0, info
    assert info["batch_major_blocks"] >= 256
    x = np.random.default_rng(3).uniform(-1.0, 1.0, m.ncols)
    more = _run_c_sizes(ctx, m.nrows, info["batch_major_blocks"], m.ncols, lanes, x, "batch-major")
    ctx.set_tunable("batch_major_xcd", 1)
    _check_pair(ctx, m.nrows, more, x, ("batch-major, xcd order", lanes))   # C: the last size, more workgroups than A
    fewer = 37 * (256 // lanes) + 3
    ctx.set_matrix(_abi.C_, _random_c(fewer, m.ncols, lanes, 7))
    _check_pair(ctx, m.nrows, fewer, x, ("batch-major, xcd order, fewer", lanes))


@pytest.mark.parametrize("lanes", [16, 32, 64])
def test_pair_on_the_stream_kernel_bitwise(ctx, lanes):
    """spmv_stream_kernel<2, 8, 0, false, true>: a 64-lane operator far below the window threshold, 3001 rows (odd: the
    last batch of two rows is half empty, the last workgroup holds one wave's worth)."""
    a = sp.random(3001, 2500, density=70 / 2500.0, random_state=70, format="csr")
    a.data[:] = np.random.default_rng(5).uniform(-1, 1, a.nnz)
    ctx.set_matrix(_abi.A, problems.Csr.from_scipy(a))
    info = ctx.matrix_info(_abi.A)
    assert (info["lanes"], info["windowed"], info["batch_major"]) == (64, 0, 0), info
    x = np.random.default_rng(4).uniform(-1.0, 1.0, 2500)
    _run_c_sizes(ctx, 3001, (1501 + 3) // 4, 2500, lanes, x, "stream")


def test_pair_that_does_not_qualify_is_refused_untouched(ctx):
    """A on spmv_kernel<16> (no pair instantiation), C with 8 lanes per row, different column counts: E_UNSUPPORTED, and
    neither output is written."""
    short = _random_c(3001, 2500, 16, 1)
    long_ = sp.random(3001, 2500, density=70 / 2500.0, random_state=70, format="csr")
    x, d = np.ones(2500), np.ones(3001)
    y, t = np.full(3001, np.nan), np.full(3001, np.nan)

    def refused():
        rc = ctx._lib.alfd_spmv_pair(ctx._h, _abi.A, _abi.C_, x.ctypes.data, d.ctypes.data, y.ctypes.data, t.ctypes.data)
        assert rc == _abi.E_UNSUPPORTED, rc
        assert np.isnan(y).all() and np.isnan(t).all()

    ctx.set_matrix(_abi.A, short)
    ctx.set_matrix(_abi.C_, short)
    assert ctx.matrix_info(_abi.A)["lanes"] == 16
    refused()
    ctx.set_matrix(_abi.A, problems.Csr.from_scipy(long_))
    ctx.set_matrix(_abi.C_, _random_c(3001, 2500, 8, 2))
    assert ctx.matrix_info(_abi.C_)["lanes"] == 8
    refused()
    ctx.set_matrix(_abi.C_, _random_c(3001, 2400, 16, 3))
    refused()
    with pytest.raises(solver.AlfdError):
        ctx.spmv_pair(_abi.A, _abi.C_, x, d, y, t)
    ctx.set_matrix(_abi.C_, short)                        # and the same call goes through once the pair qualifies
    _check_pair(ctx, 3001, 3001, x, "qualifies")


def test_argument_validation_on_a_live_context(ctx):
    """ALFD_E_INVALID for a null x, d, y or t, for t == y, an unset slot and a slot out of range, on a pair that
    qualifies; nothing is written.  The same call with valid arguments then goes through."""
    a = sp.random(300, 250, density=70 / 250.0, random_state=1, format="csr")
    ctx.set_matrix(_abi.A, problems.Csr.from_scipy(a))
    ctx.set_matrix(_abi.C_, _random_c(301, 250, 16, 4))
    assert ctx.matrix_info(_abi.A)["lanes"] == 64 and ctx.matrix_info(_abi.C_)["lanes"] == 16
    x, d = np.ones(250), np.ones(301)
    y, t = np.full(301, np.nan), np.full(301, np.nan)      # y one longer than A's rows: usable in t's place too
    px, pd, py, pt = x.ctypes.data, d.ctypes.data, y.ctypes.data, t.ctypes.data
    lib, h = ctx._lib, ctx._h
    for args in ((None, pd, py, pt), (px, None, py, pt), (px, pd, None, pt), (px, pd, py, None), (px, pd, py, py),
                 (px, pd, pt, pt)):
        assert lib.alfd_spmv_pair(h, _abi.A, _abi.C_, *args) == _abi.E_INVALID, args
    for slots in ((_abi.B, _abi.C_), (_abi.A, _abi.B), (-1, _abi.C_), (_abi.A, -1), (99, _abi.C_), (_abi.A, 99)):
        assert lib.alfd_spmv_pair(h, *slots, px, pd, py, pt) == _abi.E_INVALID, slots
    assert np.isnan(y).all() and np.isnan(t).all()
    with pytest.raises(ValueError):
        ctx.spmv_pair(_abi.A, _abi.C_, x, np.ones(2), y[:300], t)
    assert lib.alfd_spmv_pair(h, _abi.A, _abi.C_, px, pd, py, pt) == _abi.OK
    assert not np.isnan(y[:300]).any() and np.isnan(y[300]) and not np.isnan(t).any()


def _solve(ctx, rhs, fuse):
    ctx.set_tunable("ml_fuse", fuse)
    x, res = ctx.solve(rhs, raise_on_failure=False)
    return x, res, ctx.history().copy()


@pytest.mark.parametrize("batch_major", [False, True])
@pytest.mark.parametrize("name", ["stokes3d_gmg_patch", "stokes3d_gmg", "elliptic_modified_gmg_patch"])
def test_every_fuse_level_solves_bit_for_bit(built, monkeypatch, name, batch_major):
    if batch_major:    # read at alfd_create: patch and level operators of these N = 8 cases take the batch-major form
        monkeypatch.setenv("ALFD_SPMV_WINDOW_MIN_BLOCKS", "8")
    pb, cfg = cases.case(name)
    levels = cases.aggregates_of(pb, cfg)
    rhs = cases.prepared_rhs(cases.oracle_system(pb, cfg), pb, cfg)
    ctx = solver.context_from_problem(pb, cfg, aggregates=levels)
    try:
        # the lowered threshold takes effect: the fine Stokes operator (more than 8 row blocks at N = 8) is batch-major
        # in that arm only; and pairs do launch in either arm: each level of ml_fuse takes timed launches out of the solve
        info = ctx.matrix_info(_abi.A)
        stokes = name.startswith("stokes")
        if stokes:
            assert (info["batch_major"] != 0) == batch_major and info["lanes"] == 64, info
        runs, launches = [], {}
        for fuse in (3, 2, 1, 0, 3):
            ctx.enable_timing(2)
            runs.append(_solve(ctx, rhs, fuse))
            launches[fuse] = sum(v["launches"] for v in ctx.timing().values())
    finally:
        ctx.close()
    print(name, "timed launches per solve by ml_fuse:", launches)
    if stokes:
        assert launches[3] < launches[2] < launches[1] < launches[0], launches
    else:       # 9-point operators, 8 lanes per row: no pair qualifies, every level above 1 is the two launches
        assert info["lanes"] == 8 and launches[3] == launches[2] == launches[1] < launches[0], (info, launches)
    x0, r0, h0 = runs[3]
    print(name, "batch-major" if batch_major else "as is", "outer", r0.outer_iterations, "inner", r0.inner_iterations)
    assert r0.outer_iterations > 0 and r0.inner_iterations > 0
    for xa, ra, ha in runs:
        assert (ra.status, ra.outer_iterations, ra.inner_iterations, ra.mp_iterations, ra.inner_failures) == \
               (r0.status, r0.outer_iterations, r0.inner_iterations, r0.mp_iterations, r0.inner_failures)
        assert np.array_equal(ha, h0)
        assert len(xa) == len(x0)
        for a, b in zip(xa, x0):
            assert np.array_equal(a, b)


def test_every_fuse_level_removes_launches(built):
    """One application of the inner preconditioner on the N = 20 problem with the bench settings (bricks 16x4x1, A on
    the batch-major kernel): same bits with ml_fuse 1, 2 and 3, strictly fewer timed launches each time, and the same
    number of spmv_A launches -- the fine pair is one launch of that class, not none and not two."""
    pb = problems.stokes3d_sphere(20, 2)
    cfg = _abi.bench_multilevel_settings(_abi.default_config(_abi.AL_STOKES), geometric=True)
    levels = problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE)
    ctx = solver.context_from_problem(pb, cfg, aggregates=levels, row_blocks=problems.brick_row_blocks(pb.params, (16, 4, 1)))
    try:
        assert ctx.matrix_info(_abi.A)["batch_major"] == 2
        r = np.random.default_rng(9).uniform(-1.0, 1.0, pb.block_sizes[0])
        out, total, spmv_a = {}, {}, {}
        for fuse in (1, 2, 3):
            ctx.set_tunable("ml_fuse", fuse)
            ctx.enable_timing(2)                 # restarts the counters
            out[fuse] = ctx.inner_prec_apply(r)
            t = ctx.timing()
            total[fuse] = sum(v["launches"] for v in t.values())
            spmv_a[fuse] = t["spmv_A"]["launches"]
    finally:
        ctx.close()
    print("timed launches per apply:", total, "of class spmv_A:", spmv_a)
    assert np.array_equal(out[1], out[2]) and np.array_equal(out[1], out[3])
    assert total[1] > total[2] > total[3], total
    assert spmv_a[1] == spmv_a[2] == spmv_a[3] > 0, spmv_a
