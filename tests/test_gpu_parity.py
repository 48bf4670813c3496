"""GPU parity tests: the HIP path, called through the C ABI, against the CPU
oracle on the same seeded inputs, against the committed golden fixtures, and --
at a size the oracle cannot reach in seconds -- through size-independent
properties (linearity, transpose duality, A^-1 A = I through the solver).

Bar (north_star): identical iteration counts, residuals within 1e-10 relative.
The canonical arithmetic actually makes primitives and
whole solves bit-identical, which is what most asserts check."""
import json
import os

import numpy as np
import pytest

import cases
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver
from oracle import oracle

pytestmark = pytest.mark.gpu
HIST_RTOL = 1e-10          # tolerance north_star states for residuals
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rng_vec(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


@pytest.fixture(scope="module")
def ctxs(built):
    cache = {}

    def get(name):
        if name not in cache:
            pb, cfg = cases.case(name)
            cache[name] = (pb, cfg, solver.context_from_problem(pb, cfg, aggregates=cases.aggregates_of(pb, cfg)),
                           cases.oracle_system(pb, cfg))
        return cache[name]
    yield get
    for _, _, c, _ in cache.values():
        c.close()


@pytest.mark.parametrize("name", ["A", "Bt", "B", "Ct", "C", "Mp"])
@pytest.mark.parametrize("mode", [0, 1])
def test_spmv_bitwise(ctxs, name, mode):
    pb, cfg, ctx, _ = ctxs("stokes3d_sphere")
    m = pb.mats[name]
    x = _rng_vec(m.ncols, 1)
    y0 = _rng_vec(m.nrows, 2)
    got, lanes = ctx.spmv(_abi.SLOT_BY_NAME[name], x, y0, mode=mode, alpha=-0.75)
    ref, olanes = oracle.spmv(m, x, y0 if mode else None, mode=mode, alpha=-0.75)
    assert lanes == olanes
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("blocks", ["runs", "bricks", "bricks444", "ragged", "rcb", "bricks_noshare"])
def test_batch_major_format_bitwise(built, blocks):
    """The batch-major value-indexed format (kernels_vs.hpp, tunable batch_major): row blocks as runs of
    the numbering, as mesh bricks handed in through alfd_set_row_blocks, and as ragged random-size
    blocks of a random row permutation; epilogues 0 and 1 (the diagonal-scaled epilogues 2 and 3:
    tests/test_gpu_spmv_epilogues.py); against the oracle's canonical SpMV."""
    big = problems.generate(dim=3, degree=2, ncomp=3, n_cells=20, stokes=False, grad_div=True,
                            gamma_grad_div=10.0, radius=0.1, immersed_refine=0)
    m = big.mats["A"]
    rng = np.random.default_rng(11)
    ctx = solver.Context(0)
    try:
        ctx.set_tunable("batch_major", 1)
        if blocks == "bricks":
            ctx.set_row_blocks(_abi.A, *problems.brick_row_blocks(big.params, (8, 2, 2)))
        elif blocks == "bricks_noshare":            # every row stored: plain 4-row batches only
            ctx.set_tunable("batch_major_share", 0)
            ctx.set_row_blocks(_abi.A, *problems.brick_row_blocks(big.params, (16, 4, 1)))
        elif blocks == "bricks444":
            ctx.set_tunable("batch_major_waves", 8)
            ctx.set_row_blocks(_abi.A, *problems.brick_row_blocks(big.params, (4, 4, 4)))
        elif blocks == "rcb":
            ctx.set_row_blocks(_abi.A, *solver.row_blocks_from_points(problems.row_support_points(big.params), 192))
        elif blocks == "ragged":
            perm = np.argsort((np.arange(m.nrows) // 32) * 1000 + rng.integers(0, 1000, m.nrows), kind="stable")
            sizes = rng.integers(1, 48, m.nrows // 16)
            ptr = np.minimum(np.r_[0, np.cumsum(sizes)], m.nrows)
            ptr = np.unique(np.r_[ptr, m.nrows])
            ctx.set_row_blocks(_abi.A, ptr, perm)
        ctx.set_matrix(_abi.A, m)
        info = ctx.matrix_info(_abi.A)
        assert info["batch_major"] == (1 if blocks == "runs" else 2), info
        if blocks == "bricks_noshare":
            assert 3.0 * m.nnz < info["streamed_bytes"] < 3.8 * m.nnz
        else:
            assert info["streamed_bytes"] < (4.0 if blocks == "ragged" else 2.5) * m.nnz, info["streamed_bytes"] / m.nnz
        x = _rng_vec(m.ncols, 3)
        y0 = _rng_vec(m.nrows, 4)
        for mode in (0, 1):
            got, lanes = ctx.spmv(_abi.A, x, y0, mode=mode, alpha=-0.75)
            ref, olanes = oracle.spmv(m, x, y0 if mode else None, mode=mode, alpha=-0.75)
            assert lanes == olanes and np.array_equal(got, ref), (blocks, mode)
        with pytest.raises(solver.AlfdError):
            ctx.set_row_blocks(_abi.A, np.array([0, 5, m.nrows]), np.zeros(m.nrows, np.int32))   # not a partition
            ctx.set_matrix(_abi.A, m)
    finally:
        ctx.close()


def test_batch_major_format_edge_rows_bitwise(built):
    """Batch-major format with structurally EMPTY rows (class 0 batches), single-entry rows, and a few
    randomly perturbed rows that break the translate structure of their neighbours; and the refusal of a
    matrix with one row beyond 384 entries (it keeps the round-1 formats, same result)."""
    import scipy.sparse as sp
    big = problems.generate(dim=3, degree=2, ncomp=3, n_cells=20, stokes=False, grad_div=True,
                            gamma_grad_div=10.0, radius=0.1, immersed_refine=0)
    a = big.mats["A"].to_scipy().tolil()
    rng = np.random.default_rng(5)
    for r in range(0, a.shape[0], 97):
        a.rows[r], a.data[r] = [], []                      # empty rows
    for r in range(50, a.shape[0], 1013):
        a.rows[r], a.data[r] = a.rows[r][:1], a.data[r][:1]   # single-entry rows
    a = a.tocsr()
    for r in range(31, a.shape[0], 211):                   # perturbed values: no translate of anything
        a.data[a.indptr[r]:a.indptr[r + 1]] *= 1.0 + 0.25 * rng.integers(1, 4)
    m = problems.Csr.from_scipy(a)
    x = _rng_vec(m.ncols, 7)
    y0 = _rng_vec(m.nrows, 8)
    ctx = solver.Context(0)
    try:
        ctx.set_row_blocks(_abi.A, *problems.brick_row_blocks(big.params, (8, 4, 2)))
        ctx.set_matrix(_abi.A, m)
        assert ctx.matrix_info(_abi.A)["batch_major"] == 2
        for mode in (0, 1):
            got, _ = ctx.spmv(_abi.A, x, y0, mode=mode, alpha=0.5)
            ref, _ = oracle.spmv(m, x, y0 if mode else None, mode=mode, alpha=0.5)
            assert np.array_equal(got, ref)
        # one long row (> 384 entries): not representable, the other formats take over
        long = a.tolil()
        long.rows[1000] = list(range(0, 1200, 3))
        long.data[1000] = [0.5] * 400
        ml = problems.Csr.from_scipy(long.tocsr())
        ctx.set_matrix(_abi.A, ml)
        assert ctx.matrix_info(_abi.A)["batch_major"] == 0
        got, _ = ctx.spmv(_abi.A, x, y0, mode=0)
        ref, _ = oracle.spmv(ml, x, None, mode=0)
        assert np.array_equal(got, ref)
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["lap3d_L32", "q2_2d_L16", "lap2d_L8", "lap3d_perturbed"])
def test_batch_major_short_rows_bitwise(built, kind):
    """spmv_vss_kernel: the batch-major form for short rows (canonical L = 32 / 16 / 8 lanes per row): one stored
    template row per batch of translate rows.  Stencil operators of uniform grids, and one with every 7th row
    perturbed (rows without a translate partner are batches of one); epilogues 0 and 1; against the oracle."""
    gen = {"lap3d_L32": dict(dim=3, degree=1, ncomp=1, n_cells=74), "q2_2d_L16": dict(dim=2, degree=2, ncomp=1, n_cells=365),
           "lap2d_L8": dict(dim=2, degree=1, ncomp=1, n_cells=724), "lap3d_perturbed": dict(dim=3, degree=1, ncomp=1, n_cells=74)}[kind]
    m = problems.generate(radius=0.1, **gen).mats["A"]
    if kind == "lap3d_perturbed":
        v = np.array(m.val, copy=True)
        for r in range(3, m.nrows, 7):
            v[m.row_ptr[r]:m.row_ptr[r + 1]] *= 1.0 + 0.125 * (r % 5)
        m = problems.Csr(m.nrows, m.ncols, np.array(m.row_ptr), np.array(m.col), v)
    x = _rng_vec(m.ncols, 5)
    y0 = _rng_vec(m.nrows, 6)
    ctx = solver.Context(0)
    try:
        ctx.set_matrix(_abi.A, m)
        info = ctx.matrix_info(_abi.A)
        assert info["lanes"] == {"lap3d_L32": 32, "q2_2d_L16": 16, "lap2d_L8": 8, "lap3d_perturbed": 32}[kind]
        assert info["windowed"] and info["batch_major"] == 1, info
        assert info["streamed_bytes"] < 4.0 * m.nnz + 16.0 * m.nrows
        for mode in (0, 1):
            got, lanes = ctx.spmv(_abi.A, x, y0, mode=mode, alpha=-0.75)
            ref, olanes = oracle.spmv(m, x, y0 if mode else None, mode=mode, alpha=-0.75)
            assert lanes == olanes and np.array_equal(got, ref), (kind, mode)
        ctx.set_tunable("batch_major", 0)           # the L-lane window kernel on the same slot: same bits
        got, _ = ctx.spmv(_abi.A, x, y0, mode=0)
        assert np.array_equal(got, oracle.spmv(m, x, None, mode=0)[0])
    finally:
        ctx.close()


def test_divergence_and_gradient_blocks_bitwise(built):
    """B and Bt of the Stokes system at a size where the storage formats apply (N = 36: 50 653 pressure rows): B takes the
    batch-major form with blocks split for their x windows, Bt (short rows) whichever of its two forms the upload-time
    timing keeps; both equal the oracle's canonical SpMV bit for bit, in epilogues 0 and 1 (B under the scale of the
    nested grad-div term, epilogue 2: tests/test_gpu_spmv_epilogues.py)."""
    pb = problems.stokes3d_sphere(n_cells=36, immersed_refine=2)
    ctx = solver.Context(0)
    try:
        for name, slot in (("B", _abi.B), ("Bt", _abi.BT)):
            m = pb.mats[name]
            ctx.set_matrix(slot, m)
            info = ctx.matrix_info(slot)
            if name == "B":
                assert info["batch_major"] == 1 and info["streamed_bytes"] < 2.5 * m.nnz, info
            x = _rng_vec(m.ncols, 21)
            y0 = _rng_vec(m.nrows, 22)
            for mode in (0, 1):
                got, lanes = ctx.spmv(slot, x, y0, mode=mode, alpha=0.625)
                ref, olanes = oracle.spmv(m, x, y0 if mode else None, mode=mode, alpha=0.625)
                assert lanes == olanes and np.array_equal(got, ref), (name, mode)
    finally:
        ctx.close()


def test_spmv_every_kernel_family_bitwise(built):
    """Matrices that exercise each lanes-per-row kernel, the sparse-row form, the
    streaming kernel and the LDS-windowed kernel (>= 512 row blocks), incl.
    ragged rows, empty rows and a single-entry row."""
    rng = np.random.default_rng(5)
    import scipy.sparse as sp
    mats = {}
    for avg in (3, 7, 14, 30, 70, 200):
        n = 3001                          # odd: the last wave holds a partially filled set of row groups
        a = sp.random(n, 2500, density=avg / 2500.0, random_state=int(avg), format="csr")
        a.data[:] = rng.uniform(-1, 1, a.nnz)
        mats[f"rand{avg}"] = problems.Csr.from_scipy(a)
    a = sp.random(5000, 400, density=0.05, random_state=1, format="lil")
    a[10:4900, :] = 0                      # mostly empty rows -> sparse-row kernel
    mats["sparse_rows"] = problems.Csr.from_scipy(a.tocsr())
    big = problems.generate(dim=3, degree=2, ncomp=3, n_cells=20, stokes=False, grad_div=True,
                            gamma_grad_div=10.0, radius=0.1, immersed_refine=0)
    mats["windowed"] = big.mats["A"]       # 206763 rows >= 96*512 -> LDS-windowed kernel
    # value-indexed forms of the same matrix: 8-bit codes (as uploaded), 16-bit codes (every value
    # scaled by one of 9 factors: ~400 distinct per block) and raw blocks (40% unique values in the
    # first 30% of the rows); fully random values -> no dictionary
    expect_format = {"windowed": "dict"}
    for name, share in (("win_escape", 0.05), ("win_rawblocks", 0.4), ("win_novi", 1.0)):
        a = big.mats["A"]
        v = np.array(a.val, copy=True)
        pick = rng.random(v.size) < share
        if name == "win_escape":                    # 16-bit codes
            v *= (1.0 + 0.125 * rng.integers(0, 9, v.size))
            pick[:] = False
        if name == "win_rawblocks":                 # only the first 30% of the rows: those blocks go raw
            pick[int(a.row_ptr[int(0.3 * a.nrows)]):] = False
        v[pick] = rng.uniform(-1, 1, int(pick.sum()))
        mats[name] = problems.Csr(a.nrows, a.ncols, np.array(a.row_ptr), np.array(a.col), v)
        expect_format[name] = {"win_escape": "wide", "win_rawblocks": "raw", "win_novi": "none"}[name]
    # short-row window kernel (L-lane groups): L = 32 (27-point), 16 (2-D Q2), 8 (9-point), and a
    # ragged banded matrix with empty rows plus far-away columns (blocks that fall back to global x)
    mats["win32"] = problems.generate(dim=3, degree=1, ncomp=1, n_cells=74, radius=0.1).mats["A"]
    mats["win16"] = problems.generate(dim=2, degree=2, ncomp=1, n_cells=365, radius=0.1).mats["A"]
    mats["win8"] = problems.generate(dim=2, degree=1, ncomp=1, n_cells=724, radius=0.1).mats["A"]
    n = 540000
    cnt = rng.integers(0, 21, n)
    rows = np.repeat(np.arange(n), cnt)
    cols = np.clip(rows + rng.integers(-400, 401, rows.size), 0, n - 1)
    far = rng.integers(0, rows.size, 200)
    cols[far] = rng.integers(0, n, 200)
    a = sp.csr_matrix((rng.uniform(-1, 1, rows.size), (rows, cols)), shape=(n, n))
    a.sum_duplicates()
    mats["win_ragged"] = problems.Csr.from_scipy(a)
    ctx = solver.Context(0)
    try:
        for name, m in mats.items():
            # the round-1 value-indexed window forms (8-bit / 16-bit codes, raw blocks) are planned only when the
            # batch-major form does not take the matrix: switched off here so that those kernels stay covered
            ctx.set_tunable("batch_major", 0 if name in expect_format else 1)
            ctx.set_matrix(_abi.A, m)
            info = ctx.matrix_info(_abi.A)
            fmt = expect_format.get(name)
            if fmt == "dict":
                assert info["value_indexed"] and info["value_wide_nnz"] == 0 and info["value_indexed_nnz"] == m.nnz
            elif fmt == "wide":
                assert info["value_indexed"] and info["value_wide_nnz"] > m.nnz // 2
            elif fmt == "raw":
                assert info["value_indexed"] and 0 < info["value_indexed_blocks"] < info["window_blocks"]
            elif fmt == "none":
                assert info["windowed"] and not info["value_indexed"]
            if name.startswith("win") and name != "win_ragged":
                assert info["windowed"], name
            x = rng.uniform(-1, 1, m.ncols)
            y0 = rng.uniform(-1, 1, m.nrows)
            for mode in (0, 1):
                got, lanes = ctx.spmv(_abi.A, x, y0, mode=mode, alpha=1.5)
                ref, olanes = oracle.spmv(m, x, y0 if mode else None, mode=mode, alpha=1.5)
                assert lanes == olanes, name
                assert np.array_equal(got, ref), (name, mode)
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [1, 63, 4096, 4097, 100003, 1 << 20])
def test_dot_bitwise(ctxs, n):
    _, _, ctx, _ = ctxs("stokes3d_sphere")
    x, y = _rng_vec(n, 3), _rng_vec(n, 4)
    got = ctx.dot(x, y)
    assert got == oracle.dot(x, y)
    assert abs(got - float(np.dot(x, y))) <= 1e-12 * max(1.0, np.abs(x * y).sum())


@pytest.mark.parametrize("name", cases.ALL_CASES)
def test_system_and_rhs_bitwise(ctxs, name):
    pb, cfg, ctx, osys = ctxs(name)
    src = cases.rng_blocks(pb, 10)
    got = ctx.system_apply(src)
    rc, ref = osys.system_apply(cfg, src)
    assert rc == 0
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)
    if cfg.variant in (_abi.AL2, _abi.AL_STOKES, _abi.AL_STOKES_DIAG):
        rc, oref = osys.augment_rhs(cfg, cases.rhs_of(pb))
        for g, r in zip(ctx.augment_rhs(cases.rhs_of(pb)), oref):
            assert np.array_equal(g, r)
    elif cfg.variant == _abi.RATIONAL:
        with pytest.raises(solver.AlfdError):
            ctx.augment_rhs(cases.rhs_of(pb))


@pytest.mark.parametrize("name", cases.ALL_CASES)
def test_precond_vmult_parity(ctxs, name):
    """<Preconditioner>::vmult: same inner iteration counts, same vector."""
    pb, cfg, ctx, osys = ctxs(name)
    src = cases.rng_blocks(pb, 20)
    got, res = ctx.precond_apply(src)
    rc, ref, ores = osys.precond_apply(cfg, src)
    assert rc == 0
    assert res.inner_iterations == ores.inner_iterations
    assert res.mp_iterations == ores.mp_iterations
    assert res.rational_iterations == ores.rational_iterations
    assert res.mass_iterations == ores.mass_iterations
    assert res.lambda_max == ores.lambda_max
    for g, r in zip(got, ref):
        assert np.allclose(g, r, rtol=HIST_RTOL, atol=HIST_RTOL * np.abs(r).max())


def test_diagonal_spd_variant(ctxs):
    pb, cfg = cases.case("stokes3d_sphere")
    cfg.variant = _abi.AL_STOKES_DIAG
    ctx = solver.context_from_problem(pb, cfg)
    src = cases.rng_blocks(pb, 21)
    got, res = ctx.precond_apply(src)
    rc, ref, ores = oracle.system_from_problem(pb).precond_apply(cfg, src)
    assert rc == 0 and res.inner_iterations == ores.inner_iterations
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)
    ctx.close()


@pytest.mark.parametrize("name", cases.ALL_CASES)
def test_solve_matches_oracle_and_golden(ctxs, name):
    pb, cfg, ctx, osys = ctxs(name)
    rhs = cases.prepared_rhs(osys, pb, cfg)
    x, res = ctx.solve(rhs)
    hist = ctx.history()
    rc, ox, ores, ohist = osys.solve(cfg, rhs)
    assert rc == 0 and res.status == 0
    # identical iteration counts (outer, inner, pressure-mass)
    assert res.outer_iterations == ores.outer_iterations
    assert res.inner_iterations == ores.inner_iterations
    assert res.mp_iterations == ores.mp_iterations
    assert res.rational_iterations == ores.rational_iterations
    assert res.mass_iterations == ores.mass_iterations
    assert len(hist) == len(ohist)
    assert np.max(np.abs(hist - ohist) / np.abs(ohist)) <= HIST_RTOL
    for g, r in zip(x, ox):
        assert np.allclose(g, r, rtol=1e-9, atol=1e-10 * max(np.abs(r).max(), 1e-30))
    # committed golden fixture (oracle output): same counts, history within tolerance
    gold = json.load(open(os.path.join(GOLDEN, "solves.json")))[name]
    assert res.outer_iterations == gold["outer_iterations"]
    assert res.inner_iterations == gold["inner_iterations"]
    assert res.mp_iterations == gold["mp_iterations"]
    ghist = np.array([float.fromhex(h) for h in gold["history"]])
    assert np.max(np.abs(hist - ghist) / np.abs(ghist)) <= HIST_RTOL
    # the GPU solution really solves the system (independent of the oracle)
    ax = ctx.system_apply(x)
    r = np.concatenate([a - b for a, b in zip(rhs, ax)])
    if cfg.outer_solver == _abi.OUTER_MINRES:      # MinRes stops on the PRECONDITIONED residual norm
        assert np.linalg.norm(r) <= 1e-6 * np.linalg.norm(np.concatenate(rhs))
    else:
        assert np.linalg.norm(r) <= 10 * max(cfg.outer.tol, cfg.outer.reduce * res.initial_residual)


def test_depth1_calls_leave_the_resident_rhs_alone(ctxs):
    """vmult / AA.vmult between alfd_upload_rhs and alfd_solve_resident (adapter depth 1 mixed with depth 2)."""
    pb, cfg, ctx, osys = ctxs("stokes3d_sphere")
    rhs = cases.prepared_rhs(osys, pb, cfg)
    x_ref, res_ref = ctx.solve(rhs)
    ctx.upload_rhs(rhs)
    ctx.precond_apply(cases.rng_blocks(pb, 5))
    ctx.system_apply(cases.rng_blocks(pb, 6))
    ctx.augment_rhs(cases.rhs_of(pb))
    res = ctx.solve_resident()
    assert res.outer_iterations == res_ref.outer_iterations and res.last_residual == res_ref.last_residual
    for a, b in zip(ctx.download_solution(), x_ref):
        assert np.array_equal(a, b)


def test_minres_reference_shaped_classes(ctxs):
    pb, cfg, ctx, osys = ctxs("rational_minres")
    AA, P = solver.SystemOperator(ctx), solver.RationalPreconditioner(ctx)
    mr = solver.SolverMinRes(ctx)
    x = [np.zeros(n) for n in pb.block_sizes]
    mr.solve(AA, x, cases.rhs_of(pb), P)
    gold = json.load(open(os.path.join(GOLDEN, "solves.json")))["rational_minres"]
    assert mr.last_step() == gold["outer_iterations"] == 30      # tables/results.md:32 lists 30 at 1089+33
    with pytest.raises(ValueError):
        solver.SolverMinRes(ctxs("stokes3d_sphere")[2])


def test_reference_shaped_interface(ctxs):
    """solve(A, x, b, P) / vmult(dst, src) / last_step() as at the reference call
    site (stokes_immersed_boundary.cc:1067-1087)."""
    pb, cfg, ctx, osys = ctxs("stokes3d_sphere")
    AA = solver.SystemOperator(ctx)
    P = solver.BlockPreconditionerAugmentedLagrangianStokes(ctx)
    fg = solver.SolverFGMRES(ctx)
    b = ctx.augment_rhs(cases.rhs_of(pb))
    x = [np.zeros(n) for n in pb.block_sizes]
    fg.solve(AA, x, b, P)
    gold = json.load(open(os.path.join(GOLDEN, "solves.json")))["stokes3d_sphere"]
    assert fg.last_step() == gold["outer_iterations"]
    v = [np.zeros(n) for n in pb.block_sizes]
    P.vmult(v, b)
    assert P.last_result.inner_iterations > 0
    with pytest.raises(ValueError):
        solver.BlockPreconditionerAugmentedLagrangian(ctx)       # wrong variant for this context


def test_elliptic_reference_shaped_classes(ctxs):
    pb, cfg, ctx, osys = ctxs("elliptic_modified")
    P = solver.BlockTriangularALPreconditionerModified(ctx)
    v = [np.zeros(n) for n in pb.block_sizes]
    P.vmult(v, cases.rng_blocks(pb, 2))
    assert P.last_result.inner_iterations > 0
    with pytest.raises(ValueError):
        solver.BlockTriangularALPreconditioner(ctx)
    # the reference's parameter assertions (elliptic_interface.cc:874-884) surface as errors
    bad = cases.case("elliptic_modified")[1]
    bad.gamma2 = 10.0
    c2 = solver.Context(0)
    with pytest.raises(solver.AlfdError):
        solver.upload_problem(c2, pb, bad)
    c2.close()


def test_error_behaviour(ctxs):
    """NoConvergence from the inner CG (reference: throws, stokes...:1020-1024) and
    from FGMRES; ACCEPT policy; unknown slot; unconfigured context."""
    pb, cfg = cases.case("stokes3d_sphere")
    cfg.inner = _abi.Control(_abi.CTRL_ABS, 2, 1e-14, 0.0)
    ctx = solver.context_from_problem(pb, cfg)
    with pytest.raises(solver.NoConvergence) as e:
        ctx.precond_apply(cases.rng_blocks(pb, 1))
    assert e.value.status == _abi.E_NO_CONVERGENCE_INNER
    cfg.on_inner_failure = _abi.INNER_ACCEPT
    ctx.configure(cfg)
    ctx.setup(pb.block_sizes)
    _, res = ctx.precond_apply(cases.rng_blocks(pb, 1))
    assert res.inner_failures == 1 and res.inner_iterations == 2
    pb2, cfg2 = cases.case("stokes3d_sphere")
    cfg2.outer = _abi.Control(_abi.CTRL_REDUCTION, 3, 1e-30, 1e-30)
    ctx.configure(cfg2)
    ctx.setup(pb.block_sizes)
    with pytest.raises(solver.NoConvergence) as e:
        ctx.solve(cases.rhs_of(pb))
    assert e.value.status == _abi.E_NO_CONVERGENCE_OUTER
    x, res = ctx.solve(cases.rhs_of(pb), raise_on_failure=False)
    assert res.status == _abi.E_NO_CONVERGENCE_OUTER and res.outer_iterations == 3
    ctx.close()
    fresh = solver.Context(0)
    with pytest.raises(solver.AlfdError):
        fresh.setup([1, 1])
    with pytest.raises(solver.AlfdError):
        fresh.set_matrix(99, pb.mats["A"])
    fresh.close()


def test_reupload_of_ct_rederives_the_transpose(built):
    """The adapter uploads only CT / BT; C / B are derived.  Uploading a DIFFERENT CT (same sizes)
    on the same context must not leave the transpose of the old one behind."""
    pb, cfg = cases.case("stokes2d_circle")
    ctx = solver.Context(0)
    try:
        def upload(scale):
            ct = pb.mats["Ct"]
            ct2 = problems.Csr(ct.nrows, ct.ncols, ct.row_ptr, ct.col, np.asarray(ct.val) * scale)
            ctx.set_matrix(_abi.A, pb.mats["A"])
            ctx.set_matrix(_abi.CT, ct2)                 # no explicit C, no explicit B
            ctx.set_matrix(_abi.BT, pb.mats["Bt"])
            ctx.set_matrix(_abi.MP, pb.mats["Mp"])
            ctx.set_diag(_abi.INVW, pb.inv_w_diag_squared())
            ctx.set_diag(_abi.MP_LUMPED_INV, pb.mp_lumped_inv())
            ctx.configure(cfg)
            ctx.setup(pb.block_sizes)
            return ct2
        src = cases.rng_blocks(pb, 3)
        for scale in (1.0, 0.5):
            ct2 = upload(scale)
            mats = dict(pb.mats, Ct=ct2, C=ct2.transpose())
            pb2 = problems.SyntheticProblem(params=pb.params, mats=mats, vecs=pb.vecs)
            rc, ref = oracle.system_from_problem(pb2).system_apply(cfg, src)
            assert rc == 0
            for g, r in zip(ctx.system_apply(src), ref):
                assert np.array_equal(g, r), scale
        # an explicitly uploaded C is left alone by a later CT upload
        ctx.set_matrix(_abi.C_, pb.mats["C"])
        upload(0.5)
        y = ctx.system_apply(src)
        c_x = pb.mats["C"].to_scipy() @ src[0]
        assert np.allclose(y[2], c_x, rtol=0, atol=1e-12 * np.abs(c_x).max())
    finally:
        ctx.close()


def test_no_device_memory_growth_across_reupload_and_setup(built):
    """Re-uploading every slot and repeating alfd_setup (which rebuilds the multigrid
    hierarchy) must release the previous device arrays."""
    def used_mb():     # through the library's own HIP runtime (torch may have loaded another copy into the process)
        free, total = ctx.device_memory()
        return (total - free) / 1e6

    pb = problems.stokes3d_sphere(16, 1)
    cfg = _abi.default_config(_abi.AL_STOKES)
    cfg.inner.max_steps = 2000
    cfg.inner_prec = _abi.PREC_MULTILEVEL
    cfg.ml_smooth_degree, cfg.ml_smooth_ratio = 2, 8.0
    aggs = problems.geometric_aggregates(pb, a=2)
    ctx = solver.Context(0)
    used = []
    for _ in range(5):
        solver.upload_problem(ctx, pb, cfg, aggs)
        ctx.solve(ctx.augment_rhs(cases.rhs_of(pb)))
        used.append(used_mb())
    ctx.close()
    assert used[-1] - used[1] < 16.0, used          # MB


def test_properties_at_bench_scale(built):
    """BASELINE.json's full size -- the bench workload itself: N = 74 Taylor-Hood, 10.35 M
    DoF, 1.78 G nnz (far beyond what the oracle finishes in seconds), checked through
    properties the domain offers."""
    n = int(os.environ.get("ALFD_TEST_FULL_NCELLS", "74"))
    pb = problems.stokes3d_sphere(n, 4 if n >= 48 else 3)
    # bench.py's exact solver settings (one definition: _abi.bench_multilevel_settings): geometric hierarchy,
    # Chebyshev(3)/40 + degree 5 below, interface patch 15/200, explicit coarsest inverse, inner cap 100
    # (parameters_stokes_3d.prm:23-24), prolongators down to BENCH_MIN_COARSE, 16x4x1 mesh bricks
    cfg = _abi.bench_multilevel_settings(_abi.default_config(_abi.AL_STOKES), geometric=True)
    ctx = solver.context_from_problem(pb, cfg, aggregates=problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE),
                                      row_blocks=problems.brick_row_blocks(pb.params, (16, 4, 1)))
    assert ctx.matrix_info(_abi.A)["batch_major"] == 2
    rng = np.random.default_rng(0)
    xs = [[rng.uniform(-1, 1, n_) for n_ in pb.block_sizes] for _ in range(2)]
    a, b = 0.75, -1.25
    y0, y1 = ctx.system_apply(xs[0]), ctx.system_apply(xs[1])
    ysum = ctx.system_apply([a * u + b * v for u, v in zip(*xs)])
    for s_, u, v in zip(ysum, y0, y1):         # linearity of AA
        assert np.allclose(s_, a * u + b * v, rtol=0, atol=1e-11 * max(np.abs(u).max(), np.abs(v).max()))
    # AA is symmetric: <AA x0, x1> == <x0, AA x1>
    lhs = sum(float(np.dot(u, v)) for u, v in zip(y0, xs[1]))
    rhs_ = sum(float(np.dot(u, v)) for u, v in zip(xs[0], y1))
    assert abs(lhs - rhs_) <= 1e-10 * max(abs(lhs), 1.0)
    # B and B^T are transposes of each other: <B u, p> == <u, B^T p>
    u, p = rng.uniform(-1, 1, pb.block_sizes[0]), rng.uniform(-1, 1, pb.block_sizes[1])
    bu, _ = ctx.spmv(_abi.B, u, np.zeros(pb.block_sizes[1]))
    btp, _ = ctx.spmv(_abi.BT, p, np.zeros(pb.block_sizes[0]))
    assert abs(np.dot(bu, p) - np.dot(u, btp)) <= 1e-11 * np.abs(bu).sum()
    # the LDS-windowed SpMV against SciPy on the full matrix (independent summation order)
    ax, _ = ctx.spmv(_abi.A, u, np.zeros(pb.block_sizes[0]))
    ref = pb.mats["A"].to_scipy() @ u
    assert np.allclose(ax, ref, rtol=0, atol=1e-11 * np.abs(ref).max())
    # solve: the true residual of the returned x meets the stop rule, the solve is
    # repeatable bit for bit, the residual history is monotone, the count is mesh independent
    rhs = ctx.augment_rhs(cases.rhs_of(pb))
    x, res = ctx.solve(rhs)
    h1 = ctx.history()
    axx = ctx.system_apply(x)
    r = np.sqrt(sum(float(np.dot(p_ - q_, p_ - q_)) for p_, q_ in zip(rhs, axx)))
    assert res.status == 0 and r <= 2 * max(cfg.outer.tol, cfg.outer.reduce * res.initial_residual)
    assert 5 <= res.outer_iterations <= 15
    assert res.inner_iterations <= 12 * res.outer_iterations     # the reference's cap is 100 per application (prm:23)
    x2, res2 = ctx.solve(rhs)
    assert np.array_equal(ctx.history(), h1) and all(np.array_equal(p_, q_) for p_, q_ in zip(x, x2))
    assert np.all(np.diff(h1) <= 0)
    ctx.close()


def test_prolongator_validation_and_single_rank_limits(built):
    """alfd_set_prolongator refuses unsorted / out-of-range columns and a row count that does not match the level; the
    round-3 preconditioner on a partitioned context is ALFD_E_UNSUPPORTED (stated limit, not a silent fallback); a
    coarsest operator that is not positive definite fails the setup loudly."""
    pb, cfg = cases.case("stokes3d_gmg_patch")
    levels = cases.aggregates_of(pb, cfg)
    P0 = levels[0][0]
    ctx = solver.Context(0)
    try:
        bad = problems.Csr(P0.nrows, P0.ncols, P0.row_ptr.copy(), P0.col.copy(), P0.val.copy())
        k = int(np.flatnonzero(np.diff(P0.row_ptr) >= 2)[0])
        a = int(P0.row_ptr[k])
        bad.col[a], bad.col[a + 1] = bad.col[a + 1], bad.col[a]              # descending inside a row
        with pytest.raises(solver.AlfdError):
            ctx.set_prolongator(0, bad)
        bad.col[:] = P0.col
        bad.col[a] = P0.ncols                                                  # out of range
        with pytest.raises(solver.AlfdError):
            ctx.set_prolongator(0, bad)
        # wrong fine size: caught at setup
        short = problems.Csr(P0.nrows - 3, P0.ncols, P0.row_ptr[:-3].copy(), P0.col[:int(P0.row_ptr[-4])].copy(),
                             P0.val[:int(P0.row_ptr[-4])].copy())
        with pytest.raises(solver.AlfdError):
            solver.upload_problem(ctx, pb, cfg, [(short, levels[0][1])])
        # an indefinite "prolongated" coarsest operator: P with a zero column -> singular Galerkin matrix
        P1 = levels[1][0]
        sing = problems.Csr(P1.nrows, P1.ncols, P1.row_ptr.copy(), P1.col.copy(), np.where(P1.col == 0, 0.0, P1.val))
        with pytest.raises(solver.AlfdError, match="positive definite"):
            solver.upload_problem(ctx, pb, _abi.Config.from_buffer_copy(cfg), [levels[0], (sing, levels[1][1])])
        # the good hierarchy still sets up and solves on the same context afterwards
        solver.upload_problem(ctx, pb, cfg, levels)
        rhs = ctx.augment_rhs(cases.rhs_of(pb))
        _, res = ctx.solve(rhs)
        assert res.status == 0 and res.outer_iterations == 10
    finally:
        ctx.close()


def test_row_block_hint_validation_and_stale_hint(built):
    """alfd_set_row_blocks refuses a prefix that does not start at 0 / is not monotone before copying anything with it;
    a hint given for a matrix of another size is dropped at the next upload of the slot (runs of the numbering take
    over) instead of failing the upload."""
    big = problems.generate(dim=3, degree=2, ncomp=3, n_cells=14, stokes=False, grad_div=True, gamma_grad_div=10.0,
                            radius=0.1, immersed_refine=0)       # 73 k rows: both sizes take the window / batch-major forms
    small = problems.generate(dim=3, degree=2, ncomp=3, n_cells=13, stokes=False, grad_div=True, gamma_grad_div=10.0,
                              radius=0.1, immersed_refine=0)
    ctx = solver.Context(0)
    try:
        bp, rows = problems.brick_row_blocks(big.params, (8, 4, 2))
        for bad in (np.r_[1, bp[1:]], np.r_[bp[:3], bp[1], bp[4:]], np.r_[bp[:-1], -5]):
            with pytest.raises(solver.AlfdError):
                ctx.set_row_blocks(_abi.A, bad.astype(np.int64), rows)
        ctx.set_row_blocks(_abi.A, bp, rows)
        ctx.set_matrix(_abi.A, big.mats["A"])
        assert ctx.matrix_info(_abi.A)["batch_major"] == 2
        ctx.set_matrix(_abi.A, small.mats["A"])                  # other row count: the hint no longer applies
        assert ctx.matrix_info(_abi.A)["batch_major"] == 1       # runs of the numbering
        x = _rng_vec(small.mats["A"].ncols, 5)
        got, lanes = ctx.spmv(_abi.A, x, np.zeros(small.mats["A"].nrows))
        assert np.array_equal(got, oracle.spmv(small.mats["A"], x, lanes=lanes)[0])
    finally:
        ctx.close()


def test_mid_size_solve_with_the_bench_kernels_matches_oracle(built):
    """Solve-level oracle parity at a size where the kernels of the bench are the ones that run: N = 20 Taylor-Hood
    (0.21 M velocity rows) on 16x4x1 mesh bricks with bench.py's multigrid settings -- the batch-major long-row kernel
    (spmv_vs_kernel) on A and the batch-major short-row kernel (spmv_vss_kernel) on the coupling blocks sit INSIDE a
    solve whose iteration counts and residual history are compared with the oracle's."""
    n = 20
    pb = problems.stokes3d_sphere(n, 2)
    cfg = _abi.bench_multilevel_settings(_abi.default_config(_abi.AL_STOKES), geometric=True)
    levels = problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE)
    ctx = solver.context_from_problem(pb, cfg, aggregates=levels, row_blocks=problems.brick_row_blocks(pb.params, (16, 4, 1)))
    try:
        info = ctx.matrix_info(_abi.A)
        assert info["batch_major"] == 2 and info["lanes"] == 64
        short = [s for s in (_abi.BT, _abi.B, _abi.MP) if ctx.matrix_info(s)["batch_major"] and ctx.matrix_info(s)["lanes"] < 64]
        assert short, "no short-row operator landed on the batch-major form at this size"
        osys = oracle.system_from_problem(pb, aggregates=levels)
        rc, rhs = osys.augment_rhs(cfg, cases.rhs_of(pb))
        assert rc == 0
        x, res = ctx.solve(rhs)
        hist = ctx.history()
        rc, ox, ores, ohist = osys.solve(cfg, rhs)
        assert rc == 0 and res.status == 0
        assert (res.outer_iterations, res.inner_iterations, res.mp_iterations) == \
               (ores.outer_iterations, ores.inner_iterations, ores.mp_iterations)
        assert len(hist) == len(ohist) and np.max(np.abs(hist - ohist) / np.abs(ohist)) <= HIST_RTOL
        for g, r in zip(x, ox):
            assert np.allclose(g, r, rtol=1e-9, atol=1e-10 * max(np.abs(r).max(), 1e-30))
    finally:
        ctx.close()


def _reference_shaped(n, refine, numbering, frontend):
    """Stokes problem with the cell-wise assembled block (0,0) (synth.h `assembly` = 1), optionally renumbered by
    Cuthill-McKee (stokes_immersed_boundary.cc:533-541) and then by the front end (lexicographic order of the support
    points); returns (problem, prolongators in that numbering, row blocks)."""
    pb = problems.stokes3d_sphere(n, refine, assembly="cellwise")
    if numbering == "cuthill_mckee":
        problems.permute_background_nodes(pb, problems.cuthill_mckee_nodes(pb))
    perm = getattr(pb, "node_permutation", None)
    pts = problems.row_support_points(pb.params, node_permutation=perm)
    if frontend == "renumber":
        n2o = solver.numbering_from_points(pts)
        problems.permute_background_nodes(pb, n2o[::3] // 3)
        perm = pb.node_permutation
        pts = problems.row_support_points(pb.params, node_permutation=perm)
    blocks = solver.brick_blocks_from_points(pts, (16, 4, 1)) if frontend != "none" else None
    levels = problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE, node_permutation=perm)
    return pb, levels, blocks


@pytest.mark.parametrize("numbering,frontend", [("lexicographic", "bricks"), ("cuthill_mckee", "none"),
                                                ("cuthill_mckee", "renumber")])
def test_reference_shaped_operator_matches_oracle(built, numbering, frontend):
    """A cell-wise assembled operator (last bits of mathematically equal entries differ with the visiting order of the
    cells: 720 instead of 285 distinct values) in the numbering a deal.II program hands over, as is and after the front
    end's renumbering: SpMV bitwise, solve counts and history against the oracle on the SAME arrays, at a size where
    the window / batch-major kernels run (N = 16: 107 k velocity rows)."""
    pb, levels, blocks = _reference_shaped(16, 2, numbering, frontend)
    cfg = _abi.bench_multilevel_settings(_abi.default_config(_abi.AL_STOKES), geometric=True)
    ctx = solver.context_from_problem(pb, cfg, aggregates=levels, row_blocks=blocks)
    try:
        info = ctx.matrix_info(_abi.A)
        if frontend != "none":       # the fast form, with 10-bit codes because blocks hold > 512 distinct values
            assert info["batch_major"] == 2 and info["batch_major_wide"] == 1
            assert info["shared_nnz"] > 0.8 * info["nnz"]
        x = _rng_vec(pb.block_sizes[0], 7)
        got, lanes = ctx.spmv(_abi.A, x, np.zeros(pb.block_sizes[0]))
        ref, _ = oracle.spmv(pb.mats["A"], x, lanes=lanes)
        assert np.array_equal(got, ref)
        osys = oracle.system_from_problem(pb, aggregates=levels)
        rc, rhs = osys.augment_rhs(cfg, cases.rhs_of(pb))
        assert rc == 0
        xs, res = ctx.solve(rhs)
        hist = ctx.history()
        rc, ox, ores, ohist = osys.solve(cfg, rhs)
        assert rc == 0 and res.status == 0
        assert (res.outer_iterations, res.inner_iterations, res.mp_iterations) == \
               (ores.outer_iterations, ores.inner_iterations, ores.mp_iterations)
        assert len(hist) == len(ohist) and np.max(np.abs(hist - ohist) / np.abs(ohist)) <= HIST_RTOL
    finally:
        ctx.close()


def _full_size_properties(pb, cfg, rhs, aggs, outer_band, symmetric, augment, scipy_rows=None, row_blocks=None):
    """Size-independent checks on a full-size BASELINE config (no oracle at this size): linearity of the
    system operator, its symmetry where it is symmetric, the A-SpMV against SciPy, the true residual of
    the returned solution against the stop rule, bitwise repeatability, the outer-iteration band."""
    ctx = solver.context_from_problem(pb, cfg, aggregates=aggs, row_blocks=row_blocks)
    try:
        if row_blocks is not None:
            assert ctx.matrix_info(_abi.A)["batch_major"] == 2
        rng = np.random.default_rng(1)
        xs = [[rng.uniform(-1, 1, n_) for n_ in pb.block_sizes] for _ in range(2)]
        a, b = 0.75, -1.25
        y0, y1 = ctx.system_apply(xs[0]), ctx.system_apply(xs[1])
        ysum = ctx.system_apply([a * u + b * v for u, v in zip(*xs)])
        for s_, u, v in zip(ysum, y0, y1):
            assert np.allclose(s_, a * u + b * v, rtol=0, atol=1e-11 * max(np.abs(u).max(), np.abs(v).max()))
        if symmetric:
            lhs = sum(float(np.dot(u, v)) for u, v in zip(y0, xs[1]))
            rhs_ = sum(float(np.dot(u, v)) for u, v in zip(xs[0], y1))
            assert abs(lhs - rhs_) <= 1e-10 * max(abs(lhs), 1.0)
        u = xs[0][0]
        ax, _ = ctx.spmv(_abi.A, u, np.zeros(pb.block_sizes[0]))
        if scipy_rows is None:
            ref = pb.mats["A"].to_scipy() @ u
            assert np.allclose(ax, ref, rtol=0, atol=1e-11 * np.abs(ref).max())
        else:       # very large A: compare a row slice only (a SciPy copy of 2.4 G entries would take minutes)
            r0, r1 = scipy_rows
            ref = pb.mats["A"].slice_rows(r0, r1).to_scipy() @ u
            assert np.allclose(ax[r0:r1], ref, rtol=0, atol=1e-11 * np.abs(ref).max())
        if augment:
            rhs = ctx.augment_rhs(rhs)
        x, res = ctx.solve(rhs)
        h1 = ctx.history()
        axx = ctx.system_apply(x)
        r = np.sqrt(sum(float(np.dot(p_ - q_, p_ - q_)) for p_, q_ in zip(rhs, axx)))
        assert res.status == 0
        if cfg.outer.kind == _abi.CTRL_FIXED_ITERS:
            # a fixed number of outer steps: the TRUE residual of the returned x equals the residual FGMRES
            # tracks through its Givens recurrence (consistency of the Arnoldi relation), and it went down
            assert abs(r - h1[-1]) <= 1e-6 * h1[0] and np.all(np.diff(h1) <= 0) and h1[-1] < 0.2 * h1[0]
        else:
            assert r <= 10 * max(cfg.outer.tol, cfg.outer.reduce * res.initial_residual)
        assert outer_band[0] <= res.outer_iterations <= outer_band[1], res.outer_iterations
        x2, res2 = ctx.solve(rhs)
        assert np.array_equal(ctx.history(), h1) and all(np.array_equal(p_, q_) for p_, q_ in zip(x, x2))
        return res
    finally:
        ctx.close()


@pytest.mark.parametrize("prec", ["chebyshev", "geometric"])
def test_properties_cfg2_full_size(built, prec):
    """BASELINE cfg 2 at full size: immersed_laplace 3-D, Q1 on 128^3 cells (2.15 M DoF), cubed sphere with
    6146 multiplier DoFs, Circle_parameters-style controls.  Inner preconditioner: the
    Chebyshev-Jacobi sweep of north_star, and the round-3 geometric hierarchy with the bench's settings (inner CG
    within the reference's cap of 100, immersed_laplace.cc:907)."""
    pb = problems.laplace3d_sphere(128, 5)
    assert pb.block_sizes == [2146689, 6146]
    cfg = _abi.default_config(_abi.AL2)
    cfg.outer = _abi.Control(_abi.CTRL_REDUCTION, 1000, 1e-10, 1e-12)
    levels = None
    if prec == "geometric":
        _abi.bench_multilevel_settings(cfg, geometric=True)
        levels = problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE)
    else:
        cfg.inner.max_steps = 5000
    res = _full_size_properties(pb, cfg, [pb.vecs["f"], pb.vecs["g"]], levels, (4, 12), True, True)
    assert res.inner_iterations > 0
    if prec == "geometric":
        assert res.inner_iterations <= 20 * res.outer_iterations


@pytest.mark.parametrize("hierarchy", ["aggregation", "geometric"])
@pytest.mark.parametrize("beta2", [10.0, 1e3])
def test_properties_cfg3_full_size(built, beta2, hierarchy):
    """BASELINE cfg 3 at full size: elliptic_interface 2-D, modified AL, background Q1 on 1024^2, immersed Q1 on
    256^2 (1.05 M + 2 x 66 k DoF), beta_2 = 10 (parameters_modified.prm:5) and 1e3 (BASELINE.json).  Multigrid on the
    background block: round-2 aggregates, and bilinear CSR prolongators with an explicit coarsest inverse (no interface
    patch: the coupling is a VOLUME integral here, the "patch" would be the whole immersed square)."""
    pb = problems.elliptic_interface2d(1024, 256, beta2=beta2)
    assert pb.block_sizes == [1050625, 66049, 66049]
    cfg = _abi.default_config(_abi.AL_ELL_MODIFIED)
    cfg.gamma, cfg.gamma2 = 10.0, 1e-2
    cfg.inner = _abi.Control(_abi.CTRL_REDUCTION, 100000, 1e-2, 1e-20)
    cfg.outer = _abi.Control(_abi.CTRL_REDUCTION, 1000, 1e-10, 1e-10)
    cfg.inner_prec = _abi.PREC_MULTILEVEL
    if hierarchy == "geometric":
        cfg.ml_smooth_degree, cfg.ml_smooth_degree_coarse, cfg.ml_smooth_ratio, cfg.ml_coarse_direct = 3, 5, 30.0, 1024
        aggs = problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE)
    else:
        cfg.ml_smooth_degree, cfg.ml_smooth_ratio, cfg.ml_coarse_degree = 4, 256.0, 10
        aggs = problems.geometric_aggregates(pb, a=2, min_coarse=600)
    rhs = [pb.vecs["f"], pb.vecs["f2"], np.zeros(pb.block_sizes[2])]
    res = _full_size_properties(pb, cfg, rhs, aggs, (15, 60), False, False)
    if hierarchy == "geometric":
        assert res.solve_seconds < 1.0        # cfg 3 at full size below one second


def test_properties_cfg5_full_size(built):
    """BASELINE cfg 5 at full size on one GPU: elliptic_interface 3-D elasticity (elasticity.prm), vector Q1 on
    215^3 cells (30.2 M background DoF, 2.36 G nonzeros) + the immersed box, modified AL with the prm's controls,
    multigrid inner preconditioner.  The prm's inner stop rule is ABSOLUTE (1e-2 on unit-norm Krylov vectors), so
    the outer count of this synthetic instance grows with refinement (12 / 22 / 47 / 134 outer iterations at
    n = 32 / 64 / 128 / 215, the same with the single-level sweep; 134 take 100 s): the property run performs a
    FIXED number of outer steps (IterationNumberControl) instead of the full solve."""
    n = int(os.environ.get("ALFD_TEST_CFG5_NCELLS", "215"))
    pb = problems.elasticity3d(n)
    if n == 215:
        assert pb.block_sizes[0] == 30233088
    cfg = _abi.default_config(_abi.AL_ELL_MODIFIED)
    cfg.gamma, cfg.gamma2 = 10.0, 1e-2                                   # elasticity.prm:49-50
    cfg.inner = _abi.Control(_abi.CTRL_REDUCTION, 10000, 1e-2, 1e-20)    # prm:60-66
    cfg.outer = _abi.Control(_abi.CTRL_FIXED_ITERS, 12, 1e-10, 1e-6)
    cfg.inner_prec = _abi.PREC_MULTILEVEL
    cfg.ml_smooth_degree, cfg.ml_smooth_ratio, cfg.ml_coarse_degree = 4, 256.0, 10
    aggs = problems.geometric_aggregates(pb, a=2, min_coarse=600)
    rhs = [pb.vecs["f"], pb.vecs["f2"], np.zeros(pb.block_sizes[2])]
    nr = pb.block_sizes[0]
    res = _full_size_properties(pb, cfg, rhs, aggs, (12, 12), False, False, scipy_rows=(nr // 2, nr // 2 + 200000),
                                row_blocks=problems.brick_row_blocks(pb.params, (8, 4, 2)))
    print(f"cfg5 n={n}: outer {res.outer_iterations}, inner {res.inner_iterations}, {res.solve_seconds:.1f} s")


def test_algebraic_aggregates_on_condensed_operator_parity(built):
    """ALFD_PREC_MULTILEVEL without grid metadata: the library builds every level's aggregates from the uploaded
    A alone (alfd_build_aggregates) for an operator with a condensed layer of hanging nodes; the oracle gets the
    same aggregates (alfd_get_aggregates) -- identical counts, history within 1e-10."""
    pb = cases.hanging_node_variant(problems.stokes3d_sphere(8, 0))
    cfg = _abi.default_config(_abi.AL_STOKES)
    cfg.inner.max_steps = 100                       # the reference's cap (parameters_stokes_3d.prm:23)
    cfg.inner_prec = _abi.PREC_MULTILEVEL
    cfg.ml_smooth_degree, cfg.ml_smooth_ratio, cfg.ml_coarse_degree = 4, 256.0, 10
    ctx = solver.Context(0)
    try:
        ctx.set_matrix(_abi.A, pb.mats["A"])
        aggs = ctx.build_aggregates(block_size=3, threshold=0.02, max_aggregate_nodes=8, min_coarse=300)
        assert len(aggs) >= 2 and aggs[0][1] < pb.mats["A"].nrows // 8
        assert int((aggs[0][0] < 0).sum()) == int((np.diff(pb.mats["A"].row_ptr) == 1).sum())
        solver.upload_problem(ctx, pb, cfg, None)       # keeps the aggregates built above
        rhs = ctx.augment_rhs(cases.rhs_of(pb))
        x, res = ctx.solve(rhs)
        hist = ctx.history()
        osys = oracle.system_from_problem(pb, aggregates=aggs)
        rc, orhs = osys.augment_rhs(cfg, cases.rhs_of(pb))
        rc, ox, ores, ohist = osys.solve(cfg, orhs)
        assert rc == 0 and res.status == 0
        assert (res.outer_iterations, res.inner_iterations, res.mp_iterations) == \
            (ores.outer_iterations, ores.inner_iterations, ores.mp_iterations)
        assert np.max(np.abs(hist - ohist) / np.abs(ohist)) <= HIST_RTOL
        assert res.outer_iterations <= 14
    finally:
        ctx.close()
