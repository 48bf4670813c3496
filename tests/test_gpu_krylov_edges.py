"""The library's outer Krylov loops away from the zero start, against the oracle on the configurations of
tests/krylov_cases.py (tests/test_krylov_edges.py pins the oracle on the same ones to SciPy): warm starts through
alfd_solve and the resident calls, repeated resident solves, the caller's arrays, zero iterations, a full 63-vector
basis in the batched Arnoldi kernels, restart 1 and 2, an outer failure in the middle of a cycle, the limits of
`restart`, and a warm start on two ranks.

The yardstick is the one of test_gpu_parity.py::test_solve_matches_oracle_and_golden: equal status and counts, the
history within HIST_RTOL, the solution within rtol 1e-9.  Every comparison also prints whether history and solution
were bit-identical (DESIGN.md section 4 makes whole single-rank solves so), and asserts it.

The tests are ordered from the simplest path on: warm start, resident path, caller's arrays, zero iterations, full
basis, failures, limits, two ranks."""
import numpy as np
import pytest

import cases
import krylov_cases as kc
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver
from oracle import oracle

pytestmark = pytest.mark.gpu
HIST_RTOL = 1e-10          # tolerance north_star states for residuals
AL_RHS = (_abi.AL2, _abi.AL_STOKES, _abi.AL_STOKES_DIAG)


@pytest.fixture(scope="module")
def ctxs(built):
    """key -> context set up for kc.config(key), made on first use."""
    cache = {}

    def get(key):
        if key not in cache:
            pb, cfg = kc.config(key)
            cache[key] = solver.context_from_problem(pb, cfg, aggregates=cases.aggregates_of(pb, cfg))
        return cache[key]
    yield get
    for c in cache.values():
        c.close()


def _copies(blocks):
    return [b.copy() for b in blocks]


def _bits_equal(xs, ys):
    return all(np.array_equal(a, b) for a, b in zip(xs, ys))


def _check_against_oracle(what, x, res, hist, orc, ox, ores, ohist):
    """The yardstick; returns whether history and solution also have the oracle's bits."""
    assert res.status == orc
    assert res.outer_iterations == ores.outer_iterations
    assert res.inner_iterations == ores.inner_iterations
    assert res.mp_iterations == ores.mp_iterations
    assert res.rational_iterations == ores.rational_iterations
    assert res.mass_iterations == ores.mass_iterations
    assert len(hist) == len(ohist)
    dev = float(np.max(np.abs(hist - ohist) / np.abs(ohist)))
    bitwise = bool(np.array_equal(hist, ohist)) and _bits_equal(x, ox)
    print(f"{what}: status {res.status}, outer {res.outer_iterations}, inner {res.inner_iterations}, history deviation "
          f"{dev:.1e}, {'bit-identical to' if bitwise else 'NOT bit-identical to'} the oracle")
    assert dev <= HIST_RTOL
    assert res.initial_residual == hist[0] and res.last_residual == hist[-1]
    for g, r in zip(x, ox):
        assert np.allclose(g, r, rtol=1e-9, atol=1e-10 * max(np.abs(r).max(), 1e-30))
    return bitwise


_warm = {}


def _warm_solve(ctxs, key):
    """ctx.solve(rhs, x0) of a key, once per module: (x, result, history)."""
    if key not in _warm:
        r = kc.oracle_run(key)
        x, res = ctxs(key).solve(r.rhs, x0=r.x0, raise_on_failure=False)
        _warm[key] = (x, res, ctxs(key).history())
    return _warm[key]


# ------------------------------------------------------------------ a. warm start
@pytest.mark.parametrize("key", kc.X0_CASES)
def test_warm_start_matches_oracle(ctxs, key):
    r = kc.oracle_run(key)
    assert r.rc == 0
    x, res, hist = _warm_solve(ctxs, key)
    assert _check_against_oracle(key, x, res, hist, r.rc, r.x, r.res, r.hist)


# ------------------------------------------------------------------ b. resident path
@pytest.mark.parametrize("key", kc.X0_CASES)
def test_resident_solves_restart_from_the_uploaded_guess(ctxs, key):
    """alfd_upload_rhs(rhs, x0), depth-1 calls in between, alfd_solve_resident twice: both start from x0."""
    r = kc.oracle_run(key)
    ctx = ctxs(key)
    x_ref, res_ref, hist_ref = _warm_solve(ctxs, key)
    ctx.upload_rhs(r.rhs, r.x0)
    ctx.precond_apply(cases.rng_blocks(r.pb, 5))
    ctx.system_apply(cases.rng_blocks(r.pb, 6))
    if r.cfg.variant in AL_RHS:
        ctx.augment_rhs(cases.rhs_of(r.pb))
    first = ctx.solve_resident()
    hist_first = ctx.history()
    second = ctx.solve_resident()
    for res in (first, second):
        assert res.status == 0
        assert (res.outer_iterations, res.inner_iterations, res.mp_iterations) == \
            (res_ref.outer_iterations, res_ref.inner_iterations, res_ref.mp_iterations)
        assert res.initial_residual == res_ref.initial_residual and res.last_residual == res_ref.last_residual
    assert np.array_equal(hist_first, hist_ref) and np.array_equal(ctx.history(), hist_ref)
    assert _bits_equal(ctx.download_solution(), x_ref)
    # an upload without a guess after one with a guess starts from zero again
    x_zero, res_zero = ctx.solve(r.rhs)
    ctx.upload_rhs(r.rhs, r.x0)
    ctx.upload_rhs(r.rhs)
    res = ctx.solve_resident()
    assert res.initial_residual == res_zero.initial_residual != res_ref.initial_residual
    assert res.outer_iterations == res_zero.outer_iterations and res.last_residual == res_zero.last_residual
    assert _bits_equal(ctx.download_solution(), x_zero)


# ------------------------------------------------------------------ c. the caller's arrays
def test_solve_leaves_the_callers_arrays_alone(ctxs):
    key = "stokes3d_sphere"
    r = kc.oracle_run(key)
    ctx = ctxs(key)
    x_ref, res_ref, _ = _warm_solve(ctxs, key)
    x0, rhs = _copies(r.x0), _copies(r.rhs)
    x, res = ctx.solve(rhs, x0=x0)
    assert _bits_equal(x0, r.x0) and _bits_equal(rhs, r.rhs)
    assert _bits_equal(x, x_ref) and all(a is not b for a, b in zip(x, x0))
    # the reference-shaped call site: x goes in as the guess and comes out as the solution
    fg = solver.SolverFGMRES(ctx)
    xio = _copies(r.x0)
    fg.solve(solver.SystemOperator(ctx), xio, rhs, solver.BlockPreconditionerAugmentedLagrangianStokes(ctx))
    assert fg.last_step() == res_ref.outer_iterations
    assert _bits_equal(xio, x_ref) and _bits_equal(rhs, r.rhs)


def test_minres_class_takes_the_guess_from_x(ctxs):
    key = "rational_minres"
    r = kc.oracle_run(key)
    x_ref, res_ref, _ = _warm_solve(ctxs, key)
    ctx = ctxs(key)
    mr = solver.SolverMinRes(ctx)
    xio = _copies(r.x0)
    mr.solve(solver.SystemOperator(ctx), xio, r.rhs, solver.RationalPreconditioner(ctx))
    assert mr.last_step() == res_ref.outer_iterations and _bits_equal(xio, x_ref)


# ------------------------------------------------------------------ d. zero iterations
@pytest.mark.parametrize("key", kc.X0_CASES)
def test_zero_iterations(ctxs, key):
    r = kc.oracle_run(key)
    ctx = ctxs(key)
    x_sol, res_sol, hist_sol = _warm_solve(ctxs, key)
    control = kc.control_met_at_the_solution(r.cfg, res_sol, hist_sol)
    original = _abi.Control(r.cfg.outer.kind, r.cfg.outer.max_steps, r.cfg.outer.tol, r.cfg.outer.reduce)
    ctx.set_controls(outer=control)
    try:
        x, res = ctx.solve(r.rhs, x0=x_sol)
        hist = ctx.history()
    finally:
        ctx.set_controls(outer=original)
    assert res.status == 0 and res.outer_iterations == 0 and len(hist) == 1
    assert _bits_equal(x, x_sol)
    assert np.isfinite(hist[0]) and np.isfinite(res.last_residual) and res.last_residual == hist[0]
    orc, ox, ores, ohist = r.osys.solve(kc.copy_config(r.cfg, outer=control), r.rhs, x0=x_sol)
    assert orc == 0 and ores.outer_iterations == 0
    assert (res.inner_iterations, res.mp_iterations, res.rational_iterations, res.mass_iterations) == \
        (ores.inner_iterations, ores.mp_iterations, ores.rational_iterations, ores.mass_iterations)
    assert abs(hist[0] - ohist[0]) <= HIST_RTOL * ohist[0]
    if r.cfg.outer_solver == _abi.OUTER_MINRES:     # one preconditioner application before the first check
        assert res.inner_iterations > 0
    else:
        assert res.inner_iterations == 0
    # b = 0 from the zero start
    zero = [np.zeros(n) for n in r.pb.block_sizes]
    x, res = ctx.solve(zero)
    hist = ctx.history()
    assert res.status == 0 and res.outer_iterations == 0
    assert np.array_equal(hist, [0.0]) and res.last_residual == 0.0 and res.initial_residual == 0.0
    for a in x:
        assert np.array_equal(a, np.zeros_like(a))


# ------------------------------------------------------------------ e. full basis
@pytest.mark.parametrize("key", kc.LONG_BASIS)
def test_full_basis_matches_oracle(ctxs, key):
    """63 vectors in multi_dot_partial_kernel / multi_axpy_neg_kernel / multi_axpy_kernel, a wrap after a full basis."""
    r = kc.oracle_run(key)
    assert r.res.outer_iterations > 2 * kc.LONG_RESTART          # first: the case still fills the basis
    assert r.rc == 0 and r.cfg.restart == 63
    x, res, hist = _warm_solve(ctxs, key)
    assert res.outer_iterations > 2 * kc.LONG_RESTART
    assert _check_against_oracle(key, x, res, hist, r.rc, r.x, r.res, r.hist)


# ------------------------------------------------------------------ f. failure
@pytest.mark.parametrize("key", kc.FAILING)
def test_outer_failure_matches_oracle(ctxs, key):
    r = kc.oracle_run(key)
    assert r.rc == _abi.E_NO_CONVERGENCE_OUTER
    ctx = ctxs(key)
    x, res, hist = _warm_solve(ctxs, key)
    assert res.status == _abi.E_NO_CONVERGENCE_OUTER and res.outer_iterations == r.cfg.outer.max_steps
    assert _check_against_oracle(key, x, res, hist, r.rc, r.x, r.res, r.hist)
    with pytest.raises(solver.NoConvergence) as e:
        ctx.solve(r.rhs, x0=r.x0)
    assert e.value.status == _abi.E_NO_CONVERGENCE_OUTER
    if key == "mid_cycle_failure":
        # the same context solves the system once the step limit is back: long_basis(CGS2)
        good = kc.oracle_run("long_basis:cgs2")
        ctx.set_controls(outer=_abi.Control(good.cfg.outer.kind, good.cfg.outer.max_steps, good.cfg.outer.tol,
                                            good.cfg.outer.reduce))
        try:
            x, res = ctx.solve(good.rhs, x0=good.x0)
            hist = ctx.history()
        finally:
            ctx.set_controls(outer=_abi.Control(r.cfg.outer.kind, r.cfg.outer.max_steps, r.cfg.outer.tol,
                                                r.cfg.outer.reduce))
        assert _check_against_oracle("after the failure", x, res, hist, good.rc, good.x, good.res, good.hist)


# ------------------------------------------------------------------ g. limits
def test_restart_limits(built):
    pb, cfg = kc.long_basis(_abi.ORTH_CGS2)
    ctx = solver.Context(0)
    try:
        for bad in (64, 0):
            with pytest.raises(solver.AlfdError) as e:
                solver.upload_problem(ctx, pb, kc.copy_config(cfg, restart=bad))
            assert e.value.status == _abi.E_INVALID
        solver.upload_problem(ctx, pb, kc.copy_config(cfg, restart=63))
    finally:
        ctx.close()


# ------------------------------------------------------------------ h. two ranks in one process
def test_warm_start_on_two_ranks_matches_oracle_emulation(built):
    from test_gpu_multirank import _run_ranks
    world, n, ref = 2, 8, 0
    cfg = cases.case("stokes3d_sphere")[1]
    full = problems.stokes3d_sphere(n, ref)
    x0 = kc.x0_of(full)
    plan, out = _run_ranks(world, n, ref, cfg, x0=x0)
    osys = oracle.system_from_problem(full, nranks_emulated=world, part_offsets=plan.offsets)
    rc, orhs = osys.augment_rhs(cfg, cases.rhs_of(full))
    rc, ox, ores, ohist = osys.solve(cfg, orhs, x0=x0)
    assert rc == 0
    for r in range(world):
        res = out[r]["res"]
        assert res["status"] == 0
        assert res["outer_iterations"] == ores.outer_iterations
        assert res["inner_iterations"] == ores.inner_iterations
        assert res["mp_iterations"] == ores.mp_iterations
        assert np.array_equal(out[r]["hist"], out[0]["hist"])          # every rank sees the same scalars
        assert len(out[r]["hist"]) == len(ohist)
        assert np.max(np.abs(out[r]["hist"] - ohist) / np.abs(ohist)) <= HIST_RTOL
    for b in range(3):
        xs = np.concatenate([out[r]["x"][b] for r in range(world)])
        assert np.allclose(xs, ox[b], rtol=1e-9, atol=1e-10 * max(np.abs(ox[b]).max(), 1e-30))
    # the start really was x0: the first residual is the warm one, not |b|
    assert not np.isclose(ohist[0], np.linalg.norm(np.concatenate(orhs)), rtol=1e-3)
