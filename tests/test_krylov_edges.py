"""The oracle's outer Krylov loops away from the zero start: warm starts, a full 63-vector basis, restart 1 and 2,
an outer failure in the middle of a cycle, zero iterations.  Every reference here involves neither the library nor
the oracle: the block system K is assembled with SciPy from the problem's matrices (krylov_cases.assemble), residuals
and K @ x are taken in np.longdouble, the Laplace solution comes from SuperLU, and the warm-started Krylov sequence is
pinned by the shift identity  solve(b, x0) == x0 + solve(b - K x0, 0),  whose right side is the zero-start solve the
rest of the suite already pins.  tests/test_gpu_krylov_edges.py then holds the library to the oracle on the same
configurations (tests/krylov_cases.py).

Measured tables, from what the tests print (python -m pytest tests/test_krylov_edges.py -s):

Shift identity, outer control SolverControl(1e-8) so that both runs stop by the same rule; relative difference of the
two solutions in the 2-norm:

    case               outer    inner      |x - (x0 + d)| / |x0 + d|
    laplace2d_circle   17/17    308/308    1.0e-13
    laplace2d_jacobi   16/16    499/499    3.8e-14
    laplace3d_sphere   7/7      78/78      1.8e-13
    stokes3d_sphere    13/13    286/286    4.2e-14
    long_basis:cgs2    185/185  555/555    2.0e-11
    stokes3d_fgmres95  20/20    484/484    7.8e-11

SHIFT_TOL is the largest entry times 64 (the margin of precond_reference.py).  The residual histories of the two runs
are not compared entry by entry: their tails differ by up to 2.4e-4 relative (long_basis, entries 1e-10 of |r0|).
test_shift_tolerance_is_what_the_identity_measures repeats the measurement and fails when it leaves the table.

Reported against true residual, |last_residual - |b - K x|| / |b - K x| with the true one in longdouble (asserted to
rtol 1e-3, the bound of test_oracle.py::test_stokes_solution_satisfies_the_system):

    converged from the random start (items 2 and 7)               failed: x is the partial-cycle iterate (item 6)
    laplace2d_circle    3.0e-05    stokes3d_restart   4.6e-09     stagnating:1           4.4e-15
    laplace2d_jacobi    4.0e-05    elliptic_modified  2.5e-06     stagnating:2           2.2e-15
    laplace3d_sphere    3.3e-06    long_basis:mgs     5.4e-08     stagnating:2:dealii95  5.9e-15
    stokes3d_sphere     2.9e-07    long_basis:cgs     7.9e-09     mid_cycle_failure      2.5e-11
    stokes3d_fgmres95   3.9e-09    long_basis:cgs2    8.9e-08
    stokes3d_gmg_patch  1.6e-06

After a failure the last column still has to reach x.  Where the iteration has stagnated to rounding (restart 1, and
restart 2 in the 9.5 loop: the last column changes the residual by 1e-15) no residual can tell; stagnating:2 (1.9e-5)
and mid_cycle_failure (7.7e-6, against a disagreement of 1.5e-15) can, and do.

Initial residual hist[0] against |b - K x0| in longdouble: relative difference 0.0 on every FGMRES case but
laplace3d_sphere (1.3e-16); the asserted bound is derived from the data in test_initial_residual_is_b_minus_K_x0.
"""
import functools
import math

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import krylov_cases as kc
from fictitious_domain_al_preconditioners_amd import _abi
from oracle import oracle

CHUNK = 4096                   # dot chunk = padding granule of a block vector
U = 2.0 ** -53                 # unit roundoff of float64

FGMRES_X0 = [k for k in kc.X0_CASES if kc.config(k)[1].outer_solver == _abi.OUTER_FGMRES]
MINRES_X0 = [k for k in kc.X0_CASES if k not in FGMRES_X0]

SHIFT_CASES = ["laplace2d_circle", "laplace2d_jacobi", "laplace3d_sphere", "stokes3d_sphere", "long_basis:cgs2",
               "stokes3d_fgmres95"]
# key -> (outer, inner, relative solution difference): the table of the module docstring
SHIFT_MEASURED = {
    "laplace2d_circle": (17, 308, 1.0e-13),
    "laplace2d_jacobi": (16, 499, 3.8e-14),
    "laplace3d_sphere": (7, 78, 1.8e-13),
    "stokes3d_sphere": (13, 286, 4.2e-14),
    "long_basis:cgs2": (185, 555, 2.0e-11),
    "stokes3d_fgmres95": (20, 484, 7.8e-11),
}
SHIFT_MARGIN = 64.0
SHIFT_TOL = SHIFT_MARGIN * max(v[2] for v in SHIFT_MEASURED.values())
assert SHIFT_TOL <= 1e-8, "a tolerance above 1e-8 means a case of the shift identity is ill-posed"


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than float64 on this machine"
    return built


@functools.lru_cache(maxsize=None)
def _K(key):
    s = kc.system(key)
    return kc.assemble(s.pb, s.cfg)


def _true_residual(key, b, x):
    return kc.norm_ld(kc.residual_ld(_K(key), b, x))


def _stop_bound(cfg, initial):
    return max(cfg.outer.tol, cfg.outer.reduce * initial)


def _assert_stopped_by_the_rule(cfg, hist):
    """ReductionControl relative to hist[0], restated: the last value meets |r| <= tol or |r| < reduce * |r0|, and no
    earlier one did -- so the solve neither stopped early nor ran on, whichever of the two bounds was the active one."""
    met = (hist <= cfg.outer.tol) | (hist < cfg.outer.reduce * hist[0])
    assert met[-1] and not met[:-1].any(), np.nonzero(met)[0]


def _cycle_steps(cfg):
    """History entries one cycle adds: m for the 9.6 loop, m - 1 for the 9.5 one (its check lags one vector)."""
    return cfg.restart - 1 if cfg.fgmres_flavour == _abi.FGMRES_DEALII_95 else cfg.restart


def _padded(blocks):
    out = []
    for b in blocks:
        out.append(b)
        out.append(np.zeros(-b.size % CHUNK))
    return np.concatenate(out)


# ------------------------------------------------------------------ 1. the initial residual
@pytest.mark.parametrize("key", FGMRES_X0)
def test_initial_residual_is_b_minus_K_x0(key):
    """hist[0] = |b - K x0|_2.  With L the longest row of K, float64 evaluation of a row of b - K x0 errs by at most
    (L + 2) u (|K||x0| + |b|) (L products, L - 1 additions, the subtraction; u = 2^-53), and the n-term dot behind
    the norm by n u |r0| relatively to first order: the bound is the 2-norm of the first plus the second."""
    r = kc.oracle_run(key)
    K = _K(key)
    x0, b = np.concatenate(r.x0), np.concatenate(r.rhs)
    true0 = kc.norm_ld(kc.residual_ld(K, b, x0))
    L = int(np.diff(K.indptr).max())
    elementwise = (L + 2) * U * (kc.matvec_ld(abs(K), np.abs(x0)) + np.abs(b).astype(np.longdouble))
    bound = kc.norm_ld(elementwise) + x0.size * U * true0
    print(f"{key}: hist[0] = {r.hist[0]:.17g}, |b - K x0| = {true0:.17g}, relative difference "
          f"{abs(r.hist[0] - true0) / true0:.1e}, bound {bound / true0:.1e}")
    assert bound <= 1e-9 * true0                # the bound itself is tight enough to mean something
    assert abs(r.hist[0] - true0) <= bound
    assert not np.isclose(r.hist[0], np.linalg.norm(b), rtol=1e-3)      # and it is not the zero-start value


@pytest.mark.parametrize("key", MINRES_X0)
def test_minres_initial_value_is_the_preconditioned_norm_of_r0(key):
    """MinRes reports sqrt(<P r0, r0>), not |r0|: finite, positive, and the oracle's own precond_apply on
    r0 = b - AA x0 through its canonical dot gives the same number."""
    r = kc.oracle_run(key)
    rc, kx = r.osys.system_apply(r.cfg, r.x0)
    assert rc == 0
    r0 = [b - a for b, a in zip(r.rhs, kx)]
    rc, v, _ = r.osys.precond_apply(r.cfg, r0)
    assert rc == 0
    value = math.sqrt(oracle.dot(_padded(v), _padded(r0)))
    print(f"{key}: hist[0] = {r.hist[0]:.17g}, sqrt(<P r0, r0>) = {value:.17g}, |r0| = "
          f"{np.linalg.norm(np.concatenate(r0)):.6g}")
    assert np.isfinite(r.hist[0]) and r.hist[0] > 0
    assert r.hist[0] == value
    assert r.res.initial_residual == r.hist[0]


# ------------------------------------------------------------------ 2. the stop rule is relative to that r0
@pytest.mark.parametrize("key", FGMRES_X0)
def test_stop_rule_is_relative_to_the_warm_start_residual(key):
    r = kc.oracle_run(key)
    assert r.rc == 0 and r.res.status == 0
    assert r.res.initial_residual == r.hist[0]
    assert len(r.hist) == r.res.outer_iterations + 1
    true = _true_residual(key, r.rhs, r.x)
    print(f"{key}: reported {r.res.last_residual:.6e}, true {true:.6e}, agreement "
          f"{abs(true - r.res.last_residual) / true:.1e}")
    assert true <= 2 * _stop_bound(r.cfg, r.hist[0])
    assert np.isclose(true, r.res.last_residual, rtol=1e-3)
    _assert_stopped_by_the_rule(r.cfg, r.hist)
    # GMRES residuals are monotone within one cycle
    d = np.diff(r.hist)
    inside = np.arange(d.size) % _cycle_steps(r.cfg) != 0
    inside[0] = True
    assert np.all(d[inside] <= 1e-12 * r.hist[0])


@pytest.mark.parametrize("key", MINRES_X0)
def test_minres_warm_start_reaches_the_system(key):
    """MinRes stops on the preconditioned norm, so the true residual is only held to the 1e-6 of
    test_oracle.py::test_minres_with_diagonal_spd_al_preconditioner, here relative to |b - K x0|."""
    r = kc.oracle_run(key)
    assert r.rc == 0 and r.res.initial_residual == r.hist[0]
    assert r.res.last_residual == r.hist[-1]
    _assert_stopped_by_the_rule(r.cfg, r.hist)
    assert _true_residual(key, r.rhs, r.x) <= 1e-6 * _true_residual(key, r.rhs, r.x0)
    assert np.all(np.diff(r.hist) <= 0)             # MinRes residual estimates are monotone


# ------------------------------------------------------------------ 3. the shift identity
@functools.lru_cache(maxsize=None)
def _shift(key):
    """(outer, inner) of both runs and |x - (x0 + d)| / |x0 + d| for x = solve(b, x0), d = solve(b - K x0, 0)."""
    s = kc.system(key)
    cfg = kc.copy_config(s.cfg, outer=_abi.Control(_abi.CTRL_ABS, s.cfg.outer.max_steps, 1e-8, 0.0))
    rc, x, res, _ = s.osys.solve(cfg, s.rhs, x0=s.x0)
    assert rc == 0
    shifted = np.asarray(kc.residual_ld(_K(key), s.rhs, s.x0), np.float64)      # longdouble, rounded once
    rc, d, dres, _ = s.osys.solve(cfg, np.split(shifted, np.cumsum(s.pb.block_sizes)[:-1]))
    assert rc == 0
    ref = np.concatenate(s.x0) + np.concatenate(d)
    rel = float(np.linalg.norm(np.concatenate(x) - ref) / np.linalg.norm(ref))
    return (res.outer_iterations, res.inner_iterations), (dres.outer_iterations, dres.inner_iterations), rel


@pytest.mark.parametrize("key", SHIFT_CASES)
def test_warm_start_equals_zero_start_on_the_shifted_system(key):
    warm, zero, rel = _shift(key)
    print(f"shift identity {key}: outer {warm[0]}/{zero[0]}, inner {warm[1]}/{zero[1]}, difference {rel:.1e}")
    assert warm == zero
    assert rel <= SHIFT_TOL


def test_shift_tolerance_is_what_the_identity_measures():
    assert sorted(SHIFT_MEASURED) == sorted(SHIFT_CASES)
    for key in SHIFT_CASES:
        warm, zero, rel = _shift(key)
        print(f"shift identity {key}: outer {warm[0]}/{zero[0]}, inner {warm[1]}/{zero[1]}, difference {rel:.1e}")
        assert warm == zero == SHIFT_MEASURED[key][:2], (key, warm, zero)
        assert rel <= 1.05 * SHIFT_MEASURED[key][2], (key, rel)          # the table is printed to two digits
    assert SHIFT_TOL == SHIFT_MARGIN * max(v[2] for v in SHIFT_MEASURED.values())


# ------------------------------------------------------------------ 4. SuperLU
def test_laplace_warm_start_lands_on_the_sparse_direct_solution():
    """Laplace only: the Stokes solutions differ by 2e-3 between starts at this tolerance (pressure mode)."""
    r = kc.oracle_run("laplace2d_circle")
    assert r.rc == 0
    xs = spla.spsolve(_K("laplace2d_circle").tocsc(), np.concatenate(r.rhs))
    n0 = r.pb.block_sizes[0]
    assert np.linalg.norm(r.x[0] - xs[:n0]) <= 1e-8 * np.linalg.norm(xs)
    cu = r.pb.mats["C"].to_scipy() @ r.x[0]
    assert np.linalg.norm(cu - r.pb.vecs["g"]) <= 1e-8 * np.linalg.norm(r.pb.vecs["g"])


# ------------------------------------------------------------------ 5. zero iterations
@pytest.mark.parametrize("key", kc.X0_CASES)
def test_start_at_the_solution_takes_no_iteration(key):
    r = kc.oracle_run(key)
    cfg = kc.copy_config(r.cfg, outer=kc.control_met_at_the_solution(r.cfg, r.res, r.hist))
    rc, x, res, hist = r.osys.solve(cfg, r.rhs, x0=r.x)
    assert rc == 0 and res.status == 0
    assert res.outer_iterations == 0 and len(hist) == 1
    assert np.isfinite(hist[0]) and res.last_residual == hist[0] == res.initial_residual
    for a, b in zip(x, r.x):
        assert np.array_equal(a, b)
    if r.cfg.outer_solver == _abi.OUTER_MINRES:     # one preconditioner application before the first check
        assert res.inner_iterations > 0 and res.precond_applications == 1
    else:
        assert res.inner_iterations == 0 and res.mp_iterations == 0 and res.precond_applications == 0


@pytest.mark.parametrize("key", kc.X0_CASES)
def test_zero_right_hand_side(key):
    r = kc.oracle_run(key)
    zero = [np.zeros(n) for n in r.pb.block_sizes]
    rc, x, res, hist = r.osys.solve(r.cfg, zero)
    assert rc == 0 and res.status == 0 and res.outer_iterations == 0
    assert np.array_equal(hist, [0.0]) and res.last_residual == 0.0 and res.initial_residual == 0.0
    for a in x:
        assert np.array_equal(a, np.zeros_like(a))
    # from a random start the homogeneous system is solved like any other
    rc, x, res, hist = r.osys.solve(r.cfg, zero, x0=r.x0)
    assert rc == 0 and res.outer_iterations > 0 and np.all(np.isfinite(np.concatenate(x)))
    kx = kc.norm_ld(kc.matvec_ld(_K(key), np.concatenate(x)))
    if r.cfg.outer_solver == _abi.OUTER_MINRES:
        assert kx <= 1e-6 * kc.norm_ld(kc.matvec_ld(_K(key), np.concatenate(r.x0)))
    else:
        assert kx <= 2 * _stop_bound(r.cfg, hist[0])


# ------------------------------------------------------------------ 6. failure
@pytest.mark.parametrize("key", kc.FAILING)
def test_outer_failure_returns_the_partial_cycle_iterate(key):
    r = kc.oracle_run(key)
    assert r.rc == _abi.E_NO_CONVERGENCE_OUTER
    assert r.res.outer_iterations == r.cfg.outer.max_steps and len(r.hist) == r.cfg.outer.max_steps + 1
    if key == "mid_cycle_failure":                  # column 37 of the second cycle
        assert r.cfg.outer.max_steps % _cycle_steps(r.cfg) == 37
    true = _true_residual(key, r.rhs, r.x)
    print(f"{key}: reported {r.res.last_residual:.6e}, true {true:.6e}, agreement "
          f"{abs(true - r.res.last_residual) / true:.1e}, start {r.hist[0]:.6e}")
    assert np.isclose(true, r.res.last_residual, rtol=1e-3)
    assert true < r.hist[0] and r.res.last_residual > _stop_bound(r.cfg, r.hist[0])


# ------------------------------------------------------------------ 7. a full basis
def test_long_basis_fills_the_basis_and_the_orthogonalisations_agree():
    runs = {key: kc.oracle_run(key) for key in kc.LONG_BASIS}
    for key, r in runs.items():
        assert r.res.outer_iterations > 2 * kc.LONG_RESTART, key       # first: the case still fills the basis
        assert r.cfg.restart == kc.LONG_RESTART == 63
    ref = np.concatenate(runs["long_basis:cgs2"].x)
    for key, r in runs.items():
        assert r.rc == 0
        assert r.res.outer_iterations == runs["long_basis:cgs2"].res.outer_iterations
        assert r.res.inner_iterations == 3 * r.res.outer_iterations
        rel = np.linalg.norm(np.concatenate(r.x) - ref) / np.linalg.norm(ref)
        true = _true_residual(key, r.rhs, r.x)
        print(f"{key}: outer {r.res.outer_iterations}, solution against cgs2 {rel:.1e}, reported "
              f"{r.res.last_residual:.6e}, true {true:.6e}, agreement {abs(true - r.res.last_residual) / true:.1e}")
        assert rel <= SHIFT_TOL
        assert np.isclose(true, r.res.last_residual, rtol=1e-3)
        assert true <= 2 * _stop_bound(r.cfg, r.hist[0])
