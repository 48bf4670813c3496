"""Host-only parts of the drivers' sanity checks (no GPU): the extreme eigenvalues of the CG-Lanczos tridiagonal
matrix (alfd_host_tridiagonal_extremes) against SciPy, its argument checks, and the NULL-context answers of
alfd_estimate_spectrum / alfd_constraint_residual."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla

from fictitious_domain_al_preconditioners_amd import _abi, problems, solver

EPS = np.finfo(np.float64).eps

CASES = {
    "stokes2d_16_3": lambda: problems.stokes2d_circle(16, 3),
    "elliptic2d_32_8": lambda: problems.elliptic_interface2d(32, 8),
    "stokes3d_8_2": lambda: problems.stokes3d_sphere(8, 2),
    "laplace2d_32_4": lambda: problems.laplace2d_circle(32, immersed_refine=4),
    "laplace2d_32_6": lambda: problems.laplace2d_circle(32, immersed_refine=6),
}


def numpy_cg_coefficients(pb, max_steps=None, tol=1e-12):
    """float64 NumPy CG on C Ct, b = 1, x0 = 0, SolverControl(n_lambda, 1e-12): (alpha_1..k, beta_1..k-1, res)."""
    Ct = pb.mats["Ct"].to_scipy().tocsr()
    Cm = Ct.T.tocsr()
    n = Cm.shape[0]
    max_steps = n if max_steps is None else max_steps
    r = np.ones(n)
    p = r.copy()
    rr = float(r @ r)
    alpha, beta = [], []
    for _ in range(max_steps):
        Ap = Cm @ (Ct @ p)
        pAp = float(p @ Ap)
        assert pAp > 0.0
        a = rr / pAp
        alpha.append(a)
        r = r - a * Ap
        rr_new = float(r @ r)
        if np.sqrt(rr_new) <= tol or len(alpha) == max_steps:
            rr = rr_new
            break
        beta.append(rr_new / rr)
        p = r + beta[-1] * p
        rr = rr_new
    return np.array(alpha), np.array(beta), np.sqrt(rr)


def lanczos_matrix(alpha, beta):
    k = alpha.size
    d = 1.0 / alpha
    d[1:] += beta[:k - 1] / alpha[:k - 1]
    e = np.sqrt(beta[:k - 1]) / alpha[:k - 1]
    return d, e


@pytest.fixture(scope="module")
def coefficients():
    return {name: numpy_cg_coefficients(make()) for name, make in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_extremes_against_scipy(coefficients, name):
    """|theta - theta_scipy| <= 4 k eps ||T_k||_inf for both extremes (the form of the backward-error bound of a
    symmetric tridiagonal eigensolver) on the alpha, beta of a float64 NumPy CG.  The factor 4 is 40x the 0.1 a plain
    Sturm bisection showed on these inputs when the bound was chosen.  Measured with the library's routine, largest
    over both ends, in units of k eps ||T_k||_inf: 0.167 (stokes2d_16_3, k = 5, i.e. 0.8 eps ||T||), 0.026
    (elliptic2d_32_8, k = 62), 0.096 (stokes3d_8_2, k = 65), 0.023 (laplace2d_32_4, k = 64), 0.017 (laplace2d_32_6,
    k = 256)."""
    alpha, beta, _ = coefficients[name]
    k = alpha.size
    d, e = lanczos_matrix(alpha, beta)
    ref = sla.eigvalsh_tridiagonal(d, e) if k > 1 else d
    norm = np.max(np.abs(d) + np.concatenate(([0.0], np.abs(e))) + np.concatenate((np.abs(e), [0.0])))
    lo, hi = solver.host_tridiagonal_extremes(alpha, beta)
    err = max(abs(lo - ref[0]), abs(hi - ref[-1])) / (k * EPS * norm)
    print(f"{name}: k = {k}, kappa = {hi / lo:.6g}, error = {err:.3g} k eps ||T||_inf")
    assert abs(lo - ref[0]) <= 4 * k * EPS * norm
    assert abs(hi - ref[-1]) <= 4 * k * EPS * norm
    assert 0.0 < lo <= hi


def test_numpy_cg_matches_the_expected_counts(coefficients):
    """The shapes behave as the issue's table says (expectations of the float64 run, loose on purpose)."""
    a, _, res = coefficients["stokes2d_16_3"]
    assert a.size <= 8 and res <= 1e-12
    a, _, res = coefficients["laplace2d_32_4"]
    assert a.size == 64 and res > 1e-12           # full rank, but the cap n_lambda is hit
    a, _, res = coefficients["laplace2d_32_6"]
    assert a.size == 256 and res > 1e-12          # rank-deficient C Ct
    assert np.all(np.isfinite(a)) and np.all(a > 0)


def test_one_step_gives_the_reciprocal_twice():
    lo, hi = solver.host_tridiagonal_extremes([0.3], [])
    assert lo == hi == 1.0 / 0.3
    lib = solver.load_library()
    a = np.array([0.3])
    l0, l1 = C.c_double(), C.c_double()
    assert lib.alfd_host_tridiagonal_extremes(1, a.ctypes.data, None, C.byref(l0), C.byref(l1)) == _abi.OK
    assert l0.value == l1.value == 1.0 / 0.3


def test_two_by_two_is_the_closed_form():
    alpha, beta = np.array([0.5, 0.25]), np.array([0.09])
    d, e = lanczos_matrix(alpha, beta)
    mean, rad = 0.5 * (d[0] + d[1]), np.hypot(0.5 * (d[0] - d[1]), e[0])
    lo, hi = solver.host_tridiagonal_extremes(alpha, beta)
    assert abs(lo - (mean - rad)) <= 8 * EPS * (mean + rad)
    assert abs(hi - (mean + rad)) <= 8 * EPS * (mean + rad)


@pytest.mark.parametrize("alpha,beta", [
    ([], []),                                  # k = 0
    ([0.0, 1.0], [0.5]), ([-1.0, 1.0], [0.5]), ([1.0, np.nan], [0.5]), ([np.inf, 1.0], [0.5]),
    ([1.0, 1.0], [-0.5]), ([1.0, 1.0], [np.nan]), ([1.0, 1.0], [np.inf]),
])
def test_bad_coefficients_are_rejected(alpha, beta):
    lib = solver.load_library()
    a, b = np.array(alpha, np.float64), np.array(beta, np.float64)
    l0, l1 = C.c_double(), C.c_double()
    rc = lib.alfd_host_tridiagonal_extremes(a.size, a.ctypes.data if a.size else None,
                                            b.ctypes.data if b.size else None, C.byref(l0), C.byref(l1))
    assert rc == _abi.E_INVALID
    with pytest.raises(solver.AlfdError):
        solver.host_tridiagonal_extremes(alpha, beta)


def test_null_context_is_invalid():
    lib = solver.load_library()
    out, linf = _abi.Spectrum(), C.c_double()
    assert lib.alfd_estimate_spectrum(None, _abi.SPECTRUM_CCT, None, C.byref(out)) == _abi.E_INVALID
    assert lib.alfd_constraint_residual(None, None, None, C.byref(linf)) == _abi.E_INVALID
    assert lib.alfd_get_cg_coefficients(None, None, None, 0, None) == _abi.E_INVALID
    assert C.sizeof(_abi.Spectrum) == 48
