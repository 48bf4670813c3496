"""The inner preconditioner M^-1 (Jacobi, the Chebyshev sweep, the multigrid V-cycle over aggregates or CSR prolongators,
the interface patch, the explicit coarsest inverse) of the ORACLE against tests/precond_reference.py, an independent
restatement from the definitions, through the primitive orc_h_inner_prec_apply (z = M^-1 r with no CG around it).

Checks (letters as in the GPU file, tests/test_gpu_inner_preconditioner.py, which repeats them for the library):
  a. vectors against the restatement;  b. the whole operator, every column;  c. symmetry;  d. definiteness;
  e. the power-iteration estimate (safety factor included) bounds the true lambda_max(D^-1 Aug) on every level and on
     the patch.
The configurations, inputs and measures defined here are shared with the GPU file."""
import numpy as np
import pytest

import cases
import precond_reference as pr
from fictitious_domain_al_preconditioners_amd import _abi, problems

OP_NAME = {_abi.INNER_OP_AUG: "aug", _abi.INNER_OP_A22: "a22", _abi.INNER_OP_AUG2: "aug2"}


class Config:
    """One row of the table: problem, alfd_config, hierarchy (the list the library and the oracle take), inner operator."""

    def __init__(self, name, pb, cfg, levels=None, op=_abi.INNER_OP_AUG):
        self.name, self.pb, self.cfg, self.levels, self.op = name, pb, cfg, levels, op

    def inv_w(self):
        return self.pb.inv_w_diag_of_mass_squared() if "A2" in self.pb.mats else self.pb.inv_w_diag_squared()

    def reference(self, dtype=np.float64):
        hierarchy = []
        for e in self.levels or []:
            hierarchy.append(e[0].to_scipy() if hasattr(e[0], "row_ptr") else (e[0], e[1], e[3] if len(e) > 3 else None))
        m = self.pb.mats
        return pr.InnerPreconditioner(self.cfg, m["A"].to_scipy(), m["Ct"].to_scipy(), self.inv_w(), hierarchy, dtype,
                                      op=OP_NAME[self.op], A2=m["A2"].to_scipy() if "A2" in m else None,
                                      M=m["M"].to_scipy() if "A2" in m else None)

    def oracle(self):
        from oracle import oracle
        osys = oracle.system_from_problem(self.pb, aggregates=self.levels)
        return osys, osys.open(self.cfg)


def _operator_form(n, refine):
    pb = problems.laplace2d_circle(n, refine, surface_mass=True)
    a_op, gamma_h, inv_w = problems.operator_form(pb)
    pb.mats = dict(pb.mats, A=a_op)
    pb.inv_w_override = inv_w
    cfg = _abi.default_config(_abi.AL2)
    cfg.gamma, cfg.aug_assembled = gamma_h, 1
    return pb, cfg


def _weights(agg, seed):
    """Prolongation entries for the weighted-aggregate rows: positive, not constant, reproducible."""
    return 0.5 + np.random.default_rng(seed).uniform(0.0, 1.0, agg.size)


# "small": every column of the operator is affordable (n_0 = 2187 / 1089 / 1170), at least two coarse levels where a
# hierarchy is used, a non-empty patch where one is asked for
SMALL = ["jacobi_al2", "cheb1_al2", "cheb2_operator_form", "cheb4_stokes", "ell_modified_aug", "ell_modified_a22",
         "ell_ideal_aug2", "ml_aggregates", "ml_aggregates_weighted", "ml_gmg", "ml_gmg_patch", "ml_gmg_patch_bench",
         "ml_operator_form_patch"]
# the sizes of tests/cases.py: vector checks only
CASES = ["laplace2d_jacobi", "laplace2d_circle", "stokes3d_sphere", "laplace2d_operator_form", "elliptic_modified",
         "elliptic_modified:a22", "elliptic_ideal", "stokes3d_multilevel", "stokes3d_gmg", "stokes3d_gmg_patch",
         "laplace2d_operator_form_gmg_patch"]
_cache = {}


def config(name):
    if name not in _cache:
        _cache[name] = _make(name)
    return _cache[name]


def _make(name):
    if name in CASES:
        base, _, which = name.partition(":")
        pb, cfg = cases.case(base)
        op = _abi.INNER_OP_A22 if which == "a22" else _abi.INNER_OP_AUG2 if cfg.variant == _abi.AL_ELL_IDEAL \
            else _abi.INNER_OP_AUG
        return Config(name, pb, cfg, cases.aggregates_of(pb, cfg), op)
    if name in ("jacobi_al2", "cheb1_al2"):
        pb, cfg = problems.laplace2d_circle(32, 3), _abi.default_config(_abi.AL2)
        cfg.inner_prec, cfg.cheb_degree = (_abi.PREC_JACOBI, 4) if name == "jacobi_al2" else (_abi.PREC_CHEBYSHEV, 1)
        return Config(name, pb, cfg)
    if name == "cheb2_operator_form":
        pb, cfg = _operator_form(32, 3)
        cfg.cheb_degree = 2
        return Config(name, pb, cfg)
    if name == "cheb4_stokes":
        return Config(name, problems.stokes3d_sphere(4, 1), _abi.default_config(_abi.AL_STOKES))
    if name.startswith("ell_"):
        pb = problems.elliptic_interface2d(32, 8)
        ideal = name == "ell_ideal_aug2"
        cfg = _abi.default_config(_abi.AL_ELL_IDEAL if ideal else _abi.AL_ELL_MODIFIED)
        cfg.gamma, cfg.gamma2 = 10.0, (10.0 if ideal else 1e-2)
        op = _abi.INNER_OP_AUG2 if ideal else _abi.INNER_OP_A22 if name.endswith("a22") else _abi.INNER_OP_AUG
        return Config(name, pb, cfg, None, op)
    if name == "ml_operator_form_patch":                 # the settings of cases "laplace2d_operator_form_gmg_patch"
        pb, cfg = _operator_form(32, 3)
        cfg.inner_prec = _abi.PREC_MULTILEVEL
        cfg.ml_smooth_degree, cfg.ml_smooth_degree_coarse, cfg.ml_smooth_ratio = 2, 3, 20.0
        cfg.ml_patch_degree, cfg.ml_patch_ratio, cfg.ml_coarse_direct = 6, 50.0, 1024
        return Config(name, pb, cfg, problems.tensor_prolongators(pb.params, min_coarse=50))
    pb, cfg = problems.stokes3d_sphere(4, 1), _abi.default_config(_abi.AL_STOKES)
    cfg.inner_prec = _abi.PREC_MULTILEVEL
    if name.startswith("ml_aggregates"):                 # the settings of cases "stokes3d_multilevel": coarsest Chebyshev
        cfg.ml_smooth_degree, cfg.ml_smooth_ratio = 2, 8.0
        levels = problems.geometric_aggregates(pb, a=2, min_coarse=50)
        if name.endswith("weighted"):
            levels = [(agg, nc, None, _weights(agg, 5 + l)) for l, (agg, nc) in enumerate(levels)]
        return Config(name, pb, cfg, levels)
    cfg.ml_smooth_degree, cfg.ml_smooth_ratio = 4, 30.0
    if name == "ml_gmg":                                 # cases "stokes3d_gmg": coarsest Chebyshev(12) / 100, no patch
        cfg.ml_coarse_degree, cfg.ml_coarse_ratio, cfg.ml_coarse_direct = 12, 100.0, -1
    elif name == "ml_gmg_patch":                         # cases "stokes3d_gmg_patch": patch 5 / 30, explicit inverse
        cfg.ml_patch_degree, cfg.ml_patch_ratio, cfg.ml_coarse_direct = 5, 30.0, 1024
    elif name == "ml_gmg_patch_bench":                   # ml_smooth_degree_coarse > 0, as the benchmark runs it
        _abi.bench_multilevel_settings(cfg, geometric=True)
    else:
        raise KeyError(name)
    return Config(name, pb, cfg, problems.tensor_prolongators(pb.params, min_coarse=50))


def inputs(cf):
    """The right-hand sides of check (a): uniform(-1, 1) with two seeds, a constant, the indicator of the patch rows
    S, a unit vector on a Dirichlet row (a row of the operator's stiffness block holding only its diagonal)."""
    m = cf.pb.mats
    n0, n1 = m["A"].nrows, (m["A2"].nrows if "A2" in m else 0)
    n = {_abi.INNER_OP_AUG: n0, _abi.INNER_OP_A22: n1, _abi.INNER_OP_AUG2: n0 + n1}[cf.op]
    out = {"uniform seed 11": np.random.default_rng(11).uniform(-1, 1, n),
           "uniform seed 12": np.random.default_rng(12).uniform(-1, 1, n), "constant": np.ones(n)}
    if cf.op != _abi.INNER_OP_A22:
        ind = np.zeros(n)
        ind[:n0][np.diff(m["Ct"].row_ptr) > 0] = 1.0
        assert ind.any()
        out["patch indicator"] = ind
    stiff = m["A2"] if cf.op == _abi.INNER_OP_A22 else m["A"]
    lone = np.flatnonzero(np.diff(stiff.row_ptr) == 1)
    if lone.size:
        e = np.zeros(n)
        e[lone[lone.size // 2]] = 1.0
        out["unit vector on a Dirichlet row"] = e
    return out


def rel(z, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(np.asarray(z, np.float64) - ref)) / np.max(np.abs(ref)))


def dense_operator(apply, n):
    """Column j = apply(e_j), all n columns."""
    out = np.empty((n, n))
    e = np.zeros(n)
    for j in range(n):
        e[j] = 1.0
        out[:, j] = apply(e)
        e[j] = 0.0
    return out


def asymmetry(m):
    return float(np.max(np.abs(m - m.T)) / np.max(np.abs(m)))


def definiteness(m, aug0):
    """(smallest eigenvalue of (M + M^T)/2, [lambda_min, lambda_max] of L^T M L = the spectrum of M Aug_0)."""
    low = float(np.linalg.eigvalsh((m + m.T) / 2)[0])
    L = np.linalg.cholesky(np.asarray(pr._dense(aug0), np.float64))
    k = L.T @ m @ L
    ev = np.linalg.eigvalsh((k + k.T) / 2)
    return low, float(ev[0]), float(ev[-1])


def check_operator(tag, name, m, ref, m_ref=None):
    """Checks (b), (c), (d) of one implementation's dense operator m against the float64 restatement."""
    m_ref = ref.dense() if m_ref is None else m_ref
    err = float(np.max(np.abs(m - m_ref)) / np.max(np.abs(m_ref)))
    asym, asym_ref = asymmetry(m), asymmetry(m_ref)
    low, lmin, lmax = definiteness(m, ref.levels[0].aug)
    _, rmin, rmax = definiteness(m_ref, ref.levels[0].aug)
    print(f"{tag} {name}: n = {m.shape[0]}, max|M - M_ref|/max|M_ref| = {err:.2e}, asymmetry {asym:.2e} "
          f"(restatement {asym_ref:.2e}), min eig sym(M) = {low:.3e}, spectrum of M Aug_0 = [{lmin:.4f}, {lmax:.4f}] "
          f"(restatement [{rmin:.4f}, {rmax:.4f}])")
    assert err <= pr.TOL, (name, err)                                     # (b)
    assert asym <= 64 * asym_ref, (name, asym, asym_ref)                  # (c)
    # ... and the definition itself is symmetric, so that (c) still bites when restatement and implementations are
    # changed alike: M_ref and M_ref^T both round the same exact operator, whose float64 rounding tol bounds.  (The
    # 2-block operator of the ideal elliptic variant is symmetric as well: alfd_setup insists on gamma == gamma2.)
    assert asym_ref <= pr.TOL, (name, asym_ref)
    assert low > 0 and lmin > 0, (name, low, lmin)                        # (d)
    assert rmin > 0
    assert abs(lmax / lmin - rmax / rmin) <= 0.01 * (rmax / rmin), (name, lmax / lmin, rmax / rmin)
    return m_ref


def check_estimates(name, ref):
    """Check (e): lambda_l incl. the safety factor >= the true lambda_max(D_l^-1 Aug_l), every level and the patch."""
    ratios = []
    for what, aug, d, lam in ref.estimates():
        true = pr.true_lambda_max(aug, d)
        ratios.append((what, aug.shape[0], float(lam) / true))
    print(f"(e) {name}: " + ", ".join(f"{w} (n = {n}) estimate / true = {r:.4f}" for w, n, r in ratios))
    bad = [x for x in ratios if not x[2] >= 1.0]
    assert not bad, (name, bad)
    return ratios


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def test_tolerance_is_what_the_restatement_measures():
    """tol of (a), (b), (g): the float64 against the longdouble run of the restatement, times 64, floored at 1e-13 --
    the table in precond_reference's docstring."""
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than float64 on this machine"
    worst = 0.0
    for name in SMALL:
        cf = config(name)
        r64, rld = cf.reference(np.float64), cf.reference(np.longdouble)
        diffs = [rel(r64.apply(r), rld.apply(r)) for r in inputs(cf).values()]
        print(f"f64 vs longdouble {name}: n = {r64.n}, max over {len(diffs)} inputs = {max(diffs):.2e}")
        worst = max(worst, max(diffs))
    print(f"largest difference {worst:.2e} -> tol = {max(pr.TOL_FLOOR, pr.TOL_MARGIN * worst):.2e}")
    assert worst <= pr.MEASURED_F64_VS_LONGDOUBLE, worst
    assert pr.TOL == max(pr.TOL_FLOOR, pr.TOL_MARGIN * pr.MEASURED_F64_VS_LONGDOUBLE) and pr.TOL <= 1e-9


@pytest.mark.parametrize("name", SMALL + CASES)
def test_oracle_vectors_and_eigenvalue_bound(name):
    """(a) and (e) for the oracle; level 0's estimate equals the oracle's alfd_result.lambda_max."""
    cf = config(name)
    ref = cf.reference()
    osys, h = cf.oracle()
    try:
        for what, r in inputs(cf).items():
            rc, z = osys.handle_inner_prec_apply(h, r, cf.op)
            assert rc == 0
            err = rel(z, ref.apply(r))
            print(f"(a) oracle {name}, {what}: {err:.2e}")
            assert err <= pr.TOL, (name, what, err)
        check_estimates(name, ref)
        if cf.op != _abi.INNER_OP_A22 and cf.cfg.inner_prec in (_abi.PREC_CHEBYSHEV, _abi.PREC_MULTILEVEL):
            one = _abi.Control(_abi.CTRL_FIXED_ITERS, 1, 0.0, 0.0)
            rc, _, res = osys.handle_precond_apply(h, cases.rng_blocks(cf.pb, 3), inner=one)
            assert rc == 0
            lam = float(ref.levels[0].lam)
            print(f"(e) {name}: lambda_0 restatement {lam!r}, oracle {res.lambda_max!r}")
            assert abs(res.lambda_max - lam) <= pr.TOL * lam
    finally:
        osys.close_handle(h)


@pytest.mark.parametrize("name", SMALL)
def test_oracle_operator_symmetry_definiteness(name):
    """(b), (c), (d) for the oracle, every column of the operator."""
    cf = config(name)
    ref = cf.reference()
    osys, h = cf.oracle()
    try:
        def apply(e):
            rc, z = osys.handle_inner_prec_apply(h, e, cf.op)
            assert rc == 0
            return z
        check_operator("oracle", name, dense_operator(apply, ref.n), ref)
    finally:
        osys.close_handle(h)


def test_wrong_operator_is_invalid():
    cf = config("cheb1_al2")
    osys, h = cf.oracle()
    try:
        for op in (_abi.INNER_OP_A22, _abi.INNER_OP_AUG2, 7):
            from oracle import oracle
            z = np.zeros(cf.pb.block_sizes[0])
            assert oracle.lib().orc_h_inner_prec_apply(h, op, z.ctypes.data, z.ctypes.data) == _abi.E_INVALID
    finally:
        osys.close_handle(h)
