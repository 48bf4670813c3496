"""The drivers' sanity checks on the GPU (elliptic_interface.cc:973-1009): cond(C Ct) by unpreconditioned CG with
recorded coefficients (alfd_estimate_spectrum) and the constraint residual (alfd_constraint_residual).

* the CG bit for bit against a restatement from the frozen oracle's spmv / dot alone, on six shapes;
* device-stepped = host-stepped, launch counts, compaction through the patch = the library's own extraction;
* no side effects on a resident solve; Ritz values against a dense eigvalsh; the constraint residual against
  system_apply."""
import functools
import math

import numpy as np
import pytest

import cases
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver
from oracle import oracle

pytestmark = pytest.mark.gpu

# name -> (generator, variant, max_steps or None = n_lambda)
SHAPES = {
    "stokes2d_16_3": (lambda: problems.stokes2d_circle(16, 3), _abi.AL_STOKES, None),
    "elliptic2d_32_8": (lambda: problems.elliptic_interface2d(32, 8), _abi.AL_ELL_MODIFIED, None),
    "stokes3d_8_2": (lambda: problems.stokes3d_sphere(8, 2), _abi.AL_STOKES, None),          # u: 4 chunks, S = 375
    "laplace2d_32_4": (lambda: problems.laplace2d_circle(32, immersed_refine=4), _abi.AL2, None),   # cap hit
    "laplace2d_32_6": (lambda: problems.laplace2d_circle(32, immersed_refine=6), _abi.AL2, None),   # rank-deficient
    "laplace2d_256_11": (lambda: problems.laplace2d_circle(256, immersed_refine=11), _abi.AL2, 48),  # lambda: 2 chunks
}


@functools.lru_cache(maxsize=None)
def problem(name):
    return SHAPES[name][0]()


def config(name):
    cfg = _abi.default_config(SHAPES[name][1])
    if SHAPES[name][1] == _abi.AL_ELL_MODIFIED:
        cfg.gamma, cfg.gamma2 = 10.0, 1e-2
        cfg.inner = _abi.Control(_abi.CTRL_REDUCTION, 100000, 1e-2, 1e-20)
        cfg.outer = _abi.Control(_abi.CTRL_REDUCTION, 1000, 1e-10, 1e-10)
    return cfg


def control(name):
    ms = SHAPES[name][2]
    return None if ms is None else _abi.Control(_abi.CTRL_ABS, ms, 1e-12, 0.0)


def open_ctx(name):
    return solver.context_from_problem(problem(name), config(name))


def lanes_of(ctx, pb):
    return {k: ctx.spmv(s, np.zeros(pb.mats[k].ncols), np.zeros(pb.mats[k].nrows))[1]
            for s, k in ((_abi.C_, "C"), (_abi.CT, "Ct"))}


def identity_csr(n):
    return problems.Csr(n, n, np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), np.ones(n))


def oracle_cg(pb, lanes, max_steps=None, tol=1e-12):
    """pcg() with the identity preconditioner on y = C (Ct x), b = 1, x0 = 0, from oracle.spmv / oracle.dot only;
    the fma updates are oracle.spmv of an identity CSR with mode = 1.  Scalars are Python floats."""
    C, Ct = pb.mats["C"], pb.mats["Ct"]
    n = C.nrows
    max_steps = n if max_steps is None else max_steps
    I = identity_csr(n)
    r, x, p = np.ones(n), np.zeros(n), None
    rr = oracle.dot(r, r)
    res0 = res = math.sqrt(rr)
    alpha, beta, paps = [], [], []
    steps, converged = 0, res0 <= tol
    while not converged and steps < max_steps and not math.isnan(res):
        steps += 1
        if steps == 1:
            p = r.copy()
        else:
            beta.append(rr / rr_old)
            p, _ = oracle.spmv(I, p, r, mode=1, alpha=beta[-1])        # p = fma(beta, p, r)
        t, _ = oracle.spmv(Ct, p, lanes=lanes["Ct"])
        Ap, _ = oracle.spmv(C, t, lanes=lanes["C"])
        pap = oracle.dot(p, Ap)
        paps.append(pap)
        a = rr / pap
        alpha.append(a)
        x, _ = oracle.spmv(I, p, x, mode=1, alpha=a)                   # x = fma(alpha, p, x)
        r, _ = oracle.spmv(I, Ap, r, mode=1, alpha=-a)                 # r = fma(-alpha, Ap, r)
        rr_old, rr = rr, oracle.dot(r, r)
        res = math.sqrt(rr)
        converged = res <= tol
    return dict(steps=steps, converged=int(converged), alpha=np.array(alpha), beta=np.array(beta),
                initial_residual=res0, last_residual=res, pap=np.array(paps))


@functools.lru_cache(maxsize=None)
def estimate(name):
    """One device-stepped estimate per shape (default group), with the oracle's restatement: shared by the tests."""
    pb = problem(name)
    ctx = open_ctx(name)
    try:
        lanes = lanes_of(ctx, pb)
        out = ctx.estimate_spectrum(control=control(name)).as_dict()
        alpha, beta = ctx.cg_coefficients()
    finally:
        ctx.close()
    return out, alpha, beta, oracle_cg(pb, lanes, SHAPES[name][2])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", list(SHAPES))
def test_cg_equals_the_oracle_primitives_bit_for_bit(built, name):
    out, alpha, beta, ref = estimate(name)
    print(name, out, "oracle steps", ref["steps"], "min p.Ap", ref["pap"].min())
    assert out["steps"] == ref["steps"] and out["converged"] == ref["converged"]
    assert alpha.size == ref["steps"] and beta.size == ref["steps"] - 1
    assert np.array_equal(bits(alpha), bits(ref["alpha"]))
    assert np.array_equal(bits(beta), bits(ref["beta"]))
    assert bits(out["initial_residual"]) == bits(ref["initial_residual"])
    assert bits(out["last_residual"]) == bits(ref["last_residual"])
    lo, hi = solver.host_tridiagonal_extremes(alpha, beta)
    assert bits(out["lambda_min"]) == bits(lo) and bits(out["lambda_max"]) == bits(hi)
    assert bits(out["condition"]) == bits(hi / lo)


def test_expected_verdicts(built):
    """What the shapes are there for: convergence in a handful of steps; the cap n_lambda hit with full rank; a
    rank-deficient C Ct (256 multipliers on 102 coupled rows) that runs to the cap without NaN or p.Ap <= 0; the
    two-chunk multiplier block stopped at 48 steps with finite coefficients."""
    out, alpha, _, _ = estimate("stokes2d_16_3")
    assert out["converged"] == 1 and out["steps"] <= 8
    out, alpha, _, _ = estimate("laplace2d_32_4")
    assert out["converged"] == 0 and out["steps"] == 64 and math.isfinite(out["condition"])
    out, alpha, beta, ref = estimate("laplace2d_32_6")
    assert out["converged"] == 0 and out["steps"] == 256
    assert np.all(np.isfinite(alpha)) and np.all(alpha > 0) and np.all(np.isfinite(beta)) and np.all(ref["pap"] > 0)
    assert math.isfinite(out["condition"]) and out["condition"] > 1e4
    out, alpha, beta, _ = estimate("laplace2d_256_11")
    assert out["steps"] == 48 and np.all(np.isfinite(beta)) and np.all(np.isfinite(alpha))


@pytest.mark.parametrize("name", ["stokes3d_8_2", "laplace2d_256_11"])
def test_device_stepped_equals_host_stepped(built, name):
    ref_out, ref_alpha, ref_beta, _ = estimate(name)      # device-stepped, default group
    ctx = open_ctx(name)
    try:
        runs = []
        for host, group in ((1, None), (0, 1), (0, 3)):
            ctx.set_tunable("spectrum_host_stepped", host)
            if group is not None:
                ctx.set_tunable("spectrum_group", group)
            out = ctx.estimate_spectrum(control=control(name)).as_dict()
            runs.append((out, *ctx.cg_coefficients()))
    finally:
        ctx.close()
    for out, alpha, beta in runs:
        assert out["steps"] == ref_out["steps"] and out["converged"] == ref_out["converged"]
        assert np.array_equal(bits(alpha), bits(ref_alpha)) and np.array_equal(bits(beta), bits(ref_beta))
        for key in ("initial_residual", "last_residual", "lambda_min", "lambda_max", "condition"):
            assert bits(out[key]) == bits(ref_out[key]), key


def _launches(pb, variant, max_steps, group):
    ctx = solver.context_from_problem(pb, _abi.default_config(variant))
    try:
        ctx.set_tunable("spectrum_group", group)
        ctl = _abi.Control(_abi.CTRL_ABS, max_steps, 1e-12, 0.0)
        ctx.estimate_spectrum(control=ctl)                  # warm-up: builds the extractions
        ctx.enable_timing(2)
        out = ctx.estimate_spectrum(control=ctl)
        total = sum(v["launches"] for v in ctx.timing().values())
    finally:
        ctx.close()
    return out.steps, total


def test_launch_count(built):
    """Timing class 2 counts every launch of the device-stepped run: 2 at the start (first update, stop rule of step
    0), 6 per enqueued iteration (p, Ct p, C t, p.Ap, update, stop rule) and one mirror launch per group.  The
    mirror launches are total - 2 - 6 * enqueued, at most ceil(steps / group) + 2; the count per iteration does not
    depend on n_u (1089 against 16641 background unknowns at the same 20 steps; the float64 NumPy CG needs 64 and 27
    steps there, so both runs end at the cap)."""
    group, max_steps = 5, 20
    counts = {}
    for n in (32, 128):
        steps, total = _launches(problems.laplace2d_circle(n, immersed_refine=4), _abi.AL2, max_steps, group)
        assert steps == max_steps
        groups = math.ceil(steps / group)
        enqueued = min(groups * group, max_steps)
        mirrors = total - 2 - 6 * enqueued
        print(f"n = {n}: {total} launches, {enqueued} iterations enqueued, {mirrors} mirror launches")
        assert 1 <= mirrors <= groups + 2
        counts[n] = total
    assert counts[32] == counts[128]
    # a solve that converges early still reads the state once per group only
    steps, total = _launches(problems.stokes2d_circle(16, 3), _abi.AL_STOKES, 64, 4)
    groups = math.ceil(steps / 4)
    assert 1 <= total - 2 - 6 * groups * 4 <= groups + 2


def test_patch_operators_and_own_extraction_give_the_same_bits(built):
    """With the interface patch on (ml_patch_degree > 0, multilevel) the estimate runs on the patch's C[:,S] /
    Ct[S,:]; without it on the library's own extractions: the same coefficients."""
    pb = problem("stokes3d_8_2")
    ref_out, ref_alpha, ref_beta, _ = estimate("stokes3d_8_2")       # Chebyshev inner preconditioner: own extraction
    cfg = _abi.default_config(_abi.AL_STOKES)
    cfg.inner_prec = _abi.PREC_MULTILEVEL
    cfg.ml_smooth_degree, cfg.ml_smooth_ratio, cfg.ml_coarse_degree = 4, 256.0, 10
    cfg.ml_patch_degree = 4
    ctx = solver.Context(0)
    try:
        ctx.set_matrix(_abi.A, pb.mats["A"])
        ctx.set_matrix(_abi.C_, pb.mats["C"])
        ctx.set_matrix(_abi.CT, pb.mats["Ct"])
        ctx.set_diag(_abi.INVW, pb.inv_w_diag_squared())
        ctx.configure(cfg)
        levels = ctx.build_smoothed_aggregation(block_size=3, damping=4.0 / 3.0, min_coarse=300)
        assert levels
        solver.upload_problem(ctx, pb, cfg, None)
        out = ctx.estimate_spectrum().as_dict()
        alpha, beta = ctx.cg_coefficients()
    finally:
        ctx.close()
    assert out["steps"] == ref_out["steps"] and out["converged"] == ref_out["converged"]
    assert np.array_equal(bits(alpha), bits(ref_alpha)) and np.array_equal(bits(beta), bits(ref_beta))
    assert bits(out["condition"]) == bits(ref_out["condition"])


def test_no_side_effects_and_error_codes(built):
    pb = problem("stokes2d_16_3")
    cfg = config("stokes2d_16_3")
    ctx = solver.Context(0)
    try:
        out = _abi.Spectrum()
        import ctypes as C
        assert ctx._lib.alfd_estimate_spectrum(ctx._h, _abi.SPECTRUM_CCT, None, C.byref(out)) == _abi.E_NOT_SETUP
        linf = C.c_double()
        assert ctx._lib.alfd_constraint_residual(ctx._h, None, None, C.byref(linf)) == _abi.E_NOT_SETUP
        solver.upload_problem(ctx, pb, cfg)
        with pytest.raises(solver.AlfdError) as e:
            ctx.cg_coefficients()
        assert e.value.status == _abi.E_NOT_SETUP
        with pytest.raises(solver.AlfdError) as e:
            ctx.estimate_spectrum(op=7)
        assert e.value.status == _abi.E_INVALID
        with pytest.raises(solver.AlfdError) as e:
            ctx.estimate_spectrum(control=_abi.Control(_abi.CTRL_ABS, 0, 1e-12, 0.0))
        assert e.value.status == _abi.E_INVALID
        rhs = ctx.augment_rhs(cases.rhs_of(pb))
        ctx.upload_rhs(rhs)
        r1 = ctx.solve_resident()
        x1, h1 = ctx.download_solution(), ctx.history()
        s1 = ctx.estimate_spectrum().as_dict()
        a1, b1 = ctx.cg_coefficients()
        r2 = ctx.solve_resident()
        x2, h2 = ctx.download_solution(), ctx.history()
        s2 = ctx.estimate_spectrum().as_dict()
        a2, b2 = ctx.cg_coefficients()
    finally:
        ctx.close()
    assert r1.status == 0 and r2.status == 0
    assert (r1.outer_iterations, r1.inner_iterations, r1.mp_iterations) == \
           (r2.outer_iterations, r2.inner_iterations, r2.mp_iterations)
    for b in range(3):
        assert np.array_equal(bits(x1[b]), bits(x2[b]))
    assert np.array_equal(bits(h1), bits(h2))
    assert {k: bits(v).tolist() for k, v in s1.items()} == {k: bits(v).tolist() for k, v in s2.items()}
    assert np.array_equal(bits(a1), bits(a2)) and np.array_equal(bits(b1), bits(b2))
    ref_out, ref_alpha, _, _ = estimate("stokes2d_16_3")
    assert np.array_equal(bits(a1), bits(ref_alpha)) and s1["steps"] == ref_out["steps"]


@pytest.mark.parametrize("name", ["stokes2d_16_3", "elliptic2d_32_8", "stokes3d_8_2"])
def test_ritz_values_against_the_true_spectrum(built, name):
    """Where the CG converged.  Interlacing puts the Ritz values inside the spectrum of C Ct (1e-8 relative slack for
    rounding).  On the two small 2-D shapes kappa agrees with the true condition number to 1e-6 relative; not on
    stokes3d_8_2, whose all-ones right-hand side does not see the lowest eigenvector (1.31e7 against 1.60e7)."""
    out, _, _, _ = estimate(name)
    assert out["converged"] == 1
    Ct = problem(name).mats["Ct"].to_scipy().toarray()
    lam = np.linalg.eigvalsh(Ct.T @ Ct)
    print(name, "kappa", out["condition"], "true", lam[-1] / lam[0])
    assert lam[0] * (1 - 1e-8) <= out["lambda_min"]
    assert out["lambda_max"] <= lam[-1] * (1 + 1e-8)
    if name != "stokes3d_8_2":
        assert abs(out["condition"] - lam[-1] / lam[0]) <= 1e-6 * lam[-1] / lam[0]


@pytest.mark.parametrize("name,gen,variant", [
    ("laplace2d_16_3", lambda: problems.laplace2d_circle(16, immersed_refine=3), _abi.AL2),
    ("stokes2d_16_3", lambda: problem("stokes2d_16_3"), _abi.AL_STOKES),
    ("elliptic2d_32_8", lambda: problem("elliptic2d_32_8"), _abi.AL_ELL_MODIFIED),
])
def test_constraint_residual_equals_system_apply(built, name, gen, variant):
    pb = gen()
    cfg = config(name) if name in SHAPES else _abi.default_config(variant)
    ctx = solver.context_from_problem(pb, cfg)
    try:
        x = cases.rng_blocks(pb, 11)
        g = np.random.default_rng(12).uniform(-1.0, 1.0, pb.block_sizes[-1])
        last = ctx.system_apply(x)[-1]
        got_g, got_0 = ctx.constraint_residual(x, g), ctx.constraint_residual(x)
        # one entry of x[0] that the coupling touches: the result is NaN, not the maximum of the rest
        touched = int(np.flatnonzero(np.diff(pb.mats["Ct"].row_ptr) > 0)[0])
        xn = [b.copy() for b in x]
        xn[0][touched] = np.nan
        got_nan = ctx.constraint_residual(xn, g)
    finally:
        ctx.close()
    assert bits(got_g) == bits(np.max(np.abs(last - g)))
    assert bits(got_0) == bits(np.max(np.abs(last)))
    assert math.isnan(got_nan)


def test_constraint_residual_after_an_elliptic_solve(built):
    """Property: after a converged outer solve the last block row C u - M u2 of the residual is below the configured
    stop rule's bound on the whole residual, max(tol, reduce * ||rhs||_2) (zero start), in the max norm."""
    pb, cfg = problem("elliptic2d_32_8"), config("elliptic2d_32_8")
    ctx = solver.context_from_problem(pb, cfg)
    try:
        rhs = ctx.augment_rhs(cases.rhs_of(pb))
        x, res = ctx.solve(rhs)
        got = ctx.constraint_residual(x, rhs[-1])
    finally:
        ctx.close()
    assert res.status == 0
    bound = max(cfg.outer.tol, cfg.outer.reduce * float(np.linalg.norm(np.concatenate(rhs))))
    print("constraint residual", got, "bound", bound, "last outer residual", res.last_residual)
    assert got <= bound
