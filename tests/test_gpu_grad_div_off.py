"""Stokes without grad-div (grad_div_in_A = 0) on the GPU: Aug = A + gamma Ct invW C + gamma_gd Bt Mp^-1 B with a
nested lumped-Jacobi CG on Mp in every application of Aug (stokes_immersed_boundary.cc:991-995).

* system_apply bit for bit against the frozen oracle's primitives, composed in the order of DESIGN section 4;
* the device-stepped nested CG against the host-stepped one (same vectors, histories, counts) and its launch count;
* identity / Chebyshev inner CG solves on the 2 eps:eps Stokes problem against SciPy, determinism, the multilevel
  refusal and a 2-rank in-process run."""
import math
import threading

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from fictitious_domain_al_preconditioners_amd import _abi, partition, problems, solver
from oracle import oracle

pytestmark = pytest.mark.gpu


def stokes_nogd(dim, n, ref, row_ranges=None):
    """stokes3d_sphere / stokes2d_circle with the reference's 2 eps(u):eps(v) velocity block and no grad-div."""
    if dim == 3:
        return problems.generate(dim=3, degree=2, ncomp=3, n_cells=n, stokes=True, sym_grad=True,
                                 center=(0.5, 0.5, 0.5), radius=0.1, immersed_refine=ref, coupling_nq=4,
                                 body_force=(1.0, 0.0, 0.0), embedded_value=(-1.0, 1.0, 0.0), row_ranges=row_ranges)
    return problems.generate(dim=2, degree=2, ncomp=2, n_cells=n, stokes=True, sym_grad=True,
                             center=(0.5, 0.5, 0.0), radius=0.2, immersed_refine=ref, coupling_nq=3,
                             body_force=(1.0, 0.0), embedded_value=(-1.0, 1.0))


def nogd_config(variant=_abi.AL_STOKES, inner_prec=_abi.PREC_IDENTITY, w_inverse=_abi.W_DIAGONAL):
    cfg = _abi.default_config(variant)
    cfg.grad_div_in_A = 0
    cfg.gamma_grad_div = 10.0
    cfg.inner_prec = inner_prec
    cfg.inner.max_steps = 1000
    cfg.w_inverse = w_inverse
    if variant == _abi.AL_STOKES_DIAG:
        cfg.outer_solver = _abi.OUTER_MINRES
    return cfg


def rhs_zero_p(pb):
    """[f, 0, g]: with a zero pressure rhs the AL terms vanish at the solution (as in the reference)."""
    return [pb.vecs["f"].copy(), np.zeros(pb.block_sizes[1]), pb.vecs["g"].copy()]


@pytest.mark.parametrize("dim,n,ref", [(2, 8, 2), (3, 6, 0)])
@pytest.mark.parametrize("w_inverse", [_abi.W_DIAGONAL, _abi.W_MASS_INV_SQUARED])
def test_system_apply_equals_oracle_primitives_bit_for_bit(built, dim, n, ref, w_inverse):
    pb = stokes_nogd(dim, n, ref)
    cfg = nogd_config(w_inverse=w_inverse)
    ctx = solver.context_from_problem(pb, cfg)
    rng = np.random.default_rng(7)
    x = [rng.uniform(-1.0, 1.0, m) for m in pb.block_sizes]
    got = ctx.system_apply(x)
    lanes = {s: ctx.spmv(s, np.zeros(pb.mats[k].ncols), np.zeros(pb.mats[k].nrows))[1]
             for s, k in ((_abi.B, "B"), (_abi.BT, "Bt"), (_abi.CT, "Ct"))}
    ctx.close()
    osys = oracle.system_from_problem(pb)
    ocfg = nogd_config(w_inverse=w_inverse)
    ocfg.grad_div_in_A = 1
    z = [np.zeros(m) for m in pb.block_sizes]
    # q = Mp^-1 (B x0): the preconditioner's pressure block of the block-diagonal variant with gamma_gd = 1
    bx0, _ = oracle.spmv(pb.mats["B"], x[0], lanes=lanes[_abi.B])
    pcfg = nogd_config(_abi.AL_STOKES_DIAG, w_inverse=w_inverse)
    pcfg.grad_div_in_A, pcfg.gamma_grad_div = 1, 1.0
    rc, v, pres = osys.precond_apply(pcfg, [z[0], bx0, z[2]])
    assert rc == 0 and pres.mp_iterations > 0
    q = v[1]
    # 1. A x0, 2. the AL term (oracle system_apply with x1 = x2 = 0), 3. fma(gamma_gd, Bt q, y0), 4. + Bt x1, + Ct x2
    rc, y = osys.system_apply(ocfg, [x[0], z[1], z[2]])
    assert rc == 0
    y0, _ = oracle.spmv(pb.mats["Bt"], q, y[0], mode=1, alpha=cfg.gamma_grad_div, lanes=lanes[_abi.BT])
    y0, _ = oracle.spmv(pb.mats["Bt"], x[1], y0, mode=1, alpha=1.0, lanes=lanes[_abi.BT])
    y0, _ = oracle.spmv(pb.mats["Ct"], x[2], y0, mode=1, alpha=1.0, lanes=lanes[_abi.CT])
    assert np.array_equal(got[0], y0)
    assert np.array_equal(got[1], bx0)
    assert np.array_equal(got[2], y[2])


def _solve(ctx, pb):
    rhs = ctx.augment_rhs(rhs_zero_p(pb))
    x, res = ctx.solve(rhs)
    return x, res, ctx.history()


@pytest.mark.parametrize("variant", [_abi.AL_STOKES, _abi.AL_STOKES_DIAG])
@pytest.mark.parametrize("n", [6, 16])    # Mp: 343 rows (one 4096-row chunk), 4913 rows (two chunks)
def test_device_and_host_stepped_nested_cg_agree(built, variant, n):
    pb = stokes_nogd(3, n, 0)
    cfg = nogd_config(variant, _abi.PREC_CHEBYSHEV)
    ctx = solver.context_from_problem(pb, cfg)
    ctx.set_tunable("nested_mp_host_stepped", 1)
    xh, rh, hh = _solve(ctx, pb)
    ctx.set_tunable("nested_mp_host_stepped", 0)
    xd, rd, hd = _solve(ctx, pb)
    ctx.set_tunable("nested_mp_group", 3)
    x3, r3, h3 = _solve(ctx, pb)
    ctx.close()
    assert rd.status == 0 and rd.mp_iterations > 0
    for other, ro, ho in ((xh, rh, hh), (x3, r3, h3)):
        for b in range(3):
            assert np.array_equal(xd[b], other[b])
        assert np.array_equal(hd, ho)
        assert (rd.outer_iterations, rd.inner_iterations, rd.mp_iterations) == \
               (ro.outer_iterations, ro.inner_iterations, ro.mp_iterations)


def test_nested_launch_count(built):
    """system_apply launches, grad-div off minus on (same operators, timing class 2), device-stepped: 5 per
    enqueued nested iteration, 1 state read (mirror) per group of K, and 3 once (the first update and stop-rule
    kernels, the Bt q SpMV).  With n nested iterations: 5 K ceil(n/K) + ceil(n/K) + 3 <= 5 n + ceil(n/K) + c,
    c = 5 (K - 1) + 3."""
    pb = stokes_nogd(3, 6, 0)
    rng = np.random.default_rng(3)
    x = [rng.uniform(-1.0, 1.0, m) for m in pb.block_sizes]
    launches = {}
    for gd in (1, 0):
        cfg = nogd_config()
        cfg.grad_div_in_A = gd
        ctx = solver.context_from_problem(pb, cfg)
        K = 4
        ctx.set_tunable("nested_mp_host_stepped", 0)
        ctx.set_tunable("nested_mp_group", K)
        ctx.system_apply(x)          # warm-up
        ctx.enable_timing(2)
        ctx.system_apply(x)
        launches[gd] = sum(v["launches"] for v in ctx.timing().values())
        ctx.close()
    osys = oracle.system_from_problem(pb)
    pcfg = nogd_config(_abi.AL_STOKES_DIAG)
    pcfg.grad_div_in_A, pcfg.gamma_grad_div = 1, 1.0
    bx0, _ = oracle.spmv(pb.mats["B"], x[0])
    z = [np.zeros(m) for m in pb.block_sizes]
    rc, _, pres = osys.precond_apply(pcfg, [z[0], bx0, z[2]])
    n = pres.mp_iterations
    extra = launches[0] - launches[1]
    groups = math.ceil(n / K)
    assert extra == 5 * K * groups + groups + 3, (extra, n)
    assert extra <= 5 * n + groups + 5 * (K - 1) + 3


def _saddle_point_velocity(pb, rhs):
    """SciPy spsolve of the unaugmented system [[A, Bt, Ct], [B, 0, 0], [C, 0, 0]] with pressure dof 0 pinned
    (the pressure is defined up to a constant); returns the velocity block, which is unique."""
    A, Bt, Ct = (pb.mats[k].to_scipy().tocsr() for k in ("A", "Bt", "Ct"))
    B, C = Bt.T.tocsr(), Ct.T.tocsr()
    K = sp.bmat([[A, Bt, Ct], [B, None, None], [C, None, None]]).tocsc()
    b = np.concatenate(rhs)
    keep = np.ones(K.shape[0], bool)
    keep[A.shape[0]] = False
    sol = spla.spsolve(K[keep][:, keep], b[keep])
    return sol[:A.shape[0]]


@pytest.mark.parametrize("dim,n,ref", [(2, 16, 3), (3, 8, 0)])
@pytest.mark.parametrize("inner_prec", [_abi.PREC_IDENTITY, _abi.PREC_JACOBI, _abi.PREC_CHEBYSHEV])
def test_solve_converges_and_matches_scipy(built, dim, n, ref, inner_prec):
    pb = stokes_nogd(dim, n, ref)
    cfg = nogd_config(inner_prec=inner_prec)
    ctx = solver.context_from_problem(pb, cfg)
    x1, r1, h1 = _solve(ctx, pb)
    x2, r2, h2 = _solve(ctx, pb)
    ctx.close()
    assert r1.status == 0 and r1.inner_failures == 0
    assert r1.last_residual <= max(cfg.outer.tol, cfg.outer.reduce * r1.initial_residual)
    assert r1.mp_iterations > r1.precond_applications          # nested solves counted with the pressure block's
    for b in range(3):
        assert np.array_equal(x1[b], x2[b])
    assert np.array_equal(h1, h2) and r1.inner_iterations == r2.inner_iterations
    u = _saddle_point_velocity(pb, rhs_zero_p(pb))
    assert np.linalg.norm(x1[0] - u) <= 1e-6 * np.linalg.norm(u)


def _numpy_lambda_max(pb, cfg):
    """lambda_max(D^-1 S) * safety by the library's power iteration (integer-hash start vector, cheb_power_its
    steps), assembled independently in SciPy: S = A + gamma Ct W C + gamma_gd Bt L B, D = diag(S),
    W = 1/M_ii^2, L = the lumped inverse of Mp -- the surrogate the inner preconditioner sees."""
    A, Bt, Ct = (pb.mats[k].to_scipy().tocsr() for k in ("A", "Bt", "Ct"))
    w, l = pb.inv_w_diag_squared(), pb.mp_lumped_inv()
    S = (A + cfg.gamma * (Ct @ sp.diags(w) @ Ct.T) + cfg.gamma_grad_div * (Bt @ sp.diags(l) @ Bt.T)).tocsr()
    dinv = 1.0 / S.diagonal()
    i = np.arange(A.shape[0], dtype=np.uint64)
    v = 1.0 + ((i * np.uint64(2654435761)) & np.uint64(1023)).astype(np.float64) / 1024.0
    lam = 0.0
    for _ in range(cfg.cheb_power_its):
        v = v * (1.0 / np.sqrt(v @ v))
        v = dinv * (S @ v)
        lam = np.sqrt(v @ v)
    return lam * cfg.cheb_safety


@pytest.mark.parametrize("dim,n,ref", [(2, 8, 2), (3, 6, 0)])
def test_surrogate_diagonal_and_operator_give_the_scipy_lambda_max(built, dim, n, ref):
    pb = stokes_nogd(dim, n, ref)
    cfg = nogd_config(inner_prec=_abi.PREC_CHEBYSHEV)
    ctx = solver.context_from_problem(pb, cfg)
    rng = np.random.default_rng(5)
    _, res = ctx.precond_apply([rng.uniform(-1.0, 1.0, m) for m in pb.block_sizes])
    ctx.close()
    want = _numpy_lambda_max(pb, cfg)
    assert res.lambda_max == pytest.approx(want, rel=1e-9)
    # the grad-div term matters: without it the estimate is clearly different
    cfg0 = nogd_config(inner_prec=_abi.PREC_CHEBYSHEV)
    cfg0.gamma_grad_div = 0.0
    assert abs(_numpy_lambda_max(pb, cfg0) - want) > 1e-4 * want


def test_multilevel_is_refused(built):
    pb = stokes_nogd(3, 6, 0)
    cfg = nogd_config(inner_prec=_abi.PREC_MULTILEVEL)
    with pytest.raises(solver.AlfdError) as e:
        solver.context_from_problem(pb, cfg, aggregates=problems.geometric_aggregates(pb))
    assert e.value.status == _abi.E_UNSUPPORTED
    ctx = solver.Context(0)
    for slot, m in ((_abi.A, pb.mats["A"]),):
        ctx.set_matrix(slot, m)
    ctx.configure(nogd_config())
    with pytest.raises(solver.AlfdError) as e:
        ctx.build_aggregates(block_size=3)
    assert e.value.status == _abi.E_UNSUPPORTED
    ctx.close()


def test_two_ranks_match_single_rank(built):
    n, ref, world = 8, 0, 2
    cfg = nogd_config(inner_prec=_abi.PREC_CHEBYSHEV)
    plan = partition.slab_partition_stokes3d(n, ref, world)
    group = solver.LocalGroup(world)
    out, errs = [None] * world, []

    def work(rank):
        try:
            pb = stokes_nogd(3, n, ref, row_ranges=plan.generator_ranges(rank))
            ctx = solver.Context(0)
            ctx.comm_init_local(group.handle, rank)
            ctx.set_partition(plan.offsets)
            solver.upload_problem(ctx, pb, cfg)
            x, res = ctx.solve(ctx.augment_rhs(rhs_zero_p(pb)))
            out[rank] = dict(x=x, res=res, hist=ctx.history())
            ctx.close()
        except Exception as e:   # noqa: BLE001
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    group.close()
    assert not errs, errs
    pb = stokes_nogd(3, n, ref)
    ctx = solver.context_from_problem(pb, cfg)
    x1, res, h1 = _solve(ctx, pb)
    ctx.close()
    # the stitched velocity equals the single-rank one and SciPy's: the partitioned operator (halo exchanges of
    # B, Bt and of the lumped Mp inverse in the surrogate diagonal included) is the same operator
    u = np.concatenate([out[r]["x"][0] for r in range(world)])
    assert np.linalg.norm(u - x1[0]) <= 1e-6 * np.linalg.norm(x1[0])
    u_ref = _saddle_point_velocity(pb, rhs_zero_p(pb))
    assert np.linalg.norm(u - u_ref) <= 1e-6 * np.linalg.norm(u_ref)
    # rank-ordered dots change only rounding: the same lambda_max to rounding, the same outer count, and inner
    # CG solves to an absolute tolerance that may end a step apart in a few solves
    for r in range(world):
        assert np.array_equal(out[r]["hist"], out[0]["hist"])
        assert out[r]["res"].status == 0 and out[r]["res"].mp_iterations > 0
        assert out[r]["res"].lambda_max == pytest.approx(res.lambda_max, rel=1e-10)
        assert out[r]["res"].outer_iterations == res.outer_iterations
        assert abs(out[r]["res"].inner_iterations - res.inner_iterations) <= 0.01 * res.inner_iterations
        assert np.allclose(out[r]["hist"], h1, rtol=5e-2)
