"""alfd_setup_coupling: the re-setup after a change of the coupling alone (the immersed body moved over a fixed background
mesh, or a new penalty weight) against the only reference there is for it, a FRESH context -- alfd_create, every upload,
alfd_setup -- holding the same operators, prolongators and config.  "Equal" is np.array_equal on the solution blocks,
the residual history, the outer / inner / Mp / mass counts and on alfd_inner_prec_apply of a fixed pseudo-random vector
for every inner operator of the variant.  What ran is read from alfd_get_setup_counts, nothing is timed.

  1. Stokes N = 8, tensor prolongators, patch, direct coarsest solve: c0 -> c1 -> c0 (S grows and shrinks), the oracle
  2. no patch + Chebyshev coarsest sweep; no hierarchy at all       3. gamma alone
  4. both hierarchies of the elliptic modified variant; gamma2 alone 5. exact W^-1 (M uploaded again, mass counts)
  6. frozen smoothed-aggregation transfers                           7. nothing changed; ten updates do not grow
  8. the refusals, each followed by alfd_setup and a correct solve; a gamma / gamma2 that alfd_setup refuses"""
import threading

import numpy as np
import pytest

import cases
import test_immersed_hierarchy as base
from fictitious_domain_al_preconditioners_amd import _abi, partition, problems, solver

pytestmark = pytest.mark.gpu

C0, C1 = (0.5, 0.5, 0.5), (0.56, 0.47, 0.52)


def _stokes3d(n, refine, center):
    """problems.stokes3d_sphere with the body somewhere else"""
    return problems.generate(dim=3, degree=2, ncomp=3, n_cells=n, stokes=True, grad_div=True, gamma_grad_div=10.0,
                             center=center, radius=0.1, immersed_refine=refine, coupling_nq=4,
                             body_force=(1.0, 0.0, 0.0), embedded_value=(-1.0, 1.0, 0.0))


def _stokes2d(center):
    """problems.stokes2d_circle(16, 3), likewise"""
    return problems.generate(dim=2, degree=2, ncomp=2, n_cells=16, stokes=True, grad_div=True, gamma_grad_div=10.0,
                             center=center, radius=0.2, immersed_refine=3, coupling_nq=3, body_force=(1.0, 0.0),
                             embedded_value=(-1.0, 1.0))


def _same_matrix(a, b):
    return (a.nrows, a.ncols) == (b.nrows, b.ncols) and np.array_equal(a.row_ptr, b.row_ptr) and \
        np.array_equal(a.col, b.col) and np.array_equal(a.val, b.val)


def _copy(cfg):
    return _abi.Config.from_buffer_copy(cfg)


@pytest.fixture(scope="module")
def stokes():
    """The two body positions at N = 8: the background operators are the same bits, the coupling is not"""
    pb0, pb1 = _stokes3d(8, 1, C0), _stokes3d(8, 1, C1)
    for name in ("A", "B", "Bt", "Mp"):
        assert _same_matrix(pb0.mats[name], pb1.mats[name]), name
    assert pb0.block_sizes == pb1.block_sizes == [14739, 729, 78]
    assert pb0.mats["Ct"].nnz != pb1.mats["Ct"].nnz
    rows = [int(np.count_nonzero(np.diff(p.mats["Ct"].row_ptr))) for p in (pb0, pb1)]
    assert rows[0] != rows[1], rows                      # |S|: the patch changes size
    return pb0, pb1


def _ops(cfg):
    if cfg.variant == _abi.AL_ELL_MODIFIED:
        return [_abi.INNER_OP_AUG, _abi.INNER_OP_A22]
    if cfg.variant == _abi.AL_ELL_IDEAL:
        return [_abi.INNER_OP_AUG2]
    return [_abi.INNER_OP_AUG]


def _rhs(ctx, pb, cfg):
    rhs = cases.rhs_of(pb)
    return ctx.augment_rhs(rhs) if cfg.variant in (_abi.AL2, _abi.AL_STOKES, _abi.AL_STOKES_DIAG) else rhs


def _snapshot(ctx, pb, cfg):
    """Everything the contract names: solution, history, counts, one application of every inner preconditioner, of the
    outer preconditioner and of the system; and the condition estimate of C Ct"""
    bs = ctx.block_sizes
    prec = {}
    for op in _ops(cfg):
        n = {_abi.INNER_OP_AUG: bs[0], _abi.INNER_OP_A22: bs[1]}.get(op, bs[0] + bs[1])
        prec[op] = ctx.inner_prec_apply(np.random.default_rng(11 + op).uniform(-1.0, 1.0, n), op)
    src = cases.rng_blocks(pb, 5)
    x, res = ctx.solve(_rhs(ctx, pb, cfg))
    spectrum = ctx.estimate_spectrum().as_dict()         # its compacted C[:,S], Ct[S,:] follow the coupling too
    return dict(x=x, hist=ctx.history(), prec=prec, pv=ctx.precond_apply(src)[0], sv=ctx.system_apply(src), spectrum=spectrum,
                counts=(res.status, res.outer_iterations, res.inner_iterations, res.mp_iterations, res.mass_iterations))


def _assert_equal(got, ref):
    assert got["counts"] == ref["counts"]
    assert ref["counts"][0] == 0
    assert np.array_equal(got["hist"], ref["hist"])
    for what in ("x", "pv", "sv"):
        for b, (g, r) in enumerate(zip(got[what], ref[what])):
            assert np.array_equal(g, r), (what, b, float(np.abs(g - r).max()))
    for op in ref["prec"]:
        assert np.array_equal(got["prec"][op], ref["prec"][op]), op
    assert got["spectrum"] == ref["spectrum"] and ref["spectrum"]["steps"] > 0


def _fresh(pb, cfg, levels, immersed_levels=None):
    ctx = solver.context_from_problem(pb, _copy(cfg), aggregates=levels, immersed_levels=immersed_levels)
    try:
        return _snapshot(ctx, pb, cfg)
    finally:
        ctx.close()


def _move(ctx, pb, M=True):
    """the uploads of a moved body: CT (and its transpose), INVW and M, then alfd_setup_coupling"""
    return solver.update_coupling(ctx, pb.mats["Ct"], inv_w=pb.inv_w_diag_squared(), M=pb.mats["M"] if M else None,
                                  C=pb.mats["C"])


def _upload_stokes(ctx, pb):
    """the uploads of solver.upload_problem for a Stokes problem, without hierarchy, configure and setup"""
    ctx.set_matrix(_abi.A, pb.mats["A"])
    ctx.set_matrix(_abi.C_, pb.mats["C"])
    ctx.set_matrix(_abi.CT, pb.mats["Ct"])
    ctx.set_diag(_abi.INVW, pb.inv_w_diag_squared())
    ctx.set_matrix(_abi.B, pb.mats["B"])
    ctx.set_matrix(_abi.BT, pb.mats["Bt"])
    ctx.set_matrix(_abi.MP, pb.mats["Mp"])
    ctx.set_diag(_abi.MP_LUMPED_INV, pb.mp_lumped_inv())


def _counts(ctx, **expected):
    k = ctx.setup_counts()
    print(k)
    for name, v in expected.items():
        assert k[name] == v, (name, k)
    return k


# --------------------------------------------------------------------------------------------------------------- 1
def test_moved_body_and_back_equals_fresh_contexts_and_the_oracle(built, stokes):
    pb0, pb1 = stokes
    _, cfg = cases.case("stokes3d_gmg_patch")
    levels = cases.aggregates_of(pb0, cfg)
    nlev = len(levels)
    assert nlev >= 2
    fresh1 = _fresh(pb1, cfg, levels)
    ctx = solver.context_from_problem(pb0, _copy(cfg), aggregates=levels)
    try:
        full = _counts(ctx, products_a=2 * nlev, products_c=nlev, level_a_uploads=nlev, transfer_uploads=2 * nlev,
                       patch_builds=1)
        first = _snapshot(ctx, pb0, cfg)
        update = dict(products_a=0, level_a_uploads=0, transfer_uploads=0, products_c=nlev, patch_builds=1,
                      power_iterations=full["power_iterations"])
        _move(ctx, pb1)
        _counts(ctx, **update)
        moved = _snapshot(ctx, pb1, cfg)
        _assert_equal(moved, fresh1)
        # the oracle set up on c1, as tests/test_gpu_parity.py compares this case
        osys = cases.oracle_system(pb1, cfg)
        rc, ox, ores, ohist = osys.solve(cfg, cases.prepared_rhs(osys, pb1, cfg))
        assert rc == 0
        assert moved["counts"] == (0, ores.outer_iterations, ores.inner_iterations, ores.mp_iterations, ores.mass_iterations)
        assert len(moved["hist"]) == len(ohist)
        print("history against the oracle: max rel deviation", float(np.max(np.abs(moved["hist"] - ohist) / np.abs(ohist))))
        assert np.array_equal(moved["hist"], ohist)
        for g, r in zip(moved["x"], ox):                     # the solution as tests/test_gpu_parity.py compares it
            assert np.allclose(g, r, rtol=1e-9, atol=1e-10 * max(np.abs(r).max(), 1e-30))
        _move(ctx, pb0)
        _counts(ctx, **update)
        _assert_equal(_snapshot(ctx, pb0, cfg), first)       # S shrank again, nothing of c1 is left
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("kind", ["gmg_chebyshev_coarse", "chebyshev"])
def test_without_patch_and_without_hierarchy(built, stokes, kind):
    pb0, pb1 = stokes
    if kind == "chebyshev":                                  # no hierarchy: the diagonal and lambda_max alone
        cfg = _abi.default_config(_abi.AL_STOKES)
        cfg.inner.max_steps = 1000
        levels = None
    else:
        _, cfg = cases.case("stokes3d_gmg")                  # ml_patch_degree = 0, Chebyshev sweep on the coarsest level
        levels = cases.aggregates_of(pb0, cfg)
    ctx = solver.context_from_problem(pb0, _copy(cfg), aggregates=levels)
    try:
        _move(ctx, pb1)
        _counts(ctx, products_a=0, level_a_uploads=0, transfer_uploads=0, patch_builds=0,
                products_c=len(levels) if levels else 0, power_iterations=1 + (len(levels) if levels else 0))
        _assert_equal(_snapshot(ctx, pb1, cfg), _fresh(pb1, cfg, levels))
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------------------------------- 3
def test_gamma_alone(built, stokes):
    pb0, _ = stokes
    _, cfg = cases.case("stokes3d_gmg_patch")
    levels = cases.aggregates_of(pb0, cfg)
    assert cfg.gamma == 10.0
    cfg25 = _copy(cfg)
    cfg25.gamma = 25.0
    fresh25 = _fresh(pb0, cfg25, levels)
    ctx = solver.context_from_problem(pb0, _copy(cfg), aggregates=levels)
    try:
        ctx.configure(_copy(cfg25))
        ctx.setup_coupling()
        _counts(ctx, products_a=0, products_c=0, level_a_uploads=0, transfer_uploads=0, patch_builds=1)
        _assert_equal(_snapshot(ctx, pb0, cfg25), fresh25)
    finally:
        ctx.close()
    # the same sweep through the helper: no upload, the config it was handed stays as it was
    mine = _copy(cfg)
    ctx = solver.context_from_problem(pb0, mine, aggregates=levels)
    try:
        assert solver.update_coupling(ctx, None, gamma=25.0) is ctx
        assert mine.gamma == 10.0 and ctx.cfg.gamma == 25.0
        _counts(ctx, products_a=0, products_c=0, level_a_uploads=0, transfer_uploads=0, patch_builds=1)
        _assert_equal(_snapshot(ctx, pb0, cfg25), fresh25)
        with pytest.raises(ValueError):
            solver.update_coupling(ctx, None, C=pb0.mats["C"])
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------------------------------- 4
def test_elliptic_both_hierarchies_and_gamma2_alone(built):
    """The box moves from (-0.14, 0.47) to (-0.20, 0.41): A stays, A2 / M / K move in the last bits, so the updated and the
    comparison context both hold Ct, C (and g) of the moved problem and everything else of the original."""
    pb0, cfg = cases.case("elliptic_modified_gmg_patch")
    pbm = problems.generate(dim=2, degree=1, ncomp=1, n_cells=64, lo=-1.0, hi=1.0, beta=1.0, coupling_nq=3,
                            body_force=(1.0,), embedded_value=(0.0,), immersed_box=(-0.20, 0.41, 16), beta2=9.0)
    assert _same_matrix(pb0.mats["A"], pbm.mats["A"]) and not _same_matrix(pb0.mats["Ct"], pbm.mats["Ct"])
    comp = problems.SyntheticProblem(params=pb0.params, mats=dict(pb0.mats, Ct=pbm.mats["Ct"], C=pbm.mats["C"]),
                                     vecs=dict(pb0.vecs, g=pbm.vecs["g"]))
    levels0 = cases.aggregates_of(pb0, cfg)
    levels1 = problems.immersed_tensor_prolongators(pb0.params, min_coarse=base.IMM_MIN_COARSE)
    n0, n1 = len(levels0), len(levels1)
    assert n0 >= 1 and n1 >= 1
    ctx = solver.context_from_problem(pb0, _copy(cfg), aggregates=levels0, immersed_levels=levels1)
    try:
        _counts(ctx, products_a=2 * (n0 + n1), products_c=n0 + n1, level_a_uploads=n0 + n1)
        solver.update_coupling(ctx, comp.mats["Ct"], C=comp.mats["C"])
        # block 1 is not touched: the products are hierarchy 0's, the power iterations those of the two inner operators,
        # of hierarchy 0's levels and of the patch
        _counts(ctx, products_a=0, level_a_uploads=0, transfer_uploads=0, products_c=n0, patch_builds=1,
                power_iterations=2 + n0 + 1)
        _assert_equal(_snapshot(ctx, comp, cfg), _fresh(comp, cfg, levels0, levels1))
        # gamma2 alone: the penalty parts of hierarchy 1 (and of hierarchy 0) again, no product of any kind
        cfg2 = _copy(cfg)
        cfg2.gamma2 = 2e-2
        ctx.configure(_copy(cfg2))
        ctx.setup_coupling()
        _counts(ctx, products_a=0, level_a_uploads=0, transfer_uploads=0, products_c=0, power_iterations=2 + n0 + 1 + n1)
        _assert_equal(_snapshot(ctx, comp, cfg2), _fresh(comp, cfg2, levels0, levels1))
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------------------------------- 5
def test_exact_w_inverse_with_a_new_mass_matrix(built):
    _, cfg = cases.case("stokes2d_exact_w")
    pb0, pb1 = _stokes2d((0.5, 0.5, 0.0)), _stokes2d((0.53, 0.48, 0.0))
    for name in ("A", "B", "Bt", "Mp"):
        assert _same_matrix(pb0.mats[name], pb1.mats[name]), name
    assert pb0.block_sizes == pb1.block_sizes and not _same_matrix(pb0.mats["Ct"], pb1.mats["Ct"])
    ctx = solver.context_from_problem(pb0, _copy(cfg))
    try:
        _move(ctx, pb1)
        got, ref = _snapshot(ctx, pb1, cfg), _fresh(pb1, cfg, None)
        assert ref["counts"][4] > 0                          # the mass solves ran
        _assert_equal(got, ref)
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------------------------------- 6
def test_frozen_smoothed_aggregation_transfers(built):
    """The P built with the coupling of c0 stay; the comparison context is handed the same P (alfd_get_prolongator ->
    alfd_set_prolongator) on the moved operators."""
    pb0, pb1 = _stokes3d(6, 0, C0), _stokes3d(6, 0, C1)
    assert _same_matrix(pb0.mats["A"], pb1.mats["A"]) and pb0.block_sizes == pb1.block_sizes
    assert not _same_matrix(pb0.mats["Ct"], pb1.mats["Ct"])
    cfg = _abi.default_config(_abi.AL_STOKES)
    cfg.inner.max_steps = 100
    cfg.inner_prec = _abi.PREC_MULTILEVEL
    cfg.ml_smooth_degree, cfg.ml_smooth_ratio, cfg.ml_coarse_degree = 4, 256.0, 10

    ctx = solver.Context(0)
    try:
        _upload_stokes(ctx, pb0)
        ctx.configure(_copy(cfg))
        levels = ctx.build_smoothed_aggregation(block_size=3, threshold=0.02, min_coarse=60, drop_tolerance=0.0,
                                                max_row_entries=4)
        print("levels", [nc for _, nc in levels])
        assert len(levels) >= 1
        ctx.setup(pb0.block_sizes)
        _move(ctx, pb1)
        _counts(ctx, products_a=0, level_a_uploads=0, transfer_uploads=0, products_c=len(levels))
        _assert_equal(_snapshot(ctx, pb1, cfg), _fresh(pb1, cfg, levels))
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------------------------------- 7
def test_nothing_changed_and_ten_updates_do_not_grow(built, stokes):
    pb0, pb1 = stokes
    _, cfg = cases.case("stokes3d_gmg_patch")
    levels = cases.aggregates_of(pb0, cfg)
    ctx = solver.context_from_problem(pb0, _copy(cfg), aggregates=levels)
    try:
        first = _snapshot(ctx, pb0, cfg)
        ctx.setup_coupling()                                 # nothing uploaded, nothing configured
        _counts(ctx, products_a=0, products_c=0, level_a_uploads=0, transfer_uploads=0, patch_builds=1)
        _assert_equal(_snapshot(ctx, pb0, cfg), first)
        free = {}
        for k in range(1, 11):
            _move(ctx, pb1 if k % 2 else pb0)
            free[k] = ctx.device_memory()[0]
        print("free device bytes after each update:", free)
        assert [free[k] for k in (4, 6, 8, 10)] == [free[2]] * 4, free
        _assert_equal(_snapshot(ctx, pb0, cfg), first)
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------------------------------- 8
def _refused(ctx, status, needs_setup):
    with pytest.raises(solver.AlfdError) as e:
        ctx.setup_coupling()
    assert e.value.status == status, str(e.value)
    if needs_setup:
        assert "needs alfd_setup" in str(e.value), str(e.value)
    return str(e.value)


def test_refusals_that_need_alfd_setup(built, stokes):
    pb0, _ = stokes
    _, cfg = cases.case("stokes3d_gmg_patch")
    levels = cases.aggregates_of(pb0, cfg)
    ref = _fresh(pb0, cfg, levels)

    def recover():
        ctx.setup(pb0.block_sizes)
        _assert_equal(_snapshot(ctx, pb0, cfg), ref)
        ctx.setup_coupling()                                 # and the context takes updates again

    ctx = solver.Context(0)
    try:
        # never set up: everything is uploaded and configured, alfd_setup has not run
        _upload_stokes(ctx, pb0)
        for level, (P, _) in enumerate(levels):
            ctx.set_prolongator(level, P)
        ctx.configure(_copy(cfg))
        assert "alfd_setup" in _refused(ctx, _abi.E_NOT_SETUP, False)
        recover()
        # A uploaded again
        ctx.set_matrix(_abi.A, pb0.mats["A"])
        _refused(ctx, _abi.E_INVALID, True)
        recover()
        # a prolongator set again
        ctx.set_prolongator(len(levels) - 1, levels[-1][0])
        _refused(ctx, _abi.E_INVALID, True)
        recover()
        # CT with another column count (one more multiplier, coupled to nothing)
        ct, c = pb0.mats["Ct"], pb0.mats["C"]
        ctx.set_matrix(_abi.C_, problems.Csr(c.nrows + 1, c.ncols, np.append(c.row_ptr, c.row_ptr[-1]), c.col, c.val))
        ctx.set_matrix(_abi.CT, problems.Csr(ct.nrows, ct.ncols + 1, ct.row_ptr, ct.col, ct.val))
        _refused(ctx, _abi.E_INVALID, True)
        ctx.set_matrix(_abi.C_, c)
        ctx.set_matrix(_abi.CT, ct)
        recover()
        # a config that differs in ml_smooth_degree
        other = _copy(cfg)
        other.ml_smooth_degree += 1
        ctx.configure(other)
        _refused(ctx, _abi.E_INVALID, True)
        ctx.configure(_copy(cfg))
        recover()
    finally:
        ctx.close()


@pytest.mark.parametrize("name,status", [("laplace2d_operator_form_gmg_patch", _abi.E_INVALID),
                                         ("rational_minres", _abi.E_UNSUPPORTED),
                                         ("stokes3d_multilevel", _abi.E_UNSUPPORTED)])
def test_refusals_by_kind_of_context(built, name, status):
    """aug_assembled = 1 keeps the coupling inside A; the rational variant and a hierarchy given as aggregates keep using
    alfd_setup"""
    pb, cfg = cases.case(name)
    ctx = solver.context_from_problem(pb, _copy(cfg), aggregates=cases.aggregates_of(pb, cfg))
    try:
        x, res = ctx.solve(_rhs(ctx, pb, cfg))
        hist = ctx.history()
        _refused(ctx, status, status == _abi.E_INVALID)
        x2, res2 = ctx.solve(_rhs(ctx, pb, cfg))                 # the context is as before the call: still set up
        assert np.array_equal(ctx.history(), hist)
        ctx.setup(pb.block_sizes)
        x3, res3 = ctx.solve(_rhs(ctx, pb, cfg))
        assert res3.status == 0 and np.array_equal(ctx.history(), hist)
        for a, b in zip(x, x3):
            assert np.array_equal(a, b)
    finally:
        ctx.close()


@pytest.mark.parametrize("name,field,value", [("elliptic_ideal", "gamma", 12.0), ("elliptic_modified", "gamma2", 25.0)])
def test_penalty_weights_that_alfd_setup_refuses_are_refused(built, name, field, value):
    """The checks alfd_setup makes on gamma / gamma2 (ideal variant: gamma == gamma2; modified: gamma2 <= 20 and not within
    0.1 of gamma) hold for the update too: same status, same message, nothing modified."""
    pb, cfg = cases.case(name)
    bad = _copy(cfg)
    setattr(bad, field, value)
    ctx = solver.context_from_problem(pb, _copy(cfg))
    try:
        _, res = ctx.solve(_rhs(ctx, pb, cfg))
        hist = ctx.history()
        assert res.status == 0
        ctx.configure(_copy(bad))
        message = _refused(ctx, _abi.E_INVALID, False)
        # nothing was modified: with the old weights back the context takes an update at once
        ctx.configure(_copy(cfg))
        ctx.setup_coupling()
        ctx.solve(_rhs(ctx, pb, cfg))
        assert np.array_equal(ctx.history(), hist)
        # alfd_setup gives the same answer to the same config, and sets the legal one up
        ctx.configure(_copy(bad))
        with pytest.raises(solver.AlfdError) as e:
            ctx.setup(pb.block_sizes)
        assert e.value.status == _abi.E_INVALID and str(e.value) == message
        ctx.configure(_copy(cfg))
        ctx.setup(pb.block_sizes)
        ctx.solve(_rhs(ctx, pb, cfg))
        assert np.array_equal(ctx.history(), hist)
    finally:
        ctx.close()


def test_partitioned_context_is_refused_on_every_rank(built):
    """Two ranks in one process: both get ALFD_E_UNSUPPORTED without an exchange (a rank that waited for its peer would
    hang the other's following collective setup), then set up and solve again."""
    world, n = 2, 8
    cfg = _abi.default_config(_abi.AL_STOKES)
    cfg.inner.max_steps = 1000
    plan = partition.slab_partition_stokes3d(n, 0, world)
    group = solver.LocalGroup(world)
    out, errs = [None] * world, []

    def work(rank):
        try:
            pb = problems.stokes3d_sphere(n, 0, row_ranges=plan.generator_ranges(rank))
            ctx = solver.Context(0)
            ctx.comm_init_local(group.handle, rank)
            ctx.set_partition(plan.offsets)
            solver.upload_problem(ctx, pb, _copy(cfg))
            rhs = ctx.augment_rhs(cases.rhs_of(pb))
            ctx.solve(rhs)
            hist = ctx.history()
            if rank == 0:                                    # rank 1 does not call at all before the collective setup below
                with pytest.raises(solver.AlfdError) as e:
                    ctx.setup_coupling()
                status = e.value.status
            ctx.setup(pb.block_sizes)
            if rank == 1:
                with pytest.raises(solver.AlfdError) as e:
                    ctx.setup_coupling()
                status = e.value.status
            _, res = ctx.solve(rhs)
            out[rank] = (status, res.status, np.array_equal(ctx.history(), hist))
            ctx.close()
        except BaseException as e:   # noqa: BLE001
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    group.close()
    assert not errs, errs
    assert out == [(_abi.E_UNSUPPORTED, 0, True)] * world, out
