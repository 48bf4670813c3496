"""The multigrid hierarchy of the immersed block (block 1: alfd_set_prolongator_block, alfd_build_smoothed_aggregation_block)
on the device, against tests/immersed_hierarchy_reference.py, the NumPy restatement -- the oracle has no block-1 hierarchy.
Configurations and tolerances come from tests/test_immersed_hierarchy.py, which measures them on the CPU.

  a. alfd_inner_prec_apply(A22) against the restatement        b. the same for the 2-block operator of the ideal variant
  c. 3 components, 3-D, odd immersed cell counts               d. symmetry of the dense operator
  e. the library's own smoothed-aggregation levels of block 1  f. a solve with and without the hierarchy, per-operator counts
  g. the ideal variant solves with both hierarchies            h. error paths
  i. the coarse tail in one launch ("ml_tail_rows") against the launch-per-step path, bit for bit"""
import ctypes as C
import threading

import numpy as np
import pytest
import scipy.sparse as sp

import cases
import immersed_hierarchy_reference as ihr
import test_immersed_hierarchy as base
import truncation_reference as tr
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver

pytestmark = pytest.mark.gpu


def _context(cf, immersed=True, cfg=None):
    cfg = _abi.Config.from_buffer_copy(cf.cfg if cfg is None else cfg)
    return solver.context_from_problem(cf.pb, cfg, aggregates=cf.levels0,
                                       immersed_levels=cf.levels1 if immersed else None)


def _vectors(name):
    cf = base.config(name)
    ref = cf.reference()
    ctx = _context(cf)
    try:
        for what, r in ihr.inputs(ref.n).items():
            err = ihr.rel(ctx.inner_prec_apply(r, cf.op), ref.apply(r))
            print(f"{name}, {what}: {err:.2e} (tolerance {ihr.tol(name):.2e})")
            assert err <= ihr.tol(name), (name, what, err)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["a22_multilevel", "a22_gmg"])
def test_a22_vcycle_against_the_restatement(built, name):
    """(a) 64 / 16, levels 289 / 81 / 25, the setting pairs of elliptic_modified_multilevel and elliptic_modified_gmg_patch."""
    _vectors(name)


@pytest.mark.parametrize("name", ["aug2_gmg_64", "aug2_gmg_patch_64"])
def test_ideal_block_diagonal_against_the_restatement(built, name):
    """(b) z = [ml_apply(r0); V1(r1)] of the ideal variant, block 0 without and with the interface patch."""
    _vectors(name)


def test_three_components_in_3d(built):
    """(c) elasticity3d(8) with 5 x 3 x 3 immersed cells: node-major components, trilinear transfers, odd cell counts."""
    _vectors("a22_elasticity")


def test_dense_operator_is_symmetric(built):
    """(d) every column of the library's V-cycle at 289 unknowns: symmetric within 64 times the restatement's asymmetry,
    and the operator itself within the tolerance of (a)."""
    cf = base.config("a22_gmg")
    ref = cf.reference()
    ctx = _context(cf)
    try:
        eye = np.eye(ref.n)
        m = np.stack([ctx.inner_prec_apply(eye[j], cf.op) for j in range(ref.n)], axis=1)
    finally:
        ctx.close()
    asym = ihr.asymmetry(m)
    print(f"asymmetry {asym:.2e} (allowed {ihr.sym_tol('a22_gmg'):.2e}); against the restatement {ihr.rel(m, ref.dense()):.2e}")
    assert asym <= ihr.sym_tol("a22_gmg")
    assert ihr.rel(m, ref.dense()) <= ihr.tol("a22_gmg")
    assert np.linalg.eigvalsh((m + m.T) / 2)[0] > 0.0


# ------------------------------------------------------------------------------------------ (e) the library's builder
def _restated_prolongator(aug, agg, nc, omega):
    """P_tent - omega D^-1 A22 P_tent in SciPy (rows with agg < 0 empty)."""
    rows = np.nonzero(agg >= 0)[0]
    Pt = sp.csr_matrix((np.ones(rows.size), (rows, agg[rows])), shape=(aug.shape[0], nc))
    keep = sp.diags((agg >= 0).astype(np.float64))
    return (keep @ (Pt - omega * (sp.diags(1.0 / aug.diagonal()) @ (aug @ Pt)))).tocsr()


def _row_rel(P, ref):
    diff = abs(P.to_scipy() - ref).tocsr()
    scale = abs(ref).max(axis=1).toarray().ravel()
    return float(np.max(diff.max(axis=1).toarray().ravel() / np.maximum(scale, 1e-300)))


@pytest.mark.parametrize("cap", [0, 4])
def test_smoothed_aggregation_of_block_1(built, cap):
    """(e) 128 / 32: every P_l of build_smoothed_aggregation(block=1) is P_tent - omega D^-1 A22_l P_tent formed in NumPy
    from the library's own aggregates (alfd_get_aggregates_block) and omega; with cap 4 the truncation of it."""
    cf = base.config("a22_gmg_32")
    pb, cfg = cf.pb, _abi.Config.from_buffer_copy(cf.cfg)
    ctx = solver.Context(0)
    try:
        ctx.set_matrix(_abi.A2, pb.mats["A2"])
        ctx.set_matrix(_abi.M, pb.mats["M"])
        ctx.set_diag(_abi.INVW, cf.inv_w())
        ctx.configure(cfg)
        kw = dict(block_size=1, threshold=0.02, max_aggregate_nodes=8)
        levels, omega = ctx.build_smoothed_aggregation(damping=4.0 / 3.0, min_coarse=30, return_omega=True,
                                                       max_row_entries=cap, block=1, **kw)
        aggs = [ctx.aggregates(level, block=1) for level in range(len(levels))]
        with pytest.raises(solver.AlfdError):          # block 0 of this context was never built
            ctx.prolongator(0, block=0)
        # the hierarchy stays in the context: the whole problem sets up and solves with it
        solver.upload_problem(ctx, pb, cfg, cf.levels0)
        x, res = ctx.solve(cases.rhs_of(pb))
        counts = ctx.inner_iterations()
    finally:
        ctx.close()
    assert len(levels) >= 2 and levels[0][0].nrows == pb.block_sizes[1]
    assert res.status == 0 and counts["a22"] > 0
    A2, M, w = pb.mats["A2"].to_scipy(), pb.mats["M"].to_scipy(), cf.inv_w()
    for level, (P, nc) in enumerate(levels):
        agg, nca = aggs[level]
        if level == 0:                               # the aggregation of alfd_build_aggregates, on A2 alone
            assert np.array_equal(agg, solver.host_aggregate_level(pb.mats["A2"], **kw)[0])
        assert nca == nc == P.ncols and P.nrows == A2.shape[0], level
        aug = (A2 + cfg.gamma2 * (M.T @ sp.diags(w) @ M)).tocsr()
        ref = _restated_prolongator(aug, agg, nc, omega[level])
        tol = 1e-14 if level == 0 else 1e-12
        if cap == 0:
            err = _row_rel(P, ref)
            print(f"level {level}: {P.nrows} -> {nc}, omega {omega[level]:.4f}, row-relative difference {err:.2e}")
            assert err <= tol, level
        else:
            assert int(np.diff(P.row_ptr).max()) <= cap
            tr.check_against_untruncated(P, ref, agg, 1, 0.0, cap, tol)
        Ps = P.to_scipy()
        A2 = (Ps.T @ (A2 @ Ps)).tocsr()
        M = (M @ Ps).tocsr()


# ------------------------------------------------------------------------------------------------------ (f), (g) solves
def _true_residual(ctx, rhs, x):
    ax = ctx.system_apply(x)
    return np.sqrt(sum(float(np.dot(p - q, p - q)) for p, q in zip(rhs, ax)))


def _solve_modified(immersed):
    cf = base.config("a22_gmg_jump")
    cfg = _abi.Config.from_buffer_copy(cf.cfg)
    cfg.inner = _abi.Control(_abi.CTRL_REDUCTION, 1000, 1e-30, 1e-8)     # counts must not hinge on the absolute tolerance
    ctx = _context(cf, immersed, cfg)
    try:
        rhs = cases.rhs_of(cf.pb)
        x, res = ctx.solve(rhs)
        return cfg, res, ctx.inner_iterations(), _true_residual(ctx, rhs, x), ctx.history()
    finally:
        ctx.close()


def test_solve_with_and_without_the_immersed_hierarchy(built):
    """(f) modified variant, 64 / 16, beta2 = 1e3, inner rule: reduce by 1e-8."""
    out = {}
    for immersed in (False, True):
        cfg, res, counts, r, hist = _solve_modified(immersed)
        print(f"hierarchy 1 {'on' if immersed else 'off'}: outer {res.outer_iterations}, inner {res.inner_iterations} "
              f"{counts}, true residual {r:.3e}")
        assert res.status == 0
        assert r <= 2 * max(cfg.outer.tol, cfg.outer.reduce * res.initial_residual)
        assert counts["aug"] > 0 and counts["a22"] > 0 and counts["aug2"] == 0
        assert counts["aug"] + counts["a22"] == res.inner_iterations
        out[immersed] = (res, counts)
    assert 2 * out[True][1]["a22"] <= out[False][1]["a22"]


def test_ideal_variant_solves_with_both_hierarchies(built):
    """(g) the 2x2 block CG of the ideal variant under the block-diagonal multilevel preconditioner; without the
    block-1 hierarchy ALFD_E_UNSUPPORTED as before."""
    cf = base.config("aug2_gmg_patch_64")
    cfg = _abi.Config.from_buffer_copy(cf.cfg)
    ctx = _context(cf)
    try:
        rhs = cases.rhs_of(cf.pb)
        x, res = ctx.solve(rhs)
        counts = ctx.inner_iterations()
        r = _true_residual(ctx, rhs, x)
        print(f"ideal: outer {res.outer_iterations}, inner {counts}, true residual {r:.3e}")
        assert res.status == 0 and r <= 2 * max(cfg.outer.tol, cfg.outer.reduce * res.initial_residual)
        assert counts["aug2"] == res.inner_iterations > 0 and counts["aug"] == counts["a22"] == 0
        ctx.clear_hierarchy(1)
        with pytest.raises(solver.AlfdError) as e:
            ctx.setup(cf.pb.block_sizes)
        assert e.value.status == _abi.E_UNSUPPORTED
        with pytest.raises(solver.AlfdError):
            ctx.prolongator(0, block=1)
    finally:
        ctx.close()
    with pytest.raises(solver.AlfdError) as e:
        _context(cf, immersed=False)
    assert e.value.status == _abi.E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------ (h) error paths
def test_error_paths(built):
    cf, small = base.config("a22_gmg"), base.config("a22_gmg_8")
    cfg = _abi.Config.from_buffer_copy(cf.cfg)
    P0 = cf.levels1[0][0]
    ctx = solver.Context(0)
    try:
        args = (P0.nrows, P0.ncols, P0.row_ptr.ctypes.data, P0.col.ctypes.data, P0.val.ctypes.data)
        for block in (2, -1):
            assert ctx._lib.alfd_set_prolongator_block(ctx._h, block, 0, *args) == _abi.E_INVALID
            assert ctx._lib.alfd_clear_hierarchy(ctx._h, block) == _abi.E_INVALID
        nlev = C.c_int32(0)
        assert ctx._lib.alfd_build_smoothed_aggregation_block(ctx._h, 1, 1, 0.02, 8, 4.0 / 3.0, 0.0, 0, 30, 7,
                                                              C.byref(nlev), None) == _abi.E_INVALID    # no slot A2
        # wrong sizes: the 81-row transfers of the 8^2-cell mesh on the 289 unknowns of the 16^2-cell one
        with pytest.raises(solver.AlfdError) as e:
            solver.upload_problem(ctx, cf.pb, cfg, cf.levels0, immersed_levels=small.levels1)
        assert e.value.status == _abi.E_INVALID
        # a second level that does not continue the first
        with pytest.raises(solver.AlfdError) as e:
            solver.upload_problem(ctx, cf.pb, cfg, cf.levels0, immersed_levels=[cf.levels1[0], cf.levels1[0]])
        assert e.value.status == _abi.E_INVALID
        # a singular coarsest operator: a zero column in the last prolongator
        P1 = cf.levels1[1][0]
        sing = problems.Csr(P1.nrows, P1.ncols, P1.row_ptr.copy(), P1.col.copy(), np.where(P1.col == 0, 0.0, P1.val))
        with pytest.raises(solver.AlfdError, match="positive definite"):
            solver.upload_problem(ctx, cf.pb, cfg, cf.levels0, immersed_levels=[cf.levels1[0], (sing, cf.levels1[1][1])])
        # the good hierarchy still sets up on the same context
        solver.upload_problem(ctx, cf.pb, cfg, cf.levels0, immersed_levels=cf.levels1)
        r = ihr.inputs(P0.nrows)["uniform(seed 11)"]
        assert ihr.rel(ctx.inner_prec_apply(r, _abi.INNER_OP_A22), cf.reference().apply(r)) <= ihr.tol("a22_gmg")
        # block 1 on a variant without A2
        pb2, cfg2 = cases.case("laplace3d_gmg_patch")
        with pytest.raises(solver.AlfdError) as e:
            solver.upload_problem(ctx, pb2, cfg2, cases.aggregates_of(pb2, cfg2))      # block 1 is still set
        assert e.value.status == _abi.E_INVALID
        ctx.clear_hierarchy(1)
        solver.upload_problem(ctx, pb2, cfg2, cases.aggregates_of(pb2, cfg2))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------- (i) the coarse tail in one launch
TAIL_ROWS = (0, 32, 128, 4096)


def _launches(ctx, work):
    ctx.enable_timing(2)
    work()
    n = sum(v["launches"] for v in ctx.timing().values())
    ctx.enable_timing(0)
    return n


@pytest.mark.parametrize("name, direct", [("a22_multilevel", None), ("a22_gmg", None), ("a22_gmg_8", None), ("a22_gmg_8", 0)])
def test_tail_vectors_bit_for_bit(built, name, direct):
    """(i) z of (a) with ml_tail_rows 0 / 32 / 128 / 4096 on ONE context: 64 / 16 with both setting pairs (Chebyshev and
    explicit coarsest step) and 32 / 8 (81 -> 25: the tail is the coarsest level alone; with the explicit inverse and,
    direct = 0, with the Chebyshev coarsest sweep).  Same bits for every value; fewer timed launches with the tail on --
    except where the tail is the single product with the explicit inverse (one launch for one launch: equal)."""
    cf = base.config(name)
    cfg = _abi.Config.from_buffer_copy(cf.cfg)
    if direct is not None:
        cfg.ml_coarse_direct = direct
    sizes = [cf.pb.block_sizes[1]] + [int(nc) for _, nc in cf.levels1]
    ctx = _context(cf, cfg=cfg)
    try:
        z, launches = {}, {}
        for rows in TAIL_ROWS:
            ctx.set_tunable("ml_tail_rows", rows)
            z[rows] = [ctx.inner_prec_apply(r, cf.op) for r in ihr.inputs(sizes[0]).values()]
            launches[rows] = _launches(ctx, lambda: ctx.inner_prec_apply(np.ones(sizes[0]), cf.op))
        with pytest.raises(solver.AlfdError):
            ctx.set_tunable("ml_tail_rows", -1)
    finally:
        ctx.close()
    print(f"{name} (levels {sizes}, ml_coarse_direct {cfg.ml_coarse_direct}): timed launches {launches}")
    for rows in TAIL_ROWS[1:]:
        for a, b in zip(z[rows], z[0]):
            assert np.array_equal(a, b), (name, rows)
        tail_levels = [n for n in sizes[1:] if n <= rows]
        assert tail_levels, (name, rows)
        if len(tail_levels) == 1 and cfg.ml_coarse_direct >= tail_levels[0]:
            assert launches[rows] == launches[0], (name, rows, launches)
        else:
            assert launches[rows] < launches[0], (name, rows, launches)


@pytest.mark.parametrize("name", ["a22_gmg_jump", "a22_gmg_8"])
def test_tail_solve_bit_for_bit(built, name):
    """(i) the solve of (f) (64 / 16, beta2 = 1e3, inner rule: reduce by 1e-8) and the same at 32 / 8 with every
    ml_tail_rows: the whole residual history and the solution are the same bits, the counts with them."""
    cf = base.config(name)
    cfg = _abi.Config.from_buffer_copy(cf.cfg)
    cfg.inner = _abi.Control(_abi.CTRL_REDUCTION, 1000, 1e-30, 1e-8)
    ctx = _context(cf, cfg=cfg)
    try:
        rhs = cases.rhs_of(cf.pb)
        out = {}
        for rows in TAIL_ROWS:
            ctx.set_tunable("ml_tail_rows", rows)
            x, res = ctx.solve(rhs)
            out[rows] = (x, ctx.history(), res.outer_iterations, ctx.inner_iterations(), res.status)
    finally:
        ctx.close()
    x0, h0, outer0, counts0, status0 = out[0]
    assert status0 == 0 and counts0["a22"] > 0
    for rows in TAIL_ROWS[1:]:
        x, h, outer, counts, status = out[rows]
        assert status == 0 and outer == outer0 and counts == counts0, (rows, counts, counts0)
        assert np.array_equal(h, h0), rows
        assert all(np.array_equal(a, b) for a, b in zip(x, x0)), rows


def test_partitioned_context_is_unsupported(built):
    P0 = base.config("a22_gmg").levels1[0][0]
    group = solver.LocalGroup(2)
    rcs, errs = [None, None], []

    def work(rank):
        try:
            ctx = solver.Context(0)
            ctx.comm_init_local(group.handle, rank)
            rcs[rank] = ctx._lib.alfd_set_prolongator_block(ctx._h, 1, 0, P0.nrows, P0.ncols, P0.row_ptr.ctypes.data,
                                                            P0.col.ctypes.data, P0.val.ctypes.data)
            ctx.close()
        except Exception as e:   # noqa: BLE001
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    group.close()
    assert not errs, errs
    assert rcs == [_abi.E_UNSUPPORTED, _abi.E_UNSUPPORTED]
