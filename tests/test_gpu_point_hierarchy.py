"""alfd_build_geometric_from_points on the device context: the hierarchy the library builds from support points against
the same hierarchy handed over level by level through alfd_set_prolongator[_block] (problems.tensor_prolongators,
refined_prolongators, immersed_tensor_prolongators).  "Equal" is bit for bit: every alfd_get_prolongator level, the
solution blocks, the residual history, every iteration count and the applications of the preconditioners
(test_gpu_setup_coupling's snapshot).

  1. stokes3d_gmg_patch (N = 8), constrained = None (the lone diagonals of the resident A); tests/golden/solves.json
  2. the same on a Cuthill-McKee-permuted problem under set_numbering_from_points, against the hand-permuted route
  3. the locally refined (6, 1) sphere with base = 6             4. both blocks of elliptic_modified_gmg_patch at 32 / 8
  5. build, alfd_setup, a new CT, alfd_setup_coupling             6. the refusals, each followed by a correct solve
  7. replay.py --inner-prec gmg on a dumped system"""
import json
import os
import threading

import numpy as np
import pytest

import cases
import refined_cases as rc
import test_gpu_setup_coupling as sc
import test_immersed_hierarchy as base
from fictitious_domain_al_preconditioners_amd import _abi, partition, problems, solver

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HIST_RTOL = 1e-10          # as tests/test_gpu_parity.py compares a GPU history with the golden one


def _same_levels(ctx, levels, block=0):
    for level, (P, n_coarse) in enumerate(levels):
        got = ctx.prolongator(level, block)
        assert got.ncols == n_coarse and sc._same_matrix(got, P), (block, level)
        assert got.val.tobytes() == P.val.tobytes(), (block, level)
    with pytest.raises(solver.AlfdError):                    # and no level beyond
        ctx.prolongator(len(levels), block)


def _snapshot_of(pb, cfg, **kw):
    ctx = solver.context_from_problem(pb, sc._copy(cfg), **kw)
    try:
        return sc._snapshot(ctx, pb, cfg)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def stokes(built):
    """stokes3d_gmg_patch with its hand-set hierarchy: the reference of tests 1, 5 and 6, computed once, read-only"""
    pb, cfg = cases.case("stokes3d_gmg_patch")
    levels = problems.tensor_prolongators(pb.params, min_coarse=100)
    return pb, cfg, levels, _snapshot_of(pb, cfg, aggregates=levels)


# --------------------------------------------------------------------------------------------------------------- 1
def test_stokes_gmg_patch_from_points_equals_set_prolongator_and_golden(stokes):
    pb, cfg, levels, ref = stokes
    ctx = solver.context_from_problem(pb, sc._copy(cfg), hierarchy_from_points=dict(
        points=problems.row_support_points(pb), min_coarse=100))
    try:
        _same_levels(ctx, levels)
        got = sc._snapshot(ctx, pb, cfg)
    finally:
        ctx.close()
    sc._assert_equal(got, ref)
    gold = json.load(open(os.path.join(GOLDEN, "solves.json")))["stokes3d_gmg_patch"]
    status, outer, inner, mp, _ = got["counts"]
    assert (status, outer, inner, mp) == (0, gold["outer_iterations"], gold["inner_iterations"], gold["mp_iterations"])
    ghist = np.array([float.fromhex(h) for h in gold["history"]])
    assert len(got["hist"]) == len(ghist) and np.max(np.abs(got["hist"] - ghist) / np.abs(ghist)) <= HIST_RTOL
    # the solution against the golden block norms: tests/test_gpu_parity.py admits |x - x_oracle| <= 1e-9 |x_oracle| +
    # 1e-10 max|x_oracle| per entry, and a norm moves by at most the norm of the difference (max|x| <= ||x||)
    for b, norm_hex in zip(got["x"], gold["x_block_norms"]):
        norm = float.fromhex(norm_hex)
        assert abs(float(np.sqrt((b * b).sum())) - norm) <= (1e-9 + 1e-10 * np.sqrt(b.size)) * norm


# --------------------------------------------------------------------------------------------------------------- 2
def _hand_permuted(pb, n2o, levels):
    """problem and level-0 transfer in the new numbering, by solver.permute_csr and numpy (tests/numbering_worker.py)"""
    o2n = np.empty_like(n2o)
    o2n[n2o] = np.arange(n2o.size)
    mats = dict(pb.mats)
    mats["A"] = solver.permute_csr(pb.mats["A"], n2o, o2n)
    for rows, cols in (("Ct", "C"), ("Bt", "B")):
        mats[rows] = solver.permute_csr(pb.mats[rows], n2o, None)
        mats[cols] = solver.permute_csr(pb.mats[cols], None, o2n)
    vecs = dict(pb.vecs)
    vecs["f"] = np.ascontiguousarray(pb.vecs["f"][n2o])
    out = problems.SyntheticProblem(params=dict(pb.params), mats=mats, vecs=vecs)
    out.inv_w_override = pb.inv_w_override
    return out, [(solver.permute_csr(levels[0][0], n2o, None), levels[0][1])] + list(levels[1:])


def test_cuthill_mckee_under_numbering_from_points_equals_the_hand_permuted_route(built):
    pb, cfg = cases.case("stokes3d_gmg_patch")
    problems.permute_background_nodes(pb, problems.cuthill_mckee_nodes(pb))
    pts = problems.row_support_points(pb)
    levels = problems.tensor_prolongators(pb.params, min_coarse=100, node_permutation=pb.node_permutation)
    n2o = solver.numbering_from_points(pts)
    pbh, levels_h = _hand_permuted(pb, n2o, levels)
    ctx = solver.context_from_problem(pb, sc._copy(cfg), numbering=pts,
                                      hierarchy_from_points=dict(points=pts, min_coarse=100))
    ref = solver.context_from_problem(pbh, sc._copy(cfg), aggregates=levels_h,
                                      row_blocks=solver.brick_blocks_from_points(pts[n2o], (16, 4, 1)))
    try:
        assert np.array_equal(ctx.numbering(), n2o)
        _same_levels(ctx, levels)                            # in the caller's numbering, as they would have been set
        _same_levels(ref, levels_h)
        rhs_h = ref.augment_rhs(cases.rhs_of(pbh))
        rhs = ctx.augment_rhs(cases.rhs_of(pb))
        assert np.array_equal(rhs[0][n2o], rhs_h[0])
        x_h, res_h = ref.solve(rhs_h)
        hist_h = ref.history()
        x, res = ctx.solve(rhs)
        assert (res.status, res.outer_iterations, res.inner_iterations, res.mp_iterations) == \
            (0, res_h.outer_iterations, res_h.inner_iterations, res_h.mp_iterations)
        assert np.array_equal(ctx.history(), hist_h)
        assert np.array_equal(x[0][n2o], x_h[0]) and all(np.array_equal(a, b) for a, b in zip(x[1:], x_h[1:]))
    finally:
        ctx.close()
        ref.close()


# --------------------------------------------------------------------------------------------------------------- 3
def test_refined_sphere_with_base_grid(built):
    name = "stokes3d_sphere"
    pb, cfg = rc.problem(name), rc.config(name, "multilevel")
    levels = problems.refined_prolongators(pb, min_coarse=100, q1_level=False)
    ref = _snapshot_of(pb, cfg, aggregates=levels)
    pts = problems.row_support_points(pb)
    ctx = solver.Context(0)
    try:
        ctx.set_matrix(_abi.A, pb.mats["A"])
        with pytest.raises(solver.AlfdError) as e:          # an incomplete lattice without base
            ctx.build_geometric_from_points(pts, min_coarse=100)
        assert e.value.status == _abi.E_INVALID
        built_levels, cells = ctx.build_geometric_from_points(pts, base=6, min_coarse=100, return_cells=True)
        assert [n for _, n in built_levels] == [n for _, n in levels]
        assert cells.tolist() == [[24] * 3, [6] * 3, [3] * 3]
        solver.upload_problem(ctx, pb, sc._copy(cfg))       # keeps the hierarchy built above
        _same_levels(ctx, levels)
        got = sc._snapshot(ctx, pb, cfg)
    finally:
        ctx.close()
    sc._assert_equal(got, ref)


# --------------------------------------------------------------------------------------------------------------- 4
def test_elliptic_both_blocks_from_points(built):
    cf = base.config("a22_gmg_8")
    pb, cfg = cf.pb, cf.cfg
    ref = _snapshot_of(pb, cfg, aggregates=cf.levels0, immersed_levels=cf.levels1)
    ctx = solver.context_from_problem(pb, sc._copy(cfg), hierarchy_from_points=dict(
        points=problems.row_support_points(pb), min_coarse=100,
        immersed_points=problems.immersed_support_points(pb), immersed_min_coarse=base.IMM_MIN_COARSE))
    try:
        _same_levels(ctx, cf.levels0, block=0)
        _same_levels(ctx, cf.levels1, block=1)
        got = sc._snapshot(ctx, pb, cfg)
    finally:
        ctx.close()
    sc._assert_equal(got, ref)


# --------------------------------------------------------------------------------------------------------------- 5
def test_build_setup_new_coupling_setup_coupling_equals_fresh(built):
    pb0, pb1 = sc._stokes3d(8, 1, sc.C0), sc._stokes3d(8, 1, sc.C1)
    _, cfg = cases.case("stokes3d_gmg_patch")
    levels = problems.tensor_prolongators(pb0.params, min_coarse=100)
    ref = _snapshot_of(pb1, cfg, aggregates=levels)
    ctx = solver.context_from_problem(pb0, sc._copy(cfg), hierarchy_from_points=dict(
        points=problems.row_support_points(pb0), min_coarse=100))
    try:
        sc._move(ctx, pb1, M=False)                          # the build preceded the last alfd_setup: no refusal
        k = ctx.setup_counts()
        assert k["products_a"] == 0 and k["level_a_uploads"] == 0 and k["transfer_uploads"] == 0, k
        got = sc._snapshot(ctx, pb1, cfg)
        sc._assert_equal(got, ref)
        # a build AFTER the last setup is a new hierarchy input: alfd_setup_coupling asks for alfd_setup
        ctx.build_geometric_from_points(problems.row_support_points(pb0), min_coarse=100)
        with pytest.raises(solver.AlfdError) as e:
            ctx.setup_coupling()
        assert e.value.status == _abi.E_INVALID and "needs alfd_setup" in str(e.value)
        ctx.setup(pb1.block_sizes)
        sc._assert_equal(sc._snapshot(ctx, pb1, cfg), ref)
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------------------------------- 6
def test_refusals_keep_the_context_and_its_hierarchy(stokes):
    pb, cfg, levels, ref = stokes
    pts = problems.row_support_points(pb)
    ctx = solver.Context(0)
    try:
        with pytest.raises(solver.AlfdError) as e:          # no slot A yet
            ctx.build_geometric_from_points(pts)
        assert e.value.status == _abi.E_NOT_SETUP
        solver.upload_problem(ctx, pb, sc._copy(cfg), aggregates=levels)
        moved = pts.copy()
        moved[300, 0] += 0.3 * (pts[3, 0] - pts[0, 0])
        for bad, kw in ((pts[:-3], {}), (moved, {}), (pts, dict(base=40)), (pts, dict(block=2)),
                        (pts, dict(block=1))):               # n != rows of A; no lattice; base_d > m_d; block; no slot A2
            with pytest.raises(solver.AlfdError) as e:
                ctx.build_geometric_from_points(bad, **kw)
            want = _abi.E_NOT_SETUP if kw.get("block") == 1 else _abi.E_INVALID
            assert e.value.status == want, (kw, e.value.status)
        _same_levels(ctx, levels)                            # the hierarchy it had
        sc._move(ctx, pb, M=False)                           # nothing was touched: no "needs alfd_setup"
        sc._assert_equal(sc._snapshot(ctx, pb, cfg), ref)
    finally:
        ctx.close()


def test_partitioned_context_is_refused_on_every_rank(built):
    """Two ranks in one process: ALFD_E_UNSUPPORTED on each without an exchange, then the same solve as before."""
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
            solver.upload_problem(ctx, pb, sc._copy(cfg))
            rhs = ctx.augment_rhs(cases.rhs_of(pb))
            ctx.solve(rhs)
            hist = ctx.history()
            pts = problems.row_support_points(pb.params, node_range=plan.generator_ranges(rank)[:2])
            assert pts.shape[0] == pb.mats["A"].nrows
            with pytest.raises(solver.AlfdError) as e:
                ctx.build_geometric_from_points(pts)
            _, res = ctx.solve(rhs)                          # still set up: nothing was touched
            out[rank] = (e.value.status, res.status, np.array_equal(ctx.history(), hist))
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


# --------------------------------------------------------------------------------------------------------------- 7
def test_replay_with_the_bench_preconditioner_from_support_points(built, tmp_path):
    """bench/reference_cmake/replay.py --inner-prec gmg on a dumped Stokes system: the counts of a context that was handed
    tensor_prolongators with the bench settings (the tool permutes the dump by its points first, hence counts only)."""
    import subprocess
    import sys
    from fictitious_domain_al_preconditioners_amd import opfile
    pb, _ = cases.case("stokes3d_gmg_patch")
    cfg = _abi.bench_multilevel_settings(_abi.default_config(_abi.AL_STOKES), geometric=True)
    ctx = solver.context_from_problem(pb, sc._copy(cfg), aggregates=problems.tensor_prolongators(
        pb.params, min_coarse=_abi.BENCH_MIN_COARSE))
    try:
        rhs = ctx.augment_rhs(cases.rhs_of(pb))
        _, ref = ctx.solve(rhs)
    finally:
        ctx.close()
    mats = {_abi.SLOT_BY_NAME[k]: pb.mats[k] for k in ("A", "Bt", "B", "Ct", "C", "Mp")}
    diags = {_abi.INVW: pb.inv_w_diag_squared(), _abi.MP_LUMPED_INV: pb.mp_lumped_inv()}
    dump, points = str(tmp_path / "stokes.alfd"), str(tmp_path / "points.npy")
    opfile.save(dump, mats, diags, rhs, _abi.default_config(_abi.AL_STOKES))
    np.save(points, problems.row_support_points(pb))
    tool = os.path.join(os.path.dirname(GOLDEN), os.pardir, "bench", "reference_cmake", "replay.py")
    run = subprocess.run([sys.executable, tool, dump, "--inner-prec", "gmg", "--support-points", points],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    out = json.loads(run.stdout.strip().splitlines()[-1])["gpu"]
    assert "geometric hierarchy from the support points" in run.stdout
    assert (out["outer"], out["inner"], out["mp"]) == (ref.outer_iterations, ref.inner_iterations, ref.mp_iterations)
    # without the points the tool says what it needs instead of falling back to another preconditioner
    run = subprocess.run([sys.executable, tool, dump, "--inner-prec", "gmg"], capture_output=True, text=True, timeout=60)
    assert run.returncode != 0 and "--support-points" in run.stderr
