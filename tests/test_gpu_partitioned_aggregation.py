"""Smoothed-aggregation hierarchies on row-partitioned contexts (in-process rank groups, one host thread per rank, as
tests/test_gpu_multirank.py; ranks take row slices of the GLOBAL operators).

First half: the node graph of the algebraic aggregation formed on the device from the resident rows of A
(alfd_build_strength_graph: sa_node_diag_kernel, sa_node_graph_kernel), on one rank and on partitions.  The kernel is
compared with the HOST routine alfd_host_strength_graph on the global operator (which tests/test_strength_graph.py pins
to a NumPy statement of the rule), bit for bit and whatever the partition; the greedy passes on the gathered rows then
give the single-rank aggregates.

Second half: alfd_build_smoothed_aggregation[_truncated] on partitioned contexts against a single-rank context on the
full operators (P_l, aggregates and omega bit for bit), the solve with the built hierarchy against the oracle's
emulation of the partition, and the edges: a rank without multiplier rows, joint errors and recovery, block 1, and
caller-supplied prolongators, which keep their halo condition."""
import threading

import numpy as np
import pytest

import cases
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver

pytestmark = pytest.mark.gpu

BS, THETA, MAX_NODES = 3, 0.02, 8


def run_ranks(world, work, timeout=120):
    """work(rank, group) on one thread per rank; a rank that raises or does not come back fails the test."""
    group = solver.LocalGroup(world)
    out, errs = [None] * world, []

    def run(rank):
        try:
            out[rank] = work(rank, group)
        except Exception as e:   # noqa: BLE001
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=timeout)
    hung = [r for r, t in enumerate(th) if t.is_alive()]
    assert not hung, f"ranks {hung} did not return"
    group.close()
    assert not errs, errs
    return out


def rank_context(group, rank, offsets, A):
    """A context of the group holding the rows [offsets[rank], offsets[rank + 1]) of the GLOBAL operator A."""
    ctx = solver.Context(0)
    ctx.comm_init_local(group.handle, rank)
    ctx.set_partition([np.asarray(offsets, np.int64), np.zeros(len(offsets), np.int64)])
    ctx.set_matrix(_abi.A, A.slice_rows(int(offsets[rank]), int(offsets[rank + 1])))
    return ctx


def graph_slice(g, n0, n1):
    """The rows of the nodes [n0, n1) of a node graph."""
    p = g["node_ptr"]
    return dict(d=g["d"][n0:n1], fixed=g["fixed"][n0:n1], node_ptr=p[n0:n1 + 1] - p[n0],
                nbr=g["nbr"][p[n0]:p[n1]], weight=g["weight"][p[n0]:p[n1]])


def assert_same_graph(got, ref, what):
    for key in ("d", "fixed", "node_ptr", "nbr", "weight"):
        assert got[key].dtype == ref[key].dtype, (what, key)
        assert got[key].tobytes() == ref[key].tobytes(), (what, key)


def gather_graph(parts):
    ptr = [np.zeros(1, np.int64)]
    for g in parts:
        ptr.append(g["node_ptr"][1:] + ptr[-1][-1])
    return dict(d=np.concatenate([g["d"] for g in parts]), fixed=np.concatenate([g["fixed"] for g in parts]),
                node_ptr=np.concatenate(ptr), nbr=np.concatenate([g["nbr"] for g in parts]),
                weight=np.concatenate([g["weight"] for g in parts]))


@pytest.fixture(scope="module")
def sphere(built):
    """stokes3d_sphere(8, 1): 14 739 velocity rows, 4913 nodes; the host graph and aggregates of the global operator."""
    A = problems.stokes3d_sphere(8, 1).mats["A"]
    assert A.nrows == 14739
    g = solver.host_strength_graph(A, BS, THETA)
    agg, nc = solver.host_aggregate_level(A, BS, THETA, MAX_NODES)
    return A, g, agg, nc


def _offsets(nn, kind):
    if kind == "uneven2":
        return np.array([0, nn // 5, nn], np.int64) * BS          # the cut falls inside an x-line of the grid
    world = int(kind[-1])
    return np.array([nn * p // world for p in range(world + 1)], np.int64) * BS


@pytest.mark.parametrize("kind", ["world2", "world3", "uneven2"])
def test_device_graph_of_a_partition_is_the_host_graph(sphere, kind):
    A, g, agg, nc = sphere
    nn = A.nrows // BS
    offs = _offsets(nn, kind)
    world = offs.size - 1

    def work(rank, group):
        ctx = rank_context(group, rank, offs, A)
        out = ctx.build_strength_graph(BS, THETA)
        ctx.close()
        return out

    parts = run_ranks(world, work)
    cross = 0
    for r, got in enumerate(parts):
        n0, n1 = int(offs[r]) // BS, int(offs[r + 1]) // BS
        assert got["on_device"]
        assert_same_graph(got, graph_slice(g, n0, n1), (kind, r))
        cross += int(np.sum((got["nbr"] < n0) | (got["nbr"] >= n1)))
    assert cross > 0                                               # edges to halo nodes: d_J came over the wire
    # at least one aggregate of the global aggregation has nodes on two ranks: slab-local aggregation would differ
    owner = np.searchsorted(offs, np.arange(A.nrows), side="right") - 1
    has = agg >= 0
    lo = np.full(nc, world, np.int64)
    hi = np.full(nc, -1, np.int64)
    np.minimum.at(lo, agg[has], owner[has])
    np.maximum.at(hi, agg[has], owner[has])
    assert np.any(hi > lo)
    agg2, nc2 = solver.host_aggregate_graph(gather_graph(parts), BS, MAX_NODES)
    assert nc2 == nc and np.array_equal(agg2, agg)


def test_device_graph_single_rank(sphere):
    A, g, _, _ = sphere
    ctx = solver.Context(0)
    ctx.set_matrix(_abi.A, A)
    got = ctx.build_strength_graph(BS, THETA)
    assert got["on_device"]
    assert_same_graph(got, g, "one rank")
    for theta in (0.0, 0.3):
        assert_same_graph(ctx.build_strength_graph(BS, theta), solver.host_strength_graph(A, BS, theta), theta)
    ctx.close()


def test_device_graph_with_constrained_rows(built):
    """Hanging-node rows (lone diagonals) and new values next to them; bs = 3 and bs = 1 on two ranks."""
    A = cases.hanging_node_variant(problems.stokes3d_sphere(6, 0)).mats["A"]
    for bs in (3, 1):
        g = solver.host_strength_graph(A, bs, THETA)
        assert g["fixed"].sum() > 0
        nn = A.nrows // bs
        offs = np.array([0, (nn * 2 // 5), nn], np.int64) * bs

        def work(rank, group):
            ctx = rank_context(group, rank, offs, A)
            out = ctx.build_strength_graph(bs, THETA)
            ctx.close()
            return out

        for r, got in enumerate(run_ranks(2, work)):
            assert got["on_device"]
            assert_same_graph(got, graph_slice(g, int(offs[r]) // bs, int(offs[r + 1]) // bs), (bs, r))


def _wide_row_matrix():
    """A 1-D Laplace chain of 1500 unknowns whose row 3 also reaches 600 others: more neighbour nodes than the
    kernel's set holds (512), on the first rank only."""
    import scipy.sparse as sp
    n = 1500
    m = sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tolil()
    far = np.arange(200, 1400, 2)
    m[3, far] = -0.5 - 0.001 * np.arange(far.size)
    return problems.Csr.from_scipy(m.tocsr())


def test_row_overflow_is_a_joint_host_fallback(built):
    A = _wide_row_matrix()
    g = solver.host_strength_graph(A, 1, THETA)
    assert g["node_ptr"][4] - g["node_ptr"][3] > 512
    offs = np.array([0, 700, 1500], np.int64)

    def work(rank, group):
        ctx = rank_context(group, rank, offs, A)
        out = ctx.build_strength_graph(1, THETA)
        ctx.close()
        return out

    for r, got in enumerate(run_ranks(2, work)):
        assert not got["on_device"]                                # both ranks, though only rank 0 holds the row
        assert_same_graph(got, graph_slice(g, int(offs[r]), int(offs[r + 1])), r)
    ctx = solver.Context(0)
    ctx.set_matrix(_abi.A, A)
    got = ctx.build_strength_graph(1, THETA)
    assert not got["on_device"]
    assert_same_graph(got, g, "one rank")
    ctx.close()


def test_bad_arguments_fail_on_every_rank_and_the_contexts_recover(sphere):
    A, g, _, _ = sphere
    nn = A.nrows // BS
    bad = np.array([0, (nn // 2) * BS + 1, A.nrows], np.int64)     # a node cut in two
    good = _offsets(nn, "world2")

    def work(rank, group):
        ctx = solver.Context(0)
        ctx.comm_init_local(group.handle, rank)
        status = []
        for call in (lambda: ctx.build_strength_graph(BS, THETA),):                       # nothing uploaded yet
            with pytest.raises(solver.AlfdError) as e:
                call()
            status.append(e.value.status)
        ctx.set_partition([bad, np.zeros(3, np.int64)])
        ctx.set_matrix(_abi.A, A.slice_rows(int(bad[rank]), int(bad[rank + 1])))
        for call in (lambda: ctx.build_strength_graph(BS, THETA), lambda: ctx.build_strength_graph(BS, -1.0),
                     lambda: ctx.build_strength_graph(0, THETA)):
            with pytest.raises(solver.AlfdError) as e:
                call()
            status.append(e.value.status)
        ctx.set_partition([good, np.zeros(3, np.int64)])
        ctx.set_matrix(_abi.A, A.slice_rows(int(good[rank]), int(good[rank + 1])))
        out = ctx.build_strength_graph(BS, THETA)                   # the same contexts, now correct
        ctx.close()
        return status, out

    for r, (status, got) in enumerate(run_ranks(2, work)):
        assert status == [_abi.E_INVALID] * 4, (r, status)
        assert_same_graph(got, graph_slice(g, int(good[r]) // BS, int(good[r + 1]) // BS), r)


# ---------------------------------------------------------------------------------------------------------------------
# alfd_build_smoothed_aggregation[_truncated] on row-partitioned contexts: the single-rank hierarchy, bit for bit,
# whatever the partition; then the existing yardstick of partitioned solves (the oracle's emulation of the partition).
from oracle import oracle   # noqa: E402

DAMPING = 4.0 / 3.0
BUILD = dict(block_size=BS, threshold=THETA, max_aggregate_nodes=MAX_NODES, damping=DAMPING, min_coarse=300)


def build_cfg():
    cfg = _abi.default_config(_abi.AL_STOKES)
    cfg.inner_prec = _abi.PREC_MULTILEVEL
    cfg.inner.max_steps = 100
    cfg.ml_smooth_degree, cfg.ml_smooth_degree_coarse, cfg.ml_smooth_ratio = 3, 4, 30.0
    cfg.ml_coarse_direct = 1024
    return cfg


def upload_operators(ctx, pb, cfg):
    ctx.set_matrix(_abi.A, pb.mats["A"])
    ctx.set_matrix(_abi.C_, pb.mats["C"])
    ctx.set_matrix(_abi.CT, pb.mats["Ct"])
    ctx.set_diag(_abi.INVW, pb.inv_w_diag_squared())
    ctx.configure(cfg)


def aggregates_of(ctx, level):
    import ctypes as C
    nf, nc = C.c_int64(0), C.c_int64(0)
    assert ctx._lib.alfd_get_aggregates(ctx._h, level, None, 0, C.byref(nf), C.byref(nc)) == _abi.OK
    agg = np.empty(nf.value, np.int32)
    assert ctx._lib.alfd_get_aggregates(ctx._h, level, agg.ctypes.data, agg.size, C.byref(nf), C.byref(nc)) == _abi.OK
    return agg, int(nc.value)


def local_problem(full, offsets, rank):
    """This rank's row slices of the GLOBAL operators and vectors (alfd_set_matrix: local rows, global columns)."""
    (u0, u1), (p0, p1), (l0, l1) = ((int(o[rank]), int(o[rank + 1])) for o in offsets)
    m = full.mats
    mats = dict(A=m["A"].slice_rows(u0, u1), Bt=m["Bt"].slice_rows(u0, u1), Ct=m["Ct"].slice_rows(u0, u1),
                B=m["B"].slice_rows(p0, p1), Mp=m["Mp"].slice_rows(p0, p1), C=m["C"].slice_rows(l0, l1))
    vecs = dict(f=full.vecs["f"][u0:u1].copy(), rhs_p=full.vecs["rhs_p"][p0:p1].copy(), g=full.vecs["g"][l0:l1].copy())
    pb = problems.SyntheticProblem(params=dict(full.params), mats=mats, vecs=vecs)
    pb.inv_w_override = full.inv_w_diag_squared()[l0:l1]
    return pb


def part_offsets(full, kind):
    """[velocity, pressure, multiplier] offsets; the velocity cut of "uneven2" falls inside an x-line of the grid."""
    nn = full.mats["A"].nrows // BS
    npr, nl = full.mats["B"].nrows, full.mats["C"].nrows
    if kind == "uneven2":
        return [np.array([0, nn // 5, nn], np.int64) * BS, np.array([0, npr // 3, npr], np.int64),
                np.array([0, nl // 2, nl], np.int64)]
    if kind == "nomult3":                                   # the slab plan of test_rank_without_multiplier_rows
        from fictitious_domain_al_preconditioners_amd import partition
        plan = partition.slab_partition_stokes3d(full.params["n_cells"], full.params["immersed_refine"], 3)
        return [plan.offsets[0], plan.offsets[1], np.array([0, 0, nl // 2, nl], np.int64)]
    world = int(kind[-1])
    even = lambda n: np.array([n * p // world for p in range(world + 1)], np.int64)      # noqa: E731
    return [even(nn) * BS, even(npr), even(nl)]


def single_rank_build(full, tau, cap):
    ctx = solver.Context(0)
    try:
        upload_operators(ctx, full, build_cfg())
        levels, omega = ctx.build_smoothed_aggregation(return_omega=True, drop_tolerance=tau, max_row_entries=cap, **BUILD)
        aggs = [aggregates_of(ctx, level) for level in range(len(levels))]
    finally:
        ctx.close()
    return levels, omega, aggs


def partitioned_build(full, offsets, tau, cap, then=None):
    world = offsets[0].size - 1

    def work(rank, group):
        pb = local_problem(full, offsets, rank)
        ctx = solver.Context(0)
        try:
            ctx.comm_init_local(group.handle, rank)
            ctx.set_partition(offsets)
            upload_operators(ctx, pb, build_cfg())
            levels, omega = ctx.build_smoothed_aggregation(return_omega=True, drop_tolerance=tau, max_row_entries=cap,
                                                           **BUILD)
            out = dict(levels=levels, omega=omega, aggs=[aggregates_of(ctx, level) for level in range(len(levels))])
            if then:
                out["then"] = then(ctx, pb, rank)
        finally:
            ctx.close()
        return out

    return run_ranks(world, work)


def assert_same_csr(a, b, what):
    assert (a.nrows, a.ncols) == (b.nrows, b.ncols), what
    for x, y in ((a.row_ptr, b.row_ptr), (a.col, b.col), (a.val, b.val)):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), what


def assert_single_rank_hierarchy(parts, ref, offsets, what):
    levels, omega, aggs = ref
    u = offsets[0]
    for r, got in enumerate(parts):
        assert len(got["levels"]) == len(levels), what
        assert got["omega"].tobytes() == omega.tobytes(), (what, r)               # the same on all ranks
        assert_same_csr(got["levels"][0][0], levels[0][0].slice_rows(int(u[r]), int(u[r + 1])), (what, r, "P_0"))
        assert got["aggs"][0][1] == aggs[0][1]
        assert np.array_equal(got["aggs"][0][0], aggs[0][0][int(u[r]):int(u[r + 1])]), (what, r)
        for level in range(1, len(levels)):                                         # whole on every rank
            assert_same_csr(got["levels"][level][0], levels[level][0], (what, r, level))
            assert got["aggs"][level][1] == aggs[level][1] and np.array_equal(got["aggs"][level][0], aggs[level][0])


def library_coarse_offsets(nc, world):
    """The split of the coarse ids the builder chooses (alfd.h): whole nodes, evenly."""
    return np.array([(nc // BS) * p // world * BS for p in range(world + 1)], np.int64)


def hard_paths(full, ref, offsets):
    """(aggregates with nodes on two ranks, coarse columns whose fine support leaves the forming rank's rows + halo)"""
    levels, _, aggs = ref
    agg, nc = aggs[0]
    u = offsets[0]
    world = u.size - 1
    owner = np.searchsorted(u, np.arange(agg.size), side="right") - 1
    has = agg >= 0
    lo, hi = np.full(nc, world, np.int64), np.full(nc, -1, np.int64)
    np.minimum.at(lo, agg[has], owner[has])
    np.maximum.at(hi, agg[has], owner[has])
    spanning = int(np.sum(hi > lo))
    P0, A = levels[0][0], full.mats["A"]
    coff = library_coarse_offsets(nc, world)
    rows = np.repeat(np.arange(P0.nrows), np.diff(P0.row_ptr))
    former = np.searchsorted(coff, P0.col, side="right") - 1
    leaving = set()
    for p in range(world):
        reach = np.zeros(A.nrows, bool)
        reach[int(u[p]):int(u[p + 1])] = True
        reach[A.col[A.row_ptr[int(u[p])]:A.row_ptr[int(u[p + 1])]]] = True      # own rows + halo of A
        bad = (former == p) & ~reach[rows]
        leaving.update(P0.col[bad].tolist())
    return spanning, len(leaving)


@pytest.fixture(scope="module")
def sphere81(built):
    full = problems.stokes3d_sphere(8, 1)
    assert full.mats["A"].nrows == 14739
    return full, single_rank_build(full, 0.0, 4)


@pytest.mark.parametrize("kind", ["world2", "world3", "uneven2"])
def test_partitioned_build_is_the_single_rank_hierarchy(sphere81, kind):
    full, ref = sphere81
    offsets = part_offsets(full, kind)
    spanning, leaving = hard_paths(full, ref, offsets)
    assert spanning >= 1 and leaving >= 1, (spanning, leaving)
    assert len(ref[0]) >= 2
    assert_single_rank_hierarchy(partitioned_build(full, offsets, 0.0, 4), ref, offsets, kind)


@pytest.mark.parametrize("tau,cap", [(0.0, 0), (0.1, 8)])
def test_partitioned_build_untruncated_and_by_tolerance(built, tau, cap):
    full = problems.stokes3d_sphere(6, 0)
    ref = single_rank_build(full, tau, cap)
    offsets = part_offsets(full, "world2")
    assert_single_rank_hierarchy(partitioned_build(full, offsets, tau, cap), ref, offsets, (tau, cap))


@pytest.mark.parametrize("world,patch", [(2, True), (3, True), (2, False)])
def test_partitioned_solve_with_the_built_hierarchy_matches_oracle_emulation(sphere81, world, patch):
    """The settings and tolerances of test_gpu_multirank.test_partitioned_geometric_multigrid_matches_oracle_emulation,
    with the hierarchy the partitioned contexts built themselves."""
    full, ref = sphere81
    offsets = part_offsets(full, f"world{world}")
    cfg = build_cfg()
    if patch:
        cfg.ml_patch_degree, cfg.ml_patch_ratio = 6, 40.0

    def solve(ctx, pb, rank):
        solver.upload_problem(ctx, pb, cfg, None)                   # keeps the hierarchy built above
        x, res = ctx.solve(ctx.augment_rhs(cases.rhs_of(pb)))
        return dict(x=x, res=res.as_dict(), hist=ctx.history())

    parts = partitioned_build(full, offsets, 0.0, 4, then=solve)
    assert_single_rank_hierarchy(parts, ref, offsets, "solve")
    glevels = [(P, nc) for P, nc in ref[0]]                        # = the gathered P_l (asserted above)
    osys = oracle.system_from_problem(full, nranks_emulated=world, part_offsets=offsets, aggregates=glevels)
    rc, orhs = osys.augment_rhs(cfg, cases.rhs_of(full))
    rc, ox, ores, ohist = osys.solve(cfg, orhs)
    assert rc == 0
    out = [p["then"] for p in parts]
    for r in range(world):
        res = out[r]["res"]
        assert res["status"] == 0
        assert (res["outer_iterations"], res["inner_iterations"], res["mp_iterations"]) == \
            (ores.outer_iterations, ores.inner_iterations, ores.mp_iterations)
        assert np.array_equal(out[r]["hist"], out[0]["hist"])
        assert np.max(np.abs(out[r]["hist"] - ohist) / np.abs(ohist)) <= 1e-10
    for b in range(3):
        xs = np.concatenate([out[r]["x"][b] for r in range(world)])
        assert np.allclose(xs, ox[b], rtol=1e-9, atol=1e-10 * max(np.abs(ox[b]).max(), 1e-30))


def test_partitioned_build_on_a_rank_without_multiplier_rows(sphere81):
    full, ref = sphere81
    offsets = part_offsets(full, "nomult3")
    assert offsets[2][1] == 0
    assert_single_rank_hierarchy(partitioned_build(full, offsets, 0.0, 4), ref, offsets, "nomult3")


def test_partitioned_build_errors_are_joint_and_the_contexts_recover(sphere81):
    """Offsets that cut a node and bad arguments: ALFD_E_INVALID on every rank; block 1: ALFD_E_UNSUPPORTED as before;
    then a correct build and solve on the SAME contexts."""
    full, ref = sphere81
    good = part_offsets(full, "world2")
    bad = [good[0].copy(), good[1], good[2]]
    bad[0][1] += 1
    cfg = build_cfg()

    def work(rank, group):
        ctx = solver.Context(0)
        ctx.comm_init_local(group.handle, rank)
        ctx.set_partition(bad)
        upload_operators(ctx, local_problem(full, bad, rank), cfg)
        status = []
        for kw in (dict(BUILD), dict(BUILD, damping=-1.0), dict(BUILD, drop_tolerance=1.5), dict(BUILD, block=1)):
            with pytest.raises(solver.AlfdError) as e:
                ctx.build_smoothed_aggregation(max_row_entries=4, **kw)
            status.append(e.value.status)
        pb = local_problem(full, good, rank)
        ctx.set_partition(good)
        upload_operators(ctx, pb, cfg)
        with pytest.raises(solver.AlfdError) as e:
            ctx.build_smoothed_aggregation(max_row_entries=4, **dict(BUILD, threshold=-1.0))     # right offsets, bad argument
        status.append(e.value.status)
        levels, omega = ctx.build_smoothed_aggregation(return_omega=True, max_row_entries=4, **BUILD)
        out = dict(levels=levels, omega=omega, aggs=[aggregates_of(ctx, level) for level in range(len(levels))])
        solver.upload_problem(ctx, pb, cfg, None)
        x, res = ctx.solve(ctx.augment_rhs(cases.rhs_of(pb)))
        out["status"], out["res"] = status, res.as_dict()
        ctx.close()
        return out

    parts = run_ranks(2, work)
    for r, got in enumerate(parts):
        assert got["status"] == [_abi.E_INVALID] * 3 + [_abi.E_UNSUPPORTED, _abi.E_INVALID], (r, got["status"])
        assert got["res"]["status"] == 0
    assert parts[0]["res"]["outer_iterations"] == parts[1]["res"]["outer_iterations"]
    assert_single_rank_hierarchy(parts, ref, good, "recovered")


def test_caller_supplied_prolongators_keep_the_halo_condition(sphere81):
    """The same prolongators handed over through alfd_set_prolongator: a coarse unknown whose fine support leaves its
    rank's rows + halo of A is still refused, with the message it always had."""
    full, ref = sphere81
    offsets = part_offsets(full, "world2")
    assert hard_paths(full, ref, offsets)[1] >= 1
    levels = ref[0]
    coff = library_coarse_offsets(levels[0][1], 2)
    cfg = build_cfg()

    def work(rank, group):
        pb = local_problem(full, offsets, rank)
        ctx = solver.Context(0)
        ctx.comm_init_local(group.handle, rank)
        ctx.set_partition(offsets)
        u = offsets[0]
        mine = [(levels[0][0].slice_rows(int(u[rank]), int(u[rank + 1])), levels[0][1], coff)] + \
               [(P, nc, None) for P, nc in levels[1:]]
        with pytest.raises(solver.AlfdError) as e:
            solver.upload_problem(ctx, pb, cfg, mine)
        ctx.close()
        return e.value.status, str(e.value)

    for status, msg in run_ranks(2, work):
        assert status == _abi.E_INVALID
        assert "a coarse unknown's fine support leaves its rank's rows + halo of A" in msg
