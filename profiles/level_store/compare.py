"""Everything the multigrid setup decides, as hashes: run under two builds of libalfd.so, the outputs must be the same lines.

    python profiles/level_store/compare.py --lib <libalfd.so> --out <file.jsonl> [--configs a,b,c,d,e,f]

The library is loaded in a fresh child process (solver.LIB_PATH is set there before the first load).  Per configuration
and rank one JSON line: sha256 of the residual history and of every solution block, lambda_max, the iteration counts,
the timed launches per class of one more solve under alfd_enable_timing(ctx, 2), and for hierarchies the library built
the sha256 of every level's prolongator arrays and the damping factors.  No wall times: a line depends on the build only.

  a  one rank, stokes3d_sphere(8, 1), CSR prolongators, patch, explicit coarsest inverse   csr_level, level_init, patch_setup
  b  one rank, stokes3d_sphere(8, 0), geometric aggregates                                 the galerkin path of ml_setup
  c  three ranks, slab aggregates, ALFD_ML_REPLICATE unset and 0                           replicated tail of ml_setup, the gather
  d  two and three ranks, CSR prolongators, patch                                          ml_setup_rep_prolongators, patch_setup_rep
  e  two ranks, truncated smoothed aggregation built by the library, then the solve with   build_sa_partitioned; with a 600-entry
     the patch; the same build on a chain with one 600-entry row                           row (aggregates of 2 nodes) its host fallback
  f  elliptic interface 64 / 16, both hierarchies, ml_tail_rows 0 and 4096                 hierarchy 1, build_tail_table"""
import argparse, hashlib, json, os, subprocess, sys, threading

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--lib", required=True)
ap.add_argument("--out", required=True)
ap.add_argument("--configs", default="a,b,c,d,e,f")
ap.add_argument("--child", action="store_true", help="(internal) this process loads the library")
args = ap.parse_args()
if not args.child:
    sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__), "--child", "--lib", os.path.abspath(args.lib),
                              "--out", os.path.abspath(args.out), "--configs", args.configs]))

sys.path.insert(0, ROOT)
import numpy as np
from fictitious_domain_al_preconditioners_amd import _abi, partition, problems, solver
solver.LIB_PATH = args.lib
os.makedirs(os.path.dirname(args.out), exist_ok=True)
out_file = open(args.out, "w")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def emit(config, rank, **fields):
    line = json.dumps(dict(config=config, rank=rank, **fields), sort_keys=True)
    print(line, flush=True)
    out_file.write(line + "\n")
    out_file.flush()


def rhs_of(pb):
    if "A2" in pb.mats:
        return [pb.vecs["f"].copy(), pb.vecs["f2"].copy(), np.zeros(pb.block_sizes[2])]
    return [pb.vecs["f"].copy(), pb.vecs["rhs_p"].copy(), pb.vecs["g"].copy()]


def solve_facts(ctx, rhs):
    """One solve for the bits, one more with every launch timed for the counts."""
    x, res = ctx.solve(rhs)
    facts = dict(hist=sha(ctx.history()), x=[sha(b) for b in x], lambda_max=res.lambda_max, status=int(res.status),
                 outer=int(res.outer_iterations), inner=int(res.inner_iterations), mp=int(res.mp_iterations),
                 inner_by_operator=ctx.inner_iterations())
    ctx.enable_timing(2)
    ctx.solve(rhs)
    facts["launches"] = {k: v["launches"] for k, v in ctx.timing().items()}
    ctx.enable_timing(0)
    return facts


def hierarchy_facts(levels, omega):
    return dict(prolongators=[[sha(P.row_ptr), sha(P.col), sha(P.val)] for P, _ in levels], omega=[float(w) for w in omega])


def run_ranks(config, world, work):
    """work(rank, group) -> fields of the rank's line; one host thread per rank on the in-process rank group."""
    group = solver.LocalGroup(world)
    lines = [None] * world

    def run(rank):
        try:
            lines[rank] = work(rank, group)
        except solver.AlfdError as e:
            lines[rank] = dict(error=[int(e.status), str(e)])

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    if any(t.is_alive() for t in th) or any(line is None for line in lines):
        emit(config, -1, error="a rank did not return")
        os._exit(1)
    for rank, line in enumerate(lines):
        emit(config, rank, **line)
    group.close()


def gmg_cfg(patch):
    cfg = _abi.default_config(_abi.AL_STOKES)
    cfg.inner_prec = _abi.PREC_MULTILEVEL
    cfg.inner.max_steps = 100
    cfg.ml_smooth_degree, cfg.ml_smooth_degree_coarse, cfg.ml_smooth_ratio = 3, 4, 30.0
    cfg.ml_coarse_direct = 1024
    if patch:
        cfg.ml_patch_degree, cfg.ml_patch_ratio = 6, 40.0
    return cfg


def aggregate_cfg():
    cfg = _abi.default_config(_abi.AL_STOKES)
    cfg.inner.max_steps = 1000
    cfg.inner_prec = _abi.PREC_MULTILEVEL
    cfg.ml_smooth_degree, cfg.ml_smooth_ratio = 2, 8.0
    return cfg


def config_a():
    pb = problems.stokes3d_sphere(8, 1)
    ctx = solver.context_from_problem(pb, gmg_cfg(True), aggregates=problems.tensor_prolongators(pb.params, min_coarse=100))
    emit("a", 0, **solve_facts(ctx, ctx.augment_rhs(rhs_of(pb))))
    ctx.close()


def config_b():
    pb = problems.stokes3d_sphere(8, 0)
    ctx = solver.context_from_problem(pb, aggregate_cfg(), aggregates=problems.geometric_aggregates(pb, a=2, min_coarse=100))
    emit("b", 0, **solve_facts(ctx, ctx.augment_rhs(rhs_of(pb))))
    ctx.close()


def slab_ranks(config, world, n, ref, cfg, local_levels):
    plan = partition.slab_partition_stokes3d(n, ref, world)

    def work(rank, group):
        pb = problems.stokes3d_sphere(n, ref, row_ranges=plan.generator_ranges(rank))
        ctx = solver.Context(0)
        ctx.comm_init_local(group.handle, rank)
        ctx.set_partition(plan.offsets)
        solver.upload_problem(ctx, pb, cfg, local_levels(plan, rank))
        facts = solve_facts(ctx, ctx.augment_rhs(rhs_of(pb)))
        ctx.close()
        return facts

    run_ranks(config, world, work)


def config_c():
    n, ref, world = 8, 0, 3
    full = problems.stokes3d_sphere(n, ref)
    plan = partition.slab_partition_stokes3d(n, ref, world)
    levels = partition.partitioned_geometric_aggregates(full.params, plan, a=2, min_coarse=100)
    for env in (None, "0"):
        os.environ.pop("ALFD_ML_REPLICATE", None)
        if env is not None:
            os.environ["ALFD_ML_REPLICATE"] = env       # read when a context is created
        slab_ranks(f"c replicate={env}", world, n, ref, aggregate_cfg(), lambda plan, rank: partition.local_aggregates(levels, rank))
    os.environ.pop("ALFD_ML_REPLICATE", None)


def config_d():
    n, ref = 8, 1
    full = problems.stokes3d_sphere(n, ref)
    glevels = problems.tensor_prolongators(full.params, min_coarse=100)
    for world in (2, 3):
        slab_ranks(f"d world={world}", world, n, ref, gmg_cfg(True),
                   lambda plan, rank: partition.local_prolongators(glevels, full.params, plan, rank))


BUILD = dict(threshold=0.02, max_aggregate_nodes=8, damping=4.0 / 3.0, min_coarse=300, return_omega=True)


def config_e():
    full = problems.stokes3d_sphere(8, 1)
    m = full.mats
    nn, npr, nl = m["A"].nrows // 3, m["B"].nrows, m["C"].nrows
    offsets = [np.array([0, nn // 2, nn], np.int64) * 3, np.array([0, npr // 2, npr], np.int64), np.array([0, nl // 2, nl], np.int64)]
    cfg = gmg_cfg(True)

    def work(rank, group):
        (u0, u1), (p0, p1), (l0, l1) = ((int(o[rank]), int(o[rank + 1])) for o in offsets)
        mats = dict(A=m["A"].slice_rows(u0, u1), Bt=m["Bt"].slice_rows(u0, u1), Ct=m["Ct"].slice_rows(u0, u1),
                    B=m["B"].slice_rows(p0, p1), Mp=m["Mp"].slice_rows(p0, p1), C=m["C"].slice_rows(l0, l1))
        vecs = dict(f=full.vecs["f"][u0:u1].copy(), rhs_p=full.vecs["rhs_p"][p0:p1].copy(), g=full.vecs["g"][l0:l1].copy())
        pb = problems.SyntheticProblem(params=dict(full.params), mats=mats, vecs=vecs)
        pb.inv_w_override = full.inv_w_diag_squared()[l0:l1]
        ctx = solver.Context(0)
        ctx.comm_init_local(group.handle, rank)
        ctx.set_partition(offsets)
        ctx.set_matrix(_abi.A, mats["A"])
        ctx.set_matrix(_abi.C_, mats["C"])
        ctx.set_matrix(_abi.CT, mats["Ct"])
        ctx.set_diag(_abi.INVW, pb.inv_w_diag_squared())
        ctx.configure(cfg)
        levels, omega = ctx.build_smoothed_aggregation(block_size=3, drop_tolerance=0.1, max_row_entries=8, **BUILD)
        facts = hierarchy_facts(levels, omega)
        solver.upload_problem(ctx, pb, cfg, None)                   # keeps the hierarchy built above
        facts.update(solve_facts(ctx, ctx.augment_rhs(rhs_of(pb))))
        ctx.close()
        return facts

    run_ranks("e truncated build, solve", 2, work)

    import scipy.sparse as sp                                       # the chain of test_row_overflow_is_a_joint_host_fallback
    n = 1500
    chain = sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tolil()
    far = np.arange(200, 1400, 2)
    chain[3, far] = -0.5 - 0.001 * np.arange(far.size)
    A = problems.Csr.from_scipy(chain.tocsr())
    offs = np.array([0, 700, 1500], np.int64)

    def wide(rank, group):
        ctx = solver.Context(0)
        ctx.comm_init_local(group.handle, rank)
        ctx.set_partition([offs, np.zeros(3, np.int64)])
        ctx.set_matrix(_abi.A, A.slice_rows(int(offs[rank]), int(offs[rank + 1])))
        try:
            facts = {}
            # aggregates of 8 nodes (the test's): only the node graph falls back; of 2 nodes: row 3 of P_0 reaches 601
            # aggregates, beyond the 512 of the prolongator kernels, so its rows come from the host routines as well
            for nodes in (8, 2):
                for tau, cap in ((0.0, 0), (0.1, 8)):
                    levels, omega = ctx.build_smoothed_aggregation(block_size=1, drop_tolerance=tau, max_row_entries=cap,
                                                                   **dict(BUILD, max_aggregate_nodes=nodes))
                    facts[f"nodes={nodes} tau={tau} cap={cap}"] = hierarchy_facts(levels, omega)
        finally:
            ctx.close()
        return facts

    run_ranks("e row of 600 entries", 2, wide)


def config_f():
    pb = problems.elliptic_interface2d(64, 16, beta2=1e3)
    cfg = _abi.default_config(_abi.AL_ELL_MODIFIED)
    cfg.gamma, cfg.gamma2 = 10.0, 1e-2
    cfg.inner = _abi.Control(_abi.CTRL_REDUCTION, 1000, 1e-30, 1e-8)
    cfg.outer = _abi.Control(_abi.CTRL_REDUCTION, 1000, 1e-10, 1e-10)
    cfg.inner_prec = _abi.PREC_MULTILEVEL
    cfg.ml_smooth_degree, cfg.ml_smooth_ratio, cfg.ml_coarse_direct = 4, 30.0, 1024
    cfg.ml_patch_degree, cfg.ml_patch_ratio = 5, 30.0
    ctx = solver.context_from_problem(pb, cfg, aggregates=problems.tensor_prolongators(pb.params, min_coarse=100),
                                      immersed_levels=problems.immersed_tensor_prolongators(pb.params, min_coarse=30))
    for rows in (0, 4096):
        ctx.set_tunable("ml_tail_rows", rows)
        emit(f"f ml_tail_rows={rows}", 0, **solve_facts(ctx, rhs_of(pb)))
    ctx.close()


for name in args.configs.split(","):
    {"a": config_a, "b": config_b, "c": config_c, "d": config_d, "e": config_e, "f": config_f}[name]()
out_file.close()
