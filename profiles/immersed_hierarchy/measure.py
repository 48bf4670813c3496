"""cfg 3 at full size (1024^2 / 256^2, modified AL, the settings of test_properties_cfg3_full_size, geometric hierarchy on
block 0) with and without the multigrid hierarchy of the immersed block: counts, solve seconds, timed launches, setup
seconds.  Arms alternate in one process after a warm-up solve each:
chebyshev (no block-1 hierarchy), hierarchy (block-1 hierarchy, coarse tail off), tailN (the same with ml_tail_rows = N)."""
import argparse, json, os, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--n-bg", type=int, default=1024)
ap.add_argument("--n-fg", type=int, default=256)
ap.add_argument("--beta2", default="10,1e3")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--arms", default="chebyshev,hierarchy,tail256,tail1024,tail4096", help="chebyshev: no block-1 hierarchy (the behaviour before it existed)")
ap.add_argument("--min-coarse", type=int, default=30)
ap.add_argument("--once", action="store_true", help="one solve per arm, no timing of launches (for a profiler run)")
ap.add_argument("--root", default=None, help="import the library from this checkout instead of the one this file is in "
                "(the parent commit, arm chebyshev only)")
ap.add_argument("--out", required=True)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root) if args.root
                else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)


def median_spread(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


with open(args.out, "a") as out:
    for beta2 in [float(b) for b in args.beta2.split(",")]:
        t = time.time()
        pb = problems.elliptic_interface2d(args.n_bg, args.n_fg, beta2=beta2)
        print(f"problem {args.n_bg}^2 / {args.n_fg}^2, beta2 = {beta2:g}: {time.time() - t:.1f} s, blocks {pb.block_sizes}", flush=True)
        cfg = _abi.default_config(_abi.AL_ELL_MODIFIED)
        cfg.gamma, cfg.gamma2 = 10.0, 1e-2
        cfg.inner = _abi.Control(_abi.CTRL_REDUCTION, 100000, 1e-2, 1e-20)
        cfg.outer = _abi.Control(_abi.CTRL_REDUCTION, 1000, 1e-10, 1e-10)
        cfg.inner_prec = _abi.PREC_MULTILEVEL
        cfg.ml_smooth_degree, cfg.ml_smooth_degree_coarse, cfg.ml_smooth_ratio, cfg.ml_coarse_direct = 3, 5, 30.0, 1024
        levels0 = problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE)
        levels1 = problems.immersed_tensor_prolongators(pb.params, min_coarse=args.min_coarse) if args.arms != "chebyshev" else []
        rhs = [pb.vecs["f"], pb.vecs["f2"], np.zeros(pb.block_sizes[2])]
        arms, setup = {}, {}
        for arm in args.arms.split(","):
            t0 = time.time()
            kw = dict(immersed_levels=levels1) if arm != "chebyshev" else {}
            ctx = solver.context_from_problem(pb, _abi.Config.from_buffer_copy(cfg), aggregates=levels0, **kw)
            if arm.startswith("tail"):
                ctx.set_tunable("ml_tail_rows", int(arm[4:]))
            setup[arm] = dict(wall_s=time.time() - t0, **ctx.setup_seconds())
            ctx.upload_rhs(rhs)
            ctx.solve_resident()                                   # warm-up
            arms[arm] = ctx
        seconds = {arm: [] for arm in arms}
        rec = {}
        for rep in range(1 if args.once else args.repeats):
            for arm, ctx in arms.items():                          # alternated
                ctx.upload_rhs(rhs)
                res = ctx.solve_resident()
                seconds[arm].append(res.solve_seconds)
                rec[arm] = res
        for arm, ctx in arms.items():
            res = rec[arm]
            counts = ctx.inner_iterations() if hasattr(ctx, "inner_iterations") else None
            launches = None
            if not args.once:
                ctx.enable_timing(2)
                ctx.upload_rhs(rhs)
                ctx.solve_resident()
                launches = {k: v["launches"] for k, v in ctx.timing().items()}
                ctx.enable_timing(0)
            med, lo, hi = median_spread(seconds[arm])
            line = dict(n_bg=args.n_bg, n_fg=args.n_fg, beta2=beta2, arm=arm,
                        immersed_levels=[pb.block_sizes[1]] + [int(nc) for _, nc in levels1] if arm != "chebyshev" else [],
                        status=int(res.status), outer=int(res.outer_iterations), inner=int(res.inner_iterations),
                        inner_by_operator=counts, solve_s_median=med, solve_s_min=lo, solve_s_max=hi,
                        solve_s_all=seconds[arm], timed_launches=launches,
                        timed_launches_total=None if launches is None else int(sum(launches.values())), setup=setup[arm])
            print(json.dumps(line), flush=True)
            out.write(json.dumps(line) + "\n")
            out.flush()
        for ctx in arms.values():
            ctx.close()
