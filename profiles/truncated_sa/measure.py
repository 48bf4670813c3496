"""Build / setup / solve seconds and counts of the plain, smoothed and truncated hierarchies."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import cases
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, required=True)
ap.add_argument("--kinds", default="plain,smoothed,t04,t018")
ap.add_argument("--plain-operator", action="store_true", help="stokes3d_sphere(N, 0) itself, no hanging nodes")
ap.add_argument("--inner-max", type=int, default=1000)
ap.add_argument("--out", required=True)
args = ap.parse_args()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
import threading
T0 = time.time()
def _beat():
    while True:
        time.sleep(60)
        print(f"[{time.time() - T0:.0f} s] working", flush=True)
threading.Thread(target=_beat, daemon=True).start()
t = time.time()
pb = problems.stokes3d_sphere(args.n, 0)
if not args.plain_operator:
    pb = cases.hanging_node_variant(pb)
print(f"problem N = {args.n}: {time.time() - t:.1f} s, rows {pb.mats['A'].nrows}, nnz {pb.mats['A'].nnz}", flush=True)
cfg = _abi.default_config(_abi.AL_STOKES)
cfg.inner.max_steps = args.inner_max
cfg.inner_prec = _abi.PREC_MULTILEVEL
cfg.ml_smooth_degree, cfg.ml_smooth_ratio, cfg.ml_coarse_degree = 4, 256.0, 10
RULES = {"smoothed": (0.0, 0), "t04": (0.0, 4), "t018": (0.1, 8)}
with open(args.out, "a") as out:
    for kind in args.kinds.split(","):
        ctx = solver.Context(0)
        try:
            ctx.set_matrix(_abi.A, pb.mats["A"]); ctx.set_matrix(_abi.C_, pb.mats["C"]); ctx.set_matrix(_abi.CT, pb.mats["Ct"])
            ctx.set_diag(_abi.INVW, pb.inv_w_diag_squared()); ctx.configure(cfg)
            kw = dict(block_size=3, threshold=0.02, max_aggregate_nodes=8, min_coarse=300)
            t0 = time.time()
            if kind == "plain":
                levels = ctx.build_aggregates(**kw)
                desc = [int(nc) for _, nc in levels]
                omega = []
            else:
                tau, k = RULES[kind]
                levels, omega = ctx.build_smoothed_aggregation(damping=4.0 / 3.0, return_omega=True, drop_tolerance=tau,
                                                               max_row_entries=k, **kw)
                desc = [(int(nc), int(P.nnz)) for P, nc in levels]
            t1 = time.time()
            print(f"built in {t1 - t0:.1f} s: {desc}", flush=True)
            solver.upload_problem(ctx, pb, cfg, None)
            t2 = time.time()
            print(f"upload + setup {t2 - t1:.1f} s", flush=True)
            rhs = ctx.augment_rhs(cases.rhs_of(pb))
            x, res = ctx.solve(rhs)
            t3 = time.time()
            rec = dict(N=args.n, kind=kind, levels=desc, omega=[float(o) for o in omega], build_s=t1 - t0,
                       upload_setup_s=t2 - t1, solve_s=res.solve_seconds, solve_wall_s=t3 - t2, status=int(res.status),
                       outer=int(res.outer_iterations), inner=int(res.inner_iterations),
                       initial_residual=res.initial_residual, final_residual=res.last_residual)
        except Exception as e:   # noqa: BLE001
            rec = dict(N=args.n, kind=kind, error=repr(e), after_s=time.time() - t0)
        finally:
            ctx.close()
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n"); out.flush()
        if "error" in rec and "HIP" in rec["error"]:
            sys.exit(3)                      # a device error: start nothing more
