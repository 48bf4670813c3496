"""The solve rate of the locally refined mesh with and without the Q1 level of the refined mesh in its hierarchy
(problems.refined_prolongators(q1_level=True)) and with and without the side rows' tails behind the launch with the
block-end tail ("ml_tail_side_rows"), bench settings, one GPU (README.md beside this file).  Modelled on
profiles/side_rows/measure.py: problems.stokes3d_sphere(N, ., assembly="cellwise", local_refine=1) in the front end's
numbering with its brick row blocks, "batch_major_side_rows" = 1, of two resident solves the second is timed.

One process measures ONE arm (--arm); the caller alternates the arms:
  today       refined_prolongators(q1_level=False), ml_tail_side_rows 0 (what the commit before could run)
  q1          the Q1 level, ml_tail_side_rows 0
  q1_tail     the Q1 level, ml_tail_side_rows 1
  today_tail  today's levels, ml_tail_side_rows 1
One JSON line per process, appended to --out."""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver  # noqa: E402

ARMS = {"today": (False, 0), "q1": (True, 0), "q1_tail": (True, 1), "today_tail": (False, 1)}
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--arm", choices=sorted(ARMS), required=True)
ap.add_argument("--bricks", default="16,4,1")
ap.add_argument("--out", required=True)
args = ap.parse_args()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
T0 = time.time()


def _beat():
    while True:
        time.sleep(60)
        print(f"[{time.time() - T0:.0f} s] working", flush=True)


threading.Thread(target=_beat, daemon=True).start()
q1_level, tail = ARMS[args.arm]
refine = max(0, int(round(np.log2(args.n / 64.0))) + 4)           # bench.py's immersed mesh for this size
pb = problems.stokes3d_sphere(n_cells=args.n, immersed_refine=refine, assembly="cellwise", local_refine=1)
nc = pb.params["ncomp"]
problems.permute_background_nodes(pb, problems.cuthill_mckee_nodes(pb))       # the numberings as the front end makes them
n2o = solver.numbering_from_points(problems.row_support_points(pb))
problems.permute_background_nodes(pb, n2o[::nc] // nc)
blocks = solver.brick_blocks_from_points(problems.row_support_points(pb), tuple(int(v) for v in args.bricks.split(",")))
print(f"[{time.time() - T0:.0f} s] problem: rows {pb.mats['A'].nrows}, nnz {pb.mats['A'].nnz}", flush=True)
t = time.time()
levels = problems.refined_prolongators(pb, min_coarse=_abi.BENCH_MIN_COARSE, q1_level=q1_level)
rec = dict(arm=args.arm, n_cells=args.n, q1_level=q1_level, ml_tail_side_rows=tail, rows=int(pb.mats["A"].nrows),
           level_sizes=[int(n) for _, n in levels], level_nnz=[int(p.nnz) for p, _ in levels], hierarchy_s=time.time() - t)
cfg = _abi.default_config(_abi.AL_STOKES)
_abi.bench_multilevel_settings(cfg, True)
cfg.on_inner_failure = _abi.INNER_ACCEPT                          # a capped inner solve is counted, not thrown
ctx = solver.Context(0)
try:
    ctx.set_tunable("batch_major_side_rows", 1)
    ctx.set_tunable("ml_tail_side_rows", tail)
    t = time.time()
    solver.upload_problem(ctx, pb, cfg, levels, blocks)
    rec["setup_s"] = time.time() - t
    info = ctx.matrix_info(_abi.A)
    rec["batch_major"], rec["side_list"] = int(info["batch_major"]), ctx.side_rows(_abi.A)
    ctx.upload_rhs(ctx.augment_rhs([pb.vecs["f"], pb.vecs["rhs_p"], pb.vecs["g"]]))
    ctx.solve_resident(raise_on_failure=False)
    before = ctx.fused_tail_launches()
    res = ctx.solve_resident(raise_on_failure=False)
    rec.update(status=int(res.status), outer=int(res.outer_iterations), inner=int(res.inner_iterations),
               solve_s=res.solve_seconds, final_residual=res.last_residual,
               fused_tail_launches=int(ctx.fused_tail_launches() - before),
               iterations_per_s=res.outer_iterations / res.solve_seconds if res.solve_seconds > 0 else 0.0)
except Exception as e:   # noqa: BLE001
    rec["error"] = repr(e)
finally:
    ctx.close()
print(json.dumps(rec), flush=True)
with open(args.out, "a") as out:
    out.write(json.dumps(rec) + "\n")
if "error" in rec:
    sys.exit(3)                                                   # start nothing more
