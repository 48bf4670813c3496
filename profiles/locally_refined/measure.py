"""Uniform against locally refined background mesh at one size, bench settings, one GPU (README.md beside this file).

Each mesh (assembly="cellwise"; the refined one with local_refine=1) is solved in three forms: as generated
(lexicographic), after problems.cuthill_mckee_nodes, and after the front end's renumbering from support points
(solver.numbering_from_points) with row blocks from solver.brick_blocks_from_points.  The uniform mesh runs the
bench's geometric hierarchy (problems.tensor_prolongators), the refined one problems.refined_prolongators and, in the
forms named by --sa-forms, the truncated smoothed-aggregation hierarchy built on the device.  One JSON line per leg,
appended to --out as soon as the leg is done."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--meshes", default="uniform,refined")
ap.add_argument("--forms", default="as_generated,cuthill_mckee,front_end")
ap.add_argument("--sa-forms", default="front_end", help="forms of the refined mesh that also run the truncated SA hierarchy")
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
BRICK = tuple(int(v) for v in args.bricks.split(","))
REFINE = max(0, int(round(np.log2(args.n / 64.0))) + 4)           # bench.py's immersed mesh for this size


def config(geometric):
    cfg = _abi.default_config(_abi.AL_STOKES)
    _abi.bench_multilevel_settings(cfg, geometric)
    cfg.on_inner_failure = _abi.INNER_ACCEPT                      # a capped inner solve is counted, not thrown
    return cfg


def storage(info):
    if info["batch_major"]:
        return "batch-major" + (" (10-bit codes)" if info["batch_major_wide"] else "")
    return "value-indexed window" if info["value_indexed"] else "window" if info["windowed"] else "csr"


def measure(pb, mesh, form, hierarchy, blocks):
    refined = bool(pb.params.get("local_refine"))
    rec = dict(n_cells=args.n, mesh=mesh, form=form, hierarchy=hierarchy, rows=int(pb.mats["A"].nrows),
               nnz=int(pb.mats["A"].nnz), longest_row=int(np.diff(pb.mats["A"].row_ptr).max()),
               hanging_rows=int(pb.vecs["u_hanging"].sum()) * pb.params["ncomp"] if refined else 0,
               pressure_rows=int(pb.mats["B"].nrows), multiplier_rows=int(pb.mats["C"].nrows))
    cfg = config(hierarchy != "truncated_sa")
    ctx = solver.Context(0)
    try:
        t0 = time.time()
        if hierarchy == "truncated_sa":
            if blocks is not None:
                ctx.set_row_blocks(_abi.A, *blocks)
            ctx.set_matrix(_abi.A, pb.mats["A"])
            ctx.set_matrix(_abi.C_, pb.mats["C"])
            ctx.set_matrix(_abi.CT, pb.mats["Ct"])
            ctx.set_diag(_abi.INVW, pb.inv_w_diag_squared())
            ctx.configure(cfg)
            levels = ctx.build_smoothed_aggregation(block_size=3, threshold=0.02, max_aggregate_nodes=8,
                                                    damping=4.0 / 3.0, min_coarse=300, max_row_entries=4)
            rec["hierarchy_s"] = time.time() - t0
            solver.upload_problem(ctx, pb, cfg, None, blocks)
        else:
            th = time.time()
            if refined:
                levels = problems.refined_prolongators(pb, min_coarse=_abi.BENCH_MIN_COARSE)
            else:
                levels = problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE,
                                                      node_permutation=getattr(pb, "node_permutation", None))
            rec["hierarchy_s"] = time.time() - th
            t0 = time.time()
            solver.upload_problem(ctx, pb, cfg, levels, blocks)
        rec["setup_s"] = time.time() - t0
        rec["levels"] = [[int(nc), int(P.nnz)] for P, nc in levels]
        info = ctx.matrix_info(_abi.A)
        rec["storage"] = storage(info)
        rec["bytes_per_nnz"] = info["streamed_bytes"] / max(info["nnz"], 1)
        rec["shared_share"] = info["shared_nnz"] / max(info["nnz"], 1)
        ms, nbytes = ctx.bench_spmv(_abi.A, 20)
        rec["spmv_A_ms"], rec["spmv_A_family"] = ms, ctx.last_spmv_launch()["family_name"]
        ctx.upload_rhs(ctx.augment_rhs([pb.vecs["f"], pb.vecs["rhs_p"], pb.vecs["g"]]))
        ctx.solve_resident(raise_on_failure=False)
        res = ctx.solve_resident(raise_on_failure=False)
        rec.update(status=int(res.status), outer=int(res.outer_iterations), inner=int(res.inner_iterations),
                   mp=int(res.mp_iterations), inner_failures=int(res.inner_failures), solve_s=res.solve_seconds,
                   final_residual=res.last_residual,
                   iterations_per_s=res.outer_iterations / res.solve_seconds if res.solve_seconds > 0 else 0.0)
    except Exception as e:   # noqa: BLE001
        rec["error"] = repr(e)
    finally:
        ctx.close()
    print(json.dumps(rec), flush=True)
    with open(args.out, "a") as out:
        out.write(json.dumps(rec) + "\n")
    if "error" in rec and "HIP" in rec["error"]:
        sys.exit(3)                                               # a device error: start nothing more


for mesh in args.meshes.split(","):
    t = time.time()
    pb = problems.stokes3d_sphere(n_cells=args.n, immersed_refine=REFINE, assembly="cellwise",
                                  local_refine=1 if mesh == "refined" else 0)
    print(f"{mesh} N = {args.n}: generated in {time.time() - t:.1f} s, rows {pb.mats['A'].nrows}, nnz {pb.mats['A'].nnz}",
          flush=True)
    nc = pb.params["ncomp"]
    blocks = None
    for form in ("as_generated", "cuthill_mckee", "front_end"):
        t = time.time()
        if form == "cuthill_mckee":
            problems.permute_background_nodes(pb, problems.cuthill_mckee_nodes(pb))
        elif form == "front_end":
            n2o = solver.numbering_from_points(problems.row_support_points(pb))
            problems.permute_background_nodes(pb, n2o[::nc] // nc)
            blocks = solver.brick_blocks_from_points(problems.row_support_points(pb), BRICK)
        print(f"{mesh} {form}: renumbered in {time.time() - t:.1f} s", flush=True)
        if form not in args.forms.split(","):
            continue
        measure(pb, mesh, form, "geometric", blocks)
        if mesh == "refined" and form in args.sa_forms.split(","):
            measure(pb, mesh, form, "truncated_sa", blocks)
    del pb
