"""The A SpMV launch and the solve rate with and without side rows ("batch_major_side_rows"), bench settings, one GPU
(README.md beside this file).  Modelled on profiles/locally_refined/measure.py: the same meshes (assembly="cellwise";
the refined one with local_refine=1), the same three numberings, the geometric hierarchy of each mesh.

Every (mesh, form) is measured once per entry of --side-rows: 0 / 1 set the tunable before the upload, `unset` leaves the
context as created (what a library without the tunable can run: the script then asks for nothing that library lacks,
so the same file measures the commit before the change from a checkout of it; --label names the library in the
records).  The A launch is timed by alfd_bench_spmv (batch-major and side launch together) --spmv-runs times with
--spmv-reps launches each; of two resident solves the second is timed.  One JSON line per leg, appended to --out."""
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
ap.add_argument("--meshes", default="refined,uniform")
ap.add_argument("--forms", default="as_generated,cuthill_mckee,front_end")
ap.add_argument("--side-rows", default="1", help="comma list of 0, 1, unset")
ap.add_argument("--label", default="change")
ap.add_argument("--bricks", default="16,4,1")
ap.add_argument("--spmv-reps", type=int, default=50)
ap.add_argument("--spmv-runs", type=int, default=3)
ap.add_argument("--no-solve", action="store_true")
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


def storage(info):
    if info["batch_major"]:
        return "batch-major" + (" (10-bit codes)" if info["batch_major_wide"] else "")
    return "value-indexed window" if info["value_indexed"] else "window" if info["windowed"] else "csr"


def measure(pb, mesh, form, levels, blocks, side):
    ln = np.diff(pb.mats["A"].row_ptr)
    rec = dict(label=args.label, n_cells=args.n, mesh=mesh, form=form, side_rows_tunable=side,
               rows=int(pb.mats["A"].nrows), nnz=int(pb.mats["A"].nnz), longest_row=int(ln.max()),
               rows_beyond_384=int((ln > 384).sum()), nnz_beyond_384=int(ln[ln > 384].sum()))
    cfg = _abi.default_config(_abi.AL_STOKES)
    _abi.bench_multilevel_settings(cfg, True)
    cfg.on_inner_failure = _abi.INNER_ACCEPT                      # a capped inner solve is counted, not thrown
    ctx = solver.Context(0)
    try:
        if side != "unset":
            ctx.set_tunable("batch_major_side_rows", int(side))
        t0 = time.time()
        solver.upload_problem(ctx, pb, cfg, levels, blocks)
        rec["setup_s"] = time.time() - t0
        info = ctx.matrix_info(_abi.A)
        rec["storage"] = storage(info)
        rec["plan"] = {k: int(info[k]) for k in ("batch_major", "batch_major_wide", "batch_major_blocks", "shared_nnz",
                                                 "dictionary_entries")}
        rec["bytes_per_nnz"] = info["streamed_bytes"] / max(info["nnz"], 1)
        rec["shared_share"] = info["shared_nnz"] / max(info["nnz"], 1)
        if hasattr(ctx, "side_rows"):
            rec["side_list"] = ctx.side_rows(_abi.A)
        rec["spmv_A_ms"] = [ctx.bench_spmv(_abi.A, args.spmv_reps)[0] for _ in range(args.spmv_runs)]
        rec["spmv_A_family"] = ctx.last_spmv_launch()["family_name"]
        if not args.no_solve:
            ctx.upload_rhs(ctx.augment_rhs([pb.vecs["f"], pb.vecs["rhs_p"], pb.vecs["g"]]))
            ctx.solve_resident(raise_on_failure=False)
            res = ctx.solve_resident(raise_on_failure=False)
            rec.update(status=int(res.status), outer=int(res.outer_iterations), inner=int(res.inner_iterations),
                       solve_s=res.solve_seconds, final_residual=res.last_residual,
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
    order = ("as_generated", "cuthill_mckee", "front_end")        # each numbering is made from the one before
    for form in order[:max(order.index(f) for f in args.forms.split(",")) + 1]:
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
        t = time.time()
        if mesh == "refined":
            levels = problems.refined_prolongators(pb, min_coarse=_abi.BENCH_MIN_COARSE)
        else:
            levels = problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE,
                                                  node_permutation=getattr(pb, "node_permutation", None))
        print(f"{mesh} {form}: hierarchy in {time.time() - t:.1f} s", flush=True)
        for side in args.side_rows.split(","):
            measure(pb, mesh, form, levels, blocks, side)
    del pb
