#!/usr/bin/env python3
"""Wall seconds of the geometric hierarchy of the bench workload (stokes3d_sphere, Q2 velocity, min_coarse of the bench)
by the two routes, one JSON line per measurement appended to --out:

  parent  problems.tensor_prolongators(params) + one Context.set_prolongator per level
  points  alfd_build_geometric_from_points(row_support_points), constrained = NULL (flags from the resident A)

    python profiles/points_hierarchy/measure.py --n 64 --out profiles/points_hierarchy/gpu.jsonl [--end-to-end]
    python profiles/points_hierarchy/measure.py --n 64 --host-only --out profiles/points_hierarchy/cpu_host.jsonl

--host-only needs no GPU: no context exists there, so it times the host routines behind the build as a caller uses them
(solver.point_hierarchy: per level a sizing call, the allocation, a fill call -- every level is formed twice) against
tensor_prolongators alone, on synthetic points (no operators are generated).
--end-to-end: the whole setup (uploads, hierarchy, alfd_setup) and one solve by each route on fresh contexts, --reps
rounds after one untimed warm-up context; the iteration counts and the solution bytes must agree."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver  # noqa: E402


def emit(out, **rec):
    rec["threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or len(os.sched_getaffinity(0))
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def host_only(n, reps, out):
    params = dict(dim=3, degree=2, ncomp=3, n_cells=n, lo=0.0, hi=1.0)
    pts = problems.row_support_points(params)
    for rep in range(reps):
        t = time.perf_counter()
        ref = problems.tensor_prolongators(params, min_coarse=_abi.BENCH_MIN_COARSE)
        t_parent = time.perf_counter() - t
        # what a caller of the host routines pays: per level a sizing call, the allocation of the arrays and a fill call
        # (solver.point_hierarchy), so every level is formed twice
        t = time.perf_counter()
        got = solver.point_hierarchy(pts, ncomp=3, min_coarse=_abi.BENCH_MIN_COARSE)
        t_points = time.perf_counter() - t
        same = all(np.array_equal(p.row_ptr, q.row_ptr) and np.array_equal(p.col, q.col) and p.val.tobytes() == q.val.tobytes()
                   for (p, _), (q, _) in zip(got, ref)) and len(got) == len(ref)
        emit(out, what="host_routines", n=n, rep=rep, rows=int(pts.shape[0]), levels=[int(k) for _, k in ref],
             parent_tensor_prolongators_s=t_parent, points_two_call_host_routines_s=t_points, equal=bool(same))
        del ref, got


def build_only(pb, n, reps, out):
    pts = problems.row_support_points(pb)
    ctx = solver.Context(0)
    try:
        ctx.set_matrix(_abi.A, pb.mats["A"])
        for rep in range(reps):
            t = time.perf_counter()
            levels = problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE)
            t_build = time.perf_counter() - t
            for level, (P, _) in enumerate(levels):
                ctx.set_prolongator(level, P)
            t_parent = time.perf_counter() - t
            t = time.perf_counter()
            nlev = ctx.build_geometric_from_points(pts, min_coarse=_abi.BENCH_MIN_COARSE, return_levels=False)
            t_points = time.perf_counter() - t
            same = nlev == len(levels)
            if rep == 0:                                      # the stored levels are the parent's, bit for bit
                for level, (P, _) in enumerate(levels):
                    Q = ctx.prolongator(level)
                    same = same and np.array_equal(P.row_ptr, Q.row_ptr) and np.array_equal(P.col, Q.col) and \
                        P.val.tobytes() == Q.val.tobytes()
            emit(out, what="build", n=n, rep=rep, rows=int(pts.shape[0]), levels=[int(k) for _, k in levels],
                 parent_tensor_prolongators_s=t_build, parent_with_set_prolongator_s=t_parent,
                 points_build_geometric_from_points_s=t_points, equal=bool(same))
    finally:
        ctx.close()


def end_to_end(pb, n, reps, out):
    """replay.py-style: one thread, the hierarchy in line with the uploads.  parent: tensor_prolongators, then the uploads
    with one set_prolongator per level; points: the uploads with the build after the operators are resident (the caller
    has its support points already); parent_overlapped: as bench.py hides the Python builder, on a helper thread beside
    the uploads."""
    digest = {}
    pts = problems.row_support_points(pb)
    routes = ("parent", "points", "parent_overlapped")
    for rnd in range(-1, reps):                            # round -1: one untimed context (first use of the device)
        order = routes[:1] if rnd < 0 else routes[rnd % 3:] + routes[:rnd % 3]
        for route in order:
            cfg = _abi.bench_multilevel_settings(_abi.default_config(_abi.AL_STOKES), geometric=True)
            ctx = solver.Context(0)
            try:
                t = time.perf_counter()
                if route == "parent":
                    solver.upload_problem(ctx, pb, cfg, problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE))
                elif route == "points":
                    solver.upload_problem(ctx, pb, cfg, hierarchy_from_points=dict(points=pts, min_coarse=_abi.BENCH_MIN_COARSE))
                else:
                    solver.upload_problem(ctx, pb, cfg, lambda: problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE))
                t_setup = time.perf_counter() - t
                if rnd < 0:
                    continue
                rhs = ctx.augment_rhs([pb.vecs["f"], pb.vecs["rhs_p"], pb.vecs["g"]])
                x, res = ctx.solve(rhs)
                h = hashlib.sha256()
                for b in x:
                    h.update(np.ascontiguousarray(b).tobytes())
                digest[(rnd, route)] = (res.outer_iterations, int(res.inner_iterations), int(res.mp_iterations), h.hexdigest())
                emit(out, what="end_to_end", n=n, round=rnd, route=route, setup_s=t_setup, solve_s=res.solve_seconds,
                     outer=res.outer_iterations, inner=int(res.inner_iterations), mp=int(res.mp_iterations),
                     solution_sha256=h.hexdigest())
            finally:
                ctx.close()
    equal = len(set(digest.values())) == 1
    emit(out, what="end_to_end_equal", n=n, equal=equal)
    assert equal, digest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", required=True)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--end-to-end", action="store_true")
    args = ap.parse_args()
    if args.host_only:
        return host_only(args.n, args.reps, args.out)
    t = time.perf_counter()
    refine = max(0, int(round(np.log2(args.n / 64.0))) + 4)       # the immersed mesh of bench.py at this size
    pb = problems.stokes3d_sphere(n_cells=args.n, immersed_refine=refine)
    print(f"generated N = {args.n} in {time.perf_counter() - t:.1f} s", flush=True)
    build_only(pb, args.n, args.reps, args.out)
    if args.end_to_end:
        end_to_end(pb, args.n, args.reps, args.out)


if __name__ == "__main__":
    main()
