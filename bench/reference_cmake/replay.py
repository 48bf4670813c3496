#!/usr/bin/env python3
"""Replays a .alfd dump of a reference run (bench/reference_cmake: ALFD_EXPORT=ON) through libalfd on the GPU and
prints both iteration counts side by side -- the one route by which parity with a real deal.II + Trilinos run can be
pinned (needs a deal.II install, which this repository's pipeline does not have).

    python bench/reference_cmake/replay.py run/stokes_immersed_boundary.alfd [--reference-log run/stokes.log]
                                           [--inner-prec multilevel|sa-multilevel|gmg|chebyshev] [--support-points points.npy]
                                           [--base-cells N]
                                           [--sa-drop-tolerance TAU] [--sa-max-row-entries K]

A dump with grad_div_in_A = 0 (`Grad-div stabilization = false`) replays with the identity inner preconditioner, the
reference's, or with --inner-prec chebyshev; never multilevel.

The inner preconditioner differs from the reference's by construction (Trilinos ML there; here the algebraic aggregation
of alfd_build_aggregates on the dumped A, or geometric transfers when the caller supplies them; sa-multilevel builds
ML's algorithm, smoothed aggregation, from the dumped operators with alfd_build_smoothed_aggregation;
--sa-drop-tolerance / --sa-max-row-entries truncate its prolongators as ML does, e.g. --sa-max-row-entries 4; gmg is the
preconditioner bench.py measures -- the geometric hierarchy, built by alfd_build_geometric_from_points from the
--support-points and the lone-diagonal rows of the dumped A, with the interface patch and the explicit coarsest inverse
of the bench; a locally refined mesh also needs --base-cells, its `Initial refinement` cells per axis), so OUTER counts
are the comparable quantity: both inner solvers stop at the same absolute tolerance (parameters_stokes_3d.prm:23-24)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("alfd_file")
    ap.add_argument("--reference-log", help="stdout of the reference run (scrape_deallog.py)")
    ap.add_argument("--inner-prec", choices=["multilevel", "sa-multilevel", "gmg", "chebyshev"], default="multilevel")
    ap.add_argument("--inner-max", type=int, default=0, help="override the inner CG cap of the dump (0 = keep)")
    ap.add_argument("--support-points", help=".npy with one support point per row of block 0: front-end renumbering + mesh bricks")
    ap.add_argument("--block-size", type=int, default=0, help="components per node of block 0 (default: 3 for Stokes dumps, else 1)")
    ap.add_argument("--sa-drop-tolerance", type=float, default=0.0,
                    help="sa-multilevel: drop the entries of P below this fraction of their row's maximum (0 = none)")
    ap.add_argument("--sa-max-row-entries", type=int, default=0,
                    help="sa-multilevel: keep at most this many entries per row of P (0 = no cap)")
    ap.add_argument("--base-cells", type=int, default=0,
                    help="gmg: cells per axis of the uniform base grid (needed when the mesh is locally refined)")
    args = ap.parse_args()
    if args.inner_prec == "gmg" and not args.support_points:
        ap.error("--inner-prec gmg needs --support-points")
    import numpy as np
    from fictitious_domain_al_preconditioners_amd import _abi, opfile, solver
    import scrape_deallog

    mats, diags, rhs, x0, cfg = opfile.load(args.alfd_file)
    nblocks = len(rhs)
    bs = args.block_size or (3 if _abi.BT in mats else 1)
    if args.inner_max:
        cfg.inner.max_steps = args.inner_max
    cfg.log_level = 1
    ctx = solver.Context(0)
    perm = None
    if args.support_points:
        pts = np.load(args.support_points)
        perm = solver.numbering_from_points(pts)
        inv = np.empty_like(perm)
        inv[perm] = np.arange(perm.size)
        for slot in (_abi.A, _abi.BT, _abi.CT):
            if slot in mats:
                mats[slot] = solver.permute_csr(mats[slot], row_new_to_old=perm, col_old_to_new=inv if slot == _abi.A else None)
        for slot in (_abi.B, _abi.C_):
            if slot in mats:
                mats[slot] = solver.permute_csr(mats[slot], col_old_to_new=inv)
        rhs[0] = rhs[0][perm]
        if x0 is not None:
            x0[0] = x0[0][perm]
        ctx.set_row_blocks(_abi.A, *solver.brick_blocks_from_points(pts[perm], (16, 4, 1)))
    for slot, m in mats.items():
        ctx.set_matrix(slot, m)
    for slot, d in diags.items():
        ctx.set_diag(slot, d)
    gd_off = cfg.variant in (_abi.AL_STOKES, _abi.AL_STOKES_DIAG) and not cfg.grad_div_in_A
    if gd_off and args.inner_prec in ("multilevel", "sa-multilevel", "gmg"):
        # Aug = A + gamma Ct invW C + gamma_gd Bt Mp^-1 B has no multilevel preconditioner (ExcNotImplemented in the
        # reference): such dumps replay with the identity inner preconditioner of the reference, or --inner-prec chebyshev
        print("grad_div_in_A = 0: no multilevel inner preconditioner; replaying with the identity inner preconditioner")
        cfg.inner_prec = _abi.PREC_IDENTITY
    elif args.inner_prec == "gmg" and cfg.variant in (_abi.AL2, _abi.AL_STOKES, _abi.AL_STOKES_DIAG):
        _abi.bench_multilevel_settings(cfg, geometric=True)
        levels, cells = ctx.build_geometric_from_points(pts[perm], base=args.base_cells or None,
                                                        min_coarse=_abi.BENCH_MIN_COARSE, return_cells=True)
        print(f"geometric hierarchy from the support points: lattice {cells[0].tolist()} cells, coarse grids "
              f"{cells[1:].tolist()}, levels {[nc for _, nc in levels]}")
    elif args.inner_prec in ("multilevel", "sa-multilevel") and cfg.variant in (_abi.AL2, _abi.AL_STOKES, _abi.AL_STOKES_DIAG):
        cfg.inner_prec = _abi.PREC_MULTILEVEL
        cfg.ml_smooth_degree, cfg.ml_smooth_ratio, cfg.ml_coarse_degree = 4, 256.0, 10
        ctx.configure(cfg)
        if args.inner_prec == "sa-multilevel":
            levels, omega = ctx.build_smoothed_aggregation(block_size=bs, threshold=0.02, max_aggregate_nodes=8,
                                                           damping=4.0 / 3.0, min_coarse=3000, return_omega=True,
                                                           drop_tolerance=args.sa_drop_tolerance,
                                                           max_row_entries=args.sa_max_row_entries)
            cut = ""
            if args.sa_drop_tolerance or args.sa_max_row_entries:
                cut = (f", truncated (drop tolerance {args.sa_drop_tolerance}, at most {args.sa_max_row_entries} per row): "
                       f"nnz of P {[int(P.nnz) for P, _ in levels]}")
            print(f"smoothed aggregation (ML's threshold 0.02 and damping 4/3, utilities.h:304-317): levels "
                  f"{[nc for _, nc in levels]}, omega {[float(o) for o in omega]}{cut}")
        else:
            levels = ctx.build_aggregates(block_size=bs, threshold=0.02, max_aggregate_nodes=8, min_coarse=3000)
            print(f"algebraic aggregation (ML's threshold 0.02, utilities.h:312): levels {[nc for _, nc in levels]}")
    else:
        cfg.inner_prec = _abi.PREC_CHEBYSHEV
    ctx.configure(cfg)
    ctx.setup([b.size for b in rhs])
    x, res = ctx.solve(rhs, x0)
    info = ctx.matrix_info(_abi.A)
    out = {"gpu": {"outer": res.outer_iterations, "inner": int(res.inner_iterations), "mp": int(res.mp_iterations),
                   "initial_residual": res.initial_residual, "final_residual": res.last_residual,
                   "solve_seconds": res.solve_seconds, "outer_iterations_per_s": res.outer_iterations / res.solve_seconds,
                   "A_storage": ("batch-major" if info["batch_major"] else "value-indexed window" if info["value_indexed"] else
                                 "window 10 B/nnz" if info["windowed"] else "csr"),
                   "A_bytes_per_nnz": info["streamed_bytes"] / max(info["nnz"], 1)},
           "blocks": [int(b.size) for b in rhs]}
    if args.reference_log:
        ref = scrape_deallog.scrape(open(args.reference_log).read())
        out["reference"] = {"outer": ref["outer"]["steps"], "inner": ref["inner"]["steps_total"],
                            "initial_residual": ref["outer"]["initial"], "final_residual": ref["outer"]["final"],
                            "solve_system_s": ref["timers"].get("Solve system", {}).get("wall_s"),
                            "outer_iterations_per_s": ref.get("outer_iterations_per_s")}
        r, g = out["reference"], out["gpu"]
        print(f"{'':24s}{'reference (deal.II + ML)':>28s}{'libalfd (MI355X)':>22s}")
        for key in ("outer", "inner", "initial_residual", "final_residual", "outer_iterations_per_s"):
            print(f"{key:24s}{str(r.get(key)):>28s}{str(g.get(key)):>22s}")
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
