"""What alfd_setup_coupling saves when the immersed body moves over a fixed background mesh.

One process, one GPU, the benchmark's solver settings (bench.py: Stokes, Taylor-Hood on N^3 cells, geometric hierarchy,
interface patch, brick row blocks).  The body alternates between two positions; after every move the context is brought
up to date by one of two arms, alternating, at least three pairs:

  (a) upload C / CT / INVW of the new position, then alfd_setup           -- the only way before this entry point
  (b) the same uploads, then alfd_setup_coupling

Each arm writes one JSON line: the per-phase seconds of alfd_get_setup_seconds, the counts of alfd_get_setup_counts, the
wall seconds of the uploads and of the setup call (host clock; both calls end device-synchronised) and the seconds of
the solve that follows.  Arm (a) is the yardstick.  There is no CPU path: without a GPU the script fails.

    python profiles/coupling_update/measure.py --n-cells 32 --n-cells 74 --pairs 3 --out coupling_update.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fictitious_domain_al_preconditioners_amd import _abi, problems, solver  # noqa: E402

CENTERS = ((0.5, 0.5, 0.5), (0.56, 0.47, 0.52))


def stokes(n, refine, center):
    """problems.stokes3d_sphere with the body at `center`"""
    return problems.generate(dim=3, degree=2, ncomp=3, n_cells=n, stokes=True, grad_div=True, gamma_grad_div=10.0,
                             center=center, radius=0.1, immersed_refine=refine, coupling_nq=4,
                             body_force=(1.0, 0.0, 0.0), embedded_value=(-1.0, 1.0, 0.0))


def coupling_of(pb):
    """Copies of what moves with the body (the problem itself, 21 GB of A at N = 74, can go)"""
    own = lambda m: problems.Csr(m.nrows, m.ncols, m.row_ptr.copy(), m.col.copy(), m.val.copy())
    return dict(Ct=own(pb.mats["Ct"]), C=own(pb.mats["C"]), inv_w=pb.inv_w_diag_squared().copy(), g=pb.vecs["g"].copy())


def measure(n, pairs, out):
    refine = max(0, int(round(np.log2(n / 64.0))) + 4)                 # bench.py's rule
    moved = stokes(n, refine, CENTERS[1])
    block_sizes = moved.block_sizes
    pos = [None, coupling_of(moved)]
    del moved
    pb = stokes(n, refine, CENTERS[0])
    assert pb.block_sizes == block_sizes, "the two positions must give the same blocks"
    pos[0] = coupling_of(pb)
    cfg = _abi.bench_multilevel_settings(_abi.default_config(_abi.AL_STOKES), geometric=True)
    levels = problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE)
    ctx = solver.Context(0)
    solver.upload_problem(ctx, pb, cfg, levels, problems.brick_row_blocks(pb.params, (16, 4, 1)))
    first = dict(n_cells=n, arm="first_setup", seconds=ctx.setup_seconds(), counts=ctx.setup_counts())
    out.write(json.dumps(first) + "\n")
    f, rhs_p = pb.vecs["f"].copy(), pb.vecs["rhs_p"].copy()
    del pb, levels                                                     # the host copy of A is not needed any more
    ctx.solve(ctx.augment_rhs([f, rhs_p, pos[0]["g"]]))               # warm-up: every kernel of the solve has run once
    where = 0
    for pair in range(pairs):
        for arm in ("a", "b") if pair % 2 == 0 else ("b", "a"):
            where = 1 - where
            p = pos[where]
            t0 = time.perf_counter()
            ctx.set_matrix(_abi.C_, p["C"])
            ctx.set_matrix(_abi.CT, p["Ct"])
            ctx.set_diag(_abi.INVW, p["inv_w"])
            t1 = time.perf_counter()
            if arm == "a":
                ctx.setup(block_sizes)
            else:
                ctx.setup_coupling()
            t2 = time.perf_counter()
            _, res = ctx.solve(ctx.augment_rhs([f, rhs_p, p["g"]]))
            rec = dict(n_cells=n, pair=pair, arm=arm, position=where, upload_s=t1 - t0, setup_call_s=t2 - t1,
                       seconds=ctx.setup_seconds(), counts=ctx.setup_counts(), solve_s=res.solve_seconds,
                       outer=res.outer_iterations, inner=res.inner_iterations, status=res.status)
            out.write(json.dumps(rec) + "\n")
            out.flush()
            print(json.dumps(rec), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-cells", type=int, action="append", default=None, help="repeatable; default 32 and 74")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default="coupling_update.jsonl")
    args = ap.parse_args()
    if args.pairs < 3:
        ap.error("at least three pairs")
    with open(args.out, "w") as out:
        for n in args.n_cells or [32, 74]:
            measure(n, args.pairs, out)


if __name__ == "__main__":
    main()
