"""Wall time of one solve call with the vectors on the host (Context.solve = alfd_solve: upload, solve, download over
PCIe) and on the device (Context.solve_device = alfd_solve_device: pack, the same solve, unpack in HBM) at the bench
size, alternating, on one context.  The code behind alfd_solve did not change with the device calls, so the host leg
is also the figure of the commit before them.

    python profiles/device_vectors/measure.py [--n-cells 74] [--reps 5] --out profiles/device_vectors/measure_n74.jsonl

One JSON line per call: leg, wall seconds of the call (host clock; both calls return device-synchronised),
alfd_result::solve_seconds (the Krylov loop alone), counts; a last line says whether the two legs returned the same
bits.  Set-up as bench.py: geometric multigrid + interface patch, brick row blocks."""
import argparse
import json
import os
import sys
import time

import torch  # before the library is loaded: one HIP runtime for the tensors and the library
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n-cells", type=int, default=74)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", required=True)
args = ap.parse_args()

n = args.n_cells
refine = max(0, int(round(np.log2(n / 64.0))) + 4)
pb = problems.stokes3d_sphere(n_cells=n, immersed_refine=refine)
cfg = _abi.bench_multilevel_settings(_abi.default_config(_abi.AL_STOKES), True)
levels = problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE)
blocks = problems.brick_row_blocks(pb.params, (16, 4, 1))
ctx = solver.context_from_problem(pb, cfg, aggregates=levels, row_blocks=blocks)
rhs = ctx.augment_rhs([pb.vecs["f"], pb.vecs["rhs_p"], pb.vecs["g"]])
rhs_d = [torch.from_numpy(b).cuda() for b in rhs]
x_d = [torch.zeros(s, dtype=torch.float64, device="cuda") for s in pb.block_sizes]
vector_mb = sum(pb.block_sizes) * 8 / 1e6

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
out = open(args.out, "w")


def emit(**kw):
    out.write(json.dumps(kw) + "\n")
    out.flush()
    print(json.dumps(kw), flush=True)


def host_leg():
    t0 = time.perf_counter()
    x, res = ctx.solve(rhs)                                   # x0 = zeros made inside: part of what a host caller pays
    return time.perf_counter() - t0, res, x


def device_leg():
    for t in x_d:
        t.zero_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ctx.solve_device(rhs_d, x_d)
    return time.perf_counter() - t0, res, x_d


emit(n_cells=n, dof=int(sum(pb.block_sizes)), block_vector_mb=vector_mb, device=torch.cuda.get_device_name(0),
     hip_runtimes=[os.path.basename(p) for p in solver._hip_runtimes()])
host_leg(), device_leg()                                       # warm-up of both
xh = xd = None
for rep in range(args.reps):                                   # alternating
    for leg, fn in (("host", host_leg), ("device", device_leg)):
        wall, res, x = fn()
        emit(leg=leg, rep=rep, call_seconds=wall, solve_seconds=res.solve_seconds, outer=res.outer_iterations,
             inner=int(res.inner_iterations), status=res.status)
        if leg == "host":
            xh = x
        else:
            xd = [t.cpu().numpy() for t in x]
emit(same_bits=bool(all(np.array_equal(a, b) for a, b in zip(xh, xd))))
