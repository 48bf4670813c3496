"""Wall time of one solve call on the cell-wise, Cuthill-McKee operator of bench.py's reference_shaped_leg, by the route
the caller's vectors take, alternating, warm, repeated (the method of profiles/device_vectors/measure.py):

  a_scatter / a_gather  the library numbering (alfd_set_numbering_from_points) on caller-order DEVICE vectors
                        (alfd_solve_device), block 0 leaving through unpack_blocks_perm_scatter_kernel /
                        unpack_blocks_perm_kernel, the default (tunable "numbering_unpack_scatter" = 1 / 0)
  b_floor               the same operators hand-permuted, no numbering, device vectors already in the internal order:
                        the plain pack / unpack kernels, the only way to use device vectors with such an operator before
  c_host_loops          what a caller had before: host vectors, block 0 permuted by a single-threaded loop on the way in
                        (right-hand side and guess) and back on the way out (numpy fancy indexing, as the adapter's
                        loops did), around alfd_solve on the hand-permuted context

    python profiles/numbering/measure.py [--n-cells 64] [--reps 5] --out profiles/numbering/measure_n64.jsonl

One JSON line per call: leg, wall seconds of the call (host clock; every call returns device-synchronised),
alfd_result::solve_seconds (the Krylov loop alone), counts; the last lines say whether the routes returned the same
bits.  call - solve loop is the pack + unpack (+ copies) of the route."""
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
ap.add_argument("--n-cells", type=int, default=64)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", required=True)
args = ap.parse_args()

n = args.n_cells
refine = max(0, int(round(np.log2(n / 64.0))) + 4)
cfg = _abi.bench_multilevel_settings(_abi.default_config(_abi.AL_STOKES), True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
out = open(args.out, "w")


def emit(**kw):
    out.write(json.dumps(kw) + "\n")
    out.flush()
    print(json.dumps(kw), flush=True)


# the caller's problem: cell-wise sums, Cuthill-McKee numbering; everything the caller holds is in that numbering
t0 = time.time()
pb = problems.stokes3d_sphere(n_cells=n, immersed_refine=refine, assembly="cellwise")
problems.permute_background_nodes(pb, problems.cuthill_mckee_nodes(pb))
pts = problems.row_support_points(pb)
levels = problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE, node_permutation=pb.node_permutation)
t_problem = time.time() - t0
print(f"# problem, points and transfers in the caller's numbering: {t_problem:.1f} s", flush=True)
t0 = time.time()
ctx_a = solver.context_from_problem(pb, cfg, aggregates=levels, numbering=pts)
t_upload_a = time.time() - t0
print(f"# numbering from points, uploads, setup: {t_upload_a:.1f} s", flush=True)
n2o = ctx_a.numbering()
rhs = ctx_a.augment_rhs([pb.vecs["f"], pb.vecs["rhs_p"], pb.vecs["g"]])
info_a = ctx_a.matrix_info(_abi.A)
sizes = list(pb.block_sizes)

# the hand-permuted route of before: the problem itself renumbered (node-wise, as bench.py does), bricks from the points
nc = pb.params["ncomp"]
t0 = time.time()
problems.permute_background_nodes(pb, n2o[::nc] // nc)
pts_b = problems.row_support_points(pb)
levels_b = problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE, node_permutation=pb.node_permutation)
blocks_b = solver.brick_blocks_from_points(pts_b, (16, 4, 1))
ctx_b = solver.context_from_problem(pb, cfg, aggregates=levels_b, row_blocks=blocks_b)
t_upload_b = time.time() - t0
info_b = ctx_b.matrix_info(_abi.A)
rhs_b = [np.ascontiguousarray(rhs[0][n2o])] + rhs[1:]

emit(n_cells=n, dof=int(sum(sizes)), block0=int(sizes[0]), block_vector_mb=sum(sizes) * 8 / 1e6,
     device=torch.cuda.get_device_name(0), problem_s=t_problem, upload_setup_a_s=t_upload_a, hand_route_s=t_upload_b,
     bytes_per_nnz_a=info_a["streamed_bytes"] / info_a["nnz"], bytes_per_nnz_b=info_b["streamed_bytes"] / info_b["nnz"],
     same_form=bool(all(info_a[k] == info_b[k] for k in ("batch_major", "batch_major_wide", "shared_nnz", "streamed_bytes"))))

rhs_d = [torch.from_numpy(b).cuda() for b in rhs]
rhs_bd = [torch.from_numpy(b).cuda() for b in rhs_b]
x_d = [torch.zeros(s, dtype=torch.float64, device="cuda") for s in sizes]
in0, guess0, out0 = np.empty(sizes[0]), np.empty(sizes[0]), np.empty(sizes[0])
zeros = [np.zeros(s) for s in sizes]


def device_leg(ctx, r, scatter=None):
    if scatter is not None:
        ctx.set_tunable("numbering_unpack_scatter", scatter)
    for t in x_d:
        t.zero_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ctx.solve_device(r, x_d)
    wall = time.perf_counter() - t0
    return wall, res, [t.cpu().numpy() for t in x_d]


def host_loops_leg():
    t0 = time.perf_counter()
    np.take(rhs[0], n2o, out=in0)                              # in_ptrs: the right-hand side
    np.take(zeros[0], n2o, out=guess0)                         # out_ptrs(load): the guess
    x, res = ctx_b.solve([in0] + rhs[1:], x0=[guess0] + zeros[1:])
    out0[n2o] = x[0]                                           # finish_out
    wall = time.perf_counter() - t0
    return wall, res, [out0.copy()] + x[1:]


LEGS = [("a_scatter", lambda: device_leg(ctx_a, rhs_d, 1)), ("a_gather", lambda: device_leg(ctx_a, rhs_d, 0)),
        ("b_floor", lambda: device_leg(ctx_b, rhs_bd)), ("c_host_loops", host_loops_leg)]
for _, fn in LEGS:                                             # warm-up of every leg
    fn()
last = {}
for rep in range(args.reps):                                   # alternating
    for leg, fn in LEGS:
        wall, res, x = fn()
        emit(leg=leg, rep=rep, call_seconds=wall, solve_seconds=res.solve_seconds,
             around_ms=(wall - res.solve_seconds) * 1e3, outer=res.outer_iterations, inner=int(res.inner_iterations),
             status=res.status, it_per_s=res.outer_iterations / wall)
        last[leg] = x
back = [np.empty(sizes[0])] + last["b_floor"][1:]
back[0][n2o] = last["b_floor"][0]
for leg in ("a_scatter", "a_gather", "c_host_loops"):
    emit(leg=leg, same_bits_as_b_floor=bool(all(np.array_equal(p, q) for p, q in zip(last[leg], back))))
