"""What single-precision operator values inside the inner preconditioner (alfd_set_preconditioner_values) buy on a
matrix with general values.

One process, one GPU.  The benchmark's problem (bench.py: Stokes, Taylor-Hood on N^3 cells, geometric hierarchy, interface
patch) with every entry of A multiplied by 1 + 2^-24 u_ij, u_ij = u_ji in [0, 1) from a hash of the unordered pair (i, j),
so that no value repeats; contexts are created with ALFD_SPMV_VALUE_INDEX = 0 (no dictionary-coded form is planned, as
for values that never repeat), which puts A on the 10 B/nnz window kernel.

  launch   per candidate launch shape (R, U) of the float window kernel: `repeats` x (alfd_bench_spmv of `reps` launches
           on the 8-byte values, alfd_bench_spmv_preconditioner on the copy), each after the hook's own warm-up
  solve    one context, bench settings: warm-up + `solves` solves with the option off (the baseline: the parent's
           behaviour), then the option on + alfd_setup and the same solves; device memory after each setup

One JSON line per measurement.  There is no CPU path: without a GPU the script fails.

    python profiles/prec_values/measure.py --n-cells 56 --out prec_values.jsonl
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

os.environ["ALFD_SPMV_VALUE_INDEX"] = "0"

from fictitious_domain_al_preconditioners_amd import _abi, problems, solver  # noqa: E402

SHAPES = ((2, 8), (2, 16), (4, 8), (4, 16))


def perturb_in_place(A, bits=24, chunk=1 << 22):
    """a_ij *= 1 + 2^-bits u_ij, rows in chunks (the arrays of the bench size do not fit twice)."""
    rp = np.asarray(A.row_ptr, np.int64)
    for r0 in range(0, A.nrows, chunk // 128):
        r1 = min(A.nrows, r0 + chunk // 128)
        k0, k1 = int(rp[r0]), int(rp[r1])
        row = np.repeat(np.arange(r0, r1, dtype=np.uint64), np.diff(rp[r0:r1 + 1]))
        col = A.col[k0:k1].astype(np.uint64)
        lo, hi = np.minimum(row, col), np.maximum(row, col)
        h = (lo * np.uint64(2654435761) + hi * np.uint64(40503) + (lo ^ hi) * np.uint64(2246822519)) % np.uint64(1 << 20)
        A.val[k0:k1] *= 1.0 + 2.0 ** -bits * (h.astype(np.float64) / float(1 << 20))


def stats(v):
    v = np.asarray(v, float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(v.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-cells", type=int, default=56)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--solves", type=int, default=3)
    ap.add_argument("--out", default="prec_values.jsonl")
    args = ap.parse_args()
    n = args.n_cells
    out = open(args.out, "a")

    def emit(**rec):
        out.write(json.dumps(rec) + "\n")
        out.flush()
        print(json.dumps(rec), flush=True)

    refine = max(0, int(round(np.log2(n / 64.0))) + 4)                 # bench.py's rule
    t0 = time.time()
    pb = problems.stokes3d_sphere(n_cells=n, immersed_refine=refine)
    A = pb.mats["A"]
    perturb_in_place(A)
    emit(what="problem", n_cells=n, blocks=[int(b) for b in pb.block_sizes], nnz_A=int(A.nnz), host_seconds=time.time() - t0)

    for R, U in SHAPES:
        os.environ["ALFD_SPMV_PREC32_R"], os.environ["ALFD_SPMV_PREC32_U"] = str(R), str(U)
        ctx = solver.Context(0)
        try:
            ctx.set_preconditioner_values("fp32")
            ctx.set_matrix(_abi.A, A)
            info, pv = ctx.matrix_info(_abi.A), ctx.preconditioner_values()
            assert info["windowed"] == 1 and info["batch_major"] == 0 and info["value_indexed"] == 0, info
            assert pv["stored"] == 1 and pv["family"] == 2, pv
            ms64, ms32 = [], []
            for _ in range(args.repeats):
                ms64.append(ctx.bench_spmv(_abi.A, args.reps)[0])
                ms32.append(ctx.bench_spmv_preconditioner(args.reps)[0])
            b64, b32 = pv["streamed_bytes_fp64"], pv["streamed_bytes_fp32"]
            emit(what="launch", n_cells=n, shape=[R, U], reps=args.reps, ms_fp64=stats(ms64), ms_fp32=stats(ms32),
                 ratio=float(np.median(ms32) / np.median(ms64)), bytes_fp64=b64, bytes_fp32=b32,
                 gbs_fp64=b64 / np.median(ms64) * 1e-6, gbs_fp32=b32 / np.median(ms32) * 1e-6,
                 window_blocks=info["window_blocks"], window_fallback_blocks=info["window_fallback_blocks"],
                 flushed_to_zero=pv["flushed_to_zero"])
        finally:
            ctx.close()
    os.environ.pop("ALFD_SPMV_PREC32_R"), os.environ.pop("ALFD_SPMV_PREC32_U")

    cfg = _abi.bench_multilevel_settings(_abi.default_config(_abi.AL_STOKES), geometric=True)
    levels = problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE)
    ctx = solver.Context(0)
    try:
        solver.upload_problem(ctx, pb, cfg, levels)
        rhs = ctx.augment_rhs([pb.vecs["f"], pb.vecs["rhs_p"], pb.vecs["g"]])
        for values in ("fp64", "fp32"):
            if values == "fp32":
                ctx.set_preconditioner_values("fp32")
                ctx.setup(pb.block_sizes)
            free, total = ctx.device_memory()
            secs, last = [], None
            for k in range(args.solves + 1):                         # the first is the warm-up
                t1 = time.time()
                _, res = ctx.solve(rhs)
                if k:
                    secs.append(time.time() - t1)
                last = res
            pv = ctx.preconditioner_values()
            emit(what="solve", n_cells=n, values=values, used=pv["used"], seconds=stats(secs), outer=last.outer_iterations,
                 inner=int(last.inner_iterations), mp=int(last.mp_iterations), residual=last.last_residual,
                 device_bytes_in_use=int(total - free), copy_bytes=pv["copy_bytes"])
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
