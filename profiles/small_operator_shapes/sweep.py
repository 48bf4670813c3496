"""Row-block shapes of the small long-row batch-major operators of the benchmark system, timed one by one.

    python profiles/small_operator_shapes/sweep.py [--n-cells 74] [--reps 200] [--repeats 3] [--out sweep_n74.jsonl]

Sets the benchmark system up once (bench.py's settings: N^3 Taylor-Hood, geometric hierarchy, patch, bricks 16x4x1 on A),
then times A[S,S] and A[S,:] of the interface patch and A_1, A_2 of the hierarchy with alfd_bench_operator: first as the
solver holds them (`repeats` times: the spread every other figure is read against), then re-planned at every shape of

    rows per block in {16, 32, 48, 64, 96}  x  waves per workgroup in {1, 2, 4}

(a second copy of the operator beside the solver's; 200 back-to-back launches on the solver's stream between two HIP
events, one warm-up launch first).  One JSON line per (operator, shape): microseconds per launch, blocks, batches, the
share of the entries in template-shared batches, LDS bytes of a workgroup; "rule": the shape alfd_host_small_shape gives
from the operator's 96 x 4 plan on this device.  The switch "batch_major_small" is 0 during the setup, so "as held" is
the context-wide shape."""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--n-cells", type=int, default=74)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import ctypes as C
import numpy as np
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver

HERE = os.path.dirname(os.path.abspath(__file__))
out_path = args.out or os.path.join(HERE, f"sweep_n{args.n_cells}.jsonl")
out_file = open(out_path, "w")


def emit(**fields):
    line = json.dumps(fields, sort_keys=True)
    print(line, flush=True)
    out_file.write(line + "\n")
    out_file.flush()


n = args.n_cells
refine = max(0, int(round(np.log2(n / 64.0))) + 4)
t0 = time.time()
pb = problems.stokes3d_sphere(n_cells=n, immersed_refine=refine)
cfg = _abi.bench_multilevel_settings(_abi.default_config(_abi.AL_STOKES), geometric=True)
cfg.inner.max_steps = 100
levels = problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE)
ctx = solver.Context(0)
ctx.set_tunable("batch_major_small", 0)
solver.upload_problem(ctx, pb, cfg, levels, problems.brick_row_blocks(pb.params, (16, 4, 1)))
cus = ctx.matrix_info(_abi.A)["batch_major_compute_units"]
emit(kind="system", n_cells=n, compute_units=cus, setup_wall_s=round(time.time() - t0, 1), library_phases_s=ctx.setup_seconds())

OPS = [("A[S,S]", _abi.OPERATOR_PATCH_SS, 0), ("A[S,:]", _abi.OPERATOR_PATCH_S, 0),
       ("level 1", _abi.OPERATOR_LEVEL, 1), ("level 2", _abi.OPERATOR_LEVEL, 2)]


def facts(us, info):
    return dict(us_per_launch=round(us, 3), rows=info["batch_major_rows"], waves=info["batch_major_waves"],
                blocks=info["batch_major_blocks"], batches=info["batch_major_batches"],
                shared_share=round(info["shared_nnz"] / max(info["nnz"], 1), 4), lds_bytes=info["batch_major_lds_bytes"])


for name, op, level in OPS:
    try:
        held = ctx.operator_info(op, level)
    except solver.AlfdError as e:
        emit(kind="skipped", operator=name, why=str(e))
        continue
    if not (held["batch_major"] and held["lanes"] == 64):
        emit(kind="skipped", operator=name, why="not in the long-row batch-major form", info=held)
        continue
    r, w = C.c_int32(), C.c_int32()
    rc = solver.load_library().alfd_host_small_shape(held["nrows"], held["batch_major_blocks"], held["batch_major_batches"],
                                                     held["batch_major_rows"], held["batch_major_waves"], cus, C.byref(r), C.byref(w))
    emit(kind="rule", operator=name, nrows=held["nrows"], nnz=held["nnz"], rows=r.value, waves=w.value, rc=rc)
    for k in range(args.repeats):
        us, info = ctx.bench_operator(op, level, reps=args.reps)
        emit(kind="as held", operator=name, repeat=k, nnz=info["nnz"], **facts(us, info))
    for rows in (16, 32, 48, 64, 96):
        for waves in (1, 2, 4):
            t1 = time.time()
            try:
                us, info = ctx.bench_operator(op, level, rows, waves, args.reps)
            except solver.AlfdError as e:
                emit(kind="shape", operator=name, rows=rows, waves=waves, error=str(e))
                continue
            emit(kind="shape", operator=name, plan_and_time_s=round(time.time() - t1, 2), **facts(us, info))
ctx.close()
out_file.close()
