"""alfd_estimate_spectrum on the bench operator (Stokes, N cells per direction): steps, kappa, wall milliseconds and
launches per CG iteration, device-stepped against host-stepped, alternating; and the per-launch time of the products
through the full slots ALFD_CT / ALFD_C (alfd_bench_spmv) beside the compacted ones.  One JSON line per figure."""
import argparse, json, math, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=74)
ap.add_argument("--steps", type=int, default=2000, help="cap of the timed runs (per-iteration figures)")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", required=True)
args = ap.parse_args()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
out = open(args.out, "a")


def emit(**rec):
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")
    out.flush()


t = time.time()
refine = max(0, int(round(math.log2(args.n / 64.0))) + 4)       # bench.py's choice
pb = problems.stokes3d_sphere(n_cells=args.n, immersed_refine=refine)
print(f"problem N = {args.n}: {time.time() - t:.1f} s, blocks {pb.block_sizes}", flush=True)
cfg = _abi.default_config(_abi.AL_STOKES)      # Chebyshev inner preconditioner: no patch, the library extracts C[:,S] itself
t = time.time()
ctx = solver.context_from_problem(pb, cfg)
print(f"upload + setup {time.time() - t:.1f} s", flush=True)
Ct = pb.mats["Ct"]
emit(what="operator", N=args.n, n_u=int(Ct.nrows), n_lambda=int(Ct.ncols), nnz_C=int(Ct.nnz),
     S=int(np.count_nonzero(np.diff(Ct.row_ptr))))


def run(host, ctl):
    ctx.set_tunable("spectrum_host_stepped", host)
    ctx.enable_timing(0)
    t0 = time.perf_counter()
    s = ctx.estimate_spectrum(control=ctl)      # returns after the last device synchronisation
    return s, time.perf_counter() - t0


ctl = _abi.Control(_abi.CTRL_ABS, args.steps, 1e-12, 0.0)
run(0, ctl), run(1, ctl)                        # warm-up of both paths (first use also builds the extractions)
for rep in range(args.repeats):
    for host in (0, 1):
        s, sec = run(host, ctl)
        emit(what="timed", stepping="host" if host else "device", repeat=rep, steps=int(s.steps), converged=int(s.converged),
             wall_ms=1e3 * sec, ms_per_iteration=1e3 * sec / max(s.steps, 1), kappa=s.condition)
for host in (0, 1):                             # launches per iteration (event timing on: not a timed run)
    ctx.set_tunable("spectrum_host_stepped", host)
    ctx.enable_timing(2)
    s = ctx.estimate_spectrum(control=ctl)
    tm = ctx.timing()
    n = sum(v["launches"] for v in tm.values())
    emit(what="launches", stepping="host" if host else "device", steps=int(s.steps), launches=int(n),
         launches_per_iteration=n / max(s.steps, 1), kernel_ms_by_class={k: v["ms"] for k, v in tm.items()})
ctx.enable_timing(0)
for slot, name in ((_abi.CT, "CT"), (_abi.C_, "C")):
    ms, nbytes = ctx.bench_spmv(slot, 50)
    emit(what="full_slot_spmv", slot=name, ms_per_launch=ms, algorithmic_bytes=nbytes)
ctx.set_tunable("spectrum_host_stepped", 0)
t0 = time.perf_counter()
s = ctx.estimate_spectrum()                     # the reference's control: SolverControl(n_lambda, 1e-12)
emit(what="default_control", stepping="device", steps=int(s.steps), converged=int(s.converged), kappa=s.condition,
     lambda_min=s.lambda_min, lambda_max=s.lambda_max, last_residual=s.last_residual,
     wall_ms=1e3 * (time.perf_counter() - t0))
ctx.close()
