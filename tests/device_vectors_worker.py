"""Checks of the device-resident vector calls (Context.*_device), run in a process of their own by
tests/test_gpu_device_vectors.py:  python tests/device_vectors_worker.py REPORT.json

Why a process of its own: the caller's tensors and the library must live in ONE HIP runtime.  The torch wheel ships a
HIP runtime of its own; imported BEFORE libalfd.so is loaded it serves both (the library's dependency resolves to the
copy already loaded), imported after it the process holds two runtimes and hipPointerGetAttributes of the library's
one does not know torch's allocations (the calls then refuse them with ALFD_E_INVALID).  A pytest process has loaded
the library long before this module's turn, so the checks start from a clean slate here, torch first.

Every check compares with np.array_equal against the host-pointer call on the same context and the same data: the
device calls run the same code behind one pack and one unpack launch, so no tolerance is involved.  The report maps
check name -> "ok" or the traceback; it is rewritten after every check, so a crash leaves the checks done so far."""
import ctypes as C
import json
import os
import sys
import threading
import traceback

import torch  # noqa: I001  -- before the library is loaded (see above)
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import cases  # noqa: E402
from fictitious_domain_al_preconditioners_amd import _abi, partition, problems, solver  # noqa: E402

SOLVE_CASES = ["laplace2d_circle", "stokes3d_sphere", "elliptic_modified", "rational_minres"]
# (background cells per side, immersed segments) -> block sizes [(cells + 1)^2, segments] of the 2-block AL2 system
CHUNK_CASES = {
    "exact_and_short": (63, 40),       # [4096, 40]: an exact multiple of the chunk, a block shorter than 64
    "multiple_plus_1": (16, 4097),     # [289, 4097]: three chunks, the last one holds a single entry
    "multiple_minus_1": (16, 4095),    # [289, 4095]
    "two_exact_chunks": (63, 8192),    # [4096, 8192]: three chunks, no padding at all
}


def dev(blocks):
    return [torch.from_numpy(np.ascontiguousarray(b, np.float64).copy()).cuda() for b in blocks]


def host(tensors):
    return [t.cpu().numpy() for t in tensors]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def record(res):
    d = res.as_dict()
    d.pop("solve_seconds")
    return d


_cache = {}


def context(name):
    """(problem, config, context, right-hand side as the reference hands it to the Krylov solver)"""
    if name not in _cache:
        pb, cfg = cases.case(name)
        ctx = solver.context_from_problem(pb, cfg, aggregates=cases.aggregates_of(pb, cfg))
        rhs = cases.rhs_of(pb)
        if cfg.variant in (_abi.AL2, _abi.AL_STOKES, _abi.AL_STOKES_DIAG):
            rhs = ctx.augment_rhs(rhs)
        _cache[name] = (pb, cfg, ctx, rhs)
    return _cache[name]


def solve_parity(name):
    pb, cfg, ctx, rhs = context(name)
    x0 = cases.rng_blocks(pb, 5)
    other_x = cases.rng_blocks(pb, 6)
    other_rhs = ctx.system_apply(cases.rng_blocks(pb, 7))      # a consistent right-hand side, non-zero everywhere
    # host path: a solve of other data first, then the one that is compared
    ctx.solve(other_rhs, x0=other_x, raise_on_failure=False)
    xh, resh = ctx.solve(rhs, x0=x0, raise_on_failure=False)
    hist_h, inner_h = ctx.history(), ctx.inner_iterations()
    assert resh.status == _abi.OK and resh.outer_iterations > 0 and len(hist_h) > 1
    # device path, same sequence on the same context: stale staging data or non-zero padding would show
    ro, xo = dev(other_rhs), dev(other_x)
    ctx.solve_device(ro, xo, raise_on_failure=False)
    r, x = dev(rhs), dev(x0)
    resd = ctx.solve_device(r, x, raise_on_failure=False)
    assert same(host(x), xh)
    assert np.array_equal(ctx.history(), hist_h)
    assert record(resd) == record(resh), (record(resd), record(resh))
    assert ctx.inner_iterations() == inner_h
    assert same(host(r), rhs)                                  # the right-hand side is an input only


def augment_and_resident():
    """augment_rhs_device, and upload_rhs_device / solve_resident / download_solution_device with and without a guess."""
    for name in ("laplace2d_circle", "stokes3d_sphere"):
        pb, cfg, ctx, rhs = context(name)
        raw = dev(cases.rhs_of(pb))
        ctx.augment_rhs_device(raw)
        assert same(host(raw), rhs), name
    pb, cfg, ctx, rhs = context("laplace2d_circle")
    x0 = cases.rng_blocks(pb, 11)
    for guess in (x0, None):
        ctx.upload_rhs(rhs, guess)
        resh = ctx.solve_resident()
        xh, hist_h = ctx.download_solution(), ctx.history()
        ctx.upload_rhs_device(dev(rhs), None if guess is None else dev(guess))
        resd = ctx.solve_resident()
        xd = [torch.full((n,), 7.0, dtype=torch.float64, device="cuda") for n in pb.block_sizes]
        ctx.download_solution_device(xd)
        assert same(host(xd), xh) and np.array_equal(ctx.history(), hist_h) and record(resd) == record(resh)


def chunk_edges(key):
    n_cells, segments = CHUNK_CASES[key]
    pb = problems.laplace2d_circle(n_cells, immersed_segments=segments)
    assert pb.block_sizes == [(n_cells + 1) ** 2, segments]
    cfg = _abi.default_config(_abi.AL2)
    cfg.inner.max_steps = 1000
    ctx = solver.context_from_problem(pb, cfg)
    try:
        for seed in (1, 2):                                    # twice: the second call meets the first one's staging
            src = cases.rng_blocks(pb, seed)
            ax = ctx.system_apply(src)
            pz, resh = ctx.precond_apply(src)
            s = dev(src)
            d = [torch.full((n,), 3.0, dtype=torch.float64, device="cuda") for n in pb.block_sizes]
            ctx.system_apply_device(s, d)
            assert same(host(d), ax), ("system_apply", seed)
            resd = ctx.precond_apply_device(s, d)
            assert same(host(d), pz), ("precond_apply", seed)
            assert record(resd) == record(resh)
            assert same(host(s), src)
    finally:
        ctx.close()


def odd_views(pb, blocks):
    """The blocks as slices of ONE tensor, every slice starting at an odd element: 8-byte, not 16-byte aligned."""
    buf = torch.zeros(sum(pb.block_sizes) + 2 * len(blocks) + 1, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    views, at = [], 1
    for b in blocks:
        v = buf[at:at + len(b)]
        assert v.data_ptr() % 16 == 8
        v.copy_(torch.from_numpy(np.ascontiguousarray(b)))
        views.append(v)
        at += len(b) + (len(b) + 1) % 2 + 1                    # next odd start, at least one element in between
    return buf, views


def views():
    pb, cfg, ctx, rhs = context("stokes3d_sphere")
    src = cases.rng_blocks(pb, 21)
    ax = ctx.system_apply(src)
    buf, v = odd_views(pb, src)
    _, out = odd_views(pb, [np.zeros(n) for n in pb.block_sizes])
    ctx.system_apply_device(v, out)                            # out of place, both sides views
    assert same(host(out), ax) and same(host(v), src)
    before = buf.clone()
    ctx.system_apply_device(v, v)                              # in place
    assert same(host(v), ax)
    untouched = torch.ones_like(buf, dtype=torch.bool)
    for t in v:
        o = (t.data_ptr() - buf.data_ptr()) // 8
        untouched[o:o + t.numel()] = False
    assert torch.equal(buf[untouched], before[untouched])       # nothing outside the blocks was written
    # the solution blocks alias the right-hand side blocks: x = guess = rhs on entry, the solution on return
    xh, resh = ctx.solve(rhs, x0=rhs, raise_on_failure=False)
    hist_h = ctx.history()
    _, both = odd_views(pb, rhs)
    resd = ctx.solve_device(both, both, raise_on_failure=False)
    assert same(host(both), xh) and np.array_equal(ctx.history(), hist_h) and record(resd) == record(resh)


def stream():
    """The right-hand side comes out of a chain of torch ops on a side stream that is NOT synchronised: the call has to
    wait for it on the device.  Once with the raw handle, once through torch's current stream (stream=None).
    Nothing between the chain and the call blocks the host: every tensor is made on the device BEFORE the chain (a
    copy from pageable host memory would wait for the stream, i.e. be the synchronise that must not be needed), the
    chain was run once to fill torch's allocator cache, and it writes the blocks in place over a known stale value --
    a call that did not wait reads -7 (seen once with the wait taken out of the library: this check then fails)."""
    pb, cfg, ctx, rhs = context("stokes3d_sphere")
    base = dev(rhs)
    x0 = cases.rng_blocks(pb, 31)
    side = torch.cuda.Stream()

    def chain(r, value):
        big = torch.full((1 << 25,), 0.5, dtype=torch.float64, device="cuda")
        for _ in range(40):                                    # some milliseconds of work in front of the blocks
            big = big * 0.999 + 0.001
        shift = big[::4096].sum() * 0.0 + value
        for t, b in zip(r, base):
            torch.mul(b * 3.0 + shift, 0.5, out=t)

    with torch.cuda.stream(side):                              # warm-up: allocator cache, kernels loaded
        chain([torch.empty_like(b) for b in base], 1.0)
    torch.cuda.synchronize()
    for explicit in (True, False):
        r = [torch.full_like(b, -7.0) for b in base]
        out = [torch.empty_like(b) for b in base]
        x = dev(x0)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            chain(r, 0.5 if explicit else 0.25)
            if explicit:
                ctx.system_apply_device(r, out, stream=side.cuda_stream)
            else:
                assert torch.cuda.current_stream().cuda_stream == side.cuda_stream
                res = ctx.solve_device(r, x, raise_on_failure=False)
        torch.cuda.synchronize()
        r_host = host(r)                                       # the values the chain produced
        assert not any((b == -7.0).any() for b in r_host)
        if explicit:
            assert same(host(out), ctx.system_apply(r_host))
        else:
            xh, resh = ctx.solve(r_host, x0=x0, raise_on_failure=False)
            assert same(host(x), xh) and record(res) == record(resh)


def warm_start():
    pb, cfg, ctx, rhs = context("stokes3d_sphere")
    x0 = cases.rng_blocks(pb, 41)
    # loose first solve, so that the second one has work left
    loose = _abi.Control(_abi.CTRL_REDUCTION, 1000, 1e-8, 1e-3)
    tight = _abi.Control(cfg.outer.kind, cfg.outer.max_steps, cfg.outer.tol, cfg.outer.reduce)
    try:
        ctx.set_controls(outer=loose)
        xh, _ = ctx.solve(rhs, x0=x0)
        r, x = dev(rhs), dev(x0)
        ctx.solve_device(r, x)
        assert same(host(x), xh)
        ctx.set_controls(outer=tight)
        xh2, resh = ctx.solve(rhs, x0=xh)
        hist_h, inner_h = ctx.history(), ctx.inner_iterations()
        assert resh.outer_iterations > 0
        resd = ctx.solve_device(r, x)                           # starts from the x the first call returned
        assert same(host(x), xh2) and np.array_equal(ctx.history(), hist_h)
        assert record(resd) == record(resh) and ctx.inner_iterations() == inner_h
    finally:
        ctx.set_controls(outer=tight)


def table(pointers):
    t = (C.c_void_p * len(pointers))()
    for i, p in enumerate(pointers):
        t[i] = p
    return t


def validation():
    lib = solver.load_library()
    pb, cfg, ctx, rhs = context("laplace2d_circle")
    x0 = cases.rng_blocks(pb, 51)
    xh, resh = ctx.solve(rhs, x0=x0)
    hist_h = ctx.history()

    def still_solves():
        r, x = dev(rhs), dev(x0)
        resd = ctx.solve_device(r, x)
        assert same(host(x), xh) and np.array_equal(ctx.history(), hist_h) and record(resd) == record(resh)

    good = dev(x0)
    out = [torch.zeros_like(t) for t in good]
    gp, op = [t.data_ptr() for t in good], [t.data_ptr() for t in out]
    hp = [b.ctypes.data for b in x0]                           # host (numpy) addresses
    res = _abi.Result()
    refused = [
        ("host src", lambda: lib.alfd_system_apply_device(ctx._h, table(hp), table(op), None)),
        ("host dst", lambda: lib.alfd_system_apply_device(ctx._h, table(gp), table(hp), None)),
        ("one host block", lambda: lib.alfd_system_apply_device(ctx._h, table([gp[0], hp[1]]), table(op), None)),
        ("null block", lambda: lib.alfd_system_apply_device(ctx._h, table([gp[0], None]), table(op), None)),
        ("null dst block", lambda: lib.alfd_precond_apply_device(ctx._h, table(gp), table([None, op[1]]), None, None)),
        ("host rhs", lambda: lib.alfd_solve_device(ctx._h, table(hp), table(op), C.byref(res), None)),
        ("host x", lambda: lib.alfd_solve_device(ctx._h, table(gp), table(hp), C.byref(res), None)),
        ("host upload", lambda: lib.alfd_upload_rhs_device(ctx._h, table(hp), None, None)),
        ("host guess", lambda: lib.alfd_upload_rhs_device(ctx._h, table(gp), table(hp), None)),
        ("host download", lambda: lib.alfd_download_solution_device(ctx._h, table(hp), None)),
        ("host augment", lambda: lib.alfd_augment_rhs_device(ctx._h, table(hp), None)),
        ("null table", lambda: lib.alfd_system_apply_device(ctx._h, None, table(op), None)),
    ]
    for what, call in refused:
        assert call() == _abi.E_INVALID, what
        if what != "null table":
            assert lib.alfd_last_error(ctx._h), what
        still_solves()
    assert same(host(good), x0) and all(not t.any() for t in out)      # nothing was launched on the refused blocks
    # a block that runs past the end of its allocation (unpack would write there): one 4 MiB allocation of the
    # runtime the library runs on, block 0 (n0 doubles) placed on its last double; placed on its first one it is fine
    hip = C.CDLL("libamdhip64.so.7")                         # the copy already loaded (same soname)
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    raw, size = C.c_void_p(), 4 << 20
    assert pb.block_sizes[0] * 8 < size and hip.hipMalloc(C.byref(raw), size) == 0
    try:
        last = raw.value + size - 8
        assert lib.alfd_system_apply_device(ctx._h, table(gp), table([last, op[1]]), None) == _abi.E_INVALID
        assert b"allocation" in lib.alfd_last_error(ctx._h)
        assert lib.alfd_system_apply_device(ctx._h, table([last, gp[1]]), table(op), None) == _abi.E_INVALID
        assert lib.alfd_system_apply_device(ctx._h, table(gp), table([raw.value, op[1]]), None) == _abi.OK
        still_solves()
    finally:
        hip.hipFree(raw)
    for t in out:
        t.zero_()
    # Python front end: ValueError before the library is called
    bad = [
        [good[0].float(), good[1]],                                          # dtype
        [good[0][:-1], good[1]],                                             # length
        [torch.zeros(2 * good[0].numel(), dtype=torch.float64, device="cuda")[::2], good[1]],   # not contiguous
        [good[0].reshape(-1, 1), good[1]],                                   # not 1-D
        [x0[0], x0[1]],                                                      # numpy arrays
        [good[0]],                                                           # a block short
    ]
    for blocks in bad:
        for call in (lambda b: ctx.system_apply_device(b, out), lambda b: ctx.system_apply_device(good, b),
                     lambda b: ctx.solve_device(b, out), lambda b: ctx.augment_rhs_device(b)):
            try:
                call(blocks)
            except ValueError:
                continue
            raise AssertionError(("no ValueError", [getattr(t, "shape", None) for t in blocks]))
    still_solves()
    # before alfd_setup
    fresh = solver.Context(0)
    try:
        for rc in (lib.alfd_solve_device(fresh._h, table(gp), table(op), C.byref(res), None),
                   lib.alfd_system_apply_device(fresh._h, table(gp), table(op), None),
                   lib.alfd_precond_apply_device(fresh._h, table(gp), table(op), None, None),
                   lib.alfd_upload_rhs_device(fresh._h, table(gp), None, None),
                   lib.alfd_download_solution_device(fresh._h, table(op), None),
                   lib.alfd_augment_rhs_device(fresh._h, table(op), None)):
            assert rc == _abi.E_NOT_SETUP, rc
    finally:
        fresh.close()
    # the rational variant has no right-hand side augmentation, on device blocks either
    pbr, cfgr, ctxr, rhsr = context("rational_minres")
    d = dev(rhsr)
    assert lib.alfd_augment_rhs_device(ctxr._h, table([t.data_ptr() for t in d]), None) == _abi.E_UNSUPPORTED
    try:
        ctxr.augment_rhs_device(d)
    except solver.AlfdError as e:
        assert e.status == _abi.E_UNSUPPORTED
    else:
        raise AssertionError("augment_rhs_device on the rational variant did not raise")
    assert same(host(d), rhsr)


def two_ranks(variant):
    """solver.LocalGroup(2), one thread per rank, each with its own tensors: the partitioned device-path solve equals
    the partitioned host-path solve of the same context bit for bit.  "multigrid": the aggregation multigrid on an even
    split.  "empty_rank_multigrid": the same multigrid with rank 0 owning no multiplier row -- its last block is empty
    and travels as a null pointer.  "empty_rank": that partition with the Chebyshev sweep."""
    world, n, ref = 2, 8, 0
    cfg = _abi.default_config(_abi.AL_STOKES)
    cfg.inner.max_steps = 1000
    plan = partition.slab_partition_stokes3d(n, ref, world)
    levels = None
    if variant.startswith("empty_rank"):
        nl = int(plan.offsets[-1][-1])
        plan.offsets[-1] = np.array([0, 0, nl], np.int64)
        assert plan.local_sizes(0)[-1] == 0
    if variant.endswith("multigrid"):
        cfg.inner_prec = _abi.PREC_MULTILEVEL
        cfg.ml_smooth_degree, cfg.ml_smooth_ratio = 2, 8.0
        full = problems.stokes3d_sphere(n, ref)
        levels = partition.partitioned_geometric_aggregates(full.params, plan, a=2, min_coarse=100)
    group = solver.LocalGroup(world)
    done, errs = [False] * world, []

    def work(rank):
        try:
            pb = problems.stokes3d_sphere(n, ref, row_ranges=plan.generator_ranges(rank))
            ctx = solver.Context(0)
            ctx.comm_init_local(group.handle, rank)
            ctx.set_partition(plan.offsets)
            solver.upload_problem(ctx, pb, cfg, partition.local_aggregates(levels, rank) if levels else None)
            raw = cases.rhs_of(pb)
            x0 = cases.rng_blocks(pb, 60 + rank)
            # every call below is collective: both ranks issue the same sequence
            rhs = ctx.augment_rhs(raw)
            ax = ctx.system_apply(x0)
            xh, resh = ctx.solve(rhs, x0=x0)
            hist_h, inner_h = ctx.history(), ctx.inner_iterations()
            r, x = dev(raw), dev(x0)
            if variant.startswith("empty_rank") and rank == 0:
                assert r[2].numel() == 0 and ctx._dev(r, "rhs")[2] is None
            ctx.augment_rhs_device(r)
            assert same(host(r), rhs), (rank, "augment_rhs")
            out = [torch.empty_like(t) for t in x]
            ctx.system_apply_device(x, out)
            assert same(host(out), ax), (rank, "system_apply")
            resd = ctx.solve_device(r, x)
            assert same(host(x), xh), (rank, "solution")
            assert np.array_equal(ctx.history(), hist_h) and record(resd) == record(resh), (rank, "history")
            assert ctx.inner_iterations() == inner_h and resh.outer_iterations > 0
            ctx.close()
            done[rank] = True
        except BaseException:   # noqa: BLE001
            errs.append((rank, traceback.format_exc()))

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errs, errs
    assert all(done), "RANK HUNG: a rank did not finish within the limit"
    group.close()


TWO_RANK_VARIANTS = ("multigrid", "empty_rank", "empty_rank_multigrid")
CHECKS = [(f"solve_parity[{name}]", lambda name=name: solve_parity(name)) for name in SOLVE_CASES]
CHECKS += [("augment_and_resident", augment_and_resident)]
CHECKS += [(f"chunk_edges[{key}]", lambda key=key: chunk_edges(key)) for key in CHUNK_CASES]
CHECKS += [("views", views), ("stream", stream), ("warm_start", warm_start), ("validation", validation)]
CHECKS += [(f"two_ranks[{v}]", lambda v=v: two_ranks(v)) for v in TWO_RANK_VARIANTS]


def main(path):
    import time
    report = {}
    for name, fn in CHECKS:
        t0 = time.time()
        try:
            fn()
            torch.cuda.synchronize()
            report[name] = "ok"
        except BaseException:   # noqa: BLE001
            report[name] = traceback.format_exc()
        print(f"{name}: {'ok' if report[name] == 'ok' else 'FAILED'} ({time.time() - t0:.1f} s)", flush=True)
        with open(path, "w") as f:
            json.dump(report, f)
        if any(s in report[name] for s in ("HIP error", "alfd status 2:", "hipError", "illegal memory access", "RANK HUNG")):
            print("a HIP call failed or a rank hung: nothing more is started on the device", flush=True)
            break
    sys.stdout.flush()
    os._exit(0 if all(v == "ok" for v in report.values()) else 1)   # a rank thread left in a collective must not hold the exit


if __name__ == "__main__":
    main(sys.argv[1])
