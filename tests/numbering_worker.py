"""Checks of the block-0 numbering (alfd_set_numbering), run in a process of their own by tests/test_gpu_numbering.py:
    python tests/numbering_worker.py REPORT.json
torch is imported before the library is loaded so that the tensors of the *_device calls and the library share one HIP
runtime (tests/device_vectors_worker.py has the reason).

The reference of every check is the hand-permuted route: a second context WITHOUT numbering whose operators were permuted
with solver.permute_csr, level-0 transfers and row blocks in numpy, and whose vectors are permuted in numpy.  The
feature is a pure relabelling, so everything compares as bits (np.array_equal on the uint64 view), counts and residual
histories included.  The report maps check name -> "ok" or the traceback and is rewritten after every check."""
import ctypes as C
import json
import os
import sys
import traceback

import torch  # noqa: I001  -- before the library is loaded (see above)
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import cases  # noqa: E402
import test_immersed_hierarchy as base  # noqa: E402
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver  # noqa: E402

GUARD = -12345.5
EDGE_SHAPES = ["laplace2d_81", "laplace2d_5329", "stokes2d_8"]
PERMUTATIONS = ["identity", "reversal", "random", "points_of_cuthill_mckee"]
AL = (_abi.AL2, _abi.AL_STOKES, _abi.AL_STOKES_DIAG)


# ------------------------------------------------------------------------------------------------------ helpers
def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def record(res):
    d = res.as_dict()
    d.pop("solve_seconds")
    return d


def to_internal(blocks, n2o):
    """a block vector of the caller in the numbering of the hand-permuted context"""
    return [np.ascontiguousarray(blocks[0][n2o])] + [np.array(b, np.float64) for b in blocks[1:]]


def to_caller(blocks, n2o):
    out0 = np.empty_like(blocks[0])
    out0[n2o] = blocks[0]
    return [out0] + [np.array(b, np.float64) for b in blocks[1:]]


def hand_permuted(pb, n2o, levels=None, row_blocks=None):
    """(problem, levels, row blocks) in the new numbering, by the tools a caller has today"""
    n2o = np.ascontiguousarray(n2o, np.int64)
    o2n = np.empty_like(n2o)
    o2n[n2o] = np.arange(n2o.size)
    mats = dict(pb.mats)
    mats["A"] = solver.permute_csr(pb.mats["A"], n2o, o2n)
    for rows, cols in (("Ct", "C"), ("Bt", "B")):
        if rows in pb.mats:
            mats[rows] = solver.permute_csr(pb.mats[rows], n2o, None)
            mats[cols] = solver.permute_csr(pb.mats[cols], None, o2n)
    vecs = dict(pb.vecs)
    vecs["f"] = np.ascontiguousarray(pb.vecs["f"][n2o])
    out = problems.SyntheticProblem(params=dict(pb.params), mats=mats, vecs=vecs)
    out.inv_w_override = pb.inv_w_override
    new_levels = None
    if levels is not None:
        first = levels[0]
        if hasattr(first[0], "row_ptr"):
            first = (solver.permute_csr(first[0], n2o, None),) + tuple(first[1:])
        else:
            first = (np.ascontiguousarray(np.asarray(first[0])[n2o]), first[1]) + tuple(first[2:3]) + \
                    tuple(None if w is None else np.ascontiguousarray(np.asarray(w)[n2o]) for w in first[3:4])
        new_levels = [first] + list(levels[1:])
    new_blocks = None if row_blocks is None else (row_blocks[0], o2n[np.asarray(row_blocks[1])].astype(np.int32))
    return out, new_levels, new_blocks


def guarded_views(blocks):
    """The blocks as views t[1:]-style into ONE larger tensor: every view starts at an odd element (8-byte, not 16-byte
    aligned) and has guard values before and after."""
    sizes = [len(b) for b in blocks]
    buf = torch.full((sum(sizes) + 2 * len(blocks) + 3,), GUARD, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    views, at = [], 1
    for b in blocks:
        v = buf[at:at + len(b)]
        assert len(b) == 0 or v.data_ptr() % 16 == 8
        v.copy_(torch.from_numpy(np.ascontiguousarray(b, np.float64)))
        views.append(v)
        at += len(b) + (len(b) + 1) % 2 + 1
    return buf, views


def guards_intact(buf, views):
    keep = torch.ones_like(buf, dtype=torch.bool)
    for t in views:
        o = (t.data_ptr() - buf.data_ptr()) // 8
        keep[o:o + t.numel()] = False
    return bool((buf[keep] == GUARD).all())


def host(tensors):
    return [t.cpu().numpy() for t in tensors]


def cuthill_mckee(pb):
    problems.permute_background_nodes(pb, problems.cuthill_mckee_nodes(pb))
    return pb


def permutation(kind, pb):
    n = pb.block_sizes[0]
    if kind == "identity":
        return np.arange(n, dtype=np.int64)
    if kind == "reversal":
        return np.arange(n, dtype=np.int64)[::-1].copy()
    if kind == "random":                                # single DoFs, not node-wise
        return np.random.default_rng(n).permutation(n).astype(np.int64)
    return solver.numbering_from_points(problems.row_support_points(pb))


# ------------------------------------------------------------------------------------------------ kernel edges
def edge_problem(shape, kind):
    if shape == "laplace2d_81":
        pb, want = problems.laplace2d_circle(n_cells=8), 81          # one partial chunk, odd length
    elif shape == "laplace2d_5329":
        pb, want = problems.laplace2d_circle(n_cells=72), 5329       # two chunks, the last partial and odd
    else:
        pb, want = problems.stokes2d_circle(n_cells=8), 578          # three blocks, two on the straight path
    if kind == "points_of_cuthill_mckee":
        cuthill_mckee(pb)
    assert pb.block_sizes[0] == want, pb.block_sizes
    cfg = _abi.default_config(_abi.AL_STOKES if "B" in pb.mats else _abi.AL2)
    cfg.inner.max_steps = 1000
    return pb, cfg


def kernel_edges(shape, kind):
    pb, cfg = edge_problem(shape, kind)
    n2o = permutation(kind, pb)
    pbh, _, _ = hand_permuted(pb, n2o)
    ctx = solver.context_from_problem(pb, cfg, numbering=n2o)
    ref = solver.context_from_problem(pbh, cfg)
    try:
        assert np.array_equal(ctx.numbering(), n2o) and ref.numbering() is None
        for seed in (1, 2):                                          # the second call meets the first one's staging
            src = cases.rng_blocks(pb, seed)
            want = to_caller(ref.system_apply(to_internal(src, n2o)), n2o)
            assert same(ctx.system_apply(src), want), ("host", seed)
            for scatter in (0, 1):                                   # both formulations of the unpack
                ctx.set_tunable("numbering_unpack_scatter", scatter)
                assert same(ctx.system_apply(src), want), ("host", seed, scatter)
                sbuf, s = guarded_views(src)
                dbuf, d = guarded_views([np.full(n, 3.0) for n in pb.block_sizes])
                ctx.system_apply_device(s, d)
                assert same(host(d), want), ("device", seed, scatter)
                assert same(host(s), src) and guards_intact(sbuf, s) and guards_intact(dbuf, d)
                ctx.system_apply_device(s, s)                        # dst aliases src
                assert same(host(s), want), ("in place", seed, scatter)
                assert guards_intact(sbuf, s)
            ctx.set_tunable("numbering_unpack_scatter", 0)
    finally:
        ctx.close()
        ref.close()


# --------------------------------------------------------------------------------------------------- operators
def operators():
    """alfd_spmv speaks the internal numbering (by contract): under a numbering it equals the hand-permuted context's on
    every slot the numbering touches."""
    pb, cfg = cases.case("stokes2d_circle")
    n2o = permutation("random", pb)
    pbh, _, _ = hand_permuted(pb, n2o)
    ctx = solver.context_from_problem(pb, cfg, numbering=n2o)
    ref = solver.context_from_problem(pbh, cfg)
    try:
        for slot, name in ((_abi.A, "A"), (_abi.BT, "Bt"), (_abi.B, "B"), (_abi.CT, "Ct"), (_abi.C_, "C")):
            m = pb.mats[name]
            x = np.random.default_rng(slot + 3).uniform(-1.0, 1.0, m.ncols)
            got, _ = ctx.spmv(slot, x, np.zeros(m.nrows))
            want, _ = ref.spmv(slot, x, np.zeros(m.nrows))
            assert np.array_equal(bits(got), bits(want)), name
        got = ctx.numbering()
        assert got.dtype == np.int64 and np.array_equal(got, n2o)
        n = C.c_int64(0)
        small = np.zeros(3, np.int64)                                # the capacity protocol
        assert ctx._lib.alfd_get_numbering(ctx._h, small.ctypes.data, 3, C.byref(n)) == _abi.E_INVALID
        assert n.value == n2o.size
    finally:
        ctx.close()
        ref.close()


def same_csr(a, b):
    return (a.nrows, a.ncols) == (b.nrows, b.ncols) and np.array_equal(a.row_ptr, b.row_ptr) and \
        np.array_equal(a.col, b.col) and np.array_equal(bits(a.val), bits(b.val))


def transfers():
    """The level-0 prolongator and aggregates come back as they were set, in the caller's order, and are stored in the
    internal one: the solve equals the hand-permuted context's."""
    for name in ("stokes3d_gmg", "stokes3d_multilevel"):
        pb, cfg = cases.case(name)
        levels = cases.aggregates_of(pb, cfg)
        n2o = permutation("random", pb)
        pbh, levels_h, _ = hand_permuted(pb, n2o, levels)
        ctx = solver.context_from_problem(pb, cfg, aggregates=levels, numbering=n2o)
        ref = solver.context_from_problem(pbh, cfg, aggregates=levels_h)
        try:
            if hasattr(levels[0][0], "row_ptr"):
                assert same_csr(ctx.prolongator(0), levels[0][0])
                assert same_csr(ref.prolongator(0), levels_h[0][0])
                assert not same_csr(levels[0][0], levels_h[0][0])
                if len(levels) > 1:
                    assert same_csr(ctx.prolongator(1), levels[1][0])     # below level 0 nothing is translated
            else:
                agg, nc = ctx.aggregates(0)
                assert np.array_equal(agg, np.asarray(levels[0][0], np.int32)) and nc == levels[0][1]
                assert np.array_equal(ref.aggregates(0)[0], np.asarray(levels_h[0][0], np.int32))
            whole_path_checks(pb, cfg, ctx, ref, n2o, device=False)
        finally:
            ctx.close()
            ref.close()


# -------------------------------------------------------------------------------------------------- whole path
def whole_path_checks(pb, cfg, ctx, ref, n2o, device=True):
    x0 = cases.rng_blocks(pb, 5)
    raw = cases.rhs_of(pb)
    # augment_rhs
    if cfg.variant in AL:
        rhs_ref = ref.augment_rhs(to_internal(raw, n2o))
        rhs = ctx.augment_rhs(raw)
        assert same(rhs, to_caller(rhs_ref, n2o)), "augment_rhs"
        if device:
            buf, r = guarded_views(raw)
            ctx.augment_rhs_device(r)
            assert same(host(r), rhs) and guards_intact(buf, r), "augment_rhs_device"
    else:
        rhs, rhs_ref = raw, to_internal(raw, n2o)
    # precond_apply
    pz_ref, pres_ref = ref.precond_apply(to_internal(x0, n2o))
    pz, pres = ctx.precond_apply(x0)
    assert same(pz, to_caller(pz_ref, n2o)) and record(pres) == record(pres_ref), "precond_apply"
    if device:
        sbuf, s = guarded_views(x0)
        dbuf, d = guarded_views([np.zeros(n) for n in pb.block_sizes])
        dres = ctx.precond_apply_device(s, d)
        assert same(host(d), pz) and record(dres) == record(pres_ref), "precond_apply_device"
        assert guards_intact(sbuf, s) and guards_intact(dbuf, d)
    # solve from a non-zero start
    x_ref, res_ref = ref.solve(rhs_ref, x0=to_internal(x0, n2o), raise_on_failure=False)
    hist_ref, inner_ref = ref.history(), ref.inner_iterations()
    assert res_ref.status == _abi.OK and res_ref.outer_iterations > 0 and len(hist_ref) > 1
    x, res = ctx.solve(rhs, x0=x0, raise_on_failure=False)
    assert record(res) == record(res_ref), (record(res), record(res_ref))
    assert np.array_equal(bits(ctx.history()), bits(hist_ref)) and ctx.inner_iterations() == inner_ref
    assert same(x, to_caller(x_ref, n2o)), "solve"
    if device:
        rbuf, r = guarded_views(rhs)
        xbuf, xd = guarded_views(x0)
        dres = ctx.solve_device(r, xd, raise_on_failure=False)
        assert record(dres) == record(res_ref) and np.array_equal(bits(ctx.history()), bits(hist_ref))
        assert same(host(xd), x) and same(host(r), rhs), "solve_device"
        assert guards_intact(rbuf, r) and guards_intact(xbuf, xd)
    # constraint_residual: one number, the same bits
    g = None if "A2" in pb.mats else pb.vecs["g"]
    assert bits(ctx.constraint_residual(x, g)) == bits(ref.constraint_residual(to_internal(x, n2o), g))


def whole_path_stokes3d():
    """The size and settings of test_reference_shaped_operator_matches_oracle: N = 16, cell-wise assembly, Cuthill-McKee,
    multilevel with tensor prolongators in the caller's numbering, one set_numbering_from_points call."""
    pb = cuthill_mckee(problems.stokes3d_sphere(16, 2, assembly="cellwise"))
    cfg = _abi.bench_multilevel_settings(_abi.default_config(_abi.AL_STOKES), geometric=True)
    pts = problems.row_support_points(pb)
    levels = problems.tensor_prolongators(pb.params, min_coarse=_abi.BENCH_MIN_COARSE,
                                          node_permutation=pb.node_permutation)
    n2o = solver.numbering_from_points(pts)
    pbh, levels_h, _ = hand_permuted(pb, n2o, levels)
    blocks = solver.brick_blocks_from_points(pts[n2o], (16, 4, 1))
    ctx = solver.context_from_problem(pb, cfg, aggregates=levels, numbering=pts)
    ref = solver.context_from_problem(pbh, cfg, aggregates=levels_h, row_blocks=blocks)
    try:
        assert np.array_equal(ctx.numbering(), n2o)
        got, want = ctx.matrix_info(_abi.A), ref.matrix_info(_abi.A)
        assert want["batch_major"] == 2 and want["shared_nnz"] > 0.8 * want["nnz"]
        for key in ("batch_major", "batch_major_wide", "shared_nnz", "streamed_bytes", "nnz"):
            assert got[key] == want[key], (key, got[key], want[key])
        whole_path_checks(pb, cfg, ctx, ref, n2o)
    finally:
        ctx.close()
        ref.close()


def whole_path_elliptic():
    """Elliptic interface with a hierarchy on block 1 as well: block 1 and its transfers stay as they are."""
    cf = base.config("a22_gmg_8")
    pb, cfg = cf.pb, cf.cfg
    n2o = permutation("random", pb)
    pbh, levels_h, _ = hand_permuted(pb, n2o, cf.levels0)
    ctx = solver.context_from_problem(pb, cfg, aggregates=cf.levels0, immersed_levels=cf.levels1, numbering=n2o)
    ref = solver.context_from_problem(pbh, cfg, aggregates=levels_h, immersed_levels=cf.levels1)
    try:
        assert same_csr(ctx.prolongator(0, block=1), cf.levels1[0][0])
        assert same_csr(ctx.prolongator(0, block=0), cf.levels0[0][0])
        whole_path_checks(pb, cfg, ctx, ref, n2o)
    finally:
        ctx.close()
        ref.close()


# ----------------------------------------------------------------------------------------------- setup_coupling
def setup_coupling():
    """The body moved: a new CT in the caller's order through alfd_setup_coupling gives the bits of a fresh hand-permuted
    setup (the smallest case of tests/test_gpu_setup_coupling.py: Stokes N = 8, tensor prolongators, patch)."""
    import test_gpu_setup_coupling as sc
    pb0, pb1 = sc._stokes3d(8, 1, sc.C0), sc._stokes3d(8, 1, sc.C1)
    _, cfg = cases.case("stokes3d_gmg_patch")
    levels = cases.aggregates_of(pb0, cfg)
    n2o = permutation("random", pb0)
    pbh, levels_h, _ = hand_permuted(pb1, n2o, levels)
    ctx = solver.context_from_problem(pb0, sc._copy(cfg), aggregates=levels, numbering=n2o)
    ref = solver.context_from_problem(pbh, sc._copy(cfg), aggregates=levels_h)
    try:
        sc._move(ctx, pb1, M=False)
        whole_path_checks(pb1, cfg, ctx, ref, n2o, device=False)
    finally:
        ctx.close()
        ref.close()


# ---------------------------------------------------------------------------------------------------- refusals
def refusals():
    lib = solver.load_library()
    pb = problems.laplace2d_circle(n_cells=8)
    cfg = _abi.default_config(_abi.AL2)
    cfg.inner.max_steps = 1000
    n = pb.block_sizes[0]
    n2o = permutation("random", pb)
    pbh, _, _ = hand_permuted(pb, n2o)
    x0 = cases.rng_blocks(pb, 9)
    plain = solver.context_from_problem(pb, cfg)
    hand = solver.context_from_problem(pbh, cfg)
    rhs = plain.augment_rhs(cases.rhs_of(pb))
    x_plain, res_plain = plain.solve(rhs, x0=x0)
    x_hand, res_hand = hand.solve(to_internal(rhs, n2o), x0=to_internal(x0, n2o))
    x_hand = to_caller(x_hand, n2o)
    plain.close()
    hand.close()

    def good_solve(ctx, numbered):
        x, res = ctx.solve(rhs, x0=x0)
        want, wres = (x_hand, res_hand) if numbered else (x_plain, res_plain)
        assert same(x, want) and record(res) == record(wres)

    def refused(call, status, word=None):
        try:
            call()
        except solver.AlfdError as e:
            assert e.status == status, (e.status, status, str(e))
            assert word is None or word in str(e), str(e)
        else:
            raise AssertionError("not refused")

    # a duplicate entry, non-finite points: nothing is set; then a numbering after set_matrix(A)
    ctx = solver.Context(0)
    try:
        dup = n2o.copy()
        dup[3] = dup[4]
        refused(lambda: ctx.set_numbering(dup), _abi.E_INVALID, "permutation")
        pts = problems.row_support_points(pb).copy()
        for bad in (np.nan, np.inf):
            pts[n // 2, 1] = bad
            refused(lambda: ctx.set_numbering_from_points(pts), _abi.E_INVALID, "non-finite")
        assert ctx.numbering() is None
        ctx.set_matrix(_abi.A, pb.mats["A"])
        refused(lambda: ctx.set_numbering(n2o), _abi.E_INVALID, "slot A")
        assert ctx.numbering() is None
        solver.upload_problem(ctx, pb, cfg)
        good_solve(ctx, numbered=False)
    finally:
        ctx.close()
    # wrong n at set_matrix; the same context never gets as far as a solve; cleared, it works
    ctx = solver.Context(0)
    try:
        ctx.set_numbering(np.arange(n + 1))
        refused(lambda: ctx.set_matrix(_abi.A, pb.mats["A"]), _abi.E_INVALID, "numbering")
        refused(lambda: ctx.set_matrix(_abi.CT, pb.mats["Ct"]), _abi.E_INVALID, "numbering")
        refused(lambda: ctx.set_matrix(_abi.C_, pb.mats["C"]), _abi.E_INVALID, "numbering")
        blocks = (C.c_void_p * 2)(*[b.ctypes.data for b in x0])
        res = _abi.Result()
        assert lib.alfd_solve(ctx._h, blocks, blocks, C.byref(res)) != _abi.OK     # no operator got in: no solve
        ctx.set_numbering(None)
        assert ctx.numbering() is None
        solver.upload_problem(ctx, pb, cfg, numbering=n2o)
        good_solve(ctx, numbered=True)
        # clearing (and replacing) with operators present
        refused(lambda: ctx.set_numbering(None), _abi.E_INVALID, "slot A")
        refused(lambda: ctx.set_numbering(np.arange(n)), _abi.E_INVALID, "slot A")
        assert np.array_equal(ctx.numbering(), n2o)
        good_solve(ctx, numbered=True)
    finally:
        ctx.close()
    # a partitioned context, in either call order
    group, single = solver.LocalGroup(2), solver.LocalGroup(1)
    ctx, ctx2 = solver.Context(0), solver.Context(0)
    try:
        ctx.comm_init_local(group.handle, 0)
        refused(lambda: ctx.set_numbering(n2o), _abi.E_UNSUPPORTED, "partitioned")
        assert ctx.numbering() is None
        ctx.comm_init_local(single.handle, 0)                        # one rank again
        solver.upload_problem(ctx, pb, cfg, numbering=n2o)
        good_solve(ctx, numbered=True)
        ctx2.set_numbering(n2o)
        refused(lambda: ctx2.comm_init_local(group.handle, 1), _abi.E_UNSUPPORTED, "numbering")
        solver.upload_problem(ctx2, pb, cfg)
        good_solve(ctx2, numbered=True)
    finally:
        ctx.close()
        ctx2.close()
        group.close()
        single.close()


CHECKS = [(f"kernel_edges[{s}-{k}]", lambda s=s, k=k: kernel_edges(s, k)) for s in EDGE_SHAPES for k in PERMUTATIONS]
CHECKS += [("operators", operators), ("transfers", transfers), ("whole_path[stokes3d]", whole_path_stokes3d),
           ("whole_path[elliptic]", whole_path_elliptic), ("setup_coupling", setup_coupling), ("refusals", refusals)]


def main(path, only=None):
    import time
    report = {}
    for name, fn in CHECKS:
        if only and not any(o in name for o in only):
            continue
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
        if any(s in report[name] for s in ("HIP error", "alfd status 2:", "hipError", "illegal memory access")):
            print("a HIP call failed: nothing more is started on the device", flush=True)
            break
    sys.stdout.flush()
    return 0 if all(v == "ok" for v in report.values()) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2:]))
