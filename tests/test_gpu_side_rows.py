"""Side rows of the long-row batch-major form on the device (tunable "batch_major_side_rows", spmv_side_rows_kernel):
rows beyond 384 entries leave the row blocks for a side list that a launch of its own computes behind every batch-major
launch.  The bitwise reference is spmv_reference.Case: the oracle's canonical sums (entry k in lane k mod 64, one fma
chain per lane, the canonical tree) and the np.longdouble row sums with their derived bound.

  * launch_shape_cases.long_rows(3365, "few"): six planted rows of 1025 .. 511 entries (one 64 x 8-entry pass of the side
    kernel and less, exactly two passes, two passes and one entry) among rows of 40 .. 160, empty rows, far columns.
    Tunable on: batch-major with 6 side rows, all four epilogues; off: the form is refused as before, same bits.
  * the same on the caller's row blocks, with 1, 2 and 4 waves and 24-row blocks; through alfd_spmv_pair.
  * the operators of the locally refined meshes (654 and 294 rows of 385 .. 807 entries); system, preconditioner and
    inner-preconditioner applications at every ml_fuse x ml_tail_in_spmv against the tunable off; whole solves against
    tests/golden/refined_solves.json.
  * two and three in-process ranks, the halo overlap on and off: side rows that read halo columns run after the
    exchange, the others with the interior blocks.
  * the timing hooks.

ALFD_SPMV_WINDOW_MIN_BLOCKS = 1 lets matrices of a few thousand rows take the long-row forms."""
import json
import os
import threading

import numpy as np
import pytest

import launch_shape_cases as lc
import refined_cases as rc
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver
from spmv_reference import Case

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FEW = ("long", 3365, "few")
PLANTED = (1025, 1024, 1023, 513, 512, 511)


@pytest.fixture(autouse=True)
def _small_matrices_take_the_long_row_forms(built, monkeypatch):
    monkeypatch.setenv("ALFD_SPMV_WINDOW_MIN_BLOCKS", "1")          # read when a context is created


def _context(side, blocks=None, waves=None, rows=None):
    ctx = solver.Context(0)
    ctx.set_tunable("batch_major", 1)
    if side is not None:
        ctx.set_tunable("batch_major_side_rows", side)
    if waves is not None:
        ctx.set_tunable("batch_major_waves", waves)
    if rows is not None:
        ctx.set_tunable("batch_major_rows", rows)
    if blocks is not None:
        ctx.set_row_blocks(_abi.A, *blocks)
    return ctx


def _describe(tag, ctx, slot=_abi.A):
    info, rec, side = ctx.matrix_info(slot), ctx.last_spmv_launch(), ctx.side_rows(slot)
    print(tag, {k: info[k] for k in ("batch_major", "batch_major_wide", "batch_major_blocks", "batch_major_rows",
                                     "batch_major_waves", "shared_nnz", "streamed_bytes")},
          "side", side, "launch", {k: rec[k] for k in ("family_name", "lanes", "R", "U", "epilogue", "grid")})
    return info, rec, side


def test_tunable_default_and_refused_values():
    ctx = solver.Context(0)
    try:
        ctx.set_matrix(_abi.A, lc.long_rows(3365, "few"))             # the default is 0: the planted rows refuse the form
        assert ctx.matrix_info(_abi.A)["batch_major"] == 0
        assert not any(ctx.side_rows(_abi.A).values())
        for bad in (2, -1):
            with pytest.raises(solver.AlfdError) as e:
                ctx.set_tunable("batch_major_side_rows", bad)
            assert e.value.status == _abi.E_INVALID
        ctx.set_matrix(_abi.A, lc.long_rows(3365, "few"))             # a refused value changes nothing
        assert ctx.matrix_info(_abi.A)["batch_major"] == 0
        ctx.set_tunable("batch_major_side_rows", 1)                   # takes effect at the next alfd_set_matrix
        assert ctx.matrix_info(_abi.A)["batch_major"] == 0
        ctx.set_matrix(_abi.A, lc.long_rows(3365, "few"))
        assert ctx.matrix_info(_abi.A)["batch_major"] == 1 and ctx.side_rows(_abi.A)["rows"] == 6
    finally:
        ctx.close()


@pytest.mark.parametrize("side", [1, 0])
def test_planted_rows_bitwise_with_the_tunable_on_and_off(side):
    case = lc.case(*FEW)
    ctx = _context(side)
    try:
        ctx.set_matrix(_abi.A, case.m)
        case.check(ctx, ("few", side), mode1=True)
        info, rec, sr = _describe(f"side rows {side}", ctx)
        if side:
            assert info["batch_major"] == 1 and rec["family"] == _abi.SPMV_BATCH_MAJOR
            assert sr == dict(rows=6, nnz=sum(PLANTED), longest=1025, interior_rows=0, grid=2)
            assert rec["grid"] == info["batch_major_blocks"]          # the record is the batch-major launch's
        else:
            assert info["batch_major"] == 0 and rec["family"] != _abi.SPMV_BATCH_MAJOR
            assert not any(sr.values())
    finally:
        ctx.close()


def test_no_long_row_no_side_list():
    case = lc.case("long", 3365, "few", 384)
    infos = []
    for side in (0, 1):
        ctx = _context(side)
        try:
            ctx.set_matrix(_abi.A, case.m)
            case.check(ctx, ("longest 384", side))
            assert not any(ctx.side_rows(_abi.A).values())
            infos.append(ctx.matrix_info(_abi.A))
        finally:
            ctx.close()
    assert infos[0]["batch_major"] == 1 and infos[0] == infos[1]       # the same plan


def _run_blocks(n, size):
    ptr = np.append(np.arange(0, n, size), n).astype(np.int64)
    return ptr, np.arange(n, dtype=np.int32)


@pytest.mark.parametrize("blocks,waves,rows", [("runs", 1, None), ("runs", 2, None), ("runs", 4, 24), ("runs", 8, None),
                                               ("caller", 4, None), ("caller", 2, None), ("caller", 1, None)])
def test_launch_shapes_bitwise(blocks, waves, rows):
    case = lc.case(*FEW)
    ctx = _context(1, _run_blocks(case.m.nrows, 120) if blocks == "caller" else None, waves, rows)
    try:
        ctx.set_matrix(_abi.A, case.m)
        case.check(ctx, (blocks, waves, rows), mode1=True)
        info, rec, sr = _describe(f"shape {blocks} {waves} {rows}", ctx)
        assert info["batch_major"] == (2 if blocks == "caller" else 1)
        assert rec["family"] == _abi.SPMV_BATCH_MAJOR and rec["R"] == (4 if info["batch_major_wide"] else waves)
        assert sr["rows"] == 6 and sr["nnz"] == sum(PLANTED)
        if rows:
            assert info["batch_major_rows"] == rows and info["batch_major_blocks"] >= case.m.nrows // rows
    finally:
        ctx.close()


def test_pair_launch_equals_the_separate_launches():
    case = lc.case(*FEW)
    n = case.m.ncols
    rng = np.random.default_rng(17)
    nc = 203                                                          # rows of about 16 entries, every 11th empty
    cols = [np.zeros(0, np.int64) if r % 11 == 5 else np.sort(rng.choice(n, int(rng.integers(9, 24)), replace=False))
            for r in range(nc)]
    rp = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int64)
    c = problems.Csr(nc, n, rp, np.concatenate(cols).astype(np.int32), rng.uniform(-1.0, 1.0, int(rp[-1])))
    d = rng.uniform(0.5, 2.0, nc) * np.exp2(np.arange(nc) % 41 - 20.0)
    ctx = _context(1)
    try:
        ctx.set_matrix(_abi.A, case.m)
        ctx.set_matrix(_abi.C_, c)
        ia, ic = ctx.matrix_info(_abi.A), ctx.matrix_info(_abi.C_)
        assert ia["batch_major"] == 1 and ia["batch_major_wide"] == 0 and ctx.side_rows(_abi.A)["rows"] == 6
        assert (ic["lanes"], ic["windowed"], ic["batch_major"]) == (16, 0, 0), ic
        y_ref, _ = ctx.spmv(_abi.A, case.x, np.full(n, np.nan), mode=0)
        t_ref = ctx.spmv_scaled(_abi.C_, case.x, d, np.full(nc, np.nan))
        y, t = ctx.spmv_pair(_abi.A, _abi.C_, case.x, d, np.full(n, np.nan), np.full(nc, np.nan))
        rec = ctx.last_spmv_launch()
        assert rec["family"] == _abi.SPMV_BATCH_MAJOR and rec["grid"] > ia["batch_major_blocks"]   # both parties, one grid
        assert np.array_equal(y_ref, case.s) and np.array_equal(y, y_ref) and np.array_equal(t, t_ref)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def refined(built):
    return {(6, 1): rc.problem("stokes3d_sphere"),
            (12, 2): problems.stokes3d_sphere(12, 2, assembly="cellwise", local_refine=1)}


@pytest.mark.parametrize("mesh,long_rows", [((6, 1), 294), ((12, 2), 654)])
def test_refined_mesh_operator_bitwise(refined, mesh, long_rows):
    A = refined[mesh].mats["A"]
    ln = np.diff(np.asarray(A.row_ptr))
    assert int((ln > 384).sum()) == long_rows
    case = Case(A, 77 + mesh[0])
    ctx = _context(1)
    try:
        ctx.set_matrix(_abi.A, A)
        case.check(ctx, ("refined", mesh), mode1=True)
        info, rec, sr = _describe(f"refined {mesh}", ctx)
        assert info["batch_major"] == 1 and rec["family"] == _abi.SPMV_BATCH_MAJOR
        assert sr["rows"] == long_rows and sr["nnz"] == int(ln[ln > 384].sum()) and sr["longest"] == int(ln.max())
        assert 8 * sr["nnz"] <= A.nnz
    finally:
        ctx.close()


def _multilevel_context(pb, side):
    cfg = rc.config("stokes3d_sphere", "multilevel")
    ctx = solver.Context(0)
    ctx.set_tunable("batch_major_side_rows", side)
    return solver.upload_problem(ctx, pb, cfg, rc.levels("stokes3d_sphere", "multilevel"))


def _applications(ctx, pb):
    rng = np.random.default_rng(31)
    src = [rng.uniform(-1.0, 1.0, n) for n in pb.block_sizes]
    out = list(ctx.system_apply(src))
    got, res = ctx.precond_apply(src)
    out += list(got) + [np.array([res.inner_iterations, res.mp_iterations], np.float64)]
    out.append(ctx.inner_prec_apply(src[0]))
    return out


def test_applications_at_every_fusion_level_equal_the_tunable_off(refined):
    pb = refined[(6, 1)]
    off = _multilevel_context(pb, 0)
    try:
        assert off.matrix_info(_abi.A)["batch_major"] == 0
        ref = _applications(off, pb)
    finally:
        off.close()
    ctx = _multilevel_context(pb, 1)
    try:
        assert ctx.matrix_info(_abi.A)["batch_major"] == 1 and ctx.side_rows(_abi.A)["rows"] == 294
        for fuse in range(4):
            for tail in (0, 1):
                ctx.set_tunable("ml_fuse", fuse)
                ctx.set_tunable("ml_tail_in_spmv", tail)
                got = _applications(ctx, pb)
                for k, (g, r) in enumerate(zip(got, ref)):
                    assert np.array_equal(g, r), (fuse, tail, k)
    finally:
        ctx.close()


@pytest.mark.parametrize("prec", rc.PRECONDITIONERS)
@pytest.mark.parametrize("name", rc.SOLVE_CASES)
def test_solves_reproduce_the_golden_runs(name, prec):
    pb, cfg = rc.problem(name), rc.config(name, prec)
    ctx = solver.Context(0)
    try:
        ctx.set_tunable("batch_major_side_rows", 1)
        solver.upload_problem(ctx, pb, cfg, rc.levels(name, prec))
        info, sr = ctx.matrix_info(_abi.A), ctx.side_rows(_abi.A)
        x, res = ctx.solve(ctx.augment_rhs(rc.rhs_of(pb)))
        hist = ctx.history()
    finally:
        ctx.close()
    print("refined solve with side rows", name, prec, "batch_major", info["batch_major"], "lanes", info["lanes"], sr,
          "outer", res.outer_iterations, "inner", res.inner_iterations)
    if name == "stokes3d_sphere":                                     # A really ran batch-major, its long rows aside
        assert info["batch_major"] == 1 and sr["rows"] == 294
    gold = json.load(open(os.path.join(GOLDEN, "refined_solves.json")))[f"{name}/{prec}"]
    assert res.status == 0
    assert (res.outer_iterations, res.inner_iterations, res.mp_iterations) == \
        (gold["outer_iterations"], gold["inner_iterations"], gold["mp_iterations"])
    assert [float(h).hex() for h in hist] == gold["history"]


def _run_ranks(case, offsets):
    """One context and thread per rank; per rank (matrix_info, side_rows, launch record, [y0, y1, y2, (y3, y3b)])."""
    world = len(offsets) - 1
    group = solver.LocalGroup(world)
    out, errs = [None] * world, []

    def work(rank):
        try:
            rows = slice(offsets[rank], offsets[rank + 1])
            local = lc.row_slice(case.m, rows.start, rows.stop)
            ctx = solver.Context(0)
            ctx.comm_init_local(group.handle, rank)
            ctx.set_partition([offsets, offsets])
            ctx.set_tunable("batch_major", 1)
            ctx.set_tunable("batch_major_side_rows", 1)
            ctx.set_tunable("batch_major_rows", 8)                    # 3 rows in 100 read a far column: 8-row blocks leave
            ctx.set_matrix(_abi.A, local)                             # blocks without a halo column, for the overlap
            nan = np.full(local.nrows, np.nan)
            y0, _ = ctx.spmv(_abi.A, case.x[rows], nan, mode=0)
            y1, _ = ctx.spmv(_abi.A, case.x[rows], case.y0[rows], mode=1, alpha=-0.75)
            y2 = ctx.spmv_scaled(_abi.A, case.x[rows], case.d[rows], nan)
            y3 = ctx.spmv_scaled(_abi.A, case.x[rows], case.d[rows], nan, nan)
            out[rank] = (ctx.matrix_info(_abi.A), ctx.side_rows(_abi.A), ctx.last_spmv_launch(), [y0, y1, y2, y3])
            ctx.close()
        except Exception as e:   # noqa: BLE001
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    group.close()
    assert not errs, errs
    assert all(o is not None for o in out)
    return out


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("offsets", [(0, 1700, 3365), (0, 900, 2750, 3365)])
def test_partitioned_contexts_bitwise(monkeypatch, offsets, overlap):
    """Cut at 1700, the 1025-entry row 1693 and the five rows behind the cut all read the other rank's columns; the
    middle rank of three holds all six, four of them without a halo column."""
    monkeypatch.setenv("ALFD_SPMV_OVERLAP_HALO", str(overlap))
    case = lc.case(*FEW)
    rp, col = np.asarray(case.m.row_ptr), np.asarray(case.m.col)
    ln = np.diff(rp)
    out = _run_ranks(case, list(offsets))
    seen = [0, 0]
    for rank, (info, sr, rec, _) in enumerate(out):
        lo, hi = offsets[rank], offsets[rank + 1]
        long_rows = [r for r in range(lo, hi) if ln[r] > 384]
        inside = [r for r in long_rows if np.all((col[rp[r]:rp[r + 1]] >= lo) & (col[rp[r]:rp[r + 1]] < hi))]
        print("partitioned", offsets, "overlap", overlap, "rank", rank, sr, "interior blocks",
              info["batch_major_interior_blocks"], "of", info["batch_major_blocks"], rec["family_name"], rec["grid"])
        assert info["batch_major"] == 1 and rec["family"] == _abi.SPMV_BATCH_MAJOR, (rank, info)
        assert sr["rows"] == len(long_rows) and sr["nnz"] == int(ln[long_rows].sum()), (rank, sr)
        assert sr["interior_rows"] == len(inside) and sr["longest"] == (int(ln[long_rows].max()) if long_rows else 0)
        seen[0] += len(inside)
        seen[1] += len(long_rows) - len(inside)
    assert seen[0] + seen[1] == 6 and seen[1] > 0
    if len(offsets) == 4:
        assert seen[0] > 0 and out[1][1]["rows"] == 6                  # both groups on one rank,
        assert 0 < out[1][0]["batch_major_interior_blocks"] < out[1][0]["batch_major_blocks"]   # which splits its launch
    ys = [np.concatenate([o[3][e] for o in out]) for e in range(3)]
    assert np.array_equal(ys[0], case.s), "epilogue 0"
    assert np.array_equal(ys[1], lc.mode1_reference(*FEW)), "epilogue 1"
    case.check_scaled(ys[2], "epilogue 2")
    assert np.array_equal(np.concatenate([o[3][3][0] for o in out]), case.s), "epilogue 3: y"
    case.check_scaled(np.concatenate([o[3][3][1] for o in out]), "epilogue 3: y2")


def test_timing_hooks_leave_the_operator_intact(refined):
    case = lc.case(*FEW)
    ctx = _context(1)
    try:
        ctx.set_matrix(_abi.A, case.m)
        before = ctx.side_rows(_abi.A)
        for value_index in (True, False):
            ms, nbytes = ctx.bench_spmv_format(_abi.A, reps=3, value_index=value_index)
            assert ms > 0 and nbytes > 0
        ms, _ = ctx.bench_spmv(_abi.A, reps=3)
        assert ms > 0 and ctx.side_rows(_abi.A) == before and ctx.matrix_info(_abi.A)["batch_major"] == 1
        case.check(ctx, "after the timing hooks")
    finally:
        ctx.close()
    pb = refined[(6, 1)]
    ctx = _multilevel_context(pb, 1)
    try:
        r = np.random.default_rng(5).uniform(-1.0, 1.0, pb.block_sizes[0])
        z = ctx.inner_prec_apply(r)
        timed = 0
        for op, level in ((_abi.OPERATOR_LEVEL, 1), (_abi.OPERATOR_PATCH_SS, 0), (_abi.OPERATOR_PATCH_S, 0)):
            for rows, waves in ((0, 0), (48, 2)):
                try:
                    us, shape = ctx.bench_operator(op, level, rows, waves, reps=3)
                except solver.AlfdError as e:                         # no such operator, or not in the long-row form
                    assert e.status in (_abi.E_INVALID, _abi.E_UNSUPPORTED)
                    continue
                timed += 1
                print("bench_operator", op, level, rows, waves, "%.1f us" % us, shape)
                assert us > 0
        print("operators timed:", timed)
        assert np.array_equal(ctx.inner_prec_apply(r), z)
        assert ctx.side_rows(_abi.A)["rows"] == 294
    finally:
        ctx.close()
