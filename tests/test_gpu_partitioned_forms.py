"""Every SpMV storage form on a row-partitioned context, bit for bit against the unpartitioned product.

Every kernel has a `(c < n_local) ? x[c] : x_halo[c - n_local]` branch -- the window kernels inside the staging loop and
again in the fallback path -- and tests/test_gpu_multirank.py reaches it on the long-row batch-major form alone.  Here the
matrices of launch_shape_cases.py (a few thousand rows; ALFD_SPMV_WINDOW_MIN_BLOCKS = 1 lets a rank of a few row blocks
take the window forms) are cut into row slices with global columns, one in-process rank per slice:

  * world 2, offsets [0, 1700, n]: the cut is no multiple of any row block;
  * world 3, offsets [0, 1500, 1537, n]: the 37-row rank holds less than one window block and runs another form than its
    neighbours -- the stream kernel for 64 lanes, spmv_kernel<L> for short rows (lanes follow the global matrix).

Every rank's slice references columns of every other rank (asserted).  Each rank runs epilogues 0, 1, 2 and 3 out of
NaN-prefilled outputs on its slices of x, d and y0; the concatenated rows must equal the references of the
spmv_reference.Case on the UNPARTITIONED matrix: the oracle's canonical sums bit for bit (lanes are chosen from global
statistics, so the sums do not depend on the partition) and the np.longdouble row sums within the derived bound.  Each
rank also reports its matrix_info and the family alfd_get_last_spmv_launch names, compared after the threads have
joined (an assertion inside one rank's thread would leave the others waiting in a collective).

The value-indexed forms are chosen per rank: of `coded` the leading rank holds the 8-bit and 16-bit thirds and runs the
value-indexed kernels, the trailing rank mostly random values and so the general window kernel.  alfd_set_partition
takes two blocks at least: both carry the same offsets, slot A maps block 0 to block 0."""
import threading

import numpy as np
import pytest

import launch_shape_cases as lc
from fictitious_domain_al_preconditioners_amd import _abi, solver

pytestmark = pytest.mark.gpu

F = _abi
WIN = {"ALFD_SPMV_WINDOW_MIN_BLOCKS": 1, "ALFD_SPMV_WINDOW_SHORT_MIN_BLOCKS": 1}
# form -> (case, environment, tunable batch_major, family of the large ranks (first, last), family of the 37-row rank,
#          matrix_info of the large ranks (first, last))
FORMS = {
    "plain64": (("random", 3365, 70), {"ALFD_SPMV_STREAM_R": 0}, None, (F.SPMV_PLAIN,) * 2, F.SPMV_PLAIN,
                (dict(lanes=64, windowed=0),) * 2),
    "plain32": (("random", 3365, 30), {}, None, (F.SPMV_PLAIN,) * 2, F.SPMV_PLAIN, (dict(lanes=32, windowed=0),) * 2),
    "plain16": (("random", 3365, 14), {}, None, (F.SPMV_PLAIN,) * 2, F.SPMV_PLAIN, (dict(lanes=16, windowed=0),) * 2),
    "plain8": (("random", 3365, 7), {}, None, (F.SPMV_PLAIN,) * 2, F.SPMV_PLAIN, (dict(lanes=8, windowed=0),) * 2),
    "plain4": (("random", 3365, 3), {}, None, (F.SPMV_PLAIN,) * 2, F.SPMV_PLAIN, (dict(lanes=4, windowed=0),) * 2),
    "sparse_rows": (("random", 3365, 20, 3), {}, None, (F.SPMV_SPARSE_ROWS,) * 2, F.SPMV_SPARSE_ROWS,
                    (dict(lanes=16, windowed=0),) * 2),
    "stream": (("long", 3365, "random"), {"ALFD_SPMV_WINDOW": 0}, None, (F.SPMV_STREAM,) * 2, F.SPMV_STREAM,
               (dict(lanes=64, windowed=0),) * 2),
    "window": (("long", 3365, "random"), WIN, 0, (F.SPMV_WINDOW,) * 2, F.SPMV_STREAM,
               (dict(lanes=64, windowed=1, value_indexed=0, window_fallback_blocks=0),) * 2),
    # the wide half does not fit 512 slots: the rank that holds only wide rows keeps no window form at all
    "window_maxw512": (("long", 3365, "random"), dict(WIN, ALFD_SPMV_WINDOW_MAXW=512), 0, (F.SPMV_WINDOW, F.SPMV_STREAM),
                       F.SPMV_STREAM, (dict(lanes=64, windowed=1, value_indexed=0), dict(lanes=64, windowed=0))),
    "vi_class_batched": (("long", 3365, "coded"), WIN, 0, (F.SPMV_WINDOW_VIB, F.SPMV_WINDOW), F.SPMV_STREAM,
                         (dict(lanes=64, windowed=1, value_indexed=1), dict(lanes=64, windowed=1, value_indexed=0))),
    "vi_in_order": (("long", 3365, "coded"), dict(WIN, ALFD_SPMV_VI_BATCHED=0), 0, (F.SPMV_WINDOW_VI, F.SPMV_WINDOW),
                    F.SPMV_STREAM, (dict(lanes=64, windowed=1, value_indexed=1), dict(lanes=64, windowed=1, value_indexed=0))),
    "group32": (("short", 32), WIN, 0, (F.SPMV_WINDOW_GROUP,) * 2, F.SPMV_PLAIN, (dict(lanes=32, windowed=1, batch_major=0),) * 2),
    "group16": (("short", 16), WIN, 0, (F.SPMV_WINDOW_GROUP,) * 2, F.SPMV_PLAIN, (dict(lanes=16, windowed=1, batch_major=0),) * 2),
    "group8": (("short", 8), WIN, 0, (F.SPMV_WINDOW_GROUP,) * 2, F.SPMV_PLAIN, (dict(lanes=8, windowed=1, batch_major=0),) * 2),
    "batch_major_short": (("stencil",), WIN, 1, (F.SPMV_BATCH_MAJOR_SHORT,) * 2, F.SPMV_PLAIN,
                          (dict(lanes=8, windowed=1, batch_major=1),) * 2),
    # rows of at most 384 entries: what the long-row batch-major form takes
    "batch_major_runs": (("long", 3365, "few", 384), WIN, 1, (F.SPMV_BATCH_MAJOR,) * 2, F.SPMV_STREAM,
                         (dict(lanes=64, windowed=1, value_indexed=1, batch_major=1),) * 2),
}


def _offsets(world, n):
    return [0, 1700, n] if world == 2 else [0, 1500, 1537, n]


def _run_ranks(case, offsets, batch_major):
    """One context and thread per rank; returns per rank (matrix_info, launch record, [y0, y1, y2, (y3, y3b)])."""
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
            if batch_major is not None:
                ctx.set_tunable("batch_major", batch_major)
            ctx.set_matrix(_abi.A, local)
            nan = np.full(local.nrows, np.nan)
            y0, lanes = ctx.spmv(_abi.A, case.x[rows], nan, mode=0)
            y1, _ = ctx.spmv(_abi.A, case.x[rows], case.y0[rows], mode=1, alpha=-0.75)
            y2 = ctx.spmv_scaled(_abi.A, case.x[rows], case.d[rows], nan)
            y3 = ctx.spmv_scaled(_abi.A, case.x[rows], case.d[rows], nan, nan)
            out[rank] = (ctx.matrix_info(_abi.A), ctx.last_spmv_launch(), lanes, [y0, y1, y2, y3])
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


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("form", list(FORMS))
def test_partitioned_storage_form_bitwise(built, monkeypatch, form, world):
    key, env, batch_major, large, small, infos = FORMS[form]
    case = lc.case(*key)
    offsets = _offsets(world, case.m.nrows)
    assert lc.references_every_other_rank(case.m, offsets)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))                     # read when a context is created
    out = _run_ranks(case, offsets, batch_major)
    for rank, (info, rec, lanes, _) in enumerate(out):
        print("launch record", form, world, rank, rec["family_name"], rec["lanes"], rec["R"], rec["U"], rec["grid"],
              {k: info[k] for k in ("windowed", "value_indexed", "batch_major", "window_blocks", "window_fallback_blocks")})
    for rank, (info, rec, lanes, _) in enumerate(out):
        assert lanes == case.lanes == rec["lanes"], (form, rank, lanes, rec)
        assert rec["epilogue"] == 3, (form, rank, rec)
        if rec["family"] == F.SPMV_BATCH_MAJOR:   # the split launch around the halo exchange records its second half
            blocks, interior = info["batch_major_blocks"], info["batch_major_interior_blocks"]
            assert rec["grid"] == (blocks - interior if 0 < interior < blocks else blocks), (form, rank, rec, info)
        if world == 3 and rank == 1:
            assert rec["family"] == small and not info["windowed"] and not info["batch_major"], (form, rank, rec, info)
            continue
        which = 0 if rank == 0 else 1
        assert rec["family"] == large[which], (form, rank, rec, info)
        assert {k: info[k] for k in infos[which]} == infos[which], (form, rank, info)
    if form == "window_maxw512" and world == 2:   # halo columns in staged windows AND in blocks that gather from global memory
        info = out[0][0]
        assert 0 < info["window_fallback_blocks"] < info["window_blocks"], info
    ys = [np.concatenate([o[3][e] for o in out]) for e in range(3)]
    assert np.array_equal(ys[0], case.s), (form, "epilogue 0")
    assert np.array_equal(ys[1], lc.mode1_reference(*key)), (form, "epilogue 1")
    case.check_scaled(ys[2], (form, "epilogue 2"))
    assert np.array_equal(np.concatenate([o[3][3][0] for o in out]), case.s), (form, "epilogue 3: y")
    case.check_scaled(np.concatenate([o[3][3][1] for o in out]), (form, "epilogue 3: y2"))
