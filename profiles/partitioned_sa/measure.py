"""Build seconds of the (0, 4) smoothed-aggregation hierarchy on the hanging-node operator, one rank against two
in-process ranks (one GPU).  Writes build_seconds.json beside this file.  Run from anywhere: python measure.py"""
import json
import os
import sys
import threading
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases  # noqa: E402
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver  # noqa: E402

BUILD = dict(block_size=3, threshold=0.02, max_aggregate_nodes=8, damping=4.0 / 3.0, min_coarse=300,
             drop_tolerance=0.0, max_row_entries=4)


def cfg():
    c = _abi.default_config(_abi.AL_STOKES)
    c.inner_prec = _abi.PREC_MULTILEVEL
    return c


def upload(ctx, A, C, Ct, w):
    ctx.set_matrix(_abi.A, A)
    ctx.set_matrix(_abi.C_, C)
    ctx.set_matrix(_abi.CT, Ct)
    ctx.set_diag(_abi.INVW, w)
    ctx.configure(cfg())


def one_rank(pb):
    ctx = solver.Context(0)
    upload(ctx, pb.mats["A"], pb.mats["C"], pb.mats["Ct"], pb.inv_w_diag_squared())
    t0 = time.perf_counter()
    levels = ctx.build_smoothed_aggregation(**BUILD)
    dt = time.perf_counter() - t0
    ctx.close()
    return dt, levels


def two_ranks(pb):
    A, C, Ct, w = pb.mats["A"], pb.mats["C"], pb.mats["Ct"], pb.inv_w_diag_squared()
    nn, nl = A.nrows // 3, C.nrows
    offs = [np.array([0, nn // 2, nn], np.int64) * 3, np.array([0, nl // 2, nl], np.int64)]
    group = solver.LocalGroup(2)
    out, errs = [None, None], []

    def work(rank):
        try:
            ctx = solver.Context(0)
            ctx.comm_init_local(group.handle, rank)
            ctx.set_partition(offs)
            u0, u1, l0, l1 = (int(x) for x in (offs[0][rank], offs[0][rank + 1], offs[1][rank], offs[1][rank + 1]))
            upload(ctx, A.slice_rows(u0, u1), C.slice_rows(l0, l1), Ct.slice_rows(u0, u1), w[l0:l1])
            t0 = time.perf_counter()
            levels = ctx.build_smoothed_aggregation(**BUILD)
            out[rank] = (time.perf_counter() - t0, levels)
            ctx.close()
        except Exception as e:   # noqa: BLE001
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=400)
    assert not errs and all(o is not None for o in out), errs
    group.close()
    return max(o[0] for o in out), out


res = []
for n in (16, 32):
    pb = cases.hanging_node_variant(problems.stokes3d_sphere(n, 0))
    one_rank(pb)                                       # warm-up (module load, allocator)
    t1, lev1 = one_rank(pb)
    t2, out2 = two_ranks(pb)
    same = all(np.array_equal(np.concatenate([out2[0][1][0][0].val, out2[1][1][0][0].val]), lev1[0][0].val)
               for _ in (0,)) and all(np.array_equal(out2[0][1][l][0].val, lev1[l][0].val) for l in range(1, len(lev1)))
    row = dict(N=n, rows=int(pb.mats["A"].nrows), levels=[int(nc) for _, nc in lev1], one_rank_build_s=round(t1, 3),
               two_ranks_one_gpu_build_s=round(t2, 3), same_bits=bool(same))
    print(row, flush=True)
    res.append(row)
json.dump(dict(setting="hanging-node Stokes operator, theta 0.02, <= 8 nodes, min_coarse 300, truncation (0, 4); "
                       "two in-process ranks share ONE GPU: the figure shows what the extra collectives and the "
                       "redundant coarse levels cost, not a speed-up", results=res),
          open(os.path.join(HERE, "build_seconds.json"), "w"), indent=1)
