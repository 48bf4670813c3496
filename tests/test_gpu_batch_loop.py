"""The batch loop of spmv_vs_kernel (kernels_vs.hpp) at the edges of its prefetch depths.

A wave of the kernel holds the descriptors of its current and its next batch in two registers that swap roles from batch
to batch (the loop is unrolled by two), requests the descriptor after next into the one it has used up, and fetches the
stream words of its next shared batch at the end of the batch in front.  What
can go wrong there shows at the ends of a wave's batch list and where the kinds of batch change, so the operator below --
the Q2 three-component operator with grad-div at N = 6, 6 591 rows of up to 375 entries -- is cut up so that every such
edge occurs, and ctx.spmv (modes 0 and 1) is compared bit for bit with the oracle's canonical sums:

  rows      160 rows each (321: 40) truncated to 1, 65, 127, 128, 129 and 321 entries (classes 1, 2, 3 and 6 with a remainder
            of 1, of 63 and a full last chunk; neighbouring rows alike, so that translates stay translates: shared batches
            of 16, 8 and 4 rows as well as plain ones), rows filled up to 384 entries (class 6, full last chunk), untouched rows (classes
            1..6 as the mesh gives them), every 97th row empty, and every 5th row of a run perturbed, which is then no
            translate of anything: its wave's batches alternate shared / plain / shared;
  blocks    runs of the numbering at 16, 48 and 96 rows per block and mesh bricks, at 1, 2, 4 and 8 waves: blocks with
            fewer batches than waves, and the last block of the grid a short one;
  counts    with every row stored (batch_major_share 0: plain batches of four rows of one class) row blocks of
            4 k rows of ONE class hold exactly k batches: k = 1 .. 2 NW + 1 covers waves without a batch, with one batch
            (nothing to fetch ahead), with two (no descriptor after next) and with three; the same blocks with sharing on;
  wide      the 10-bit dictionary codes (every value multiplied by one of 16 factors);
  pair      one pair launch (the second party behind the grid of the first).

Each case takes a second or two; the references are computed once per matrix."""
import numpy as np
import pytest

from fictitious_domain_al_preconditioners_amd import _abi, problems, solver
from oracle import oracle

pytestmark = pytest.mark.gpu
GEN = dict(dim=3, degree=2, ncomp=3, stokes=False, grad_div=True, gamma_grad_div=10.0, radius=0.1, immersed_refine=0)
LENGTHS = (1, 65, 127, 128, 129, 321)
ALPHA = -0.75


class Ref:
    """A matrix, its inputs and the oracle's results for modes 0 and 1: computed once, left unchanged."""

    def __init__(self, m, seed):
        rng = np.random.default_rng(seed)
        self.m = m
        self.x = rng.uniform(-1.0, 1.0, m.ncols)
        self.y0 = rng.uniform(-1.0, 1.0, m.nrows)
        self.want = [oracle.spmv(m, self.x, None, mode=0)[0], oracle.spmv(m, self.x, self.y0, mode=1, alpha=ALPHA)[0]]
        for a in (self.x, self.y0, *self.want):
            a.setflags(write=False)

    def check(self, ctx, tag):
        for mode in (0, 1):
            got, _ = ctx.spmv(_abi.A, self.x, self.y0 if mode else np.full(self.m.nrows, np.nan), mode=mode, alpha=ALPHA)
            bad = np.flatnonzero(~(got == self.want[mode]))
            assert bad.size == 0, (tag, mode, int(bad.size), int(bad[0]))


def _edge_rows(a, runs=None):
    """The operator with the rows of the module docstring; runs (a dict) receives the truncated rows by length."""
    a = a.to_scipy().tolil()
    n = a.shape[0]
    cut = set()
    for k, length in enumerate(LENGTHS):        # the first 160 rows from row 500 + 700 k on that are longer (321: 40 of all)
        first, count = (500 + 700 * k, 160) if length < 300 else (0, 40)
        run = [r for r in range(first, n) if len(a.rows[r]) > length and r not in cut][:count]
        assert len(run) == count, (length, len(run))
        cut.update(run)
        if runs is not None:
            runs[length] = run
        for r in run:
            a.rows[r], a.data[r] = a.rows[r][:length], a.data[r][:length]
    filled = 0
    long_rows = [r for r in range(7, n - 7) if len(a.rows[r]) >= 300 and r % 97 and r not in cut and not 5300 <= r < 5700]
    for r in long_rows[::9]:                    # 384 entries: the row's own and columns of rows of its component nearby
        have = set(a.rows[r])
        extra = sorted({c for q in (r - 6, r + 6) for c in a.rows[q]} - have)[:384 - len(have)]
        if len(have) + len(extra) != 384:
            continue
        cols = sorted(have | set(extra))
        old = dict(zip(a.rows[r], a.data[r]))
        a.rows[r], a.data[r] = cols, [old.get(c, 0.03125 * (1 + c % 7)) for c in cols]
        filled += 1
    assert filled >= 4, filled
    for r in range(0, n, 97):
        a.rows[r], a.data[r] = [], []
    a = a.tocsr()
    for r in range(5300, 5700, 5):
        a.data[a.indptr[r]:a.indptr[r + 1]] *= 1.25
    m = problems.Csr.from_scipy(a)
    ln = np.diff(np.asarray(m.row_ptr))
    assert ln.max() == 384 and ln.min() == 0
    assert set(LENGTHS) <= set(ln.tolist())
    assert set(range(1, 7)) <= set((-(-ln[ln > 0] // 64)).tolist())     # every class
    return m


@pytest.fixture(scope="module")
def base():
    return problems.generate(n_cells=6, **GEN)


@pytest.fixture(scope="module")
def edge(base):
    return Ref(_edge_rows(base.mats["A"]), 51)


def test_the_named_edges_are_in_the_plan(built, base):
    """What the planner makes of the rows above, from the host-side plan (alfd_host_stream_plan, no GPU): the rows cut to
    one length, planned on their own, give shared batches for every length (the cut rows are still translates of one
    another), and the run with every 5th row perturbed gives shared AND plain batches.  The plan reports no batch sizes,
    so that shared batches of 16, 8 and 4 rows all occur is not asserted here."""
    import scipy.sparse as sp
    runs = {}
    m = _edge_rows(base.mats["A"], runs)
    a = m.to_scipy().tocsr()

    def only(rows):
        keep = np.zeros(a.shape[0], bool)
        keep[rows] = True
        sel = keep[np.repeat(np.arange(a.shape[0]), np.diff(a.indptr))]
        ptr = np.r_[0, np.cumsum(np.where(keep, np.diff(a.indptr), 0))]
        return problems.Csr.from_scipy(sp.csr_matrix((a.data[sel], a.indices[sel], ptr), shape=a.shape))

    for length, run in runs.items():
        sub = only([r for r in run if r % 97])
        plan = solver.host_stream_plan(sub, row_block=96)
        assert plan["ok"] == 1 and plan["decode_mismatches"] == 0 and plan["shared_nnz"] > 0, (length, plan)
    plan = solver.host_stream_plan(only(np.arange(5300, 5700)), row_block=96)
    assert plan["ok"] == 1 and 0 < plan["shared_nnz"] < a[5300:5700].nnz, plan


@pytest.fixture
def ctx(built, monkeypatch):
    monkeypatch.setenv("ALFD_SPMV_WINDOW_MIN_BLOCKS", "20")    # read at alfd_create: 1 920 rows and more take the window forms
    c = solver.Context(0)
    yield c
    c.close()


def _planned(ctx, m, waves, wide=0):
    ctx.set_tunable("batch_major_waves", waves)
    ctx.set_matrix(_abi.A, m)
    info = ctx.matrix_info(_abi.A)
    assert info["batch_major"] in (1, 2) and info["lanes"] == 64 and info["batch_major_wide"] == wide, info
    assert info["batch_major_waves"] == waves, info
    return info


@pytest.mark.parametrize("waves", [1, 2, 4, 8])
def test_edge_rows_in_runs_and_bricks(ctx, base, edge, waves):
    for rows in (16, 48, 96):
        ctx.set_tunable("batch_major_rows", rows)
        info = _planned(ctx, edge.m, waves)
        assert 0 < info["shared_nnz"] < edge.m.nnz, info       # shared AND plain batches
        assert info["batch_major_blocks"] == -(-edge.m.nrows // rows) and edge.m.nrows % rows != 0
        edge.check(ctx, ("runs", rows, waves))
    ctx.set_tunable("batch_major_rows", 96)
    ctx.set_row_blocks(_abi.A, *problems.brick_row_blocks(base.params, (4, 2, 2)))
    info = _planned(ctx, edge.m, waves)
    assert info["batch_major"] == 2 and 0 < info["shared_nnz"] < edge.m.nnz, info
    edge.check(ctx, ("bricks", waves))


def _blocks_of_one_class(m, waves):
    """Row blocks of 4 k rows of one class each, k = 1 .. 2 waves + 1, over and over until the rows run out; the rest in
    blocks of one row.  Returns (block_ptr, rows, the k of every block)."""
    ln = np.diff(np.asarray(m.row_ptr))
    cls = -(-ln // 64)
    order = np.argsort(cls, kind="stable").astype(np.int32)
    bounds = np.searchsorted(cls[order], np.arange(0, 8))
    ptr, ks, k = [0], [], 1
    for c in range(0, 7):
        pos, end = int(bounds[c]), int(bounds[c + 1])
        while pos + 4 * k <= end:
            pos += 4 * k
            ptr.append(pos)
            ks.append(k)
            k = k % (2 * waves + 1) + 1
        while pos < end:
            pos += 1
            ptr.append(pos)
            ks.append(1)
    assert ptr[-1] == m.nrows
    return np.array(ptr, np.int64), order, ks


@pytest.mark.parametrize("waves", [1, 2, 4, 8])
def test_batch_counts_around_the_prefetch_depths(ctx, edge, waves):
    ptr, rows, ks = _blocks_of_one_class(edge.m, waves)
    assert set(range(1, 2 * waves + 2)) <= set(ks)              # fewer than NW, NW, NW + 1, 2 NW, 2 NW + 1 batches
    for share in (0, 1):
        ctx.set_tunable("batch_major_share", share)
        ctx.set_row_blocks(_abi.A, ptr, rows)
        info = _planned(ctx, edge.m, waves)
        assert info["batch_major"] == 2 and info["batch_major_blocks"] == len(ks), info
        assert (info["shared_nnz"] == 0) == (share == 0), info
        edge.check(ctx, ("one class per block", waves, share))


def test_wide_codes(ctx, edge):
    a = edge.m
    v = np.array(a.val) * (1.0 + np.random.default_rng(7).integers(0, 16, a.nnz) / 16.0)
    wide = Ref(problems.Csr(a.nrows, a.ncols, np.array(a.row_ptr), np.array(a.col), v), 52)
    _planned(ctx, wide.m, 4, wide=1)
    wide.check(ctx, "wide codes")


@pytest.mark.parametrize("waves", [1, 4])
def test_pair_launch(ctx, base, edge, waves):
    from test_gpu_pair_launch import _check_pair, _random_c
    ctx.set_row_blocks(_abi.A, *problems.brick_row_blocks(base.params, (4, 2, 2)))
    info = _planned(ctx, edge.m, waves)
    nr_c = 5 * info["batch_major_blocks"] + 3                   # more workgroups in the second party than in the first
    ctx.set_matrix(_abi.C_, _random_c(nr_c, edge.m.ncols, 32, 9))
    assert ctx.matrix_info(_abi.C_)["batch_major"] == 0
    _check_pair(ctx, edge.m.nrows, nr_c, edge.x, ("pair", waves))
    edge.check(ctx, ("after the pair launch", waves))
