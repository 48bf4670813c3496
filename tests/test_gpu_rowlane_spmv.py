"""spmv_rowlane_kernel<L, EPI> (one thread per row, tunable "short_rows_per_thread") against the
kernel it replaces and against the oracle.  Every comparison is bitwise, against two references:

  * the same context with the tunable at 0: spmv_kernel<L>, the parent's kernel;
  * the oracle's canonical sum (tests/spmv_reference.py).

The kernel emulates the L lanes of spmv_kernel<L> in registers: entry j of a row goes to accumulator j mod L, lanes
without entries stay +0.0 and are added all the same, and the tree adds the partners l^(L/2), ..., l^1.  It is taken
exactly where spmv_kernel<L, EPI, false> would run with L 4 or 8 and EPI 0 or 1, when no row has more than 2 L entries;
alfd_get_last_spmv_launch says which of the two ran.

  1. the prolongators of the vector-Q2 generator at N = 4 and N = 5 (even and odd coarsening), every level, modes 0 and 1;
     whole solves with the tunable 1 / 0 / 1 on one context;
  2. random CSR of 3 000 rows (no multiple of 64 or 256) at L = 4 and L = 8: row lengths 0 .. 2 L with empty,
     single-entry and full rows, values and x with -0.0, +0.0, subnormals, products that underflow to -0.0 (row 50: in
     every lane, so the row sum is -0.0), pairs that cancel exactly and magnitudes 2^-30 .. 2^30 (so that another order
     of the tree shows); y goes in as NaN for mode 0;
  3. refusal: one row of 2 L + 1 entries, and a sparse-row matrix, run the parent's kernels -- with the right result."""
import numpy as np
import pytest

import cases
import spmv_reference as sr
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver
from oracle import oracle

pytestmark = pytest.mark.gpu

ROWS = 3000
ALPHA = -0.75


def _csr(n, ncols, cols, vals):
    rp = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int64)
    col = (np.concatenate(cols) if rp[-1] else np.zeros(0)).astype(np.int32)
    val = (np.concatenate(vals) if rp[-1] else np.zeros(0)).astype(np.float64)
    return problems.Csr(n, ncols, rp, col, val)


TEMPLATES = 700


def random_short_rows(L, extra_long_row=False, seed=0):
    """3 000 rows of 0 .. 2 L entries, each a translate of one of 700 template rows: row i < 700 is template i, the
    others draw one; the first column is random.  Template lengths: L = 4 uniform over 0 .. 8 (mean of the non-empty rows 4.5 <= 6), L = 8 over
    1 .. 16 (mean 8.5 in (6, 12]), 5 % emptied, templates 10 .. 10 + 2 L planted with 0, 1, ..., 2 L entries; first and
    last row empty.  Column offsets: sorted, distinct, below 200.  Values: uniform(-1, 1) 2^k, k in -30 .. 30, with 3 %
    each of -0.0, +0.0, subnormals and -2^-600 (whose products with the 2^-600 entries of x round to -0.0); every third
    template of 2 entries and more starts with v, -v in ONE column (lanes 0 and 1: a row of 2 entries cancels exactly).
    Row 50: L entries -2^-600 on x = 2^-600, every lane underflows to -0.0 and so does the row sum.  Returns (Csr, x)."""
    rng = np.random.default_rng(7100 + 10 * L + seed)
    n = ncols = ROWS
    x = rng.uniform(-1.0, 1.0, ncols) * np.exp2(rng.integers(-30, 31, ncols))
    special = rng.random(ncols)
    x[special < 0.03] = -0.0
    x[(special >= 0.03) & (special < 0.06)] = 0.0
    x[(special >= 0.06) & (special < 0.09)] = 5e-324 * rng.integers(1, 1000, int(((special >= 0.06) & (special < 0.09)).sum()))
    x[(special >= 0.09) & (special < 0.12)] = 2.0 ** -600
    x[3:3 + L] = 2.0 ** -600                                      # row 50
    lengths = rng.integers(0 if L == 4 else 1, 2 * L + 1, TEMPLATES)
    lengths[rng.random(TEMPLATES) < 0.05] = 0
    lengths[10:10 + 2 * L + 1] = np.arange(2 * L + 1)
    lengths[50] = L
    templates = []
    for t in range(TEMPLATES):
        k = int(lengths[t])
        d = np.sort(rng.choice(200, k, replace=False)) if k else np.zeros(0, np.int64)
        if k:
            d -= d[0]
        v = rng.uniform(-1.0, 1.0, k) * np.exp2(rng.integers(-30, 31, k))
        s = rng.random(k)
        v[s < 0.03] = -0.0
        v[(s >= 0.03) & (s < 0.06)] = 0.0
        v[(s >= 0.06) & (s < 0.09)] = -4.9e-324
        v[(s >= 0.09) & (s < 0.12)] = -(2.0 ** -600)
        if t == 50:
            d, v = np.arange(L), np.full(L, -(2.0 ** -600))
        elif k >= 2 and t % 3 == 0:
            d[1], v[1] = 0, -v[0]
        templates.append((d, v))
    which = np.concatenate([np.arange(TEMPLATES), rng.integers(0, TEMPLATES, n - TEMPLATES)])
    first = rng.integers(0, ncols - 200, n)
    first[50] = 3
    cols, vals = [], []
    for i in range(n):
        d, v = templates[which[i]]
        if i in (0, n - 1):
            d, v = d[:0], v[:0]
        if extra_long_row and i == 1777:
            d, v = np.arange(2 * L + 1) * 3, rng.uniform(-1.0, 1.0, 2 * L + 1)
        cols.append(first[i] + d)
        vals.append(v)
    m = _csr(n, ncols, cols, vals)
    ln = np.diff(m.row_ptr)
    mean = ln[ln > 0].mean()
    assert (mean <= 6) if L == 4 else (6 < mean <= 12), mean        # the lane rule gives L
    assert (ln > 0).sum() * 2 >= n                                  # not the sparse-row form
    assert {0, 1, 2 * L} <= set(ln.tolist()) and ln.max() == 2 * L + (1 if extra_long_row else 0)
    assert n % 64 and n % 256
    return m, x


class Inputs:
    """A matrix with x, y0 and the oracle's answers for modes 0 and 1; computed once, read-only."""

    def __init__(self, m, x=None, seed=1):
        rng = np.random.default_rng(seed)
        self.m = m
        self.x = rng.uniform(-1.0, 1.0, m.ncols) if x is None else x
        self.y0 = rng.uniform(-1.0, 1.0, m.nrows)
        self.s, self.lanes = oracle.spmv(m, self.x, None, mode=0)
        self.s1 = {a: oracle.spmv(m, self.x, self.y0, mode=1, alpha=a)[0] for a in (1.0, ALPHA)}
        for a in (self.x, self.y0, self.s, *self.s1.values()):
            a.setflags(write=False)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want, tag):
    assert np.array_equal(_bits(got), _bits(want)), (tag, sr.first_bad(got, want))


def _products(ctx, inp, on, tag, want_family):
    """Modes 0 (out of NaN) and 1 (alpha = 1 and -0.75) with the tunable at `on`; the launch record of each."""
    ctx.set_tunable("short_rows_per_thread", on)
    out = []
    y, lanes = ctx.spmv(_abi.A, inp.x, np.full(inp.m.nrows, np.nan), mode=0)
    assert lanes == inp.lanes, tag
    rec = ctx.last_spmv_launch()
    assert (rec["family"], rec["lanes"], rec["epilogue"]) == (want_family, inp.lanes, 0), (tag, on, rec)
    if want_family == _abi.SPMV_ROW_LANE:
        assert rec["grid"] == -(-inp.m.nrows // 256) and rec["lds_bytes"] == 0, (tag, rec)
    _same(y, inp.s, (tag, on, "mode 0"))
    out.append(y)
    for alpha in (1.0, ALPHA):
        y, _ = ctx.spmv(_abi.A, inp.x, inp.y0, mode=1, alpha=alpha)
        rec = ctx.last_spmv_launch()
        assert (rec["family"], rec["lanes"], rec["epilogue"]) == (want_family, inp.lanes, 1), (tag, on, rec)
        _same(y, inp.s1[alpha], (tag, on, "mode 1", alpha))
        out.append(y)
    return out


def _check(ctx, inp, tag, taken):
    """Upload into slot A; tunable 1, 0, 1; the row-per-thread family exactly when `taken`."""
    ctx.set_matrix(_abi.A, inp.m)
    info = ctx.matrix_info(_abi.A)
    parent = _abi.SPMV_SPARSE_ROWS if _sparse(inp.m) else _abi.SPMV_PLAIN
    assert not info["windowed"] and not info["batch_major"], (tag, info)
    a = _products(ctx, inp, 1, tag, _abi.SPMV_ROW_LANE if taken else parent)
    b = _products(ctx, inp, 0, tag, parent)
    c = _products(ctx, inp, 1, tag, _abi.SPMV_ROW_LANE if taken else parent)
    for ya, yb, yc in zip(a, b, c):
        _same(ya, yb, (tag, "against the parent's kernel"))
        _same(yc, yb, (tag, "switched back"))


def _sparse(m):
    return int((np.diff(m.row_ptr) > 0).sum()) * 2 < m.nrows


@pytest.fixture
def ctx(built):
    c = solver.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- 1. generator transfers
@pytest.mark.parametrize("n_cells", [4, 5])
def test_generator_prolongators_every_level(ctx, n_cells):
    """Q2 -> Q1 embedding, then trilinear interpolation: 2 n -> n cells, n -> ceil(n / 2), ...: nested (weights 1, 1/2)
    when the cell count is even, not nested when it is odd (N = 5: 5 -> 3 -> 2)."""
    pb = problems.stokes3d_sphere(n_cells, 0)
    levels = problems.tensor_prolongators(pb.params, min_coarse=1)
    assert len(levels) >= 2
    taken = []
    for k, (P, n_coarse) in enumerate(levels):
        inp = Inputs(P, seed=40 + 10 * n_cells + k)
        ln = np.diff(P.row_ptr)
        assert inp.lanes in (4, 8) and ln.max() <= 8 and P.ncols == n_coarse
        take = not _sparse(P) and ln.max() <= 2 * inp.lanes
        print("N", n_cells, "level", k, "rows", P.nrows, "cols", P.ncols, "lanes", inp.lanes, "longest", int(ln.max()),
              "sparse rows", _sparse(P), "row per thread", take)
        _check(ctx, inp, (n_cells, k), take)
        taken.append(take)
    assert any(taken)


def _solve(ctx, rhs, on):
    ctx.set_tunable("short_rows_per_thread", on)
    x, res = ctx.solve(rhs, raise_on_failure=False)
    return x, res, ctx.history().copy()


@pytest.mark.parametrize("n_cells", [4, 5])
def test_solves_with_and_without_the_kernel_bit_for_bit(built, n_cells):
    """The multigrid settings of cases.case("stokes3d_gmg") on the generator at N = 4 and 5, prolongators down to the
    smallest grid: the V-cycle applies every one of them (z += P e_c) once per cycle."""
    _, cfg = cases.case("stokes3d_gmg")
    pb = problems.stokes3d_sphere(n_cells, 0)
    levels = problems.tensor_prolongators(pb.params, min_coarse=1)
    osys = oracle.system_from_problem(pb, aggregates=levels)
    rhs = cases.prepared_rhs(osys, pb, cfg)
    ctx = solver.context_from_problem(pb, cfg, aggregates=levels)
    try:
        x1, r1, h1 = _solve(ctx, rhs, 1)
        x0, r0, h0 = _solve(ctx, rhs, 0)
        x2, r2, h2 = _solve(ctx, rhs, 1)
    finally:
        ctx.close()
    print("N", n_cells, "levels", len(levels), "outer", r1.outer_iterations, "inner", r1.inner_iterations, "status", r1.status)
    assert r1.outer_iterations > 0 and r1.inner_iterations > 0
    for xa, ra, ha in ((x1, r1, h1), (x2, r2, h2)):
        assert (ra.status, ra.outer_iterations, ra.inner_iterations, ra.mp_iterations, ra.inner_failures) == \
               (r0.status, r0.outer_iterations, r0.inner_iterations, r0.mp_iterations, r0.inner_failures)
        assert np.array_equal(_bits(ha), _bits(h0))
        assert len(xa) == len(x0)
        for a, b in zip(xa, x0):
            assert np.array_equal(_bits(a), _bits(b))


# --------------------------------------------------------------------------------------------------- 2. random CSR
@pytest.mark.parametrize("L", [4, 8])
def test_random_short_rows(ctx, L):
    m, x = random_short_rows(L)
    inp = Inputs(m, x)
    assert inp.lanes == L
    assert _bits(inp.s)[50] == _bits(np.float64(-0.0))               # every lane underflowed to -0.0 ...
    assert np.any(inp.s[np.diff(m.row_ptr) == 2] == 0.0)            # ... and rows of v, -v in one column cancelled
    _check(ctx, inp, ("random", L), True)


# ------------------------------------------------------------------------------------------------------ 3. refusal
@pytest.mark.parametrize("L", [4, 8])
def test_one_row_too_long_runs_the_parents_kernel(ctx, L):
    m, x = random_short_rows(L, extra_long_row=True)
    inp = Inputs(m, x)
    assert inp.lanes == L
    _check(ctx, inp, ("2 L + 1", L), False)


def test_sparse_row_matrix_runs_the_parents_path(ctx):
    """Every third row of random_short_rows(4), the others empty: the sparse-row list (spmv_kernel<L, EPI, true>)."""
    full, x = random_short_rows(4)
    rp = np.asarray(full.row_ptr, np.int64)
    keep = np.arange(ROWS) % 3 == 0
    ln = np.where(keep, np.diff(rp), 0)
    sel = np.concatenate([np.arange(rp[i], rp[i + 1]) for i in np.flatnonzero(keep)]).astype(np.int64)
    m = problems.Csr(ROWS, ROWS, np.concatenate([[0], np.cumsum(ln)]).astype(np.int64),
                     np.asarray(full.col)[sel].astype(np.int32), np.asarray(full.val)[sel].astype(np.float64))
    assert _sparse(m)
    inp = Inputs(m, x)
    assert inp.lanes == 4
    ctx.set_matrix(_abi.A, m)
    for on in (1, 0):
        ctx.set_tunable("short_rows_per_thread", on)
        y, _ = ctx.spmv(_abi.A, inp.x, np.full(ROWS, np.nan), mode=0)
        assert ctx.last_spmv_launch()["family"] == _abi.SPMV_SPARSE_ROWS
        _same(y, inp.s, ("sparse rows", on, "mode 0"))
        y, _ = ctx.spmv(_abi.A, inp.x, inp.y0, mode=1, alpha=ALPHA)
        assert ctx.last_spmv_launch()["family"] == _abi.SPMV_SPARSE_ROWS
        _same(y, inp.s1[ALPHA], ("sparse rows", on, "mode 1"))


def test_tunable_refuses_other_values(ctx):
    for v in (0, 1):
        ctx.set_tunable("short_rows_per_thread", v)
    for v in (-1, 2):
        with pytest.raises(solver.AlfdError) as e:
            ctx.set_tunable("short_rows_per_thread", v)
        assert e.value.status == _abi.E_INVALID
