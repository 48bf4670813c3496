"""References of the diagonal-scaled SpMV epilogues (y = d .* (A x); y = A x and y2 = d .* (A x)), shared by
tests/test_gpu_spmv_epilogues.py and the partitioned split launch in tests/test_gpu_multirank.py; nothing here calls
the library.

Two references, both from the host CSR arrays:
  * bitwise: s = the oracle's canonical sum (mode 0); epilogue 2 must give y == d * s, epilogue 3 y == s and
    y2 == d * s -- one IEEE multiply in NumPy is the exact reference;
  * independent: ref = d .* (A x) in np.longdouble, with the derived row-wise bound
    |y2_r - ref_r| <= (len_r + 2) 2^-53 |d_r| (|A||x|)_r: len_r products and len_r - 1 additions (or len_r fma) of
    the row sum in any order, one multiply by d_r, second-order terms in the slack -- should oracle and library ever
    share an error.

d_r = +-uniform(0.5, 2) 2^k with k in -20..20 per row, every factor distinct (a d indexed by the block-local row, the
list position or the batch row shows), about 1 % exact zeros.  Outputs go in as NaN: a row that neither a kernel nor
the sparse-row memset writes comes back NaN."""
import numpy as np

from fictitious_domain_al_preconditioners_amd import _abi
from oracle import oracle

U = 2.0 ** -53


def scale(n, rng):
    """d_r = +-uniform(0.5, 2) 2^k, k in -20..20, all distinct, about 1 % exact zeros."""
    d = rng.uniform(0.5, 2.0, n) * np.exp2(rng.integers(-20, 21, n)) * rng.choice([-1.0, 1.0], n)
    assert np.unique(d).size == n
    d[rng.random(n) < 0.01] = 0.0
    return d


class Case:
    """One matrix with its inputs and both references, computed once and left unchanged."""

    def __init__(self, m, seed, d=None):
        rng = np.random.default_rng(seed)
        self.m = m
        self.x = rng.uniform(-1.0, 1.0, m.ncols)
        self.d = scale(m.nrows, rng) if d is None else np.ascontiguousarray(d, np.float64)
        self.y0 = rng.uniform(-1.0, 1.0, m.nrows)
        self.s, self.lanes = oracle.spmv(m, self.x, None, mode=0)
        self.ds = self.d * self.s
        rp, col = np.asarray(m.row_ptr, np.int64), np.asarray(m.col)
        val = np.asarray(m.val, np.float64)
        ln = np.diff(rp)
        prod = val.astype(np.longdouble) * self.x[col].astype(np.longdouble)
        ax, absax = np.zeros(m.nrows, np.longdouble), np.zeros(m.nrows, np.longdouble)
        ne = ln > 0
        if prod.size:           # non-empty rows are contiguous segments of the entry array
            ax[ne] = np.add.reduceat(prod, rp[:-1][ne])
            absax[ne] = np.add.reduceat(np.abs(prod), rp[:-1][ne])
        self.ref = self.d.astype(np.longdouble) * ax
        self.bound = (ln + 2) * np.longdouble(U) * np.abs(self.d).astype(np.longdouble) * absax
        for a in (self.x, self.d, self.y0, self.s, self.ds, self.ref, self.bound):
            a.setflags(write=False)

    def check(self, ctx, tag, slot=_abi.A, mode1=False):
        """Epilogues 2 and 3 through alfd_spmv_scaled and mode 0 of alfd_spmv, all out of NaN-prefilled outputs;
        mode 1 beside them where asked for."""
        nan = np.full(self.m.nrows, np.nan)
        y = ctx.spmv_scaled(slot, self.x, self.d, nan)
        self.check_scaled(y, (tag, "epilogue 2"))
        y, y2 = ctx.spmv_scaled(slot, self.x, self.d, nan, nan)
        assert np.array_equal(y, self.s), (tag, "epilogue 3: y", first_bad(y, self.s))
        self.check_scaled(y2, (tag, "epilogue 3: y2"))
        y, lanes = ctx.spmv(slot, self.x, nan, mode=0)
        assert lanes == self.lanes, tag
        assert np.array_equal(y, self.s), (tag, "epilogue 0", first_bad(y, self.s))
        if mode1:
            y, _ = ctx.spmv(slot, self.x, self.y0, mode=1, alpha=-0.75)
            assert np.array_equal(y, oracle.spmv(self.m, self.x, self.y0, mode=1, alpha=-0.75)[0]), (tag, "epilogue 1")

    def check_scaled(self, got, tag, rows=slice(None)):
        """got (the rows `rows` of the matrix) against d * s bit for bit and against the longdouble reference."""
        assert np.array_equal(got, self.ds[rows]), (tag, first_bad(got, self.ds[rows]))
        err = np.abs(got.astype(np.longdouble) - self.ref[rows])
        assert np.all(err <= self.bound[rows]), (tag, "longdouble bound", int(np.argmax(err - self.bound[rows])))


def first_bad(got, want):
    bad = np.flatnonzero(~(got == want))
    return (int(bad.size), int(bad[0]), float(got[bad[0]]), float(want[bad[0]])) if bad.size else None
