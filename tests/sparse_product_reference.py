"""Independent references of the setup's sparse product out = A P and of the rows of the smoothed prolongator, written
from DESIGN.md section 4 with NumPy, SciPy and the standard library; nothing here calls the library or the oracle.

Product.  Pattern: row i holds every column J reachable through a stored entry of A and a stored entry of P (stored
zeros count, a chain that cancels stays, as +0.0), columns ascending.  Values:
  * exact inputs (integers |k| <= 16 times 2^-3): every product is a multiple of 2^-6 and every partial sum of a chain
    stays far below 2^53 * 2^-6, so the fma chain in ANY order is the exact product and SciPy's A @ P is a bit-exact
    reference -- `exact_product` asserts that from |A| @ |P| alone;
  * general inputs: `chain_product` evaluates the canonical chain acc = fma(a_ik, p_kJ, acc) (entries of row i of A in
    CSR order, entries of row col_k of P in CSR order) with fractions.Fraction -- float(Fraction(a) * Fraction(p) +
    Fraction(acc)) is the correctly rounded fma -- and `rowwise_bound` gives sum a_ik p_kJ in np.longdouble with the
    derived bound (len + 1) 2^-53 (|A||P|)_iJ for a chain of len fma in any order (second-order terms and the
    longdouble sum's own 2^-64 len in the slack), should the chain restatement and the library ever share a mistake.

Prolongator rows (`prolongator_rows`): s = 0.0; s = s + a_ik over the entries of row i with agg[col_k] == J in CSR
order; s = s + pen_iJ; P_iJ = fma(f_i, s, [J == agg_i]) with f_i = -omega / d_i, d_i = fma(gamma, s_i, a_ii), s_i the
sequential fma over row i of Ct of (w_k c_ik) c_ik; pen = Ct Tw, Tw_kJ = (gamma w_k) T_kJ, T = C P_tent, both products
in the canonical chain order.

Matrices are `Csr` records of plain NumPy arrays (int64 row_ptr, int32 col, float64 val)."""
from collections import namedtuple
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

Csr = namedtuple("Csr", "nrows ncols row_ptr col val")
U = 2.0 ** -53


def csr(nrows, ncols, rows):
    """Csr from a list of rows, each a list of (col, val) in the order they are to be stored."""
    rp = np.zeros(nrows + 1, np.int64)
    for i, r in enumerate(rows):
        rp[i + 1] = rp[i] + len(r)
    col = np.array([c for r in rows for c, _ in r], np.int32)
    val = np.array([v for r in rows for _, v in r], np.float64)
    assert len(rows) == nrows and (col.size == 0 or (col.min() >= 0 and col.max() < ncols))
    return Csr(nrows, ncols, rp, col, val)


def bucket(J, bits=12):
    """The home slot of column J in the kernels' hash sets: 12 bits in the product, 11 in the prolongator rows."""
    return ((int(J) * 2654435761) % 2 ** 32) >> (32 - bits)


def bucket_members(b, bits, limit, count):
    """The first `count` ids below `limit` whose home slot is b."""
    J = np.arange(limit, dtype=np.uint64)
    h = ((J * np.uint64(2654435761)) % np.uint64(2 ** 32)) >> np.uint64(32 - bits)
    ids = np.flatnonzero(h == np.uint64(b))[:count]
    assert all(bucket(j, bits) == b for j in ids[:4])
    return ids.astype(np.int64)


def _pairs(A, P):
    """Every chain term: (row i, column J, a_ik, p_kJ) in the canonical order of row i."""
    ln = np.diff(P.row_ptr)[A.col]                           # terms each entry of A contributes
    arow = np.repeat(np.arange(A.nrows, dtype=np.int64), np.diff(A.row_ptr))
    rows = np.repeat(arow, ln)
    a = np.repeat(A.val, ln)
    start = np.repeat(P.row_ptr[A.col], ln)
    first = np.repeat(np.cumsum(ln) - ln, ln)
    e = start + (np.arange(ln.sum(), dtype=np.int64) - first)
    return rows, P.col[e].astype(np.int64), a, P.val[e]


def pattern(A, P):
    """(row_ptr, col) of the structural product, columns ascending."""
    rows, cols, _, _ = _pairs(A, P)
    key = np.unique(rows * max(P.ncols, 1) + cols)
    r = key // max(P.ncols, 1)
    rp = np.zeros(A.nrows + 1, np.int64)
    np.add.at(rp, r + 1, 1)
    return np.cumsum(rp), (key % max(P.ncols, 1)).astype(np.int32)


def _scipy(M, val=None):
    return sp.csr_matrix((M.val if val is None else val, M.col, M.row_ptr), shape=(M.nrows, M.ncols))


def exact_product(A, P):
    """The product of exactly representable operands: structural pattern, values from SciPy.  Asserts that every
    ordering of every chain is exact: 64 (|A| @ |P|) is integral and below 2^53."""
    for M in (A, P):
        k = M.val * 8.0
        assert np.all(k == np.rint(k)) and np.all(np.abs(k) <= 16), "operands are integers |k| <= 16 times 2^-3"
    big = (_scipy(A, np.abs(A.val)) @ _scipy(P, np.abs(P.val))).data * 64.0
    assert np.all(big == np.rint(big)) and (big.size == 0 or big.max() < 2.0 ** 53)
    rp, col = pattern(A, P)
    C = (_scipy(A) @ _scipy(P)).tocsr()
    C.sum_duplicates()
    C.sort_indices()
    nc = max(P.ncols, 1)
    have = np.repeat(np.arange(A.nrows, dtype=np.int64), np.diff(C.indptr)) * nc + C.indices
    want = np.repeat(np.arange(A.nrows, dtype=np.int64), np.diff(rp)) * nc + col
    at = np.searchsorted(have, want)
    hit = at < have.size
    hit[hit] = have[at[hit]] == want[hit]
    val = np.zeros(want.size)
    val[hit] = C.data[at[hit]]
    val = val + 0.0                                          # a cancelled chain is +0.0
    assert np.all(np.isin(have[C.data != 0.0], want))
    return Csr(A.nrows, P.ncols, rp, col, val)


def fma(a, b, c):
    """The correctly rounded a * b + c of finite doubles (Python 3.10 has no math.fma).  An exact zero comes out +0.0,
    which is what IEEE gives whenever c is +0.0, 1.0 or an accumulator that started from +0.0."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def chain_product(A, P):
    """The canonical chain of every entry, one Fraction fma per term."""
    rp, cols, vals = [0], [], []
    for i in range(A.nrows):
        acc = {}
        for k in range(A.row_ptr[i], A.row_ptr[i + 1]):
            a, j = float(A.val[k]), int(A.col[k])
            for e in range(P.row_ptr[j], P.row_ptr[j + 1]):
                J = int(P.col[e])
                acc[J] = fma(a, float(P.val[e]), acc.get(J, 0.0))
        for J in sorted(acc):
            cols.append(J)
            vals.append(acc[J])
        rp.append(len(cols))
    return Csr(A.nrows, P.ncols, np.array(rp, np.int64), np.array(cols, np.int32), np.array(vals, np.float64))


def chain_terms(A, P):
    return int(np.diff(P.row_ptr)[A.col].sum())


def rowwise_bound(A, P):
    """(row_ptr, col, ref, bound): sum a_ik p_kJ in np.longdouble on the structural pattern and the derived bound
    (len + 1) 2^-53 sum |a_ik p_kJ| of a chain of len fma."""
    rows, cols, a, p = _pairs(A, P)
    nc = max(P.ncols, 1)
    key = rows * nc + cols
    uniq, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    prod = a.astype(np.longdouble) * p.astype(np.longdouble)
    ref, mag = np.zeros(uniq.size, np.longdouble), np.zeros(uniq.size, np.longdouble)
    np.add.at(ref, inv, prod)
    np.add.at(mag, inv, np.abs(prod))
    rp, col = pattern(A, P)
    return rp, col, ref, (cnt + 1) * np.longdouble(U) * mag


def transpose(M):
    """The transpose with every row in ascending column order (what the library's transpose gives)."""
    rows = [[] for _ in range(M.ncols)]
    for i in range(M.nrows):
        for k in range(M.row_ptr[i], M.row_ptr[i + 1]):
            rows[int(M.col[k])].append((i, float(M.val[k])))
    return csr(M.ncols, M.nrows, rows)


def diagonal(A, Ct=None, w=None, gamma=0.0):
    """d_i = fma(gamma, s_i, a_ii) (a_ii alone without a penalty term)."""
    d = []
    for i in range(A.nrows):
        aii = 0.0
        for k in range(A.row_ptr[i], A.row_ptr[i + 1]):
            if A.col[k] == i:
                aii = float(A.val[k])
        if Ct is not None:
            s = 0.0
            for k in range(Ct.row_ptr[i], Ct.row_ptr[i + 1]):
                c = float(Ct.val[k])
                s = fma(float(w[Ct.col[k]]) * c, c, s)
            aii = fma(gamma, s, aii)
        d.append(aii)
    return d


def penalty_rows(Ct, w, gamma, agg, n_coarse):
    """pen = Ct Tw, Tw_kJ = (gamma w_k) T_kJ, T = C P_tent; a dict J -> pen_iJ per row."""
    n = Ct.nrows
    Pt = csr(n, n_coarse, [[(int(agg[i]), 1.0)] if agg[i] >= 0 else [] for i in range(n)])
    T = chain_product(transpose(Ct), Pt)
    scale = np.repeat(np.array([gamma * float(wk) for wk in w]), np.diff(T.row_ptr))
    Q = chain_product(Ct, T._replace(val=scale * T.val))
    return [{int(Q.col[q]): float(Q.val[q]) for q in range(Q.row_ptr[i], Q.row_ptr[i + 1])} for i in range(n)]


def prolongator_rows(A, agg, n_coarse, omega, Ct=None, w=None, gamma=0.0):
    """The untruncated rows of P = P_tent - omega D^-1 (A P_tent + pen) in the canonical order."""
    d = diagonal(A, Ct, w, gamma)
    pen = penalty_rows(Ct, w, gamma, agg, n_coarse) if Ct is not None else None
    rp, cols, vals = [0], [], []
    for i in range(A.nrows):
        g = int(agg[i])
        if g >= 0:
            s = {}
            for k in range(A.row_ptr[i], A.row_ptr[i + 1]):
                J = int(agg[A.col[k]])
                if J >= 0:
                    s[J] = s.get(J, 0.0) + float(A.val[k])
            if pen is not None:
                for J, q in pen[i].items():
                    s[J] = s.get(J, 0.0) + q
            s.setdefault(g, 0.0)
            f = -omega / d[i]
            for J in sorted(s):
                cols.append(J)
                vals.append(fma(f, s[J], 1.0 if J == g else 0.0))
        rp.append(len(cols))
    return Csr(A.nrows, n_coarse, np.array(rp, np.int64), np.array(cols, np.int32), np.array(vals, np.float64))


def same_bits(got, want):
    """None when the two CSR results agree byte for byte (+0.0 and -0.0 differ), else where they first differ."""
    if got.nrows != want.nrows or got.ncols != want.ncols:
        return ("shape", got.nrows, got.ncols, want.nrows, want.ncols)
    grp, wrp = np.asarray(got.row_ptr, np.int64), np.asarray(want.row_ptr, np.int64)
    if not np.array_equal(grp, wrp):
        i = int(np.flatnonzero(np.diff(grp) != np.diff(wrp))[0])
        return ("row length", i, int(grp[i + 1] - grp[i]), int(wrp[i + 1] - wrp[i]))
    gc, wc = np.asarray(got.col, np.int32), np.asarray(want.col, np.int32)
    if not np.array_equal(gc, wc):
        k = int(np.flatnonzero(gc != wc)[0])
        return ("column", int(np.searchsorted(wrp, k, side="right") - 1), int(gc[k]), int(wc[k]))
    gv = np.ascontiguousarray(got.val, np.float64).view(np.int64)
    wv = np.ascontiguousarray(want.val, np.float64).view(np.int64)
    if not np.array_equal(gv, wv):
        k = int(np.flatnonzero(gv != wv)[0])
        return ("value", int(np.searchsorted(wrp, k, side="right") - 1), int(wc[k]), float(got.val[k]), float(want.val[k]),
                int((gv != wv).sum()))
    return None
