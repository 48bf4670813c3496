"""Restatements of the truncation rule of the smoothed-aggregation prolongator, independent of
the library: an exact one in plain Python floats, and a tolerance-aware check of a truncated level against untruncated
values computed elsewhere (SciPy), which rounding may order differently at exact ties."""
import numpy as np

from fictitious_domain_al_preconditioners_amd import problems


def truncate_rows(P, agg, block_size, tau, k):
    """The rule, row by row, with Python floats in the stated order; returns a problems.Csr."""
    rp, cols, vals = [0], [], []
    for i in range(P.nrows):
        g = int(agg[i])
        J = [int(c) for c in P.col[P.row_ptr[i]:P.row_ptr[i + 1]]]
        p = [float(v) for v in P.val[P.row_ptr[i]:P.row_ptr[i + 1]]]
        if g >= 0 and J:
            m = max(abs(v) for v in p)
            thr = tau * m
            K0 = [t for t in range(len(J)) if abs(p[t]) >= thr or J[t] == g]
            if k > 0 and len(K0) > k:
                rest = sorted((t for t in K0 if J[t] != g), key=lambda t: (-abs(p[t]), J[t]))
                K = set(rest[:k - 1]) | {J.index(g)}
            else:
                K = set(K0)
            out = list(p)
            for c in range(block_size):
                dropped = [t for t in range(len(J)) if t not in K and J[t] % block_size == c]
                kept = [t for t in sorted(K) if J[t] % block_size == c]
                if dropped and kept:
                    t_sum = 0.0
                    for t in dropped:                      # ascending J
                        t_sum = t_sum + p[t]
                    target = min(kept, key=lambda t: (-abs(p[t]), J[t]))
                    out[target] = p[target] + t_sum
            for t in sorted(K):
                cols.append(J[t])
                vals.append(out[t])
        rp.append(len(cols))
    return problems.Csr(P.nrows, P.ncols, np.array(rp, np.int64), np.array(cols, np.int32),
                        np.array(vals, np.float64))


def check_against_untruncated(P, ref, agg, block_size, tau, k, tol, sel=1e-9):
    """P (problems.Csr): a truncated level; ref (scipy CSR): the untruncated prolongator computed independently, so its
    values carry other rounding and exact ties of the rule may fall either way.  Checked per row:
      * the aggregate's own column is kept, at most k entries (k > 0), columns ascending;
      * no dropped entry beats a kept one: it is below tau * max, or not larger than any kept entry and then the cap
        is full (both to sel * max|ref|);
      * per component that keeps an entry: at most one kept value departs from ref by more than tol * max|ref| (the
        lump target), and the kept sum equals the untruncated component sum to tol * sum|ref|;
      * rows without an aggregate are empty."""
    ref = ref.tocsr()
    ref.sort_indices()
    for i in range(P.nrows):
        g = int(agg[i])
        dc = P.col[P.row_ptr[i]:P.row_ptr[i + 1]].astype(np.int64)
        dv = P.val[P.row_ptr[i]:P.row_ptr[i + 1]]
        if g < 0:
            assert dc.size == 0, i
            continue
        rc = ref.indices[ref.indptr[i]:ref.indptr[i + 1]].astype(np.int64)
        rv = ref.data[ref.indptr[i]:ref.indptr[i + 1]]
        assert np.all(np.diff(dc) > 0) and g in dc, i
        assert k == 0 or dc.size <= k, (i, dc.size)
        big, total = np.abs(rv).max(), np.abs(rv).sum()
        at = np.searchsorted(rc, dc)
        hit = (at < rc.size) & (rc[np.minimum(at, rc.size - 1)] == dc)
        rd = np.where(hit, rv[np.minimum(at, rc.size - 1)], 0.0)        # ref at the kept columns (0: structural zero)
        dropped = ~np.isin(rc, dc)
        if dropped.any():
            b_max = np.abs(rv[dropped]).max()
            others = np.abs(rd[dc != g])
            a_min = others.min() if others.size else np.inf
            assert a_min >= tau * big * (1 - sel), (i, a_min, tau * big)
            if b_max >= tau * big * (1 + sel):                           # dropped by the cap
                assert k > 0 and dc.size == k and b_max <= a_min + sel * big, (i, b_max, a_min, dc.size)
        for c in range(block_size):
            mine = dc % block_size == c
            if not mine.any():
                continue
            diff = dv[mine] - rd[mine]
            assert int((np.abs(diff) > tol * big).sum()) <= 1, (i, c, diff)
            whole = rv[rc % block_size == c].sum()
            assert abs(dv[mine].sum() - whole) <= tol * total, (i, c, dv[mine].sum(), whole)
