"""Truncated smoothed-aggregation prolongators on the host (alfd_host_truncate_prolongator, no GPU): the library's
truncation rule against a plain-Python restatement bit for bit, its properties, the tie rule, argument checks, and its
effect on the iteration counts in the CPU oracle."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import cases
import truncation_reference as tr
from fictitious_domain_al_preconditioners_amd import _abi, problems, solver
from oracle import oracle

RULES = [(0.1, 0), (0.0, 4), (0.1, 8), (0.3, 2), (0.0, 1)]


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def _smoothed(which):
    """(P, agg, block_size) of one smoothed level; computed once per module."""
    if which == "stokes":
        pb, bs = problems.stokes3d_sphere(4, 0), 3
    else:
        pb, bs = problems.laplace2d_circle(12, 2), 1
    A = pb.mats["A"]
    agg, nc = solver.host_aggregate_level(A, block_size=bs, threshold=0.02, max_aggregate_nodes=8)
    P = solver.host_smoothed_prolongator(A, agg, nc, 0.37, Ct=pb.mats["Ct"], w_inv=pb.inv_w_diag_squared(), gamma=10.0)
    return P, agg, bs


@pytest.fixture(scope="module")
def smoothed():
    return {which: _smoothed(which) for which in ("stokes", "laplace")}


def _same_bytes(P, Q):
    return (P.nrows, P.ncols) == (Q.nrows, Q.ncols) and np.array_equal(P.row_ptr, Q.row_ptr) and \
        np.array_equal(P.col, Q.col) and P.val.tobytes() == Q.val.tobytes()


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("which", ["stokes", "laplace"])
def test_library_equals_the_restated_rule(smoothed, which, rule):
    P, agg, bs = smoothed[which]
    tau, k = rule
    got = solver.host_truncate_prolongator(P, agg, bs, tau, k)
    want = tr.truncate_rows(P, agg, bs, tau, k)
    np.testing.assert_array_equal(got.row_ptr, want.row_ptr)
    np.testing.assert_array_equal(got.col, want.col)
    assert got.val.tobytes() == want.val.tobytes()
    assert got.nnz < P.nnz                                    # every rule of the list bites


@pytest.mark.parametrize("which", ["stokes", "laplace"])
def test_no_truncation_is_the_identity(smoothed, which):
    P, agg, bs = smoothed[which]
    assert _same_bytes(solver.host_truncate_prolongator(P, agg, bs, 0.0, 0), P)
    # explicit zeros stay too
    Z = problems.Csr(P.nrows, P.ncols, P.row_ptr.copy(), P.col.copy(), P.val.copy())
    first = int(np.nonzero(np.diff(P.row_ptr) > 1)[0][0])
    e = int(P.row_ptr[first])
    e += 1 if P.col[e] == agg[first] else 0
    Z.val[e] = 0.0
    assert _same_bytes(solver.host_truncate_prolongator(Z, agg, bs, 0.0, 0), Z)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("which", ["stokes", "laplace"])
def test_properties(smoothed, which, rule):
    P, agg, bs = smoothed[which]
    tau, k = rule
    T = solver.host_truncate_prolongator(P, agg, bs, tau, k)
    assert _same_bytes(T, solver.host_truncate_prolongator(P, agg, bs, tau, k))
    np.testing.assert_array_equal(np.diff(T.row_ptr) == 0, agg < 0)
    for i in range(P.nrows):
        if agg[i] < 0:
            continue
        tc, tv = T.col[T.row_ptr[i]:T.row_ptr[i + 1]], T.val[T.row_ptr[i]:T.row_ptr[i + 1]]
        pc, pv = P.col[P.row_ptr[i]:P.row_ptr[i + 1]], P.val[P.row_ptr[i]:P.row_ptr[i + 1]]
        assert agg[i] in tc and np.all(np.diff(tc) > 0) and np.all(np.isin(tc, pc))
        assert k == 0 or tc.size <= k
        for c in range(bs):
            if (tc % bs == c).any():
                assert abs(tv[tc % bs == c].sum() - pv[pc % bs == c].sum()) <= 1e-14 * np.abs(pv).sum(), (i, c)
    if k == 1:                                                # the pattern of the tentative prolongator
        rows = np.nonzero(agg >= 0)[0]
        np.testing.assert_array_equal(T.col, agg[rows])
        np.testing.assert_array_equal(np.diff(T.row_ptr), (agg >= 0).astype(np.int64))


def _csr(nrows, ncols, rows):
    rp = np.cumsum([0] + [len(r[0]) for r in rows]).astype(np.int64)
    col = np.array([c for r in rows for c in r[0]], np.int32)
    val = np.array([v for r in rows for v in r[1]], np.float64)
    return problems.Csr(nrows, ncols, rp, col, val)


def test_tie_rule_one_component():
    """Equal magnitudes, opposite signs: the smaller column wins the place and is the lump target."""
    P = _csr(3, 4, [([0, 1, 2, 3], [1.0, 0.5, -0.5, 0.25]),     # g = 0: keeps 0 and 1 (not 2); 0 takes -0.5 + 0.25
                    ([0, 1, 2], [-0.5, 0.5, 0.125]),            # g = 2: keeps 2 and 0 (not 1); 0 takes 0.5 -> 0.0
                    ([1, 3], [2.0, 3.0])])                      # no aggregate: empty
    agg = np.array([0, 2, -1], np.int32)
    T = solver.host_truncate_prolongator(P, agg, 1, 0.0, 2)
    np.testing.assert_array_equal(T.row_ptr, [0, 2, 4, 4])
    np.testing.assert_array_equal(T.col, [0, 1, 0, 2])
    np.testing.assert_array_equal(T.val, [0.75, 0.5, 0.0, 0.125])
    assert _same_bytes(T, tr.truncate_rows(P, agg, 1, 0.0, 2))
    # the drop tolerance keeps a tie whole: |p| >= tau * max on both sides of it
    T = solver.host_truncate_prolongator(P, agg, 1, 0.5, 0)
    np.testing.assert_array_equal(T.col, [0, 1, 2, 0, 1, 2])
    np.testing.assert_array_equal(T.val, [1.25, 0.5, -0.5, -0.5, 0.5, 0.125])


def test_tie_rule_per_component():
    """Two components: each lumps its own dropped entries into its own first kept entry; a component that keeps nothing
    loses them."""
    P = _csr(2, 6, [([0, 1, 2, 3, 4], [0.5, 1.0, -0.5, 0.25, 0.5]),
                    ([0, 1], [1.0, 0.375])])
    agg = np.array([1, 0], np.int32)
    T = solver.host_truncate_prolongator(P, agg, 2, 0.0, 3)
    # row 0: g = 1 and the first two of (0: .5, 2: -.5, 4: .5, 3: .25) = 0, 2; component 0 drops 4 -> column 0,
    # component 1 drops 3 -> column 1
    np.testing.assert_array_equal(T.row_ptr, [0, 3, 5])
    np.testing.assert_array_equal(T.col, [0, 1, 2, 0, 1])
    np.testing.assert_array_equal(T.val, [1.0, 1.25, -0.5, 1.0, 0.375])
    T = solver.host_truncate_prolongator(P, agg, 2, 0.0, 1)
    np.testing.assert_array_equal(T.col, [1, 0])
    np.testing.assert_array_equal(T.val, [1.25, 1.0])           # row 1: component 1 kept nothing, 0.375 is gone
    assert _same_bytes(T, tr.truncate_rows(P, agg, 2, 0.0, 1))


def test_size_query_and_argument_validation(smoothed):
    lib = solver.load_library()
    P, agg, bs = smoothed["laplace"]
    rp = np.ascontiguousarray(P.row_ptr, np.int64)
    col = np.ascontiguousarray(P.col, np.int32)
    val = np.ascontiguousarray(P.val, np.float64)
    agg = np.ascontiguousarray(agg, np.int32)
    orp = np.empty(P.nrows + 1, np.int64)
    nnz = C.c_int64(-1)

    def call(tau=0.1, k=3, block=bs, a=agg, c=col, rp_=rp, ncoarse=P.ncols, oc=None, ov=None, cap=0):
        return lib.alfd_host_truncate_prolongator(P.nrows, ncoarse, rp_.ctypes.data, c.ctypes.data, val.ctypes.data,
                                                  a.ctypes.data, block, tau, k, orp.ctypes.data, oc, ov, cap,
                                                  C.byref(nnz))
    # size query, then too small a capacity, then the real call
    assert call() == _abi.OK
    n_nz = nnz.value
    assert 0 < n_nz < P.nnz and orp[0] == 0 and orp[-1] == n_nz
    ocol = np.empty(n_nz, np.int32)
    oval = np.empty(n_nz, np.float64)
    assert call(oc=ocol.ctypes.data, ov=oval.ctypes.data, cap=n_nz - 1) == _abi.E_INVALID
    assert call(oc=ocol.ctypes.data, ov=oval.ctypes.data, cap=n_nz) == _abi.OK
    T = solver.host_truncate_prolongator(P, agg, bs, 0.1, 3)
    np.testing.assert_array_equal(T.col, ocol)
    assert T.val.tobytes() == oval.tobytes()
    # the drop tolerance, the cap, the block size
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert call(tau=bad) == _abi.E_INVALID
    assert call(k=-1) == _abi.E_INVALID
    assert call(block=0) == _abi.E_INVALID
    # columns outside [0, n_coarse), unsorted rows
    bad = col.copy()
    bad[0] = P.ncols
    assert call(c=bad) == _abi.E_INVALID
    bad[0] = -1
    assert call(c=bad) == _abi.E_INVALID
    row = int(np.nonzero(np.diff(rp) > 1)[0][0])
    bad = col.copy()
    bad[rp[row]], bad[rp[row] + 1] = col[rp[row] + 1], col[rp[row]]
    assert call(c=bad) == _abi.E_INVALID
    bad = col.copy()
    bad[rp[row] + 1] = col[rp[row]]                            # a repeated column
    assert call(c=bad) == _abi.E_INVALID
    # agg out of range, a row that lacks its aggregate's column
    bad = agg.copy()
    bad[row] = P.ncols
    assert call(a=bad) == _abi.E_INVALID
    bad[row] = -2
    assert call(a=bad) == _abi.E_INVALID
    absent = np.setdiff1d(np.arange(P.ncols), col[rp[row]:rp[row + 1]])
    assert absent.size
    bad[row] = absent[0]
    assert call(a=bad) == _abi.E_INVALID
    bad_rp = rp.copy()
    bad_rp[0] = 1
    assert call(rp_=bad_rp) == _abi.E_INVALID
    assert call(ncoarse=0) == _abi.E_INVALID
    with pytest.raises(ValueError):
        solver.host_truncate_prolongator(P, agg[:-1], bs, 0.1, 3)


# ---- the effect, on the CPU oracle ----------------------------------------------------------------------------------

def _ml_cfg(inner_max):
    cfg = _abi.default_config(_abi.AL_STOKES)
    cfg.inner.max_steps = inner_max
    cfg.inner_prec = _abi.PREC_MULTILEVEL
    cfg.ml_smooth_degree, cfg.ml_smooth_ratio, cfg.ml_coarse_degree = 4, 256.0, 10
    return cfg


def _host_hierarchy(pb, cfg, smoothed, k=0, solve_levels=True):
    """Levels from the host routines alone (theta 0.02, <= 8 nodes, min_coarse 300): SciPy Galerkin products, lambda_max
    from eigsh.  Plain aggregation: [(agg, n_coarse)]; smoothed: [(P, n_coarse)], every row cut to k entries if k > 0."""
    A, Ct = pb.mats["A"].to_scipy().tocsr(), pb.mats["Ct"].to_scipy().tocsr()
    w = pb.inv_w_diag_squared()
    levels = []
    while len(levels) < 7:
        A.sort_indices()
        Ac = problems.Csr.from_scipy(A)
        agg, nc = solver.host_aggregate_level(Ac, block_size=3, threshold=0.02, max_aggregate_nodes=8)
        if nc < 1 or nc >= A.shape[0]:
            break
        if smoothed:
            aug = (A + cfg.gamma * (Ct @ sp.diags(w) @ Ct.T)).tocsr()
            s = sp.diags(1.0 / np.sqrt(aug.diagonal()))
            lam = float(spla.eigsh(s @ aug @ s, k=1, which="LA", return_eigenvectors=False, tol=1e-8)[0])
            Ct.sort_indices()
            P = solver.host_smoothed_prolongator(Ac, agg, nc, (4.0 / 3.0) / lam, Ct=problems.Csr.from_scipy(Ct),
                                                 w_inv=w, gamma=cfg.gamma)
            if k:
                P = solver.host_truncate_prolongator(P, agg, 3, 0.0, k)
            levels.append((P, nc))
            Ps = P.to_scipy().tocsr()
        else:
            levels.append((agg, nc))
            rows = np.nonzero(agg >= 0)[0]
            Ps = sp.csr_matrix((np.ones(rows.size), (rows, agg[rows])), shape=(A.shape[0], nc))
        if nc <= 300 or not solve_levels:
            break
        A = (Ps.T @ (A @ Ps)).tocsr()
        Ct = (Ps.T @ Ct).tocsr()
    return levels


def _oracle_counts(pb, cfg, levels):
    osys = oracle.system_from_problem(pb, aggregates=levels)
    rc, rhs = osys.augment_rhs(cfg, cases.rhs_of(pb))
    assert rc == 0
    rc, x, res, hist = osys.solve(cfg, rhs)
    assert rc == 0
    return res.outer_iterations, int(res.inner_iterations)


def test_four_entries_per_row_keep_the_gain_of_smoothing():
    """Hanging-node Stokes, N = 12: cut to <= 4 entries per row and lumped, the smoothed hierarchy needs strictly fewer
    inner iterations than plain aggregation (measured 10 / 109 against 10 / 127) with at most a quarter of the
    untruncated level-0 entries (measured 0.12)."""
    pb = cases.hanging_node_variant(problems.stokes3d_sphere(12, 0))
    cfg = _ml_cfg(inner_max=1000)
    plain = _host_hierarchy(pb, cfg, smoothed=False)
    cut = _host_hierarchy(pb, cfg, smoothed=True, k=4)
    whole = _host_hierarchy(pb, cfg, smoothed=True, solve_levels=False)
    outer_p, inner_p = _oracle_counts(pb, cfg, plain)
    outer_c, inner_c = _oracle_counts(pb, cfg, cut)
    ratio = cut[0][0].nnz / whole[0][0].nnz
    print(f"N = 12 hanging: plain {outer_p} / {inner_p}; <= 4 per row, lumped {outer_c} / {inner_c}; "
          f"level-0 P {cut[0][0].nnz} of {whole[0][0].nnz} entries ({ratio:.3f})")
    assert inner_c < inner_p, (inner_c, inner_p)
    assert ratio <= 0.25, ratio
