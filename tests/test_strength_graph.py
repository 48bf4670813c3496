"""The node graph of the algebraic aggregation on the host (alfd_host_strength_graph, alfd_host_aggregate_graph; no
GPU): the graph against a NumPy / SciPy statement of the rule written here -- bit for bit, the rule holds only max,
abs, one product, one correctly rounded square root and one comparison -- and the greedy passes on that graph against
alfd_host_aggregate_level, whose one routine was split into the two."""
import numpy as np
import pytest
import scipy.sparse as sp

import cases
from fictitious_domain_al_preconditioners_amd import problems, solver


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def _hanging():
    return cases.hanging_node_variant(problems.stokes3d_sphere(6, 0)).mats["A"], 3


def _laplace():
    return problems.generate(dim=3, degree=1, ncomp=1, n_cells=9, radius=0.1).mats["A"], 1


def _awkward():
    """bs = 2, 12 nodes: Dirichlet (diagonal-only) rows, a node whose only off-diagonal entries are explicit zeros
    (fixed all the same), an empty row, a node without a diagonal (d = 0), a negative diagonal, weak and strong ties,
    an edge that only one of the two rows of a node holds, and an edge to a fixed node (dropped)."""
    n, e = 24, []

    def put(i, j, v):
        e.append((i, j, float(v)))
    for i in range(n):
        if i not in (7, 10, 11):              # row 7 is empty, node 5 (rows 10, 11) has no diagonal
            put(i, i, -4.0 if i == 4 else 4.0 + 0.125 * i)
    put(2, 0, -1.0)                           # node 1 -> node 0, a Dirichlet node: dropped
    put(2, 4, -1.0), put(3, 5, -0.5), put(3, 4, 2.0)      # node 1 -> node 2, w = 2
    put(4, 2, -1.0), put(5, 3, 0.0)                        # node 2 -> node 1, an explicit zero beside it
    put(4, 12, 0.001), put(12, 4, 0.001)                   # weak tie node 2 <-> node 6
    put(6, 16, 0.0)                                        # node 3: row 6 holds only a zero, row 7 is empty -> fixed
    put(10, 12, -3.0), put(11, 2, 1.0)                     # node 5 (d = 0): every tie is strong
    put(12, 10, -3.0), put(13, 14, -2.0), put(14, 13, -2.0), put(15, 12, 0.25)
    put(18, 20, -1.0), put(20, 18, -1.0), put(19, 22, -1.5), put(22, 19, -1.5), put(21, 23, 0.0)
    i, j, v = (np.array(x) for x in zip(*e))
    m = sp.coo_matrix((v, (i, j)), shape=(n, n)).tocsr()   # keeps the explicit zeros
    m.sort_indices()
    out = problems.Csr(n, n, m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data.astype(np.float64))
    assert np.any(out.val == 0.0) and out.row_ptr[8] == out.row_ptr[7]
    return out, 2


CASES = {"hanging": _hanging, "laplace": _laplace, "awkward": _awkward}


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    A, bs = CASES[request.param]()
    return request.param, A, bs


def reference_graph(A, bs, theta):
    """The rule, stated with arrays: d_I = max |a_ii| of the node; a node is fixed when its rows hold no non-zero
    off-diagonal entry; W_IJ = max |a_ij| over the bs x bs block; the edge I -> J (J != I) exists when both nodes are
    free, W_IJ > 0 and W_IJ >= theta * sqrt(d_I d_J); neighbours ascending."""
    nn = A.nrows // bs
    rows = np.repeat(np.arange(A.nrows), np.diff(A.row_ptr))
    cols, absv = np.asarray(A.col, np.int64), np.abs(A.val)
    dia = rows == cols
    d = np.zeros(nn)
    np.maximum.at(d, rows[dia] // bs, absv[dia])
    fixed = np.ones(nn, np.int32)
    fixed[np.unique(rows[~dia & (A.val != 0.0)] // bs)] = 0
    I, J = rows // bs, cols // bs
    keep = (I != J) & (J < nn) & (absv > 0.0)
    keep &= (fixed[I] == 0) & (fixed[np.minimum(J, nn - 1)] == 0)
    # max-reduce duplicates: sort by (I, J, |a|) and keep the last of every (I, J)
    o = np.lexsort((absv[keep], J[keep], I[keep]))
    Ik, Jk, wk = I[keep][o], J[keep][o], absv[keep][o]
    last = np.r_[(Ik[1:] != Ik[:-1]) | (Jk[1:] != Jk[:-1]), True] if Ik.size else np.zeros(0, bool)
    Ik, Jk, wk = Ik[last], Jk[last], wk[last]
    strong = wk >= theta * np.sqrt(d[Ik] * d[Jk])
    Ik, Jk, wk = Ik[strong], Jk[strong], wk[strong]
    ptr = np.zeros(nn + 1, np.int64)
    np.add.at(ptr, Ik + 1, 1)
    return dict(d=d, fixed=fixed, node_ptr=np.cumsum(ptr), nbr=Jk.astype(np.int32), weight=wk)


@pytest.mark.parametrize("theta", [0.02, 0.0, 0.3])
def test_host_strength_graph_is_the_stated_rule(case, theta):
    name, A, bs = case
    g = solver.host_strength_graph(A, bs, theta)
    ref = reference_graph(A, bs, theta)
    for key in ("d", "fixed", "node_ptr", "nbr", "weight"):
        assert g[key].dtype == ref[key].dtype, key
        assert g[key].tobytes() == ref[key].tobytes(), (name, key)
    assert g["nbr"].size > 0 or theta == 0.3                  # the Q1 Laplace stencil has no tie that strong
    if name == "awkward":
        assert list(np.nonzero(g["fixed"])[0]) == [0, 3, 4, 8]
        assert g["d"][5] == 0.0 and g["d"][2] == 4.625          # no diagonal at all; |-4| against 4.625
        nb = lambda I: list(g["nbr"][g["node_ptr"][I]:g["node_ptr"][I + 1]])      # noqa: E731
        assert nb(1) == [2] and g["weight"][g["node_ptr"][1]] == 2.0
        assert nb(2) == {0.0: [1, 6], 0.02: [1], 0.3: []}[theta]      # w = 1 and 0.001 against 0.3 * 4.5 and 0.02 * 5.1
        assert nb(5) == [1, 6]                                   # d_5 = 0: threshold 0


@pytest.mark.parametrize("max_nodes", [8, 3])
def test_greedy_passes_on_the_graph_are_aggregate_level(case, max_nodes):
    name, A, bs = case
    for theta in (0.02, 0.3):
        agg, nc = solver.host_aggregate_level(A, bs, theta, max_nodes)
        agg2, nc2 = solver.host_aggregate_graph(solver.host_strength_graph(A, bs, theta), bs, max_nodes)
        assert nc2 == nc and np.array_equal(agg2, agg), (name, theta)
        assert nc > 0 and agg.max() == nc - 1


def test_argument_checks():
    import ctypes as C
    from fictitious_domain_al_preconditioners_amd import _abi
    lib = solver.load_library()
    A, bs = _awkward()
    nnz = C.c_int64(-1)
    rp, col, val = A.row_ptr, A.col, A.val
    call = lambda n, b, th, cap, nb: lib.alfd_host_strength_graph(      # noqa: E731
        n, rp.ctypes.data, col.ctypes.data, val.ctypes.data, b, th, None, None, None, nb, None, cap, C.byref(nnz))
    assert call(A.nrows, 2, 0.02, 0, None) == _abi.OK and nnz.value > 0        # sizing call
    nb = np.empty(nnz.value, np.int32)
    assert call(A.nrows, 2, 0.02, nnz.value - 1, nb.ctypes.data) == _abi.E_INVALID      # too small
    assert call(A.nrows, 2, 0.02, nnz.value, nb.ctypes.data) == _abi.OK
    assert call(A.nrows, 5, 0.02, 0, None) == _abi.E_INVALID                    # rows no multiple of block_size
    assert call(A.nrows, 2, -1.0, 0, None) == _abi.E_INVALID
    g = solver.host_strength_graph(A, bs)
    bad = dict(g, nbr=g["nbr"].copy())
    bad["nbr"][0] = 99
    with pytest.raises(solver.AlfdError):
        solver.host_aggregate_graph(bad, bs)
