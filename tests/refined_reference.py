"""Independent NumPy / SciPy restatement of the locally refined generator mode (generate(local_refine=1)).

The two-level space on n_cells base cells (flagged cells split once, hanging nodes constrained) is a SUBSPACE of the
uniform space on 2 n_cells cells.  So every refined operator is a Galerkin product of the uniform-fine one with the
matrix T whose column j holds the uniform-fine nodal values of refined basis function j:

    A = Tu' A_f Tu,   B = Tp' B_f Tu,   Mp = Tp' Mp_f Tp,   Ct = Tu' Ct_f,   f = Tu' f_f

with the fine operators from the EXISTING closed-form (Kronecker) generator at 2 n_cells -- a code path that shares
nothing with the cell-wise refined assembly.  The comparison runs on the free unknowns (neither Dirichlet nor
hanging): a basis function that vanishes on the boundary has zero fine coefficients there, so the Dirichlet rows the
fine generator replaced by identity never enter.

T needs no mesh data structure.  Both spaces live on the lattice of spacing h / (2 degree).  A lattice point that
lies in the closure of an UNREFINED base cell takes that cell's shape functions (1-D nested interpolation weights per
axis: 3/8, 3/4, -1/8 for Q2 at the quarter points, 1/2, 1/2 for Q1 at the midpoint, 0 / 1 at the cell's own nodes);
every other lattice point lies inside the refined region, is a node of a child cell, and is its own unknown.
"""
import numpy as np
import scipy.sparse as sp

from fictitious_domain_al_preconditioners_amd import problems


def flagged_cells(params, immersed_xyz):
    """The refinement rule: base cells (flat, x fastest) holding an immersed node -- the lower cell on a shared
    face -- and their face neighbours."""
    dim, n = params["dim"], params["n_cells"]
    h = (params["hi"] - params["lo"]) / n
    xyz = np.asarray(immersed_xyz).reshape(-1, 3)[:, :dim]
    s = (xyz - params["lo"]) / h
    c = np.floor(s)
    c = np.clip(c - (c == s), 0, n - 1).astype(np.int64)
    holds = np.zeros((n,) * dim, bool)            # indexed [c0, c1(, c2)]
    holds[tuple(c.T)] = True
    flag = holds.copy()
    for d in range(dim):
        lo = [slice(None)] * dim
        hi = [slice(None)] * dim
        lo[d], hi[d] = slice(0, n - 1), slice(1, n)
        flag[tuple(hi)] |= holds[tuple(lo)]
        flag[tuple(lo)] |= holds[tuple(hi)]
    return flag.reshape(-1, order="F")            # x fastest


def _lagrange(k, xi):
    """Values of the k + 1 equispaced Lagrange polynomials of [0, 1] at xi (array) -> [point, local node]."""
    nodes = np.arange(k + 1) / k
    out = np.ones((xi.size, k + 1))
    for i in range(k + 1):
        for j in range(k + 1):
            if j != i:
                out[:, i] *= (xi - nodes[j]) / (nodes[i] - nodes[j])
    return out


class RefinedSpace:
    """Nodes, masks and the transfer T (uniform-fine lattice points x refined nodes) of the degree-k space."""

    def __init__(self, params, flag, k, dirichlet):
        dim, n = params["dim"], params["n_cells"]
        w = 2 * k
        L = w * n + 1
        pts = np.arange(L ** dim)
        x = np.stack([(pts // L ** d) % L for d in range(dim)], axis=1)          # lattice coordinates, x fastest
        flag_nd = flag.reshape((n,) * dim, order="F")
        host = -np.ones((pts.size, dim), np.int64)      # lowest unrefined base cell whose closure holds the point
        have = np.zeros(pts.size, bool)
        in_refined = np.zeros(pts.size, bool)
        for t in range(2 ** dim):                       # candidates, lexicographic with the lower cell first
            c = np.empty_like(x)
            ok = np.ones(pts.size, bool)
            for d in range(dim):
                up = (t >> d) & 1
                on_face = x[:, d] % w == 0
                c[:, d] = np.where(on_face, x[:, d] // w - 1 + up, x[:, d] // w)
                ok &= on_face | (up == 0)               # interior along d: one candidate only
            ok &= np.all((c >= 0) & (c < n), axis=1)
            fl = np.zeros(pts.size, bool)
            fl[ok] = flag_nd[tuple(c[ok].T)]
            in_refined |= ok & fl
            new = ok & ~fl & ~have
            host[new] = c[new]
            have |= new
        odd = np.any(x % 2 == 1, axis=1)
        is_node = ~odd | in_refined
        self.k, self.L, self.dim = k, L, dim
        self.lattice = pts[is_node]
        self.hanging = (odd & have)[is_node]
        on_bnd = np.any((x == 0) | (x == L - 1), axis=1)
        self.boundary = on_bnd[is_node] if dirichlet else np.zeros(self.lattice.size, bool)
        self.free = ~self.hanging & ~self.boundary
        self.points = params["lo"] + (params["hi"] - params["lo"]) / (L - 1) * x[is_node]
        node_of = -np.ones(pts.size, np.int64)
        node_of[is_node] = np.arange(self.lattice.size)
        # T: identity where no unrefined cell holds the point, else that cell's shape functions
        rows = [pts[~have]]
        cols = [node_of[~have]]
        vals = [np.ones(int((~have).sum()))]
        p = pts[have]
        w1 = [_lagrange(k, (x[have, d] - w * host[have, d]) / w) for d in range(dim)]
        for l in range((k + 1) ** dim):
            ld = [(l // (k + 1) ** d) % (k + 1) for d in range(dim)]
            wt = np.ones(p.size)
            y = np.zeros(p.size, np.int64)
            for d in reversed(range(dim)):
                wt = wt * w1[d][:, ld[d]]
                y = y * L + (w * host[have, d] + 2 * ld[d])
            nz = wt != 0.0
            rows.append(p[nz]); cols.append(node_of[y[nz]]); vals.append(wt[nz])
        cols = np.concatenate(cols)
        assert cols.min() >= 0
        self.T = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), cols)),
                               shape=(pts.size, self.lattice.size))


def _components(T, ncomp):
    return sp.kron(T, sp.identity(ncomp)).tocsr() if ncomp > 1 else T


def reference(kwargs):
    """kwargs: generate() arguments of the refined problem without local_refine / assembly.  Returns a dict with the
    refined spaces ("U", "P" or None), the rule's flags and the Galerkin operators on ALL refined unknowns (compare on
    the free ones: masks "free_u", "free_p")."""
    fine_kw = dict(kwargs)
    fine_kw["n_cells"] = 2 * kwargs["n_cells"]
    fine = problems.generate(assembly="kronecker", **fine_kw)
    params = dict(fine.params)
    params["n_cells"] = kwargs["n_cells"]
    flag = flagged_cells(params, fine.vecs["immersed_xyz"])
    k, ncomp = params["degree"], params["ncomp"]
    U = RefinedSpace(params, flag, k, True)
    Tu = _components(U.T, ncomp)
    out = {"flag": flag, "U": U, "P": None, "free_u": np.repeat(U.free, ncomp)}
    Af = fine.mats["A"].to_scipy()
    out["A"] = (Tu.T @ Af @ Tu).tocsr()
    out["Ct"] = (Tu.T @ fine.mats["Ct"].to_scipy()).tocsr()
    out["f"] = Tu.T @ fine.vecs["f"]
    for name in ("M", "K"):
        out[name] = fine.mats[name].to_scipy()
    out["g"] = fine.vecs["g"]
    if "B" in fine.mats:
        Pq = RefinedSpace(params, flag, k - 1, False)
        out["P"], out["free_p"] = Pq, Pq.free
        out["B"] = (Pq.T.T @ fine.mats["B"].to_scipy() @ Tu).tocsr()
        out["Mp"] = (Pq.T.T @ fine.mats["Mp"].to_scipy() @ Pq.T).tocsr()
    return out
