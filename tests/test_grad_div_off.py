"""Stokes without grad-div (`Grad-div stabilization = false`), host side: the .prm mapping and the
generator's 2 eps(u):eps(v) velocity block, bit for bit against the grad-div matrix and against an
independent SciPy Kronecker assembly."""
import os

import numpy as np
import numpy.polynomial.polynomial as pl
import pytest
import scipy.sparse as sp

from fictitious_domain_al_preconditioners_amd import _abi, prm, problems

_PRM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_prm", "parameters_stokes_3d.prm")


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def _stokes_prm(grad_div, amg):
    text = open(_PRM).read()
    text = text.replace("set Grad-div stabilization             = true",
                        f"set Grad-div stabilization             = {'true' if grad_div else 'false'}")
    text = text.replace("set AMG for augmented block            = true",
                        f"set AMG for augmented block            = {'true' if amg else 'false'}")
    return prm.config_from_prm(prm.parse(text))


def test_prm_grad_div_off_without_amg_maps_to_identity_inner_cg():
    cfg, info = _stokes_prm(grad_div=False, amg=False)
    assert cfg.grad_div_in_A == 0
    assert cfg.inner_prec == _abi.PREC_IDENTITY
    assert cfg.gamma_grad_div == 10.0
    assert info["unsupported"] == []


def test_prm_grad_div_off_with_amg_stays_unsupported():
    cfg, info = _stokes_prm(grad_div=False, amg=True)
    assert cfg.grad_div_in_A == 0
    assert len(info["unsupported"]) == 1 and "Grad-div stabilization = false" in info["unsupported"][0]
    cfg_on, info_on = _stokes_prm(grad_div=True, amg=True)
    assert cfg_on.grad_div_in_A == 1 and info_on["unsupported"] == []
    assert cfg_on.inner_prec == _abi.default_config(_abi.AL_STOKES).inner_prec


def _kw(dim):
    return dict(dim=dim, degree=2, ncomp=dim, n_cells=4 if dim == 2 else 3, stokes=True, radius=0.2,
                immersed_refine=1, center=(0.5, 0.5, 0.5))


def _blocks(m, nc):
    """CSR -> {(a, b): scipy block of component a rows, component b columns} (node-major interleaving)."""
    m = m.to_scipy().tocsr()
    return {(a, b): m[a::nc, b::nc].tocsr() for a in range(nc) for b in range(nc)}


@pytest.mark.parametrize("dim", [2, 3])
def test_sym_grad_is_grad_grad_plus_block_swapped_grad_div_bit_for_bit(dim):
    eps = problems.generate(sym_grad=True, **_kw(dim)).mats["A"]
    lap = problems.generate(**_kw(dim)).mats["A"]
    gd1 = problems.generate(grad_div=True, gamma_grad_div=1.0, **_kw(dim)).mats["A"]
    # same sparsity; default output unchanged by the option being present
    assert np.array_equal(eps.row_ptr, lap.row_ptr) and np.array_equal(eps.col, lap.col)
    E, G = _blocks(eps, dim), _blocks(gd1, dim)
    for a in range(dim):
        for b in range(dim):
            want = G[(a, a)] if a == b else G[(b, a)]   # diagonal blocks: grad:grad + T_aa = grad:grad + GD_aa
            got = E[(a, b)]
            assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
            assert np.array_equal(got.data, want.data), (a, b)
    # the off-diagonal blocks of grad:grad are zero, so T itself is there: T_(b,a) == GD_(a,b)
    L = _blocks(lap, dim)
    assert all(abs(L[(a, b)]).max() == 0 for a in range(dim) for b in range(dim) if a != b)
    with pytest.raises(ValueError):
        problems.generate(sym_grad=True, **{**_kw(dim), "stokes": False, "degree": 1})


def _lagrange(nodes):
    out = []
    for i, xi in enumerate(nodes):
        c = np.array([1.0])
        for j, xj in enumerate(nodes):
            if i != j:
                c = pl.polymul(c, np.array([-xj, 1.0]) / (xi - xj))
        out.append(c)
    return out


def _integ(c):
    ci = pl.polyint(c)
    return pl.polyval(1.0, ci) - pl.polyval(0.0, ci)


def _mats1d(p, n, h):
    lr = _lagrange(np.linspace(0, 1, p + 1))
    m = sp.lil_matrix((p * n + 1, p * n + 1))
    k, g = m.copy(), m.copy()
    for c in range(n):
        for a in range(p + 1):
            for b in range(p + 1):
                m[c * p + a, c * p + b] += _integ(pl.polymul(lr[a], lr[b])) * h
                k[c * p + a, c * p + b] += _integ(pl.polymul(pl.polyder(lr[a]), pl.polyder(lr[b]))) / h
                g[c * p + a, c * p + b] += _integ(pl.polymul(pl.polyder(lr[a]), lr[b]))   # int phi_i' phi_j
    return m.tocsr(), k.tocsr(), g.tocsr()


@pytest.mark.parametrize("dim", [2, 3])
def test_sym_grad_matches_scipy_assembly_of_2_eps_eps(dim):
    """2 eps(u):eps(v) = sum_{c,d} eps_cd(u) eps_cd(v) * 2, assembled as sum over (c, d) of int d_c u_d d_c v_d +
    int d_d u_c d_c v_d from 1-D Q2 factors (x fastest), homogeneous Dirichlet rows/columns replaced by identity."""
    kw = _kw(dim)
    n = kw["n_cells"]
    M, K, G = _mats1d(2, n, 1.0 / n)
    n1 = 2 * n + 1
    nn = n1 ** dim

    def kron(fs):   # fs[0] acts on x (fastest index)
        out = fs[0]
        for f in fs[1:]:
            out = sp.kron(f, out)
        return out

    def dd(i_axis, j_axis):
        """int d_{i_axis} phi_row d_{j_axis} phi_col over the tensor grid"""
        fs = [M] * dim
        if i_axis == j_axis:
            fs[i_axis] = K
        else:
            fs[i_axis], fs[j_axis] = G, G.T
        return kron(fs)

    lap = sum(dd(c, c) for c in range(dim))
    # block (a, b): test phi_i e_a, trial phi_j e_b: delta_ab grad:grad + int d_b phi_i d_a phi_j
    big = sp.bmat([[(lap if a == b else 0 * lap) + dd(b, a) for b in range(dim)] for a in range(dim)]).tocsr()
    perm = np.array([(i % dim) * nn + i // dim for i in range(dim * nn)])
    big = big[perm][:, perm]
    idx = np.arange(nn)
    bnd = np.zeros(nn, bool)
    for d in range(dim):
        c = (idx // n1 ** d) % n1
        bnd |= (c == 0) | (c == n1 - 1)
    bd = np.repeat(bnd, dim)
    D = sp.diags((~bd).astype(float))
    ref = D @ big @ D + sp.diags(bd.astype(float))
    got = problems.generate(sym_grad=True, **kw).mats["A"].to_scipy()
    assert abs(got - ref).max() < 1e-13
    assert abs(got - got.T).max() == 0.0
