"""The multigrid hierarchy of the immersed block (block 1) on the CPU: the transfers of
problems.immersed_tensor_prolongators, and the facts the GPU tests (tests/test_gpu_immersed_hierarchy.py) lean on, taken
from the NumPy restatement tests/immersed_hierarchy_reference.py alone.  The configurations defined here are shared with
the GPU file."""
import numpy as np
import pytest
import scipy.sparse as sp

import cases
import immersed_hierarchy_reference as ihr
import precond_reference as pr
from fictitious_domain_al_preconditioners_amd import _abi, problems

IMM_MIN_COARSE = 30          # 16^2 cells: 289 / 81 / 25;  8^2: 81 / 25;  32^2: 1089 / 289 / 81 / 25


class Config:
    """problem, alfd_config, the hierarchies of both blocks, the inner operator the multilevel preconditioner is for."""

    def __init__(self, name, pb, cfg, levels0, levels1, op):
        self.name, self.pb, self.cfg, self.levels0, self.levels1, self.op = name, pb, cfg, levels0, levels1, op

    def inv_w(self):
        return self.pb.inv_w_diag_of_mass_squared()

    def reference(self, dtype=np.float64):
        m = self.pb.mats
        if self.op == _abi.INNER_OP_A22:
            return ihr.A22Preconditioner(self.cfg, m["A2"], m["M"], self.inv_w(), self.levels1, dtype)
        return ihr.IdealPreconditioner(self.cfg, m["A"], m["Ct"], self.inv_w(), self.levels0, m["A2"], m["M"],
                                       self.levels1, dtype)


def _gmg(cfg, patch):
    """The multigrid settings of cases "elliptic_modified_gmg_patch": Chebyshev(4) over [lambda / 30, lambda], explicit
    coarsest inverse; the patch (block 0 only) on request."""
    cfg.inner_prec = _abi.PREC_MULTILEVEL
    cfg.ml_smooth_degree, cfg.ml_smooth_ratio, cfg.ml_coarse_direct = 4, 30.0, 1024
    cfg.ml_patch_degree, cfg.ml_patch_ratio = (5, 30.0) if patch else (0, 30.0)
    cfg.inner.max_steps = 100
    return cfg


def _elliptic(n_bg, n_fg, beta2, ideal):
    pb = problems.elliptic_interface2d(n_bg, n_fg, beta2=beta2)
    cfg = _abi.default_config(_abi.AL_ELL_IDEAL if ideal else _abi.AL_ELL_MODIFIED)
    cfg.gamma, cfg.gamma2 = 10.0, (10.0 if ideal else 1e-2)
    cfg.inner = _abi.Control(_abi.CTRL_REDUCTION, 100000, 1e-2, 1e-20)
    cfg.outer = _abi.Control(_abi.CTRL_REDUCTION, 1000, 1e-10, 1e-10)
    return pb, cfg


# the configurations of the tolerance table (every column of the operator is affordable in longdouble)
SMALL = ["a22_multilevel", "a22_gmg", "a22_gmg_jump", "a22_gmg_8", "aug2_gmg", "aug2_gmg_patch", "a22_elasticity"]
_cache = {}


def config(name):
    if name not in _cache:
        _cache[name] = _make(name)
    return _cache[name]


def _make(name):
    if name == "a22_multilevel":                # cases "elliptic_modified_multilevel": aggregates on block 0, Chebyshev coarsest
        pb, cfg = cases.case("elliptic_modified_multilevel")
        levels0 = cases.aggregates_of(pb, cfg)
    elif name in ("a22_gmg", "a22_gmg_jump", "a22_gmg_32", "a22_gmg_8"):   # cases "elliptic_modified_gmg_patch"
        n_bg, n_fg = (128, 32) if name.endswith("32") else (32, 8) if name.endswith("8") else (64, 16)
        pb, cfg = _elliptic(n_bg, n_fg, 10.0 if name == "a22_gmg" else 1e3, ideal=False)
        _gmg(cfg, patch=True)
        levels0 = problems.tensor_prolongators(pb.params, min_coarse=100)
    elif name.startswith("aug2_gmg"):           # the ideal variant; "_64": the size of the GPU vector checks
        n_bg, n_fg = (64, 16) if name.endswith("_64") else (32, 8)
        pb, cfg = _elliptic(n_bg, n_fg, 10.0, ideal=True)
        _gmg(cfg, patch="patch" in name)
        levels0 = problems.tensor_prolongators(pb.params, min_coarse=100)
    elif name == "a22_elasticity":              # 3 components, 3-D, odd immersed cell counts
        pb = problems.elasticity3d(8, cells_fg=(5, 3, 3))
        cfg = _abi.default_config(_abi.AL_ELL_MODIFIED)
        cfg.gamma, cfg.gamma2 = 10.0, 1e-2
        cfg.inner = _abi.Control(_abi.CTRL_REDUCTION, 10000, 1e-2, 1e-20)
        cfg.outer = _abi.Control(_abi.CTRL_REDUCTION, 1000, 1e-10, 1e-6)
        _gmg(cfg, patch=False)
        levels0 = problems.tensor_prolongators(pb.params, min_coarse=100)
    else:
        raise KeyError(name)
    levels1 = problems.immersed_tensor_prolongators(pb.params, min_coarse=IMM_MIN_COARSE)
    op = _abi.INNER_OP_AUG2 if cfg.variant == _abi.AL_ELL_IDEAL else _abi.INNER_OP_A22
    return Config(name, pb, cfg, levels0, levels1, op)


# ------------------------------------------------------------------------------------------------- the transfers
def _grid(cells):
    """Node coordinates (in cells of unit length) of the box grid, x fastest: shape (nodes, dim)."""
    axes = np.meshgrid(*[np.arange(c + 1, dtype=np.float64) / c for c in reversed(cells)], indexing="ij")
    return np.stack([a.ravel() for a in reversed(axes)], axis=1)


@pytest.mark.parametrize("cells,ncomp", [((8, 8), 1), ((16, 16), 1), ((5, 5), 1), ((4, 3, 5), 3)])
def test_immersed_tensor_prolongators(cells, ncomp):
    """Shapes, P 1 = 1 and every (multi)linear function reproduced on every level, node-major for 3 components."""
    levels = problems.immersed_tensor_prolongators(dict(ncomp=ncomp, immersed_cells=cells), min_coarse=1)
    assert len(levels) >= 1
    fine = list(cells)
    for P, nc in levels:
        coarse = [(c + 1) // 2 for c in fine]
        assert P.nrows == ncomp * int(np.prod([c + 1 for c in fine]))
        assert P.ncols == nc == ncomp * int(np.prod([c + 1 for c in coarse]))
        Ps = P.to_scipy()
        assert np.max(np.abs(Ps @ np.ones(nc) - 1.0)) <= 1e-15
        assert Ps.min() >= 0.0 and np.all(np.diff(Ps.indptr) <= 2 ** len(cells))
        xf, xc = _grid(fine), _grid(coarse)
        rng = np.random.default_rng(3)
        for comp in range(ncomp):
            coef = rng.uniform(-1, 1, len(cells) + 1)
            uc, uf = np.zeros(nc), np.zeros(P.nrows)
            uc[comp::ncomp] = coef[0] + xc @ coef[1:]
            uf[comp::ncomp] = coef[0] + xf @ coef[1:]
            assert np.max(np.abs(Ps @ uc - uf)) <= 1e-14, (cells, comp)
        fine = coarse
    assert min(fine) == 1 or len(levels) == 7


def test_transfers_follow_the_generators_node_order():
    """Nested Q1 spaces: P^T A2 P and P^T M P of the 16^2-cell immersed mesh ARE the matrices of the 8^2-cell mesh --
    which holds only if the rows of P follow the generator's node numbering."""
    fine, coarse = problems.elliptic_interface2d(16, 16), problems.elliptic_interface2d(16, 8)
    P = problems.immersed_tensor_prolongators(fine.params, min_coarse=IMM_MIN_COARSE)[0][0].to_scipy()
    for name in ("A2", "M"):
        galerkin = (P.T @ fine.mats[name].to_scipy() @ P).toarray()
        want = coarse.mats[name].to_scipy().toarray()
        assert np.max(np.abs(galerkin - want)) <= 1e-12 * np.max(np.abs(want)), name


def test_needs_a_box_meshed_immersed_domain():
    with pytest.raises(ValueError):
        problems.immersed_tensor_prolongators(problems.laplace2d_circle(16, 2).params)


# ------------------------------------------------------------------------------------------ the restatement's facts
def test_tolerance_is_what_the_restatement_measures():
    """f64 against longdouble on the restatement alone and the asymmetry of the f64 operator, per configuration: the
    table of immersed_hierarchy_reference."""
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than float64 on this machine"
    assert sorted(ihr.MEASURED) == sorted(SMALL)
    for name in SMALL:
        cf = config(name)
        r64, rld = cf.reference(), cf.reference(np.longdouble)
        errs = {what: ihr.rel(r64.apply(r), rld.apply(r)) for what, r in ihr.inputs(r64.n).items()}
        err, asym = max(errs.values()), ihr.asymmetry(r64.dense())
        b1 = r64 if cf.op == _abi.INNER_OP_A22 else r64.b1
        print(f"{name}: block-1 levels {[L.n for L in b1.levels]}, f64 vs longdouble {err:.2e} "
              f"({max(errs, key=errs.get)}), asymmetry {asym:.2e}, tol {ihr.tol(name):.2e}")
        assert err <= ihr.MEASURED[name][0], (name, err)
        assert asym <= ihr.MEASURED[name][1], (name, asym)
        assert ihr.tol(name) == max(1e-13, 64 * ihr.MEASURED[name][0]) <= 1e-9


_counts = {}


def _a22_facts(name):
    """(asymmetry, smallest eigenvalue of the symmetrised V-cycle, PCG steps with the V-cycle, with Chebyshev(4))."""
    if name not in _counts:
        cf = config(name)
        ref = cf.reference()
        m = ref.dense()
        a22 = ref.operator()
        b = np.random.default_rng(7).standard_normal(ref.n)
        b /= np.linalg.norm(b)
        sweep = pr.InnerPreconditioner(ihr.plain(cf.cfg, inner_prec=pr.PREC_CHEBYSHEV), cf.pb.mats["A"].to_scipy(),
                                       cf.pb.mats["Ct"].to_scipy(), cf.inv_w(), op="a22",
                                       A2=cf.pb.mats["A2"].to_scipy(), M=cf.pb.mats["M"].to_scipy())
        _counts[name] = (ihr.asymmetry(m), float(np.linalg.eigvalsh((m + m.T) / 2)[0]),
                         ihr.pcg_iterations(a22, ref.apply, b), ihr.pcg_iterations(a22, sweep.apply, b))
    return _counts[name]


@pytest.mark.parametrize("name", ["a22_gmg", "a22_gmg_jump", "a22_gmg_32"])
def test_vcycle_is_spd_and_halves_the_chebyshev_count(name):
    """The dense V-cycle on A22 is symmetric within 64 times the measured asymmetry and positive definite; PCG to a
    reduction of 1e-8 needs at most half the iterations of the Chebyshev(4) sweep (measured 7-8 against 20 / 23 / 36)."""
    asym, lmin, n_ml, n_cheb = _a22_facts(name)
    print(f"{name}: asymmetry {asym:.1e}, smallest eigenvalue {lmin:.3e}, PCG steps V-cycle {n_ml}, Chebyshev(4) {n_cheb}")
    assert asym <= ihr.sym_tol(name)
    assert lmin > 0.0
    assert 2 * n_ml <= n_cheb


def test_vcycle_count_does_not_grow_with_refinement():
    """32^2 immersed cells need at most one PCG step more than 16^2 (same jump)."""
    assert _a22_facts("a22_gmg_32")[2] <= _a22_facts("a22_gmg_jump")[2] + 1
