"""Independent restatement of the multilevel preconditioners of the immersed block, for tests only.

Composes tests/precond_reference.py (NumPy / SciPy, written from the definitions in include/alfd/alfd.h) -- nothing here
reads the library or the oracle; the oracle has no block-1 hierarchy.

  A22 (AL_ELL_MODIFIED, ALFD_INNER_OP_A22):  the V-cycle of precond_reference.InnerPreconditioner on (A, Ct, w, gamma)
      := (A2, M, w, gamma2) with the block-1 prolongators, no interface patch (M touches every row);
  AUG2 (AL_ELL_IDEAL, ALFD_INNER_OP_AUG2):   z = [M0^-1 r0 ; V1(r1)], the block diagonal of the block-0 preconditioner
      (V-cycle, patch included when ml_patch_degree > 0) and the A22 V-cycle; every level-0 eigenvalue estimate is the
      power iteration on that block's own operator from the hash vector.

Tolerance of the comparisons against this file (tests/test_immersed_hierarchy.py, tests/test_gpu_immersed_hierarchy.py),
by the recipe of precond_reference, per configuration: max|z_f64 - z_longdouble| / max|z_longdouble| of the restatement
ALONE over the inputs (uniform(-1, 1) with two seeds, a constant, a unit vector), times 64 (margin for the kernels'
lane-split summation order), floored at 1e-13, capped at 1e-9:

  configuration   block-1 levels (+ block 0)    f64 vs longdouble   asymmetry   tol
  a22_multilevel  289 / 81 / 25                 3.9e-15             7.5e-16     2.5e-13
  a22_gmg         289 / 81 / 25                 6.1e-15             8.2e-16     3.9e-13
  a22_gmg_jump    289 / 81 / 25                 7.6e-13             2.2e-15     4.9e-11
  a22_gmg_8       81 / 25                       2.3e-12             1.6e-15     1.5e-10
  aug2_gmg        81 / 25 (+ 1089 / 225 / 49)   2.2e-15             2.5e-16     1.4e-13
  aug2_gmg_patch  81 / 25 (+ 1089 / 225 / 49)   1.8e-15             2.5e-16     1.2e-13
  a22_elasticity  288 / 108 / 36                4.6e-15             1.1e-15     2.9e-13
  a22_multilevel: elliptic 64 / 16, beta2 = 10, aggregates on block 0, Chebyshev coarsest sweep; a22_gmg / a22_gmg_jump:
  elliptic 64 / 16, beta2 = 10 / 1e3, explicit coarsest inverse; a22_gmg_8: elliptic 32 / 8, beta2 = 1e3; aug2_gmg[_patch]:
  the ideal variant at 32 / 8 without / with the interface patch on block 0; a22_elasticity: elasticity3d(8), 5x3x3 cells.
The constant vector is the near-null mode of A22 = (beta2 - beta1) K + gamma2 M W M (a pure-Neumann stiffness matrix plus
a small shift): with beta2 = 1e3 its condition number, and with it the rounding of the explicit coarsest inverse, is 100
times that of beta2 = 10 -- the a22_gmg_jump row.  The three larger configurations of the GPU checks (aug2_gmg_64,
aug2_gmg_patch_64 at 4225 + 289 unknowns, a22_gmg_32 at 1089) take the row of their small twin with the same settings
(MEASURED_AS): the longdouble restatement of the three together did not finish in ten minutes of CPU time, which no
test could repeat.  The asymmetry column is max|M - M^T| / max|M| of the float64 restatement; the symmetry
checks allow an implementation 64 times it.

``test_tolerance_is_what_the_restatement_measures`` repeats the measurement and fails when it leaves the table.
"""
import types

import numpy as np

import precond_reference as pr

TOL_MARGIN = 64.0
TOL_FLOOR = 1e-13
TOL_CAP = 1e-9
# name -> (largest f64-vs-longdouble difference, asymmetry of the f64 operator): the table above
MEASURED = {
    "a22_multilevel": (3.9e-15, 7.5e-16),
    "a22_gmg": (6.1e-15, 8.2e-16),
    "a22_gmg_jump": (7.6e-13, 2.2e-15),
    "a22_gmg_8": (2.3e-12, 1.6e-15),
    "aug2_gmg": (2.2e-15, 2.5e-16),
    "aug2_gmg_patch": (1.8e-15, 2.5e-16),
    "a22_elasticity": (4.6e-15, 1.1e-15),
}
MEASURED_AS = {"aug2_gmg_64": "aug2_gmg", "aug2_gmg_patch_64": "aug2_gmg_patch", "a22_gmg_32": "a22_gmg_jump"}


def tol(name):
    t = max(TOL_FLOOR, TOL_MARGIN * MEASURED[MEASURED_AS.get(name, name)][0])
    assert t <= TOL_CAP, "a tolerance above 1e-9 means the restatement or a case is ill-posed"
    return t


def sym_tol(name):
    return TOL_MARGIN * MEASURED[MEASURED_AS.get(name, name)][1]


def plain(cfg, **changes):
    """The scalar fields of an alfd_config mirror as a plain namespace, with changes."""
    names = [f[0] for f in cfg._fields_] if hasattr(cfg, "_fields_") else list(vars(cfg))
    ns = types.SimpleNamespace(**{k: getattr(cfg, k) for k in names})
    for k, v in changes.items():
        setattr(ns, k, v)
    return ns


def _matrices(levels):
    return [(e[0] if isinstance(e, (tuple, list)) else e) for e in levels]


def _scipy(m):
    return m.to_scipy() if hasattr(m, "to_scipy") else m


class A22Preconditioner:
    """z = V1(r): the V-cycle on A22 = A2 + gamma2 M diag(w) M through the block-1 prolongators `levels`
    ([(Csr P, n_coarse), ...] or scipy matrices)."""

    def __init__(self, cfg, A2, M, w, levels, dtype=np.float64):
        c = plain(cfg, gamma=cfg.gamma2, ml_patch_degree=0, aug_assembled=0, inner_prec=pr.PREC_MULTILEVEL)
        self.inner = pr.InnerPreconditioner(c, _scipy(A2), _scipy(M), w, hierarchy=[_scipy(p) for p in _matrices(levels)],
                                            dtype=dtype, op="aug")
        self.levels = self.inner.levels
        self.n = self.inner.n

    def apply(self, r):
        return self.inner.apply(r)

    def dense(self):
        return self.inner.dense()

    def operator(self):
        """A22 itself (level 0 of the restatement)."""
        return self.levels[0].aug


class IdealPreconditioner:
    """z = [M0^-1 r0 ; V1(r1)] for the 2-block operator of the ideal variant; levels0: the block-0 hierarchy in any form
    precond_reference takes (aggregates or prolongators)."""

    def __init__(self, cfg, A, Ct, w, levels0, A2, M, levels1, dtype=np.float64):
        c0 = plain(cfg, inner_prec=pr.PREC_MULTILEVEL)
        h0 = [(_scipy(e[0]) if hasattr(e[0], "row_ptr") else e) if isinstance(e, (tuple, list)) else e for e in levels0]
        self.b0 = pr.InnerPreconditioner(c0, _scipy(A), _scipy(Ct), w, hierarchy=h0, dtype=dtype, op="aug")
        self.b1 = A22Preconditioner(cfg, A2, M, w, levels1, dtype=dtype)
        self.n0, self.n = self.b0.n, self.b0.n + self.b1.n
        self.dtype = dtype

    def apply(self, r):
        r = np.asarray(r, self.dtype)
        return np.concatenate([self.b0.apply(r[:self.n0]), self.b1.apply(r[self.n0:])])

    def dense(self):
        return np.asarray(self.apply(np.eye(self.n, dtype=self.dtype)))


def rel(a, b):
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def asymmetry(m):
    m = np.asarray(m, np.float64)
    return float(np.max(np.abs(m - m.T)) / np.max(np.abs(m)))


def inputs(n):
    """The vectors of check (a): two uniform seeds, a constant, a unit vector."""
    unit = np.zeros(n)
    unit[n // 3] = 1.0
    return {"uniform(seed 11)": np.random.default_rng(11).uniform(-1, 1, n),
            "uniform(seed 12)": np.random.default_rng(12).uniform(-1, 1, n),
            "constant": np.ones(n), "unit vector": unit}


def pcg_iterations(aug, prec, b, reduce=1e-8, max_steps=2000):
    """Preconditioned CG on aug x = b from zero; steps until |r| < reduce * |b| (the REDUCTION rule of Control.check)."""
    x = np.zeros_like(b)
    r = b.copy()
    z = prec(r)
    p = z.copy()
    rz = r @ z
    r0 = np.sqrt(r @ r)
    for it in range(1, max_steps + 1):
        ap = aug @ p
        alpha = rz / (p @ ap)
        x += alpha * p
        r -= alpha * ap
        if np.sqrt(r @ r) < reduce * r0:
            return it
        z = prec(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return max_steps + 1
