"""Independent restatement of the inner preconditioners z = M^-1 r, for tests only.

Written from the DEFINITIONS in include/alfd/alfd.h (comments of alfd_config) and DESIGN.md section 6, not from the
library or the oracle: plain ``@`` products and NumPy sums, every derived operator formed here from the uploaded
matrices.  Imports numpy and scipy only.  Parametrised by dtype: sparse (scipy CSR) in float64, dense ndarrays in
any other dtype (np.longdouble), so that the effect of a different rounding on the operator can be MEASURED.

Definitions restated:
  Aug_0 = A + gamma Ct diag(w) C  (A alone when aug_assembled);  A_{l+1} = P^T A_l P, C_{l+1} = C_l P, Aug_l from those;
  P = the CSR prolongator, or for aggregates one entry weight_i (1 without weights) at (i, agg_i), rows agg_i < 0 empty;
  D_l = diag(Aug_l);  lambda_l = cheb_safety * |D^-1 Aug v| after cheb_power_its normalise-then-apply steps from
  v_i = 1 + ((i * 2654435761) mod 1024) / 1024;
  Chebyshev of degree k in D^-1 Aug over [lambda / ratio, lambda], zero start (Saad, Iterative Methods, Alg. 12.1);
  V-cycle: pre-smooth from zero, coarse correction, post-smooth; ml_smooth_degree_coarse (> 0) on levels >= 1; the coarsest
  level Chebyshev(ml_coarse_degree, ml_coarse_ratio) or numpy.linalg.inv when 0 < n_coarsest <= ml_coarse_direct;
  patch: S = non-empty rows of Ct, q = Chebyshev(ml_patch_degree, ml_patch_ratio) on Aug_0[S,S] with D restricted to S
  and a lambda of its own;  z1 = E q E^T r,  z2 = z1 + V(r - Aug z1),  z = z2 + E q E^T (r - Aug z2).
  A22 (elliptic, modified) = A2 + gamma2 M diag(w) M;  the 2-block operator of the ideal elliptic variant is
  [[A + gamma Ct W C, -gamma Ct W M], [-gamma2 M W C, A2 + gamma2 M W M]], its start vector the hash vector per block.

Tolerance of the comparisons against this file (tests/test_inner_preconditioner.py, tests/test_gpu_inner_preconditioner.py).
Measured from the restatement ALONE: the largest max|z_f64 - z_longdouble| / max|z_longdouble| over the inputs of check
(a) (uniform(-1,1) with two seeds, a constant, the indicator of the patch rows, a unit vector on a Dirichlet row) and the
small configurations, times 64 (margin for the kernels' lane-split summation order), floored at 1e-13:

  configuration (n_0; levels; patch rows)                         f64 vs longdouble   asymmetry of the f64 operator
  jacobi_al2              (1089)                                  1.5e-16             0
  cheb1_al2               (1089)                                  1.9e-16             0
  cheb2_operator_form     (1089)                                  2.5e-16             3.2e-17
  cheb4_stokes            (2187)                                  6.2e-16             8.6e-17
  ell_modified_aug        (1089)                                  4.9e-16             4.2e-17
  ell_modified_a22        (81)                                    5.3e-16             1.7e-16
  ell_ideal_aug2          (1089 + 81)                             3.1e-16             2.9e-17
  ml_aggregates           (2187 / 192 / 24)                       5.1e-16             1.5e-16
  ml_aggregates_weighted  (2187 / 192 / 24)                       4.7e-16             1.6e-16
  ml_gmg                  (2187 / 81 / 3)                         1.4e-15             6.1e-16
  ml_gmg_patch            (2187 / 81 / 3; 375)                    2.2e-15             8.6e-16
  ml_gmg_patch_bench      (2187 / 81 / 3; 375)                    4.2e-15             2.3e-15
  ml_operator_form_patch  (1089 / 225 / 49; 96)                   2.6e-15             3.4e-16
  largest 4.2e-15  ->  tol = 64 * 4.2e-15 = 2.7e-13 (above the floor).
The asymmetry column is max|M - M^T| / max|M| of the float64 restatement; check (c) allows an implementation 64 times it.

``test_tolerance_is_what_the_restatement_measures`` repeats the measurement and fails when it leaves the table.
"""
import numpy as np
import scipy.sparse as sp

# enum alfd_inner_prec (include/alfd/alfd.h)
PREC_IDENTITY, PREC_JACOBI, PREC_CHEBYSHEV, PREC_MULTILEVEL = range(4)

TOL_MARGIN = 64.0
TOL_FLOOR = 1e-13
MEASURED_F64_VS_LONGDOUBLE = 4.2e-15  # largest entry of the table above
TOL = max(TOL_FLOOR, TOL_MARGIN * MEASURED_F64_VS_LONGDOUBLE)
assert TOL <= 1e-9, "a tolerance above 1e-9 means the restatement or a case is ill-posed"


# ------------------------------------------------------------------ storage: sparse in float64, dense otherwise
def _op(m, dtype):
    if dtype == np.float64:
        return sp.csr_matrix(m, dtype=np.float64)
    return np.asarray(sp.csr_matrix(m).toarray(), dtype=dtype)


def _dense(m):
    return m.toarray() if sp.issparse(m) else np.asarray(m)


def _scale_rows(w, m):
    return sp.diags(w) @ m if sp.issparse(m) else w[:, None] * m


def _t(m):
    return m.T.tocsr() if sp.issparse(m) else m.T


def _add(a, b):
    s = a + b
    return s.tocsr() if sp.issparse(s) else s


def start_vector(n, dtype=np.float64):
    """v_i = 1 + ((i * 2654435761) mod 1024) / 1024: the start of every power iteration (part of the definition)."""
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(2654435761)) % np.uint64(1024)
    return 1 + h.astype(dtype) / dtype(1024)


def power_lambda(aug, d, its, safety, v, dtype=np.float64):
    """safety * |D^-1 Aug v| after `its` normalise-then-apply steps."""
    lam = dtype(0)
    for _ in range(int(its)):
        v = v / np.sqrt(np.sum(v * v))
        v = (aug @ v) / d
        lam = np.sqrt(np.sum(v * v))
    return lam * dtype(safety)


def chebyshev(aug, d, lam, ratio, degree, r):
    """Degree-`degree` Chebyshev polynomial in D^-1 Aug over [lam / ratio, lam] applied to r (a vector or the columns
    of a matrix), zero start: Saad, Alg. 12.1 with the Jacobi-preconditioned residual."""
    t = type(lam)
    lmin = lam / t(ratio)
    theta, delta = (lam + lmin) / 2, (lam - lmin) / 2
    sigma = theta / delta
    rho = 1 / sigma
    dd = d if r.ndim == 1 else d[:, None]
    res = r
    step = (res / dd) / theta
    z = step
    for _ in range(1, int(degree)):
        res = res - aug @ step
        rho_new = 1 / (2 * sigma - rho)
        step = (rho_new * rho) * step + (2 * rho_new / delta) * (res / dd)
        z = z + step
        rho = rho_new
    return z


def prolongator_from_aggregates(agg, n_coarse, weight=None):
    """One entry weight_i (1 without weights) at (i, agg_i); rows with agg_i < 0 stay empty."""
    agg = np.asarray(agg, np.int64)
    rows = np.flatnonzero(agg >= 0)
    vals = np.ones(rows.size) if weight is None else np.asarray(weight, np.float64)[rows]
    return sp.csr_matrix((vals, (rows, agg[rows])), shape=(agg.size, int(n_coarse)))


def _inverse(a, dtype):
    a = _dense(a)
    x = np.linalg.inv(np.asarray(a, np.float64))
    if dtype != np.float64:               # numpy.linalg has no extended precision: Newton steps X += X (I - A X)
        x = x.astype(dtype)
        eye = np.eye(a.shape[0], dtype=dtype)
        for _ in range(3):
            x = x + x @ (eye - a @ x)
    return x


class _Level:
    def __init__(self, aug, cfg, dtype, v0=None):
        self.aug = aug
        self.n = aug.shape[0]
        self.d = np.asarray(aug.diagonal(), dtype)
        self.lam = None
        if cfg.inner_prec in (PREC_CHEBYSHEV, PREC_MULTILEVEL):
            v0 = start_vector(self.n, dtype) if v0 is None else v0
            self.lam = power_lambda(aug, self.d, cfg.cheb_power_its, cfg.cheb_safety, v0, dtype)
        self.P = None                     # prolongator from the next coarser level


class InnerPreconditioner:
    """z = M^-1 r of one inner operator.

    cfg: any object with the fields of alfd_config.  A, Ct: scipy matrices (Ct n_0 x n_mult), w: the W^-1 diagonal.
    hierarchy (PREC_MULTILEVEL, op "aug"): one entry per level, a scipy prolongator (n_l x n_{l+1}) or a tuple
    (agg, n_coarse) / (agg, n_coarse, weight).
    op: "aug" (the augmented (1,1) block), "a22" (needs A2, M) or "aug2" (the 2-block operator; r = [r_0 ; r_1])."""

    def __init__(self, cfg, A, Ct, w, hierarchy=(), dtype=np.float64, op="aug", A2=None, M=None):
        self.cfg, self.dtype, self.op = cfg, dtype, op
        t = dtype
        w = np.asarray(w, t)
        self.prec = cfg.inner_prec
        if self.prec == PREC_MULTILEVEL and op != "aug":
            self.prec = PREC_CHEBYSHEV    # "other inner operators fall back to CHEBYSHEV"
        self.levels, self.patch, self.coarse_inverse = [], None, None
        A_l = _op(A, t)
        C_l = _op(sp.csr_matrix(Ct).T, t)
        pen = not cfg.aug_assembled

        def aug_of(A_l, C_l):
            return _add(A_l, t(cfg.gamma) * (_t(C_l) @ _scale_rows(w, C_l))) if pen else A_l

        if op == "a22" or op == "aug2":
            Mm, A2m = _op(M, t), _op(A2, t)
            a22 = _add(A2m, t(cfg.gamma2) * (Mm @ _scale_rows(w, Mm)))
            if op == "a22":
                self.levels = [_Level(a22, cfg, t)]
                return
            a11 = aug_of(A_l, C_l)
            a12 = -t(cfg.gamma) * (_t(C_l) @ _scale_rows(w, Mm))
            a21 = -t(cfg.gamma2) * (Mm @ _scale_rows(w, C_l))
            if t == np.float64:
                aug2 = sp.bmat([[a11, a12], [a21, a22]], format="csr")
            else:
                aug2 = np.block([[a11, a12], [a21, a22]])
            v0 = np.concatenate([start_vector(a11.shape[0], t), start_vector(a22.shape[0], t)])
            self.levels = [_Level(aug2, cfg, t, v0)]
            return
        if self.prec != PREC_MULTILEVEL:
            self.levels = [_Level(aug_of(A_l, C_l), cfg, t)]
            return
        if len(hierarchy) < 1:
            raise ValueError("PREC_MULTILEVEL needs a hierarchy")
        for entry in hierarchy:
            if isinstance(entry, (tuple, list)):
                P = prolongator_from_aggregates(entry[0], entry[1], entry[2] if len(entry) > 2 else None)
            else:
                P = entry
            P = _op(P, t)
            level = _Level(aug_of(A_l, C_l), cfg, t)
            level.P = P
            self.levels.append(level)
            A_l = _t(P) @ (A_l @ P)
            C_l = C_l @ P
        self.levels.append(_Level(aug_of(A_l, C_l), cfg, t))
        last = self.levels[-1]
        if cfg.ml_coarse_direct > 0 and 0 < last.n <= cfg.ml_coarse_direct:
            self.coarse_inverse = _inverse(last.aug, t)
        if cfg.ml_patch_degree > 0:
            S = np.flatnonzero(np.diff(sp.csr_matrix(Ct).indptr) > 0)
            if S.size:
                fine = self.levels[0]
                patch = _Level.__new__(_Level)
                patch.aug = fine.aug[S][:, S]
                patch.n, patch.d, patch.P, patch.S = S.size, fine.d[S], None, S
                patch.lam = power_lambda(patch.aug, patch.d, cfg.cheb_power_its, cfg.cheb_safety,
                                         start_vector(S.size, t), t)
                self.patch = patch

    # ---------------------------------------------------------------- application
    @property
    def n(self):
        return self.levels[0].n

    def _smooth(self, level, degree, ratio, r):
        return chebyshev(level.aug, level.d, level.lam, ratio, degree, r)

    def vcycle(self, l, r):
        c, L = self.cfg, self.levels[l]
        if l == len(self.levels) - 1:
            if self.coarse_inverse is not None:
                return self.coarse_inverse @ r
            return self._smooth(L, c.ml_coarse_degree, c.ml_coarse_ratio, r)
        degree = c.ml_smooth_degree_coarse if (l > 0 and c.ml_smooth_degree_coarse > 0) else c.ml_smooth_degree
        z = self._smooth(L, degree, c.ml_smooth_ratio, r)
        z = z + L.P @ self.vcycle(l + 1, _t(L.P) @ (r - L.aug @ z))
        return z + self._smooth(L, degree, c.ml_smooth_ratio, r - L.aug @ z)

    def _patch_correction(self, r):
        Q, c = self.patch, self.cfg
        e = np.zeros_like(r)
        e[Q.S] = chebyshev(Q.aug, Q.d, Q.lam, c.ml_patch_ratio, c.ml_patch_degree, r[Q.S])
        return e

    def apply(self, r):
        """M^-1 r for a vector r, or M^-1 R column by column for a matrix R."""
        r = np.asarray(r, self.dtype)
        c, fine = self.cfg, self.levels[0]
        if self.prec == PREC_IDENTITY:
            return r.copy()
        if self.prec == PREC_JACOBI:
            return r / (fine.d if r.ndim == 1 else fine.d[:, None])
        if self.prec == PREC_CHEBYSHEV:
            return self._smooth(fine, c.cheb_degree, c.cheb_eig_ratio, r)
        if self.patch is None:
            return self.vcycle(0, r)
        z1 = self._patch_correction(r)
        z2 = z1 + self.vcycle(0, r - fine.aug @ z1)
        return z2 + self._patch_correction(r - fine.aug @ z2)

    def dense(self):
        """The whole operator, column j = M^-1 e_j."""
        return np.asarray(self.apply(np.eye(self.n, dtype=self.dtype)))

    def estimates(self):
        """[(name, Aug, D, lambda incl. safety)] of every level and the patch: what check (e) bounds from below."""
        out = [(f"level {l}", L.aug, L.d, L.lam) for l, L in enumerate(self.levels) if L.lam is not None]
        if self.patch is not None:
            out.append(("patch", self.patch.aug, self.patch.d, self.patch.lam))
        return out


def true_lambda_max(aug, d, dense_limit=7000):
    """lambda_max(D^-1 Aug) of the symmetrically scaled operator: eigvalsh when small, Lanczos otherwise."""
    d = np.asarray(d, np.float64)
    s = 1.0 / np.sqrt(d)
    if aug.shape[0] <= dense_limit:
        m = np.asarray(_dense(aug), np.float64) * s[:, None] * s[None, :]
        return float(np.linalg.eigvalsh((m + m.T) / 2)[-1])
    import scipy.sparse.linalg as spla
    m = sp.diags(s) @ sp.csr_matrix(aug) @ sp.diags(s)
    return float(spla.eigsh(m, k=1, which="LA", tol=1e-10, return_eigenvectors=False)[0])
