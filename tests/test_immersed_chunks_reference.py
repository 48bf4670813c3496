"""The oracle at immersed blocks beyond one 4096-entry chunk, pinned to SciPy / NumPy.

tests/test_gpu_immersed_chunks.py compares the library with the oracle bit for bit at the keys of
tests/immersed_chunk_cases.py.  This module pins that reference itself, on the CPU, to a restatement that uses neither
the oracle nor the library: the CSR arrays of the generated problem go straight into scipy.sparse, the operators are
restated from the comments of include/alfd/alfd.h (enum alfd_variant, alfd_w_inverse) and of the system operator

    elliptic variants   s = C x0 - M x1,  t = W^-1 s,  y0 = A x0 + gamma Ct t + Ct x2,
                        y1 = A2 x1 - gamma2 M t - M x2,  y2 = s
    AL2                 s = C x0,  t = W^-1 s,  y0 = A x0 + gamma Ct t + Ct x1,  y1 = s

with W^-1 the uploaded diagonal, or (M^-1)^2 through scipy.sparse.linalg.splu(M).  Every product is evaluated in
float64 (scipy) and in np.longdouble (Mat.ld); the longdouble of the LU solves comes from three steps of iterative
refinement with longdouble residuals.

(a) system_apply, diagonal W^-1: row-wise, |y_r - ref_r| <= bound_r, derived as tests/spmv_reference.py derives its
    bound -- (len + 2) 2^-53 |A||x| per product row, one rounding per scale / add, the error of an intermediate
    propagated through the absolute values of the matrix that reads it, second-order terms in a 1 % slack:
      e_s = (len_C + len_M + 2) u (|C||x0| + |M||x1|)                     e_t = |w| e_s + u |w s|
      e_0 = (len_A + 2 len_Ct + 6) u (|A||x0| + gamma |Ct||t| + |Ct||x2|) + gamma |Ct| e_t
      e_1 = (len_A2 + 2 len_M + 6) u (|A2||x1| + gamma2 |M||t| + |M||x2|) + gamma2 |M| e_t           e_2 = e_s
(b) exact W^-1: the oracle's multiplier block -gamma W^-1 u against -gamma splu(M)(splu(M) u), relative 2-norm, within
      TOL_W = 64 dev_W + (kappa^2 + kappa) (reduce + u k (len_M + 3) kappa)
    dev_W: float64-vs-longdouble deviation of the splu restatement on these inputs (table below); reduce = 1e-14, the
    stop rule of alfd_config::mass, which bounds the recursive residual of each of the two CG solves; u k (len + 3) kappa
    the gap between recursive and true residual after k steps (Greenbaum, SIMAX 18 (1997)), k the a-priori CG step
    bound ln(2 sqrt(kappa_J) / reduce) / ln((sqrt(kappa_J) + 1) / (sqrt(kappa_J) - 1)), kappa_J = cond(D^-1/2 M D^-1/2);
    kappa = cond(M) turns residuals into errors, once per solve and once more for the first solve's error passing
    through the second.  system_apply of the exact_w keys: bound (a) with e_t = TOL_W |t|_2 in every entry.
(c) preconditioner vmult with the inner rule tightened to SolverControl(20000, 1e-12), as
    test_oracle.py::test_elliptic_modified_vmult_algebra does: every block of the oracle's result against the block
    algebra of augmented_lagrangian_preconditioner.h with sparse direct solves (splu) of Aug, A22 and the 2x2 Aug2,
    written as extended sparse systems in (x, z), W z = (coupling) x, so that neither Ct W C nor (M^-1)^2 is formed.
    Each stage takes its right-hand side from the oracle's own upstream blocks and is held to
      |Op (v - exact)|_2 <= tol + u k (len + 3) |Op|_2 |exact|_2 + 64 dev |rhs|_2
    tol = 1e-12 the absolute stop rule, the second term Greenbaum's residual gap with k the oracle's step count of that
    operator and |x_j|_2 <= |x|_2 (the iterates of CG from zero grow monotonically, Hestenes & Stiefel 1952, Thm 6:3),
    dev the float64-vs-longdouble deviation of the direct solve measured in the residual (table).  Diagonal-W keys only:
    with the exact W^-1 every Op p of the CG carries the error (b) of two nested mass solves, for which there is no
    bound of this kind that is tight enough to see anything; those keys are held to (b) and to system_apply.

Measured float64-vs-longdouble deviations of the restatement alone (test_tolerance_is_what_the_restatement_measures
repeats them and fails when one exceeds what the table records):

  key                       immersed n   recorded (measured)                       what
  ell_mod_4225              4225         stage dev 5e-11 (3.3e-11)                 a22 9.9e-13 .. 4.6e-12, aug 2.3e-11 .. 3.3e-11
  ell_ideal_4225            4225         stage dev 5e-10 (3.5e-10)                 aug2
  ell_mod_4096              4096         stage dev 3e-11 (1.9e-11)                 a22 8.2e-13 .. 9.9e-13, aug 1.7e-11 .. 1.9e-11
  ell_ideal_4096            4096         stage dev 3e-10 (2.0e-10)                 aug2
  ell_ideal_8281            8281         stage dev 1e-9  (6.4e-10)                 aug2
  ell_mod_4225_exact_w      4225         dev_W 1e-15 (6.4e-16) -> TOL_W 2.9e-10    cond(M) 15.99, cond(D^-1/2 M D^-1/2) 9.00
  ell_ideal_4225_exact_w    4225         dev_W 1e-15 (6.4e-16) -> TOL_W 2.9e-10    the same M
  al2_exact_w_4097          4097         dev_W 5e-16 (3.0e-16) -> TOL_W 7.8e-13    cond(M) 3.00 (P1 segments of a circle)
A stage dev is |Op solve_f64(rhs) - rhs|_2 / |rhs|_2 of the extended-system splu solve (its longdouble counterpart, three
refinement steps, is below 1e-18); inputs rng and the indicator of the second chunk (e_{n-1} for the 4096 keys).  The
float64 evaluation of the restated system operator itself sits at 0.18 (diagonal W), 0.30 and 0.43 (exact W, AL2) of
the row-wise bound (a) in its worst row.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import immersed_chunk_cases as icc
from fictitious_domain_al_preconditioners_amd import _abi

LD = np.longdouble
U = 2.0 ** -53
MARGIN = 64.0
SLACK = 1.01            # second-order terms of the first-order bounds
VMULT_INPUTS = ["rng", "second_chunk"]
DIAGONAL_W_KEYS = [k for k in icc.KEYS if k not in icc.EXACT_W_KEYS]

# key -> dev_W (b); key -> largest dev of a stage (c)
MEASURED_W = {"ell_mod_4225_exact_w": 1e-15, "ell_ideal_4225_exact_w": 1e-15, "al2_exact_w_4097": 5e-16}
MEASURED_STAGE = {"ell_mod_4225": 5e-11, "ell_ideal_4225": 5e-10, "ell_mod_4096": 3e-11, "ell_ideal_4096": 3e-10,
                  "ell_ideal_8281": 1e-9}


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def _sp(m):
    return sp.csr_matrix((m.val, m.col, m.row_ptr), shape=(m.nrows, m.ncols))


class Mat:
    """A scipy CSR matrix with products in np.longdouble and with |A| |x|."""

    def __init__(self, m):
        self.m = sp.csr_matrix(m)
        rp = self.m.indptr.astype(np.int64)
        self.len = np.diff(rp)
        self.ne = self.len > 0
        self.starts = rp[:-1][self.ne]
        self.col = self.m.indices
        self.val = self.m.data.astype(LD)

    def _rows(self, prod):
        out = np.zeros(self.m.shape[0], LD)
        if prod.size:               # non-empty rows are contiguous segments of the entry array
            out[self.ne] = np.add.reduceat(prod, self.starts)
        return out

    def ld(self, x):
        return self._rows(self.val * np.asarray(x, LD)[self.col])

    def abs(self, x):
        return self._rows(np.abs(self.val) * np.abs(np.asarray(x, LD))[self.col])

    def mv(self, x, dtype):
        return self.m @ np.asarray(x, np.float64) if dtype is np.float64 else self.ld(x)

    def norm2_bound(self):
        """|A|_2 <= sqrt(|A|_1 |A|_inf)."""
        a = abs(self.m)
        return float(np.sqrt(a.sum(axis=0).max() * a.sum(axis=1).max()))


def norm2(v):
    v = np.asarray(v, LD)
    return float(np.sqrt(np.sum(v * v)))


class Restated:
    """The operators of a key from its CSR arrays and its config values alone."""

    def __init__(self, key):
        s = icc.system(key)
        pb, cfg = s.pb, s.cfg
        self.key, self.sizes = key, pb.block_sizes
        self.elliptic = "A2" in pb.mats
        self.ideal = cfg.variant == _abi.AL_ELL_IDEAL
        names = ("A", "Ct", "C", "M") + (("A2",) if self.elliptic else ())
        self.m = {k: Mat(_sp(pb.mats[k])) for k in names}
        self.gamma, self.gamma2 = float(cfg.gamma), float(cfg.gamma2)
        self.exact = cfg.w_inverse == _abi.W_MASS_INV_SQUARED
        # ALFD_INVW is an input of the system (the caller's vector): 1/(M^2)_ii (elliptic) or 1/M_ii^2
        M = self.m["M"].m
        self.w = pb.inv_w_diag_of_mass_squared() if self.elliptic else pb.inv_w_diag_squared()
        want = 1.0 / (M @ M).diagonal() if self.elliptic else 1.0 / M.diagonal() ** 2
        assert np.allclose(self.w, want, rtol=1e-14, atol=0)
        self.lu = spla.splu(M.tocsc()) if self.exact else None
        self._stages = {}

    # ---- W^-1
    def mass_inv(self, b, dtype):
        x = self.lu.solve(np.asarray(b, np.float64))
        if dtype is np.float64:
            return x
        x, b = x.astype(LD), np.asarray(b, LD)
        for _ in range(3):
            x = x + self.lu.solve((b - self.m["M"].ld(x)).astype(np.float64))
        return x

    def winv(self, t, dtype):
        if not self.exact:
            return np.asarray(self.w, dtype) * np.asarray(t, dtype)
        return self.mass_inv(self.mass_inv(t, dtype), dtype)

    @functools.cached_property
    def mass_spectrum(self):
        """(cond(M), cond(D^-1/2 M D^-1/2), |M^-1|_2)."""
        M = self.m["M"].m
        d = 1.0 / np.sqrt(M.diagonal())
        J = (sp.diags(d) @ M @ sp.diags(d)).tocsc()

        def extremes(a):
            top = float(abs(a).sum(axis=1).max())        # Gershgorin: the eigenvalue next to it is the largest
            hi = float(spla.eigsh(a, k=1, sigma=top, which="LM", return_eigenvectors=False, tol=1e-8)[0])
            lo = float(spla.eigsh(a, k=1, sigma=0.0, which="LM", return_eigenvectors=False, tol=1e-8)[0])
            return lo, hi
        lo, hi = extremes(M.tocsc())
        jlo, jhi = extremes(J)
        return hi / lo, jhi / jlo, 1.0 / lo

    def tol_w(self, dev):
        """TOL_W of (b)."""
        kappa, kappa_j, _ = self.mass_spectrum
        reduce = icc.system(self.key).cfg.mass.reduce
        q = (math.sqrt(kappa_j) + 1) / (math.sqrt(kappa_j) - 1)
        k = math.ceil(math.log(2 * math.sqrt(kappa_j) / reduce) / math.log(q))
        gap = U * k * (int(self.m["M"].len.max()) + 3) * kappa
        return MARGIN * dev + (kappa * kappa + kappa) * (reduce + gap)

    # ---- the system operator
    def system(self, x, dtype):
        m, g, g2 = self.m, dtype(self.gamma), dtype(self.gamma2)
        if self.elliptic:
            s = m["C"].mv(x[0], dtype) - m["M"].mv(x[1], dtype)
            t = self.winv(s, dtype)
            y0 = m["A"].mv(x[0], dtype) + g * m["Ct"].mv(t, dtype) + m["Ct"].mv(x[2], dtype)
            y1 = m["A2"].mv(x[1], dtype) - g2 * m["M"].mv(t, dtype) - m["M"].mv(x[2], dtype)
            return [y0, y1, s]
        s = m["C"].mv(x[0], dtype)
        t = self.winv(s, dtype)
        return [m["A"].mv(x[0], dtype) + g * m["Ct"].mv(t, dtype) + m["Ct"].mv(x[1], dtype), s]

    def system_bound(self, x, tol_w=None):
        """The row-wise bounds (a); tol_w: the exact W^-1 with e_t = tol_w |t|_2 per entry."""
        m, g, g2, u = self.m, LD(self.gamma), LD(self.gamma2), LD(U)
        last = x[-1]
        if self.elliptic:
            s = m["C"].ld(x[0]) - m["M"].ld(x[1])
            e_s = (m["C"].len + m["M"].len + 2) * u * (m["C"].abs(x[0]) + m["M"].abs(x[1]))
        else:
            s = m["C"].ld(x[0])
            e_s = (m["C"].len + 2) * u * m["C"].abs(x[0])
        t = self.winv(s, LD)
        if tol_w is None:
            e_t = np.abs(self.w) * e_s + u * np.abs(t)
        else:
            e_t = np.full(t.size, LD(tol_w) * LD(norm2(t)))
        e_0 = (m["A"].len + 2 * m["Ct"].len + 6) * u * (m["A"].abs(x[0]) + g * m["Ct"].abs(t) + m["Ct"].abs(last)) \
            + g * m["Ct"].abs(e_t)
        if not self.elliptic:
            return [SLACK * e_0, SLACK * e_s]
        e_1 = (m["A2"].len + 2 * m["M"].len + 6) * u * (m["A2"].abs(x[1]) + g2 * m["M"].abs(t) + m["M"].abs(last)) \
            + g2 * m["M"].abs(e_t)
        return [SLACK * e_0, SLACK * e_1, SLACK * e_s]

    # ---- the inner operators of (c), diagonal W^-1: extended sparse systems in (x, z), diag(1/w) z = (coupling) x
    def stage(self, op):
        """SimpleNamespace(n, apply_ld, solve(b, dtype), norm_bound, maxlen) of "aug", "a22" or "aug2"."""
        assert not self.exact
        if op in self._stages:
            return self._stages[op]
        m, g, g2 = self.m, self.gamma, self.gamma2
        A, Ct, C, Mm = m["A"].m, m["Ct"].m, m["C"].m, m["M"].m
        Wi = sp.diags(1.0 / self.w)
        wmax = float(np.abs(self.w).max())
        n0, n1 = self.sizes[0], self.sizes[1]
        if op == "aug":
            n = n0
            K = sp.bmat([[A, g * Ct], [-C, Wi]], format="csc")
            norm = m["A"].norm2_bound() + g * m["Ct"].norm2_bound() * wmax * m["C"].norm2_bound()
            maxlen = int((m["A"].len + m["Ct"].len).max()) + int(m["C"].len.max())

            def apply_ld(x):
                return m["A"].ld(x) + LD(g) * m["Ct"].ld(self.winv(m["C"].ld(x), LD))
        elif op == "a22":
            n = n1
            A2 = m["A2"].m
            K = sp.bmat([[A2, g2 * Mm], [-Mm, Wi]], format="csc")
            norm = m["A2"].norm2_bound() + g2 * m["M"].norm2_bound() ** 2 * wmax
            maxlen = int((m["A2"].len + m["M"].len).max()) + int(m["M"].len.max())

            def apply_ld(x):
                return m["A2"].ld(x) + LD(g2) * m["M"].ld(self.winv(m["M"].ld(x), LD))
        else:
            n = n0 + n1
            A2 = m["A2"].m
            K = sp.bmat([[A, None, g * Ct], [None, A2, -g2 * Mm], [-C, Mm, Wi]], format="csc")
            norm = m["A"].norm2_bound() + m["A2"].norm2_bound() \
                + max(g, g2) * wmax * (m["C"].norm2_bound() + m["M"].norm2_bound()) ** 2
            maxlen = int(max((m["A"].len + m["Ct"].len).max(), (m["A2"].len + m["M"].len).max())) \
                + int((m["C"].len + m["M"].len).max())

            def apply_ld(x):
                t = self.winv(m["C"].ld(x[:n0]) - m["M"].ld(x[n0:]), LD)
                return np.concatenate([m["A"].ld(x[:n0]) + LD(g) * m["Ct"].ld(t),
                                       m["A2"].ld(x[n0:]) - LD(g2) * m["M"].ld(t)])
        lu = spla.splu(K)
        nz = K.shape[0] - n

        def solve(b, dtype):
            x = lu.solve(np.concatenate([np.asarray(b, np.float64), np.zeros(nz)]))[:n]
            if dtype is np.float64:
                return x
            x, b = x.astype(LD), np.asarray(b, LD)
            for _ in range(3):
                r = (b - apply_ld(x)).astype(np.float64)
                x = x + lu.solve(np.concatenate([r, np.zeros(nz)]))[:n]
            return x
        self._stages[op] = SimpleNamespace(n=n, apply_ld=apply_ld, solve=solve, norm_bound=norm, maxlen=maxlen)
        return self._stages[op]


@functools.lru_cache(maxsize=None)
def restated(key):
    return Restated(key)


def _rel(a, b):
    return norm2(np.asarray(a, LD) - np.asarray(b, LD)) / norm2(b)


# ------------------------------------------------------------------------------------------------- measurements
def measure_system(key):
    """Largest |y_f64 - y_longdouble|_r / bound_r of the restated system operator over the inputs and rows: where
    scipy's own summation order sits inside the row-wise bound (a)."""
    r, worst = restated(key), 0.0
    tol_w = r.tol_w(MEASURED_W[key]) if r.exact else None
    for x in icc.system(key).inputs.values():
        for a, b, e in zip(r.system(x, np.float64), r.system(x, LD), r.system_bound(x, tol_w)):
            d = np.abs(np.asarray(a, LD) - b)
            assert np.all(d[e == 0] == 0)
            worst = max(worst, float(np.max(d[e > 0] / e[e > 0], initial=0.0)))
    return worst


def measure_winv(key):
    """dev_W: largest |W^-1_f64 u - W^-1_longdouble u|_2 / |W^-1_longdouble u|_2 over the inputs' multiplier blocks."""
    r = restated(key)
    return max(_rel(r.winv(x[-1], np.float64), r.winv(x[-1], LD)) for x in icc.system(key).inputs.values())


@functools.lru_cache(maxsize=None)
def tight_vmult(key, name):
    """The oracle's vmult of an input with the inner rule SolverControl(20000, 1e-12): (v, result, counts)."""
    s = icc.system(key)
    cfg = icc.copy_config(s.cfg, inner=_abi.Control(_abi.CTRL_ABS, 20000, 1e-12, 0.0))
    h = s.osys.open(cfg)
    try:
        rc, v, res = s.osys.handle_precond_apply(h, s.inputs[name])
        counts = s.osys.handle_inner_iterations(h)
    finally:
        s.osys.close_handle(h)
    assert rc == 0 and res.inner_failures == 0
    return v, res, counts, cfg


def stages_of(key, name):
    """[(op, block slice of v as one vector, right-hand side in longdouble from the oracle's upstream blocks)]."""
    r = restated(key)
    u = icc.system(key).inputs[name]
    v = tight_vmult(key, name)[0]
    m, g = r.m, LD(r.gamma)
    if not r.elliptic:
        return [("aug", v[0], np.asarray(u[0], LD) - m["Ct"].ld(v[1]))]
    if r.ideal:
        rhs = np.concatenate([np.asarray(u[0], LD) - m["Ct"].ld(v[2]), np.asarray(u[1], LD) + m["M"].ld(v[2])])
        return [("aug2", np.concatenate([v[0], v[1]]), rhs)]
    rhs1 = np.asarray(u[1], LD) + m["M"].ld(v[2])
    rhs0 = np.asarray(u[0], LD) + g * m["Ct"].ld(r.winv(m["M"].ld(v[1]), LD)) - m["Ct"].ld(v[2])
    return [("a22", v[1], rhs1), ("aug", v[0], rhs0)]


def measure_vmult(key, name):
    """Per stage: (op, |Op (v - exact)|_2, its bound, dev, steps)."""
    r = restated(key)
    _, _, counts, cfg = tight_vmult(key, name)
    out = []
    for op, v, rhs in stages_of(key, name):
        st = r.stage(op)
        exact = st.solve(rhs, LD)
        dev = norm2(st.apply_ld(st.solve(rhs, np.float64)) - rhs) / norm2(rhs)
        err = norm2(st.apply_ld(np.asarray(v, LD) - exact))
        k = counts[op]
        bound = cfg.inner.tol + U * k * (st.maxlen + 3) * st.norm_bound * norm2(exact) + MARGIN * dev * norm2(rhs)
        out.append((op, err, bound, dev, k, _rel(v, exact)))
    return out


# ------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("key", icc.KEYS)
def test_system_apply_is_the_restated_operator(key):
    """(a): every input, every row of every block; the exact_w keys with e_t from TOL_W."""
    r, s = restated(key), icc.system(key)
    tol_w = r.tol_w(MEASURED_W[key]) if r.exact else None
    for name, x in s.inputs.items():
        got = icc.oracle_system_apply(key, name)
        ref, bound = r.system(x, LD), r.system_bound(x, tol_w)
        for b, (g, y, e) in enumerate(zip(got, ref, bound)):
            err = np.abs(np.asarray(g, LD) - y)
            worst = float(np.max(err[e > 0] / e[e > 0], initial=0.0))
            print(f"{key} {name} block {b}: largest error / bound {worst:.2e}")
            assert np.all(err <= e), (key, name, b, int(np.argmax(err - e)))


@pytest.mark.parametrize("key", ["ell_mod_4225", "ell_ideal_8281", "ell_mod_4225_exact_w", icc.AL2_KEY])
def test_the_bound_sees_every_term(key):
    """Leaving any one term out of a block of the restated operator moves some row by more than 100 times its bound,
    in the second chunk of the immersed blocks too: a wrong sign, factor or offset of a term cannot hide under (a)."""
    r, s = restated(key), icc.system(key)
    x = s.inputs["rng"]
    m, g, g2 = r.m, LD(r.gamma), LD(r.gamma2)
    bound = r.system_bound(x, r.tol_w(MEASURED_W[key]) if r.exact else None)
    if r.elliptic:
        sv = m["C"].ld(x[0]) - m["M"].ld(x[1])
        t = r.winv(sv, LD)
        terms = {0: [m["A"].ld(x[0]), g * m["Ct"].ld(t), m["Ct"].ld(x[2])],
                 1: [m["A2"].ld(x[1]), g2 * m["M"].ld(t), m["M"].ld(x[2])],
                 2: [m["C"].ld(x[0]), m["M"].ld(x[1])]}
    else:
        t = r.winv(m["C"].ld(x[0]), LD)
        terms = {0: [m["A"].ld(x[0]), g * m["Ct"].ld(t), m["Ct"].ld(x[1])], 1: [m["C"].ld(x[0])]}
    for b, ts in terms.items():
        e = bound[b]
        for i, term in enumerate(ts):
            rows = (e > 0) & (np.arange(e.size) >= (icc.CHUNK if b > 0 else 0))
            ratio = float(np.max(np.abs(term[rows]) / e[rows]))
            print(f"{key} block {b} term {i}: largest |term| / bound beyond the first chunk {ratio:.2e}")
            assert ratio > 100, (key, b, i)


@pytest.mark.parametrize("key", icc.EXACT_W_KEYS)
def test_exact_w_inverse_is_two_sparse_direct_solves(key):
    """(b): the multiplier block of the oracle's vmult, -gamma W^-1 u, for every input."""
    r, s = restated(key), icc.system(key)
    tol = r.tol_w(MEASURED_W[key])
    kappa, kappa_j, _ = r.mass_spectrum
    print(f"{key}: cond(M) {kappa:.2f}, cond(D^-1/2 M D^-1/2) {kappa_j:.2f}, TOL_W {tol:.2e}")
    assert tol <= 1e-9
    # the multiplier block does not depend on the inner rule: one CG step per inner solve keeps the oracle cheap
    h = s.osys.open(icc.copy_config(s.cfg, inner=_abi.Control(_abi.CTRL_FIXED_ITERS, 1, 0.0, 0.0)))
    for name, x in s.inputs.items():
        rc, v, res = s.osys.handle_precond_apply(h, x)
        assert rc == 0 and res.mass_iterations > 0
        ref = -LD(r.gamma) * r.winv(x[-1], LD)
        err = _rel(v[-1], ref)
        print(f"{key} {name}: oracle vs splu {err:.2e}")
        assert err <= tol, (key, name, err)
    s.osys.close_handle(h)


@pytest.mark.parametrize("name", VMULT_INPUTS)
@pytest.mark.parametrize("key", DIAGONAL_W_KEYS)
def test_vmult_is_the_block_algebra_with_direct_solves(key, name):
    """(c), and the multiplier block -gamma w u to two roundings."""
    s = icc.system(key)
    if name not in s.inputs:
        name = "e_last"          # the 4096 keys have no second chunk
    r = restated(key)
    v, res, counts, _ = tight_vmult(key, name)
    ref = -LD(r.gamma) * np.asarray(r.w, LD) * np.asarray(s.inputs[name][-1], LD)
    assert np.all(np.abs(np.asarray(v[-1], LD) - ref) <= 2 * U * np.abs(ref))
    for op, err, bound, dev, k, rel in measure_vmult(key, name):
        print(f"{key} {name} {op}: |Op (v - exact)| {err:.2e} (bound {bound:.2e}), {k} steps, "
              f"|v - exact| / |exact| {rel:.2e}, dev {dev:.1e}")
        assert k > 0 and dev <= MEASURED_STAGE[key]
        assert err <= bound, (key, name, op, err, bound)


def test_tolerance_is_what_the_restatement_measures():
    """The float64-vs-longdouble deviations of the restatement alone: the table of the module docstring."""
    assert np.finfo(LD).eps < 1e-18, "np.longdouble is no wider than float64 on this machine"
    assert sorted(MEASURED_W) == sorted(icc.EXACT_W_KEYS) and sorted(MEASURED_STAGE) == sorted(DIAGONAL_W_KEYS)
    for key in icc.KEYS:
        line = f"{key}: f64 restatement / bound (a) {measure_system(key):.2f}"
        if key in MEASURED_W:
            dev = measure_winv(key)
            line += f", dev_W {dev:.2e} -> TOL_W {restated(key).tol_w(MEASURED_W[key]):.2e}"
            assert dev <= MEASURED_W[key], (key, dev)
        else:
            names = [n if n in icc.system(key).inputs else "e_last" for n in VMULT_INPUTS]
            dev = max(st[3] for n in names for st in measure_vmult(key, n))
            line += f", largest stage dev {dev:.2e}"
            assert dev <= MEASURED_STAGE[key], (key, dev)
        print(line)
        assert measure_system(key) <= 1.0
