// alfd_oracle.cpp -- CPU ORACLE (test infrastructure, NOT product code).
//
// PARITY STATUS: "parity unpinned" with respect to a real deal.II+Trilinos run.
// The reference cannot be built here (deal.II, Trilinos ML, UMFPACK absent --
// SURVEY.md 8(c)) and ships no golden vectors for the AL path, so this file is
// a restatement of the reference's algorithm pinned only by (i) independent
// SciPy cross-checks in tests/ and (ii) the rational-approximation constants of
// rational_preconditioner.h:70-93.  Only tests/, __graft_entry__.smoke() and
// bench.py's cpu_baseline leg may load this library.
//
// What it restates (reference file:line):
//   * preconditioner algebra, verbatim order of operations:
//       augmented_lagrangian_preconditioner.h:28-34 (AL2), :62-70 (Stokes),
//       :95-103 (diagonal SPD), :225-228 (elliptic modified)
//   * operator composition / tolerances:
//       immersed_laplace.cc:880-916, stokes_immersed_boundary.cc:931-1054
//   * [EXT] deal.II algorithms written from their published descriptions:
//       SolverCG (zero initial guess through inverse_operator), SolverFGMRES
//       (9.6-style: check + ++k after every Arnoldi step, Givens), SolverControl /
//       ReductionControl / IterationNumberControl stop rules.
//   * the inner preconditioner named by north_star (Jacobi / Chebyshev sweep on
//       D^-1 Aug) in place of Trilinos ML (stokes...:1027-1045).
//
// Canonical arithmetic ("ALFD-arith v1"): every reduction
// has a fixed tree so that the HIP kernels can reproduce it bit for bit.
//   SpMV row (L lanes, V per lane): lane l accumulates entries
//       k0 + (m*L + l)*V + v  (m = 0,1,..; v = 0..V-1) with fma, then a binary
//       tree lane[l] += lane[l+s], s = L/2..1.
//   dot: 4096-element chunks; thread t of 256 accumulates elements
//       base + e*512 + 2t, +1 (e = 0..7) with fma; 64-lane tree; 4 wave sums
//       combined as (w0+w1)+(w2+w3); chunk partials reduced by one more such
//       block (thread-strided sequential adds).
//   multi-rank: local dots summed in rank order.
// Compile with -ffp-contract=off; fma only where written.

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "alfd/alfd.h"
#ifdef _OPENMP
#include <omp.h>
#endif

namespace orc {

constexpr int64_t CHUNK = 4096;  // dot chunk = block-vector padding granule

struct Csr {
  int64_t nrows = 0, ncols = 0;
  const int64_t *rp = nullptr;
  const int32_t *col = nullptr;
  const double *val = nullptr;
  int L = 64, V = 1;
  std::vector<int64_t> own_rp;  // storage when built internally (transpose)
  std::vector<int32_t> own_col;
  std::vector<double> own_val;
  bool present() const { return rp != nullptr; }
  int64_t nnz() const { return rp ? rp[nrows] : 0; }
};

// Lanes-per-row rule shared (by specification) with the HIP library:
// mean nnz over NON-EMPTY rows.
inline void choose_lanes(Csr &m) {
  int64_t nonempty = 0;
  for (int64_t r = 0; r < m.nrows; ++r) nonempty += (m.rp[r + 1] > m.rp[r]);
  const double avg = nonempty ? (double)m.nnz() / (double)nonempty : 0.0;
  m.V = 1;
  if (avg > 48)
    m.L = 64;
  else if (avg > 24)
    m.L = 32;
  else if (avg > 12)
    m.L = 16;
  else if (avg > 6)
    m.L = 8;
  else
    m.L = 4;
}

// 0 = canonical lane order (parity); 1 = plain sequential row sums, the order
// dealii::SparseMatrix::vmult uses -- ONLY for timing the cpu_baseline.
static int g_row_order = 0;

inline double row_sum(const Csr &m, int64_t r, const double *x) {
  double lane[64];
  const int64_t k0 = m.rp[r], k1 = m.rp[r + 1];
  if (g_row_order == 1) {
    double s = 0.0;
    for (int64_t k = k0; k < k1; ++k) s += m.val[k] * x[m.col[k]];
    return s;
  }
  const int L = m.L, V = m.V;
  for (int l = 0; l < L; ++l) {
    double acc = 0.0;
    for (int64_t k = k0 + (int64_t)l * V; k < k1; k += (int64_t)L * V)
      for (int v = 0; v < V && k + v < k1; ++v) acc = std::fma(m.val[k + v], x[m.col[k + v]], acc);
    lane[l] = acc;
  }
  for (int s = L / 2; s >= 1; s >>= 1)
    for (int l = 0; l < s; ++l) lane[l] = lane[l] + lane[l + s];
  return lane[0];
}

// mode 0: y = A x ; mode 1: y = fma(alpha, A x, y)
void spmv(const Csr &m, const double *x, double *y, int mode, double alpha) {
  // threads only where they pay (results do not depend on the thread count)
#pragma omp parallel for schedule(static) if (m.nrows > 0 && m.rp[m.nrows] > 32768)
  for (int64_t r = 0; r < m.nrows; ++r) {
    if (mode == 1 && m.rp[r + 1] == m.rp[r]) continue;  // empty row: y unchanged
    const double s = row_sum(m, r, x);
    y[r] = mode == 0 ? s : std::fma(alpha, s, y[r]);
  }
}

inline double tree256(double *lane) {  // 4 waves of 64, then (w0+w1)+(w2+w3)
  double w[4];
  for (int wv = 0; wv < 4; ++wv) {
    double *a = lane + 64 * wv;
    for (int s = 32; s >= 1; s >>= 1)
      for (int l = 0; l < s; ++l) a[l] = a[l] + a[l + s];
    w[wv] = a[0];
  }
  return (w[0] + w[1]) + (w[2] + w[3]);
}

double dot(int64_t n, const double *x, const double *y) {
  if (n <= 0) return 0.0;
  const int64_t nb = (n + CHUNK - 1) / CHUNK;
  std::vector<double> part(nb);
#pragma omp parallel for schedule(static) if (nb > 8)
  for (int64_t b = 0; b < nb; ++b) {
    double lane[256];
    const int64_t base = b * CHUNK;
    for (int t = 0; t < 256; ++t) {
      double acc = 0.0;
      for (int e = 0; e < 8; ++e) {
        const int64_t i = base + e * 512 + 2 * t;
        if (i < n) acc = std::fma(x[i], y[i], acc);
        if (i + 1 < n) acc = std::fma(x[i + 1], y[i + 1], acc);
      }
      lane[t] = acc;
    }
    part[b] = tree256(lane);
  }
  double lane[256];
  for (int t = 0; t < 256; ++t) {
    double acc = 0.0;
    for (int64_t i = t; i < nb; i += 256) acc = acc + part[i];
    lane[t] = acc;
  }
  return tree256(lane);
}

// ---- elementwise (padding entries are zero and stay zero)
inline void axpy(int64_t n, double a, const double *x, double *y) {
#pragma omp parallel for schedule(static) if (n > 32768)
  for (int64_t i = 0; i < n; ++i) y[i] = std::fma(a, x[i], y[i]);
}
inline void xpby(int64_t n, const double *x, double b, double *y) {  // y = x + b y
#pragma omp parallel for schedule(static) if (n > 32768)
  for (int64_t i = 0; i < n; ++i) y[i] = std::fma(b, y[i], x[i]);
}
inline void scale(int64_t n, double a, double *x) {
#pragma omp parallel for schedule(static) if (n > 32768)
  for (int64_t i = 0; i < n; ++i) x[i] = a * x[i];
}
inline void pmul(int64_t n, const double *d, const double *x, double *y) {  // y = d .* x
#pragma omp parallel for schedule(static) if (n > 32768)
  for (int64_t i = 0; i < n; ++i) y[i] = d[i] * x[i];
}
inline void pmul_scale(int64_t n, double a, const double *d, const double *x, double *y) {
#pragma omp parallel for schedule(static) if (n > 32768)
  for (int64_t i = 0; i < n; ++i) y[i] = a * (d[i] * x[i]);  // y = a (d .* x)
}
inline void sub_from(int64_t n, const double *b, double *v) {  // v = b - v
#pragma omp parallel for schedule(static) if (n > 32768)
  for (int64_t i = 0; i < n; ++i) v[i] = b[i] - v[i];
}

// ------------------------------------------------------------ stop rules
enum State { ITERATE = 0, SUCCESS = 1, FAILURE = 2 };
struct Control {
  alfd_control c;
  double initial = 0, reduced_tol = 0, last_value = 0;
  int last_step = 0;
  State check(int step, double v) {
    last_step = step;
    last_value = v;
    if (step == 0) {
      initial = v;
      reduced_tol = v * c.reduce;
    }
    if (c.kind == ALFD_CTRL_REDUCTION && v < reduced_tol) return SUCCESS;
    if (c.kind == ALFD_CTRL_FIXED_ITERS && step >= c.max_steps) return SUCCESS;
    if (v <= c.tol) return SUCCESS;
    if (step >= c.max_steps || std::isnan(v)) return FAILURE;
    return ITERATE;
  }
};

// Emulated multi-rank row partition: every reduction is a sum, in rank order,
// of the ranks' local canonical reductions (what the library does with an
// all-gather + ordered sum).
struct Partition {
  int nranks = 1;
  std::vector<std::vector<int64_t>> offs;  // [block][nranks+1]
};

// --------------------------------------------------------------- problem
struct Problem {
  Partition pt;
  Csr mat[ALFD_NSLOTS];
  const double *diag[ALFD_NDIAGS] = {nullptr, nullptr};
  int nblocks = 0;
  int64_t n[ALFD_MAX_BLOCKS] = {0, 0, 0};
  int64_t off[ALFD_MAX_BLOCKS + 1] = {0, 0, 0, 0};  // padded offsets
  alfd_config cfg;
  // setup products
  std::vector<double> dinv_aug, dinv_a22, dinv_aug2, dinv_k;  // 1/diag of the inner operators
  std::vector<double> dinv_m;                                 // 1/diag(M): Jacobi of the exact-W^-1 mass solves
  double lam_max[6] = {0, 0, 0, 0, 0, 0};             // per inner operator kind
  std::vector<Csr> shifted;                           // A_Gamma - rho p_i M (rational_preconditioner.h:42-45)
  // aggregation multigrid (ALFD_PREC_MULTILEVEL): inputs + hierarchy
  int ml_nlev = 0;
  const int32_t *ml_agg[ALFD_MAX_LEVELS] = {};
  const double *ml_wgt[ALFD_MAX_LEVELS] = {};
  int64_t ml_nc[ALFD_MAX_LEVELS] = {};
  const int64_t *ml_off[ALFD_MAX_LEVELS] = {};        // emulated ranks: offsets of level l+1's unknowns
  Csr ml_P[ALFD_MAX_LEVELS];                          // CSR prolongator of a level (replaces its aggregates)
  struct Level {
    Csr A, C, Ct, Pm, R;
    int64_t n = 0;
    std::vector<double> dinv;
    double lmax = 0;
  };
  std::vector<Level> ml;
  Csr ml_inv;                                         // explicit inverse of the coarsest operator (ml_coarse_direct)
  // interface patch (alfd_config::ml_patch_degree > 0): S = non-empty rows of Ct
  struct Patch {
    bool on = false;
    std::vector<int32_t> S, T;                        // patch rows; rows of A with a column in S
    Csr Ass, As, Ats, Cs, Cts;                        // A[S,S], A[S,:], A[T,S] (compact rows), C[:,S], Ct[S,:]
    std::vector<double> dinv;
    double lmax = 0;
  } patch;
  std::vector<std::vector<double>> shifted_dinv;
  int64_t rational_its = 0, mass_its = 0;
  int winv_status = 0;  // first failure of a nested mass solve (ALFD_OK otherwise)
  double lambda_max = 0;
  // stats
  int64_t inner_its = 0, mp_its = 0;
  int64_t inner_its_op[3] = {0, 0, 0};                // inner_its by alfd_inner_op (orc_h_inner_iterations)
  int inner_failures = 0, precond_applications = 0;
  int status = ALFD_OK;
  int64_t ntot() const { return off[nblocks]; }
};

// dot of two vectors of block `blk` under the emulated partition
static double bdot(const Problem &P, int blk, const double *x, const double *y) {
  if (P.pt.nranks <= 1) return dot(P.n[blk], x, y);
  double total = 0.0;
  for (int r = 0; r < P.pt.nranks; ++r) {
    const int64_t g0 = P.pt.offs[blk][r], nl = P.pt.offs[blk][r + 1] - g0;
    const double d = dot(nl, x + g0, y + g0);
    total = r == 0 ? d : total + d;
  }
  return total;
}

static void transpose_into(const Csr &a, Csr &t) {
  t.nrows = a.ncols;
  t.ncols = a.nrows;
  t.own_rp.assign(t.nrows + 1, 0);
  const int64_t nnz = a.nnz();
  t.own_col.resize(nnz);
  t.own_val.resize(nnz);
  for (int64_t k = 0; k < nnz; ++k) t.own_rp[a.col[k] + 1]++;
  for (int64_t r = 0; r < t.nrows; ++r) t.own_rp[r + 1] += t.own_rp[r];
  std::vector<int64_t> cur(t.own_rp.begin(), t.own_rp.end() - 1);
  for (int64_t r = 0; r < a.nrows; ++r)
    for (int64_t k = a.rp[r]; k < a.rp[r + 1]; ++k) {
      const int64_t p = cur[a.col[k]]++;
      t.own_col[p] = (int32_t)r;
      t.own_val[p] = a.val[k];
    }
  t.rp = t.own_rp.data();
  t.col = t.own_col.data();
  t.val = t.own_val.data();
}

// ---- inner operators -------------------------------------------------------
// kind 0: Aug  x = A x + gamma Ct (w .* (C x))        (stokes...:991-993, immersed_laplace.cc:883,
//                                                       A11_aug elliptic...:807)
// kind 1: Mp
// kind 2: A22  x = A2 x + gamma2 M (w .* (M x))        (A22_aug, elliptic_interface.cc:810)
// kind 3: the 2x2 block [[A11_aug, A12_aug],[A21_aug, A22_aug]] on [x0 | pad | x1]
//         (elliptic_interface.cc:927-929), with s = C x0 - M x1, t = w .* s:
//           y0 = A x0 + gamma Ct t ,  y1 = A2 x1 - gamma2 M t
// kind 4: K x = A x (no augmentation; K_inv of the rational branch, immersed_laplace.cc:617-620)
// kind 5: an explicit matrix on block 1 (the shifted immersed systems / the immersed mass)
enum { OP_AUG = 0, OP_MP = 1, OP_A22 = 2, OP_AUG2 = 3, OP_K = 4, OP_MAT = 5 };

// dst = alpha * W^-1 src on the multiplier block (defined after pcg)
static int winv_scale(Problem &P, double alpha, const double *src, double *dst);

struct InnerOp {
  Problem &P;
  int kind;
  std::vector<double> t;
  const Csr *mat = nullptr;
  int mat_blk = 1;      // OP_MAT: the block the matrix acts on
  bool exact_w = false; // apply the configured W^-1 (alfd_config::w_inverse); false: diagonal weight
  int64_t n() const {
    if (kind == OP_MAT) return P.n[mat_blk];
    return (kind == OP_AUG || kind == OP_K) ? P.n[0] : kind == OP_AUG2 ? P.off[2] : P.n[1];
  }
  int blk() const {
    if (kind == OP_MAT) return mat_blk;
    return (kind == OP_AUG || kind == OP_K) ? 0 : kind == OP_AUG2 ? -1 : 1;
  }
  void operator()(const double *x, double *y) {
    const double *w = P.diag[ALFD_INVW];
    if (kind == OP_K) {
      spmv(P.mat[ALFD_A], x, y, 0, 0.0);
    } else if (kind == OP_MAT) {
      spmv(*mat, x, y, 0, 0.0);
    } else if (kind == OP_AUG && P.cfg.aug_assembled) {
      spmv(P.mat[ALFD_A], x, y, 0, 0.0);  // operator form: A already holds the AL term
    } else if (kind == OP_AUG) {
      const Csr &C = P.mat[ALFD_C];
      spmv(P.mat[ALFD_A], x, y, 0, 0.0);
      t.resize(C.nrows);
      spmv(C, x, t.data(), 0, 0.0);
      if (exact_w && P.cfg.w_inverse != ALFD_W_DIAGONAL) winv_scale(P, 1.0, t.data(), t.data());
      else pmul(C.nrows, w, t.data(), t.data());
      spmv(P.mat[ALFD_CT], t.data(), y, 1, P.cfg.gamma);
    } else if (kind == OP_MP) {
      spmv(P.mat[ALFD_MP], x, y, 0, 0.0);
    } else if (kind == OP_A22) {
      const Csr &M = P.mat[ALFD_M];
      spmv(P.mat[ALFD_A2], x, y, 0, 0.0);
      t.resize(M.nrows);
      spmv(M, x, t.data(), 0, 0.0);
      if (exact_w && P.cfg.w_inverse != ALFD_W_DIAGONAL) winv_scale(P, 1.0, t.data(), t.data());
      else pmul(M.nrows, w, t.data(), t.data());
      spmv(M, t.data(), y, 1, P.cfg.gamma2);
    } else {
      const Csr &C = P.mat[ALFD_C], &M = P.mat[ALFD_M];
      const double *x0 = x, *x1 = x + P.off[1];
      double *y0 = y, *y1 = y + P.off[1];
      t.resize(C.nrows);
      spmv(C, x0, t.data(), 0, 0.0);
      spmv(M, x1, t.data(), 1, -1.0);                    // s = C x0 - M x1
      if (exact_w && P.cfg.w_inverse != ALFD_W_DIAGONAL) winv_scale(P, 1.0, t.data(), t.data());
      else pmul(C.nrows, w, t.data(), t.data());
      spmv(P.mat[ALFD_A], x0, y0, 0, 0.0);
      spmv(P.mat[ALFD_CT], t.data(), y0, 1, P.cfg.gamma);
      spmv(P.mat[ALFD_A2], x1, y1, 0, 0.0);
      spmv(M, t.data(), y1, 1, -P.cfg.gamma2);
      for (int64_t i = P.n[0]; i < P.off[1]; ++i) y[i] = 0.0;  // padding between the blocks
    }
  }
};

// reductions of an inner solve: one block, or blocks 0..1 of the block vector
static double idot(const Problem &P, int blk, int64_t n, const double *x, const double *y) {
  if (blk >= 0) return bdot(P, blk, x, y);
  if (P.pt.nranks <= 1) return dot(n, x, y);
  double total = 0.0;
  for (int r = 0; r < P.pt.nranks; ++r) {
    int64_t loc_off[3] = {0, 0, 0};
    for (int b = 0; b < 2; ++b) {
      const int64_t nl = P.pt.offs[b][r + 1] - P.pt.offs[b][r];
      loc_off[b + 1] = (loc_off[b] + nl + CHUNK - 1) / CHUNK * CHUNK;
    }
    std::vector<double> lx(loc_off[2], 0.0), ly(loc_off[2], 0.0);
    for (int b = 0; b < 2; ++b) {
      const int64_t g0 = P.pt.offs[b][r], nl = P.pt.offs[b][r + 1] - g0;
      std::memcpy(&lx[loc_off[b]], x + P.off[b] + g0, nl * sizeof(double));
      std::memcpy(&ly[loc_off[b]], y + P.off[b] + g0, nl * sizeof(double));
    }
    const double d = dot(loc_off[2], lx.data(), ly.data());
    total = r == 0 ? d : total + d;
  }
  return total;
}

// Preconditioners of the inner CG.
struct IdentityPrec {
  void operator()(const double *r, double *z, int64_t n) { std::memcpy(z, r, n * sizeof(double)); }
};
struct DiagPrec {
  const double *dinv;
  void operator()(const double *r, double *z, int64_t n) { pmul(n, dinv, r, z); }
};
// Chebyshev polynomial of degree k in D^-1 Op (Saad, Alg. 12.1, zero start).
struct ChebPrec {
  Problem &P;
  InnerOp &op;
  const double *dinv;
  double lmax, lmin;
  std::vector<double> d, res, tmp;
  void operator()(const double *r, double *z, int64_t n) {
    const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin);
    const double sigma = theta / delta;
    double rho = 1.0 / sigma;
    d.resize(n);
    res.resize(n);
    tmp.resize(n);
    const double inv_theta = 1.0 / theta;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i) {
      d[i] = inv_theta * (dinv[i] * r[i]);
      z[i] = d[i];
    }
    if (P.cfg.cheb_degree > 1) std::memcpy(res.data(), r, n * sizeof(double));
    for (int j = 1; j < P.cfg.cheb_degree; ++j) {
      op(d.data(), tmp.data());
      const double rho_new = 1.0 / (2.0 * sigma - rho);
      const double c1 = rho_new * rho, c2 = 2.0 * rho_new / delta;
#pragma omp parallel for schedule(static)
      for (int64_t i = 0; i < n; ++i) {
        res[i] = res[i] - tmp[i];
        d[i] = std::fma(c1, d[i], c2 * (dinv[i] * res[i]));
        z[i] = z[i] + d[i];
      }
      rho = rho_new;
    }
  }
};

// deal.II SolverCG through inverse_operator: zero initial guess [EXT].
template <class Prec>
static State pcg(const Problem &P, InnerOp &op, Prec &prec, const alfd_control &ctrl, const double *b,
                 double *x, int &its, double &last_res, int log_level, const char *tag) {
  const int64_t n = op.n();
  const int blk = op.blk();
  std::vector<double> r(b, b + n), z(n), p(n), Ap(n);
  std::fill(x, x + n, 0.0);
  Control sc{ctrl};
  double res = std::sqrt(idot(P, blk, n, r.data(), r.data()));
  State st = sc.check(0, res);
  its = 0;
  double rz_old = 0.0;
  while (st == ITERATE) {
    ++its;
    prec(r.data(), z.data(), n);
    const double rz = idot(P, blk, n, r.data(), z.data());
    if (its > 1) {
      const double beta = rz / rz_old;
      xpby(n, z.data(), beta, p.data());
    } else {
      std::memcpy(p.data(), z.data(), n * sizeof(double));
    }
    op(p.data(), Ap.data());
    const double pAp = idot(P, blk, n, p.data(), Ap.data());
    const double alpha = rz / pAp;
    axpy(n, alpha, p.data(), x);
    axpy(n, -alpha, Ap.data(), r.data());
    res = std::sqrt(idot(P, blk, n, r.data(), r.data()));
    st = sc.check(its, res);
    rz_old = rz;
    if (log_level >= 3) std::printf("DEAL:%s:cg::Check %d\t%.17g\n", tag, its, res);
  }
  last_res = res;
  return st;
}

// Exact W^-1 (immersed_laplace.cc:866-877, stokes...:979-985: UMFPACK M^-1 in the reference):
// Jacobi-preconditioned CG on the immersed mass matrix to alfd_config::mass, once (M^-1) or
// twice ((M^-1)^2), then the scalar factor.
static int winv_scale(Problem &P, double alpha, const double *src, double *dst) {
  const int last = P.nblocks - 1;
  const int64_t n = P.n[last];
  if (P.cfg.w_inverse == ALFD_W_DIAGONAL) {
    pmul_scale(n, alpha, P.diag[ALFD_INVW], src, dst);
    return ALFD_OK;
  }
  auto mass_solve = [&](const double *b, double *x) {
    InnerOp op{P, OP_MAT, {}, &P.mat[ALFD_M], last};
    DiagPrec pr{P.dinv_m.data()};
    int its = 0;
    double res = 0;
    const State st = pcg(P, op, pr, P.cfg.mass, b, x, its, res, 0, "mass");
    P.mass_its += its;
    if (st == FAILURE && P.winv_status == ALFD_OK)
      P.winv_status = std::isnan(res) ? ALFD_E_BREAKDOWN : ALFD_E_NO_CONVERGENCE_INNER;
  };
  std::vector<double> z1(n), z2(n);
  mass_solve(src, z1.data());
  const double *z = z1.data();
  if (P.cfg.w_inverse == ALFD_W_MASS_INV_SQUARED) {
    mass_solve(z1.data(), z2.data());
    z = z2.data();
  }
  for (int64_t i = 0; i < n; ++i) dst[i] = alpha * z[i];
  return P.winv_status;
}

// dinv / lambda of the inner operator `kind`
static const double *op_dinv(const Problem &P, int kind) {
  return kind == OP_AUG ? P.dinv_aug.data() : kind == OP_A22 ? P.dinv_a22.data()
         : kind == OP_K ? P.dinv_k.data() : P.dinv_aug2.data();
}

static void ml_setup(Problem &P);
static void ml_cycle(Problem &P, int l, const double *r, double *z);
struct MlPrec {
  Problem &P;
  void operator()(const double *r, double *z, int64_t) { ml_cycle(P, 0, r, z); }
};

static int inner_solve(Problem &P, int kind, const double *b, double *x) {
  InnerOp op{P, kind, {}};
  op.exact_w = true;  // the operator the CG runs on; the preconditioners keep the diagonal weight
  int its = 0;
  double res = 0;
  State st;
  if (kind == OP_MP) {
    DiagPrec pr{P.diag[ALFD_MP_LUMPED_INV]};
    st = pcg(P, op, pr, P.cfg.mp_inner, b, x, its, res, P.cfg.log_level, "mp");
    P.mp_its += its;
  } else {
    if (P.cfg.inner_prec == ALFD_PREC_IDENTITY) {
      IdentityPrec pr;
      st = pcg(P, op, pr, P.cfg.inner, b, x, its, res, P.cfg.log_level, "aug");
    } else if (P.cfg.inner_prec == ALFD_PREC_JACOBI) {
      DiagPrec pr{op_dinv(P, kind)};
      st = pcg(P, op, pr, P.cfg.inner, b, x, its, res, P.cfg.log_level, "aug");
    } else if (P.cfg.inner_prec == ALFD_PREC_MULTILEVEL && kind == OP_AUG) {
      MlPrec pr{P};
      st = pcg(P, op, pr, P.cfg.inner, b, x, its, res, P.cfg.log_level, "aug");
    } else {
      InnerOp op2{P, kind, {}};
      ChebPrec pr{P, op2, op_dinv(P, kind), P.lam_max[kind], P.lam_max[kind] / P.cfg.cheb_eig_ratio, {}, {}, {}};
      st = pcg(P, op, pr, P.cfg.inner, b, x, its, res, P.cfg.log_level, "aug");
    }
    P.inner_its += its;
    if (kind == OP_AUG || kind == OP_A22 || kind == OP_AUG2)
      P.inner_its_op[kind == OP_AUG ? ALFD_INNER_OP_AUG : kind == OP_A22 ? ALFD_INNER_OP_A22 : ALFD_INNER_OP_AUG2] += its;
  }
  if (P.winv_status != ALFD_OK) return P.winv_status;
  if (st == FAILURE) {
    if (std::isnan(res)) return ALFD_E_BREAKDOWN;
    if (P.cfg.on_inner_failure == ALFD_INNER_THROW) return ALFD_E_NO_CONVERGENCE_INNER;
    P.inner_failures++;
  }
  return ALFD_OK;
}

static void rational_setup(Problem &P);
static bool is_elliptic(int v) { return v == ALFD_AL_ELL_IDEAL || v == ALFD_AL_ELL_MODIFIED; }

// diagonals of the inner operators and lambda_max(D^-1 Op) by power iteration
// from a deterministic integer-hash start vector.
//   diag(Aug)_i = A_ii  + gamma  sum_k w_k Ct_ik^2   (sequential fma over row i of Ct)
//   diag(A22)_i = A2_ii + gamma2 sum_k w_k M_ik^2    (row i of M)
static void diag_plus(const Csr &A, const Csr &R, const double *w, double g, int64_t n, double *dinv) {
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < n; ++i) {
    double d = 0.0;
    for (int64_t k = A.rp[i]; k < A.rp[i + 1]; ++k)
      if (A.col[k] == i) d = A.val[k];
    double s = 0.0;
    for (int64_t k = R.rp[i]; k < R.rp[i + 1]; ++k) s = std::fma(w[R.col[k]] * R.val[k], R.val[k], s);
    dinv[i] = 1.0 / std::fma(g, s, d);
  }
}

static void power_iteration(Problem &P, int kind) {
  InnerOp op{P, kind, {}};
  const int64_t n = op.n();
  const int blk = op.blk();
  const double *dinv = op_dinv(P, kind);
  std::vector<double> v(n, 0.0), wv(n, 0.0);
  auto fill = [&](int64_t off, int64_t len) {
    for (int64_t i = 0; i < len; ++i)
      v[off + i] = 1.0 + (double)(((uint64_t)i * 2654435761ull) & 1023ull) * (1.0 / 1024.0);
  };
  if (kind == OP_AUG2) {
    fill(0, P.n[0]);
    fill(P.off[1], P.n[1]);
  } else {
    fill(0, n);
  }
  double lam = 0.0;
  for (int it = 0; it < P.cfg.cheb_power_its; ++it) {
    const double nv = std::sqrt(idot(P, blk, n, v.data(), v.data()));
    scale(n, 1.0 / nv, v.data());
    op(v.data(), wv.data());
    pmul(n, dinv, wv.data(), wv.data());
    lam = std::sqrt(idot(P, blk, n, wv.data(), wv.data()));
    v.swap(wv);
  }
  P.lam_max[kind] = lam * P.cfg.cheb_safety;
}

static void setup(Problem &P) {
  const double *w = P.diag[ALFD_INVW];
  for (int k = 0; k < 6; ++k) P.lam_max[k] = 0.0;
  const bool cheb = P.cfg.inner_prec == ALFD_PREC_CHEBYSHEV || P.cfg.inner_prec == ALFD_PREC_MULTILEVEL;
  if (P.cfg.variant == ALFD_RATIONAL) {
    const Csr &A = P.mat[ALFD_A];
    P.dinv_k.assign(P.n[0], 1.0);
    for (int64_t i = 0; i < P.n[0]; ++i)
      for (int64_t k = A.rp[i]; k < A.rp[i + 1]; ++k)
        if (A.col[k] == i) P.dinv_k[i] = 1.0 / A.val[k];
    if (cheb) power_iteration(P, OP_K);
    rational_setup(P);
    P.lambda_max = P.lam_max[OP_K];
    return;
  }
  if (P.cfg.w_inverse != ALFD_W_DIAGONAL) {
    const Csr &M = P.mat[ALFD_M];
    P.dinv_m.assign(M.nrows, 0.0);
    for (int64_t i = 0; i < M.nrows; ++i)
      for (int64_t k = M.rp[i]; k < M.rp[i + 1]; ++k)
        if (M.col[k] == i) P.dinv_m[i] = 1.0 / M.val[k];
  }
  P.dinv_aug.assign(P.n[0], 0.0);
  diag_plus(P.mat[ALFD_A], P.mat[ALFD_CT], w, P.cfg.aug_assembled ? 0.0 : P.cfg.gamma, P.n[0], P.dinv_aug.data());
  if (is_elliptic(P.cfg.variant)) {
    P.dinv_a22.assign(P.n[1], 0.0);
    diag_plus(P.mat[ALFD_A2], P.mat[ALFD_M], w, P.cfg.gamma2, P.n[1], P.dinv_a22.data());
    if (P.cfg.variant == ALFD_AL_ELL_IDEAL) {
      P.dinv_aug2.assign(P.off[2], 0.0);
      std::copy(P.dinv_aug.begin(), P.dinv_aug.end(), P.dinv_aug2.begin());
      std::copy(P.dinv_a22.begin(), P.dinv_a22.end(), P.dinv_aug2.begin() + P.off[1]);
      if (cheb) power_iteration(P, OP_AUG2);
    } else if (cheb) {
      power_iteration(P, OP_AUG);
      power_iteration(P, OP_A22);
    }
  } else if (cheb) {
    power_iteration(P, OP_AUG);
  }
  P.lambda_max = P.lam_max[is_elliptic(P.cfg.variant) && P.cfg.variant == ALFD_AL_ELL_IDEAL ? OP_AUG2 : OP_AUG];
  if (P.cfg.inner_prec == ALFD_PREC_MULTILEVEL && P.ml_nlev > 0) ml_setup(P);
}

// ---- aggregation multigrid for the augmented block -------------------------------
// out = R A Q for aggregation-type transfers; canonical accumulation order: fine rows
// ascending, entries in CSR order, each added to its coarse entry as met; row sorted by column.
static void galerkin(const Csr &A, const int32_t *agg_row, const double *w_row, int64_t n_rows_c,
                     const int32_t *agg_col, const double *w_col, int64_t n_cols_c, Csr &out) {
  std::vector<std::vector<int32_t>> members;
  if (agg_row) {
    members.resize(n_rows_c);
    for (int64_t i = 0; i < A.nrows; ++i)
      if (agg_row[i] >= 0) members[agg_row[i]].push_back((int32_t)i);
  }
  out.nrows = n_rows_c;
  out.ncols = n_cols_c;
  std::vector<std::vector<std::pair<int32_t, double>>> rows(n_rows_c);
#pragma omp parallel
  {
    std::vector<int64_t> marker(n_cols_c, -1);
#pragma omp for schedule(dynamic, 64)
    for (int64_t I = 0; I < n_rows_c; ++I) {
      std::vector<std::pair<int32_t, double>> &row = rows[I];
      const int64_t cnt = agg_row ? (int64_t)members[I].size() : 1;
      for (int64_t mi = 0; mi < cnt; ++mi) {
        const int64_t i = agg_row ? members[I][mi] : I;
        const double wi = w_row ? w_row[i] : 1.0;
        for (int64_t k = A.rp[i]; k < A.rp[i + 1]; ++k) {
          const int32_t j = A.col[k];
          const int32_t J = agg_col ? agg_col[j] : j;
          if (J < 0) continue;
          const double wj = w_col ? w_col[j] : 1.0;
          const double c = (w_row || w_col) ? (wi * wj) * A.val[k] : A.val[k];
          if (marker[J] < 0) {
            marker[J] = (int64_t)row.size();
            row.emplace_back(J, c);
          } else {
            row[marker[J]].second = row[marker[J]].second + c;
          }
        }
      }
      for (auto &e : row) marker[e.first] = -1;
      std::sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    }
  }
  out.own_rp.assign(n_rows_c + 1, 0);
  for (int64_t I = 0; I < n_rows_c; ++I) out.own_rp[I + 1] = out.own_rp[I] + (int64_t)rows[I].size();
  out.own_col.resize(out.own_rp[n_rows_c]);
  out.own_val.resize(out.own_rp[n_rows_c]);
#pragma omp parallel for schedule(static)
  for (int64_t I = 0; I < n_rows_c; ++I) {
    int64_t p = out.own_rp[I];
    for (auto &e : rows[I]) {
      out.own_col[p] = e.first;
      out.own_val[p++] = e.second;
    }
  }
  out.rp = out.own_rp.data();
  out.col = out.own_col.data();
  out.val = out.own_val.data();
}

static void level_op(Problem &P, int l, const double *x, double *y, std::vector<double> &t) {
  const Csr &A = l == 0 ? P.mat[ALFD_A] : P.ml[l].A;
  const Csr &C = l == 0 ? P.mat[ALFD_C] : P.ml[l].C;
  const Csr &Ct = l == 0 ? P.mat[ALFD_CT] : P.ml[l].Ct;
  spmv(A, x, y, 0, 0.0);
  if (P.cfg.aug_assembled) return;
  t.resize(C.nrows);
  spmv(C, x, t.data(), 0, 0.0);
  pmul(C.nrows, P.diag[ALFD_INVW], t.data(), t.data());
  spmv(Ct, t.data(), y, 1, P.cfg.gamma);
}

static void level_cheb(Problem &P, int l, int degree, double ratio, const double *r, double *z) {
  const Problem::Level &L = P.ml[l];
  const int64_t n = L.n;
  const double *dinv = l == 0 ? P.dinv_aug.data() : L.dinv.data();
  const double lmax = L.lmax, lmin = lmax / ratio;
  const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin);
  const double sigma = theta / delta;
  double rho = 1.0 / sigma;
  std::vector<double> d(n), res, tmp(n), t;
  const double inv_theta = 1.0 / theta;
  for (int64_t i = 0; i < n; ++i) {
    d[i] = inv_theta * (dinv[i] * r[i]);
    z[i] = d[i];
  }
  if (degree > 1) res.assign(r, r + n);
  for (int j = 1; j < degree; ++j) {
    level_op(P, l, d.data(), tmp.data(), t);
    const double rho_new = 1.0 / (2.0 * sigma - rho);
    const double c1 = rho_new * rho, c2 = 2.0 * rho_new / delta;
    for (int64_t i = 0; i < n; ++i) {
      res[i] = res[i] - tmp[i];
      d[i] = std::fma(c1, d[i], c2 * (dinv[i] * res[i]));
      z[i] = z[i] + d[i];
    }
    rho = rho_new;
  }
}

// ---- general CSR prolongators: two-step Galerkin products -------------------------
// out = A * Pm.  Every output entry (i, J) is ONE sequential fma chain: entries k of row i of A in
// CSR order, entries of row col_k of Pm in CSR order, acc_J = fma(a_ik, p_kJ, acc_J) from 0.
// The finished row is sorted by column.
static void spgemm(const Csr &A, const Csr &Pm, Csr &out) {
  out.nrows = A.nrows;
  out.ncols = Pm.ncols;
  std::vector<std::vector<std::pair<int32_t, double>>> rows(A.nrows);
#pragma omp parallel
  {
    std::vector<int64_t> marker(Pm.ncols, -1);
#pragma omp for schedule(dynamic, 256)
    for (int64_t i = 0; i < A.nrows; ++i) {
      std::vector<std::pair<int32_t, double>> &row = rows[i];
      for (int64_t k = A.rp[i]; k < A.rp[i + 1]; ++k) {
        const double a = A.val[k];
        const int64_t j = A.col[k];
        for (int64_t e = Pm.rp[j]; e < Pm.rp[j + 1]; ++e) {
          const int32_t J = Pm.col[e];
          if (marker[J] < 0) {
            marker[J] = (int64_t)row.size();
            row.emplace_back(J, std::fma(a, Pm.val[e], 0.0));
          } else {
            row[marker[J]].second = std::fma(a, Pm.val[e], row[marker[J]].second);
          }
        }
      }
      for (auto &e : row) marker[e.first] = -1;
      std::sort(row.begin(), row.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
    }
  }
  out.own_rp.assign(A.nrows + 1, 0);
  for (int64_t i = 0; i < A.nrows; ++i) out.own_rp[i + 1] = out.own_rp[i] + (int64_t)rows[i].size();
  out.own_col.resize(out.own_rp[A.nrows]);
  out.own_val.resize(out.own_rp[A.nrows]);
  for (int64_t i = 0; i < A.nrows; ++i) {
    int64_t p = out.own_rp[i];
    for (auto &e : rows[i]) {
      out.own_col[p] = e.first;
      out.own_val[p++] = e.second;
    }
  }
  out.rp = out.own_rp.data();
  out.col = out.own_col.data();
  out.val = out.own_val.data();
}

// rows `rows` of A (compact row numbering), columns kept if colmap[col] >= 0 (renumbered), or all
// columns when colmap == nullptr; CSR order preserved
static void extract(const Csr &A, const std::vector<int32_t> &rows, const int32_t *colmap, int64_t ncols, Csr &out) {
  out.nrows = (int64_t)rows.size();
  out.ncols = ncols;
  out.own_rp.assign(rows.size() + 1, 0);
  out.own_col.clear();
  out.own_val.clear();
  for (size_t q = 0; q < rows.size(); ++q) {
    const int64_t i = rows[q];
    for (int64_t k = A.rp[i]; k < A.rp[i + 1]; ++k) {
      const int32_t c = colmap ? colmap[A.col[k]] : A.col[k];
      if (c < 0) continue;
      out.own_col.push_back(c);
      out.own_val.push_back(A.val[k]);
    }
    out.own_rp[q + 1] = (int64_t)out.own_col.size();
  }
  out.rp = out.own_rp.data();
  out.col = out.own_col.data();
  out.val = out.own_val.data();
  choose_lanes(out);
}

// y = Aug_SS x on patch-compact vectors
static void patch_op(Problem &P, const double *x, double *y, std::vector<double> &t) {
  const Problem::Patch &Q = P.patch;
  spmv(Q.Ass, x, y, 0, 0.0);
  if (P.cfg.aug_assembled) return;
  t.resize(Q.Cs.nrows);
  spmv(Q.Cs, x, t.data(), 0, 0.0);
  pmul(Q.Cs.nrows, P.diag[ALFD_INVW], t.data(), t.data());
  spmv(Q.Cts, t.data(), y, 1, P.cfg.gamma);
}

// z = q(D^-1 Aug_SS) D^-1 r: Chebyshev of degree ml_patch_degree over [lmax / ml_patch_ratio, lmax]
static void patch_cheb(Problem &P, const double *r, double *z) {
  const Problem::Patch &Q = P.patch;
  const int64_t n = (int64_t)Q.S.size();
  const double *dinv = Q.dinv.data();
  const double lmax = Q.lmax, lmin = lmax / P.cfg.ml_patch_ratio;
  const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin);
  const double sigma = theta / delta;
  double rho = 1.0 / sigma;
  const int degree = P.cfg.ml_patch_degree;
  std::vector<double> d(n), res, tmp(n), t;
  const double inv_theta = 1.0 / theta;
  for (int64_t i = 0; i < n; ++i) {
    d[i] = inv_theta * (dinv[i] * r[i]);
    z[i] = d[i];
  }
  if (degree > 1) res.assign(r, r + n);
  for (int j = 1; j < degree; ++j) {
    patch_op(P, d.data(), tmp.data(), t);
    const double rho_new = 1.0 / (2.0 * sigma - rho);
    const double c1 = rho_new * rho, c2 = 2.0 * rho_new / delta;
    for (int64_t i = 0; i < n; ++i) {
      res[i] = res[i] - tmp[i];
      d[i] = std::fma(c1, d[i], c2 * (dinv[i] * res[i]));
      z[i] = z[i] + d[i];
    }
    rho = rho_new;
  }
}

static void ml_vcycle(Problem &P, int l, const double *r, double *z) {
  const alfd_config &c = P.cfg;
  const int last = (int)P.ml.size() - 1;
  if (l == last) {
    if (P.ml_inv.present()) return spmv(P.ml_inv, r, z, 0, 0.0);
    return level_cheb(P, l, c.ml_coarse_degree, c.ml_coarse_ratio, r, z);
  }
  const int64_t n = P.ml[l].n, nc = P.ml[l + 1].n;
  std::vector<double> t(n), rc(nc), ec(nc), e(n), tl;
  const int sdeg = l > 0 && c.ml_smooth_degree_coarse > 0 ? c.ml_smooth_degree_coarse : c.ml_smooth_degree;
  level_cheb(P, l, sdeg, c.ml_smooth_ratio, r, z);
  level_op(P, l, z, t.data(), tl);
  sub_from(n, r, t.data());
  spmv(P.ml[l + 1].R, t.data(), rc.data(), 0, 0.0);
  ml_vcycle(P, l + 1, rc.data(), ec.data());
  spmv(P.ml[l + 1].Pm, ec.data(), z, 1, 1.0);
  level_op(P, l, z, t.data(), tl);
  sub_from(n, r, t.data());
  level_cheb(P, l, sdeg, c.ml_smooth_ratio, t.data(), e.data());
  for (int64_t i = 0; i < n; ++i) z[i] = std::fma(1.0, e[i], z[i]);
}

// The inner preconditioner: the V-cycle, wrapped (ml_patch_degree > 0) into the two interface-patch
// corrections  z1 = E q E^T r;  z2 = z1 + V(r - Aug z1);  z = z2 + E q E^T (r - Aug z2).
static void ml_cycle(Problem &P, int l, const double *r, double *z) {
  const Problem::Patch &Q = P.patch;
  if (l != 0 || !Q.on) return ml_vcycle(P, l, r, z);
  const int64_t n = P.ml[0].n, m = (int64_t)Q.S.size();
  const bool pen = !P.cfg.aug_assembled;
  std::vector<double> rS(m), zS(m), uS(m), eS(m), rr(r, r + n), tl(Q.Cs.nrows);
  for (int64_t q = 0; q < m; ++q) rS[q] = r[Q.S[q]];
  patch_cheb(P, rS.data(), zS.data());
  // rr = r - Aug E zS: rows T of A, the penalty through C[:,S] and the full Ct
  {
    std::vector<double> y((size_t)Q.Ats.nrows);
    spmv(Q.Ats, zS.data(), y.data(), 0, 0.0);
    for (int64_t q = 0; q < Q.Ats.nrows; ++q) rr[Q.T[q]] = std::fma(-1.0, y[q], rr[Q.T[q]]);
    if (pen) {
      spmv(Q.Cs, zS.data(), tl.data(), 0, 0.0);
      pmul(Q.Cs.nrows, P.diag[ALFD_INVW], tl.data(), tl.data());
      spmv(P.mat[ALFD_CT], tl.data(), rr.data(), 1, -P.cfg.gamma);
    }
  }
  ml_vcycle(P, 0, rr.data(), z);
  for (int64_t q = 0; q < m; ++q) z[Q.S[q]] = z[Q.S[q]] + zS[q];
  // (r - Aug z) on S
  spmv(Q.As, z, uS.data(), 0, 0.0);
  if (pen) {
    spmv(P.mat[ALFD_C], z, tl.data(), 0, 0.0);
    pmul(Q.Cs.nrows, P.diag[ALFD_INVW], tl.data(), tl.data());
    spmv(Q.Cts, tl.data(), uS.data(), 1, P.cfg.gamma);
  }
  sub_from(m, rS.data(), uS.data());
  patch_cheb(P, uS.data(), eS.data());
  for (int64_t q = 0; q < m; ++q) z[Q.S[q]] = z[Q.S[q]] + eS[q];
}

static void patch_setup(Problem &P) {
  Problem::Patch &Q = P.patch;
  const Csr &A = P.mat[ALFD_A], &C = P.mat[ALFD_C], &Ct = P.mat[ALFD_CT];
  const int64_t n = P.n[0];
  Q.S.clear();
  Q.T.clear();
  std::vector<int32_t> pos(n, -1);
  for (int64_t i = 0; i < n; ++i)
    if (Ct.rp[i + 1] > Ct.rp[i]) {
      pos[i] = (int32_t)Q.S.size();
      Q.S.push_back((int32_t)i);
    }
  const int64_t m = (int64_t)Q.S.size();
  Q.on = m > 0;
  if (!Q.on) return;
  for (int64_t i = 0; i < n; ++i) {
    bool hit = false;
    for (int64_t k = A.rp[i]; k < A.rp[i + 1] && !hit; ++k) hit = pos[A.col[k]] >= 0;
    if (hit) Q.T.push_back((int32_t)i);
  }
  std::vector<int32_t> lam_rows(C.nrows);
  for (int64_t k = 0; k < C.nrows; ++k) lam_rows[k] = (int32_t)k;
  extract(A, Q.S, pos.data(), m, Q.Ass);
  extract(A, Q.S, nullptr, n, Q.As);
  extract(A, Q.T, pos.data(), m, Q.Ats);
  extract(C, lam_rows, pos.data(), m, Q.Cs);
  extract(Ct, Q.S, nullptr, Ct.ncols, Q.Cts);
  Q.dinv.resize(m);
  for (int64_t q = 0; q < m; ++q) Q.dinv[q] = P.dinv_aug[Q.S[q]];
  std::vector<double> v(m), wv(m), t;
  for (int64_t i = 0; i < m; ++i) v[i] = 1.0 + (double)(((uint64_t)i * 2654435761ull) & 1023ull) * (1.0 / 1024.0);
  double lam = 0.0;
  for (int it = 0; it < P.cfg.cheb_power_its; ++it) {
    const double nv = std::sqrt(dot(m, v.data(), v.data()));
    scale(m, 1.0 / nv, v.data());
    patch_op(P, v.data(), wv.data(), t);
    pmul(m, Q.dinv.data(), wv.data(), wv.data());
    lam = std::sqrt(dot(m, wv.data(), wv.data()));
    v.swap(wv);
  }
  Q.lmax = lam * P.cfg.cheb_safety;
}

// Explicit inverse of the coarsest Aug (dense Cholesky, row-oriented, sequential fma chains); false when
// the matrix is not positive definite.  Stored as a dense CSR so that the product runs in canonical SpMV order.
static bool coarse_inverse(Problem &P) {
  const Problem::Level &L = P.ml.back();
  const int64_t n = L.n;
  std::vector<double> D((size_t)n * n, 0.0);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t k = L.A.rp[i]; k < L.A.rp[i + 1]; ++k) D[i * n + L.A.col[k]] = L.A.val[k];
  if (!P.cfg.aug_assembled)
    for (int64_t i = 0; i < n; ++i)
      for (int64_t k = L.Ct.rp[i]; k < L.Ct.rp[i + 1]; ++k) {
        const int64_t lam = L.Ct.col[k];
        const double s = (P.cfg.gamma * P.diag[ALFD_INVW][lam]) * L.Ct.val[k];
        for (int64_t e = L.C.rp[lam]; e < L.C.rp[lam + 1]; ++e)
          D[i * n + L.C.col[e]] = std::fma(s, L.C.val[e], D[i * n + L.C.col[e]]);
      }
  for (int64_t j = 0; j < n; ++j) {
    double d = D[j * n + j];
    for (int64_t k = 0; k < j; ++k) d = std::fma(-D[j * n + k], D[j * n + k], d);
    if (!(d > 0.0)) return false;
    const double ljj = std::sqrt(d);
    D[j * n + j] = ljj;
#pragma omp parallel for schedule(static) if (n - j > 256)
    for (int64_t i = j + 1; i < n; ++i) {
      double sacc = D[i * n + j];
      for (int64_t k = 0; k < j; ++k) sacc = std::fma(-D[i * n + k], D[j * n + k], sacc);
      D[i * n + j] = sacc / ljj;
    }
  }
  Csr &X = P.ml_inv;
  X.nrows = X.ncols = n;
  X.own_rp.resize(n + 1);
  X.own_col.resize((size_t)n * n);
  X.own_val.assign((size_t)n * n, 0.0);
  for (int64_t i = 0; i <= n; ++i) X.own_rp[i] = i * n;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < n; ++j) X.own_col[i * n + j] = (int32_t)j;
#pragma omp parallel for schedule(dynamic, 8)
  for (int64_t c = 0; c < n; ++c) {
    std::vector<double> y(n, 0.0), x(n, 0.0);
    for (int64_t i = c; i < n; ++i) {
      double sacc = i == c ? 1.0 : 0.0;
      for (int64_t k = c; k < i; ++k) sacc = std::fma(-D[i * n + k], y[k], sacc);
      y[i] = sacc / D[i * n + i];
    }
    for (int64_t i = n - 1; i >= 0; --i) {
      double sacc = y[i];
      for (int64_t k = i + 1; k < n; ++k) sacc = std::fma(-D[k * n + i], x[k], sacc);
      x[i] = sacc / D[i * n + i];
    }
    for (int64_t i = 0; i < n; ++i) X.own_val[i * n + c] = x[i];
  }
  X.rp = X.own_rp.data();
  X.col = X.own_col.data();
  X.val = X.own_val.data();
  choose_lanes(X);
  return true;
}

static void ml_setup(Problem &P) {
  const int nlev = P.ml_nlev;
  P.ml.assign(nlev + 1, Problem::Level());
  P.ml_inv = Csr();
  P.patch = Problem::Patch();
  P.ml[0].n = P.n[0];
  P.ml[0].lmax = P.lam_max[OP_AUG];
  for (int l = 0; l < nlev; ++l) {
    const Csr &A = l == 0 ? P.mat[ALFD_A] : P.ml[l].A;
    const Csr &C = l == 0 ? P.mat[ALFD_C] : P.ml[l].C;
    Problem::Level &N = P.ml[l + 1];
    const int64_t n = P.ml[l].n, nc = P.ml_nc[l];
    if (P.ml_P[l].present()) {
      // general prolongator: A_c = P^T (A P), C_c = C P, Ct_c = C_c^T
      const Csr &Pm = P.ml_P[l];
      N.Pm.nrows = n;
      N.Pm.ncols = nc;
      N.Pm.rp = Pm.rp;
      N.Pm.col = Pm.col;
      N.Pm.val = Pm.val;
      transpose_into(N.Pm, N.R);
      Csr AP;
      spgemm(A, N.Pm, AP);
      spgemm(N.R, AP, N.A);
      spgemm(C, N.Pm, N.C);
      transpose_into(N.C, N.Ct);
    } else {
    const int32_t *agg = P.ml_agg[l];
    const double *w = P.ml_wgt[l];
    galerkin(A, agg, w, nc, agg, w, nc, N.A);
    galerkin(C, nullptr, nullptr, C.nrows, agg, w, nc, N.C);
    transpose_into(N.C, N.Ct);
    // P (n x nc, one entry per represented row) and R = P^T
    N.Pm.nrows = n;
    N.Pm.ncols = nc;
    N.Pm.own_rp.assign(n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
      if (agg[i] >= 0) {
        N.Pm.own_col.push_back(agg[i]);
        N.Pm.own_val.push_back(w ? w[i] : 1.0);
      }
      N.Pm.own_rp[i + 1] = (int64_t)N.Pm.own_col.size();
    }
    N.Pm.rp = N.Pm.own_rp.data();
    N.Pm.col = N.Pm.own_col.data();
    N.Pm.val = N.Pm.own_val.data();
    transpose_into(N.Pm, N.R);
    }
    for (Csr *m : {&N.A, &N.C, &N.Ct, &N.Pm, &N.R}) choose_lanes(*m);
    N.n = nc;
    N.dinv.assign(nc, 0.0);
    diag_plus(N.A, N.Ct, P.diag[ALFD_INVW], P.cfg.aug_assembled ? 0.0 : P.cfg.gamma, nc, N.dinv.data());
    std::vector<double> v(nc), wv(nc), t;
    for (int64_t i = 0; i < nc; ++i)
      v[i] = 1.0 + (double)(((uint64_t)i * 2654435761ull) & 1023ull) * (1.0 / 1024.0);
    // rank-ordered sum of the emulated ranks' local canonical dots on this level
    auto ldot = [&](const double *x, const double *y) {
      if (P.pt.nranks <= 1 || !P.ml_off[l]) return dot(nc, x, y);
      double total = 0.0;
      for (int r = 0; r < P.pt.nranks; ++r) {
        const int64_t g0 = P.ml_off[l][r], nl = P.ml_off[l][r + 1] - g0;
        const double d = dot(nl, x + g0, y + g0);
        total = r == 0 ? d : total + d;
      }
      return total;
    };
    double lam = 0.0;
    for (int it = 0; it < P.cfg.cheb_power_its; ++it) {
      const double nv = std::sqrt(ldot(v.data(), v.data()));
      scale(nc, 1.0 / nv, v.data());
      level_op(P, l + 1, v.data(), wv.data(), t);
      pmul(nc, N.dinv.data(), wv.data(), wv.data());
      lam = std::sqrt(ldot(wv.data(), wv.data()));
      v.swap(wv);
    }
    N.lmax = lam * P.cfg.cheb_safety;
  }
  if (P.cfg.ml_coarse_direct > 0 && P.ml.back().n <= P.cfg.ml_coarse_direct && P.ml.back().n > 0 && nlev > 0)
    if (!coarse_inverse(P)) P.status = ALFD_E_BREAKDOWN;
  if (P.cfg.ml_patch_degree > 0) patch_setup(P);
}

// ---- RationalPreconditioner (rational_preconditioner.h:29-63) ----------------
// numeric constants of the reference's rational approximation (:70-93)
static const double kRatRes[21] = {
    1.1133752551375149e+01,  -4.5192561264009555e+02, -5.4280235488093114e+00, -6.6119823627983498e-01,
    -1.5483255874020074e-01, -4.8435293477731435e-02, -1.7569986796633446e-02, -6.9011933591631392e-03,
    -2.8275585395562131e-03, -1.1823861060446343e-03, -4.9806992558149195e-04, -2.0975776516702764e-04,
    -8.7959042415258930e-05, -3.6650480089224726e-05, -1.5149104182285630e-05, -6.1866179967421625e-06,
    -2.4691626461139533e-06, -9.3898594542244485e-07, -3.2099152020952601e-07, -8.4169497470931466e-08,
    -7.7616172944516437e-09};
static const double kRatPoles[20] = {
    -4.9917060842594275e+01, -5.2698715191349796e+00, -1.7156755741861143e+00, -7.5569620064292298e-01,
    -3.7811376547012854e-01, -2.0130525955937850e-01, -1.1058502730933521e-01, -6.1664070123493613e-02,
    -3.4578652087400880e-02, -1.9394206381182760e-02, -1.0845568864180035e-02, -6.0343457447149737e-03,
    -3.3328397814762593e-03, -1.8198589302273998e-03, -9.7434812604726647e-04, -5.0332017175529794e-04,
    -2.4317839761161207e-04, -1.0297057301403903e-04, -3.2227929557637293e-05, -3.3293811779427837e-06};

static void rational_setup(Problem &P) {
  const Csr &K = P.mat[ALFD_KIMM], &M = P.mat[ALFD_M];
  const int64_t n = K.nrows, nnz = K.nnz();
  P.shifted.assign(20, Csr());
  P.shifted_dinv.assign(21, std::vector<double>(n, 1.0));  // entry 20: identity (M solve is unpreconditioned)
  for (int i = 0; i < 20; ++i) {
    Csr &S = P.shifted[i];
    S.nrows = K.nrows;
    S.ncols = K.ncols;
    S.rp = K.rp;
    S.col = K.col;
    S.own_val.resize(nnz);
    const double sh = -(P.cfg.rho_bound * kRatPoles[i]);  // matrix.add(-rho_bound * poles[i-1], M)
    for (int64_t k = 0; k < nnz; ++k) S.own_val[k] = std::fma(sh, M.val[k], K.val[k]);
    S.val = S.own_val.data();
    S.L = K.L;
    S.V = K.V;
    for (int64_t r = 0; r < n; ++r)
      for (int64_t k = S.rp[r]; k < S.rp[r + 1]; ++k)
        if (S.col[k] == r) P.shifted_dinv[i][r] = 1.0 / S.val[k];
  }
}

// v1 = sum_i rho res_i (A_Gamma - rho p_i M)^-1 u1 + res_0 M^-1 u1, accumulated in
// the order of rational_preconditioner.h:51-62 (poles first, the mass term last)
static int rational_apply(Problem &P, const double *u1, double *v1) {
  const int64_t n = P.n[1];
  std::vector<double> x(n);
  std::fill(v1, v1 + n, 0.0);
  for (int i = 0; i <= 20; ++i) {
    InnerOp op{P, OP_MAT, {}, i < 20 ? &P.shifted[i] : &P.mat[ALFD_M]};
    DiagPrec pr{P.shifted_dinv[i].data()};
    int its = 0;
    double res = 0;
    State st = pcg(P, op, pr, P.cfg.rational, u1, x.data(), its, res, P.cfg.log_level, "rat");
    P.rational_its += its;
    if (st == FAILURE) {
      if (std::isnan(res)) return ALFD_E_BREAKDOWN;
      if (P.cfg.on_inner_failure == ALFD_INNER_THROW) return ALFD_E_NO_CONVERGENCE_INNER;
      P.inner_failures++;
    }
    const double c = i < 20 ? P.cfg.rho_bound * kRatRes[i + 1] : kRatRes[0];
    for (int64_t e = 0; e < n; ++e) v1[e] = v1[e] + c * x[e];
  }
  return ALFD_OK;
}

// ------------------------------------------------- preconditioner vmult
// u, v: padded concatenated block vectors.
static int precond_apply(Problem &P, const double *u, double *v) {
  P.precond_applications++;
  const alfd_config &c = P.cfg;
  const double *w = P.diag[ALFD_INVW];
  std::fill(v, v + P.ntot(), 0.0);
  if (c.variant == ALFD_AL2) {
    // augmented_lagrangian_preconditioner.h:28-34
    const double *u0 = u + P.off[0], *u1 = u + P.off[1];
    double *v0 = v + P.off[0], *v1 = v + P.off[1];
    {                                                   // v1 = -gamma invW u1
      const int rc = winv_scale(P, -c.gamma, u1, v1);
      if (rc != ALFD_OK) return rc;
    }
    std::vector<double> tmp(u0, u0 + P.n[0]);
    spmv(P.mat[ALFD_CT], v1, tmp.data(), 1, -1.0);      // tmp = u0 - Ct v1
    return inner_solve(P, OP_AUG, tmp.data(), v0);      // v0 = Aug_inv tmp
  }
  if (c.variant == ALFD_AL_STOKES || c.variant == ALFD_AL_STOKES_DIAG) {
    // :62-70 (triangular) and :95-103 (diagonal SPD)
    const bool tri = c.variant == ALFD_AL_STOKES;
    const double sgn = tri ? -1.0 : 1.0;
    const double *u0 = u + P.off[0], *u1 = u + P.off[1], *u2 = u + P.off[2];
    double *v0 = v + P.off[0], *v1 = v + P.off[1], *v2 = v + P.off[2];
    int rc = winv_scale(P, sgn * c.gamma, u2, v2);      // v2 = -+gamma invW u2
    if (rc != ALFD_OK) return rc;
    std::vector<double> q(P.n[1]);
    rc = inner_solve(P, OP_MP, u1, q.data());           // Mp_inv u1
    if (rc != ALFD_OK) return rc;
    const double s1 = sgn * c.gamma_grad_div;
    for (int64_t i = 0; i < P.n[1]; ++i) v1[i] = s1 * q[i];
    std::vector<double> tmp(u0, u0 + P.n[0]);
    if (tri) {
      spmv(P.mat[ALFD_BT], v1, tmp.data(), 1, -1.0);    // - Bt v1
      spmv(P.mat[ALFD_CT], v2, tmp.data(), 1, -1.0);    // - Ct v2
    }
    return inner_solve(P, OP_AUG, tmp.data(), v0);
  }
  if (c.variant == ALFD_AL_ELL_MODIFIED) {
    // BlockTriangularALPreconditionerModified::vmult, ...preconditioner.h:225-228:
    //   d2 = -gamma invW lambda
    //   d1 = A22_inv (u2 + M d2)
    //   d0 = A11_inv (u + gamma Ct invW M d1 - Ct d2)
    const double *u0 = u + P.off[0], *u1 = u + P.off[1], *u2 = u + P.off[2];
    double *d0 = v + P.off[0], *d1 = v + P.off[1], *d2 = v + P.off[2];
    int rc = winv_scale(P, -c.gamma, u2, d2);
    if (rc != ALFD_OK) return rc;
    std::vector<double> r1(u1, u1 + P.n[1]);
    spmv(P.mat[ALFD_M], d2, r1.data(), 1, 1.0);
    rc = inner_solve(P, OP_A22, r1.data(), d1);
    if (rc != ALFD_OK) return rc;
    std::vector<double> t(P.n[2]), r0(u0, u0 + P.n[0]);
    spmv(P.mat[ALFD_M], d1, t.data(), 0, 0.0);
    if (c.w_inverse != ALFD_W_DIAGONAL) {
      rc = winv_scale(P, 1.0, t.data(), t.data());
      if (rc != ALFD_OK) return rc;
    } else {
      pmul(P.n[2], w, t.data(), t.data());
    }
    spmv(P.mat[ALFD_CT], t.data(), r0.data(), 1, c.gamma);
    spmv(P.mat[ALFD_CT], d2, r0.data(), 1, -1.0);
    return inner_solve(P, OP_AUG, r0.data(), d0);
  }
  if (c.variant == ALFD_AL_ELL_IDEAL) {
    // BlockTriangularALPreconditioner::vmult, ...preconditioner.h:130-156:
    //   v2 = -gamma invW u2 ; [v0;v1] = Aug2x2_inv [u0 - Ct v2 ; u1 + M v2]
    const double *u2 = u + P.off[2];
    double *v2 = v + P.off[2];
    {
      const int rc = winv_scale(P, -c.gamma, u2, v2);
      if (rc != ALFD_OK) return rc;
    }
    std::vector<double> uu(u, u + P.off[2]);
    spmv(P.mat[ALFD_CT], v2, uu.data(), 1, -1.0);
    spmv(P.mat[ALFD_M], v2, uu.data() + P.off[1], 1, 1.0);
    return inner_solve(P, OP_AUG2, uu.data(), v);
  }
  if (c.variant == ALFD_RATIONAL) {
    // RationalPreconditioner::vmult, rational_preconditioner.h:29-63 (block diagonal, SPD)
    int rc = inner_solve(P, OP_K, u + P.off[0], v + P.off[0]);   // v0 = K_inv u0
    if (rc != ALFD_OK) return rc;
    return rational_apply(P, u + P.off[1], v + P.off[1]);
  }
  return ALFD_E_UNSUPPORTED;
}

// AA y = ... (immersed_laplace.cc:891-892, stokes...:1000-1003, elliptic...:816-819)
static int system_apply(Problem &P, const double *x, double *y) {
  const alfd_config &c = P.cfg;
  std::fill(y, y + P.ntot(), 0.0);
  const double *w = P.diag[ALFD_INVW];
  const int last = P.nblocks - 1;
  if (c.variant == ALFD_AL2 || c.variant == ALFD_AL_STOKES || c.variant == ALFD_AL_STOKES_DIAG) {
    const double *x0 = x + P.off[0], *xl = x + P.off[last];
    double *y0 = y + P.off[0], *yl = y + P.off[last];
    const Csr &C = P.mat[ALFD_C];
    spmv(P.mat[ALFD_A], x0, y0, 0, 0.0);
    spmv(C, x0, yl, 0, 0.0);                            // y_lambda = C x0
    if (!c.aug_assembled) {
      std::vector<double> t(C.nrows);
      if (c.w_inverse != ALFD_W_DIAGONAL) {
        const int rc = winv_scale(P, 1.0, yl, t.data());
        if (rc != ALFD_OK) return rc;
      } else {
        pmul(C.nrows, w, yl, t.data());
      }
      spmv(P.mat[ALFD_CT], t.data(), y0, 1, c.gamma);   // + gamma Ct invW C x0
    }
    if (P.nblocks == 3) {
      spmv(P.mat[ALFD_BT], x + P.off[1], y0, 1, 1.0);   // + Bt x1
      spmv(P.mat[ALFD_B], x0, y + P.off[1], 0, 0.0);    // y1 = B x0
    }
    spmv(P.mat[ALFD_CT], xl, y0, 1, 1.0);               // + Ct x_lambda
    return ALFD_OK;
  }
  if (c.variant == ALFD_RATIONAL) {
    // AA = [[K, Ct],[C, 0]] (immersed_laplace.cc:596-597): no augmentation
    spmv(P.mat[ALFD_A], x + P.off[0], y + P.off[0], 0, 0.0);
    spmv(P.mat[ALFD_CT], x + P.off[1], y + P.off[0], 1, 1.0);
    spmv(P.mat[ALFD_C], x + P.off[0], y + P.off[1], 0, 0.0);
    return ALFD_OK;
  }
  if (is_elliptic(c.variant)) {
    // [[A11_aug, A12_aug, Ct],[A21_aug, A22_aug, -M],[C, -M, 0]] with
    // A12_aug = -gamma Ct invW M, A21_aug = -gamma2 M invW C (elliptic...:810-819):
    //   y2 = C x0 - M x1 ; t = w .* y2
    //   y0 = A x0 + gamma Ct t + Ct x2 ; y1 = A2 x1 - gamma2 M t - M x2
    const double *x0 = x + P.off[0], *x1 = x + P.off[1], *x2 = x + P.off[2];
    double *y0 = y + P.off[0], *y1 = y + P.off[1], *y2 = y + P.off[2];
    const Csr &M = P.mat[ALFD_M];
    spmv(P.mat[ALFD_C], x0, y2, 0, 0.0);
    spmv(M, x1, y2, 1, -1.0);
    std::vector<double> t(P.n[2]);
    if (c.w_inverse != ALFD_W_DIAGONAL) {
      const int rc = winv_scale(P, 1.0, y2, t.data());
      if (rc != ALFD_OK) return rc;
    } else {
      pmul(P.n[2], w, y2, t.data());
    }
    spmv(P.mat[ALFD_A], x0, y0, 0, 0.0);
    spmv(P.mat[ALFD_CT], t.data(), y0, 1, c.gamma);
    spmv(P.mat[ALFD_CT], x2, y0, 1, 1.0);
    spmv(P.mat[ALFD_A2], x1, y1, 0, 0.0);
    spmv(M, t.data(), y1, 1, -c.gamma2);
    spmv(M, x2, y1, 1, -1.0);
    return ALFD_OK;
  }
  return ALFD_E_UNSUPPORTED;
}

// ------------------------------------------------------------------ FGMRES
// nranks > 1: dots are summed per emulated rank (chunk-aligned local layouts), in rank order.
static double pdot(const Problem &P, const double *x, const double *y) {
  const Partition &pt = P.pt;
  if (pt.nranks <= 1) return dot(P.ntot(), x, y);
  double total = 0.0;
  for (int r = 0; r < pt.nranks; ++r) {
    // build the rank's padded local vectors
    int64_t loc_off[ALFD_MAX_BLOCKS + 1] = {0, 0, 0, 0};
    for (int b = 0; b < P.nblocks; ++b) {
      const int64_t nl = pt.offs[b][r + 1] - pt.offs[b][r];
      loc_off[b + 1] = (loc_off[b] + nl + CHUNK - 1) / CHUNK * CHUNK;
    }
    std::vector<double> lx(loc_off[P.nblocks], 0.0), ly(loc_off[P.nblocks], 0.0);
    for (int b = 0; b < P.nblocks; ++b) {
      const int64_t g0 = pt.offs[b][r], nl = pt.offs[b][r + 1] - g0;
      std::memcpy(&lx[loc_off[b]], x + P.off[b] + g0, nl * sizeof(double));
      std::memcpy(&ly[loc_off[b]], y + P.off[b] + g0, nl * sizeof(double));
    }
    const double d = dot(loc_off[P.nblocks], lx.data(), ly.data());
    total = r == 0 ? d : total + d;
  }
  return total;
}

static int fgmres(Problem &P, const double *b, double *x, alfd_result *out,
                  std::vector<double> &history) {
  const alfd_config &c = P.cfg;
  const int m = c.restart;
  const int64_t N = P.ntot();
  std::vector<std::vector<double>> V(m + 1, std::vector<double>(N)), Z(m, std::vector<double>(N));
  std::vector<double> H((size_t)(m + 1) * m, 0.0), cs(m), sn(m), g(m + 1), h(m + 2), h2(m + 2), y(m);
  Control sc{c.outer};
  int k = 0;
  State st = ITERATE;
  double res = 0;
  history.clear();
  do {
    int rc = system_apply(P, x, V[0].data());
    if (rc != ALFD_OK) return rc;
    sub_from(N, b, V[0].data());  // v0 = b - AA x
    res = std::sqrt(pdot(P, V[0].data(), V[0].data()));
    st = sc.check(k, res);
    if (k == 0) history.push_back(res);
    if (c.log_level >= 2) std::printf("DEAL:FGMRES::Check %d\t%.17g\n", k, res);
    if (st != ITERATE) break;
    if (res != 0.0) scale(N, 1.0 / res, V[0].data());
    g[0] = res;
    int j = 0;
    for (; j < m && st == ITERATE; ++j) {
      rc = precond_apply(P, V[j].data(), Z[j].data());
      if (rc != ALFD_OK) return rc;
      double *wv = V[j + 1].data();
      rc = system_apply(P, Z[j].data(), wv);
      if (rc != ALFD_OK) return rc;
      // orthogonalise wv against V[0..j]
      if (c.orthogonalization == ALFD_ORTH_MGS) {
        for (int i = 0; i <= j; ++i) {
          h[i] = pdot(P, V[i].data(), wv);
          axpy(N, -h[i], V[i].data(), wv);
        }
      } else {
        for (int i = 0; i <= j; ++i) h[i] = pdot(P, V[i].data(), wv);
        for (int i = 0; i <= j; ++i) axpy(N, -h[i], V[i].data(), wv);
        if (c.orthogonalization == ALFD_ORTH_CGS2) {
          for (int i = 0; i <= j; ++i) h2[i] = pdot(P, V[i].data(), wv);
          for (int i = 0; i <= j; ++i) axpy(N, -h2[i], V[i].data(), wv);
          for (int i = 0; i <= j; ++i) h[i] = h[i] + h2[i];
        }
      }
      h[j + 1] = std::sqrt(pdot(P, wv, wv));
      if (h[j + 1] != 0.0) scale(N, 1.0 / h[j + 1], wv);
      // Givens
      for (int i = 0; i < j; ++i) {
        const double t = cs[i] * h[i] + sn[i] * h[i + 1];
        h[i + 1] = -sn[i] * h[i] + cs[i] * h[i + 1];
        h[i] = t;
      }
      const double denom = std::sqrt(h[j] * h[j] + h[j + 1] * h[j + 1]);
      cs[j] = h[j] / denom;
      sn[j] = h[j + 1] / denom;
      h[j] = denom;
      g[j + 1] = -sn[j] * g[j];
      g[j] = cs[j] * g[j];
      for (int i = 0; i <= j; ++i) H[(size_t)i * m + j] = h[i];
      res = std::fabs(g[j + 1]);
      ++k;
      st = sc.check(k, res);
      history.push_back(res);
      if (c.log_level >= 2) std::printf("DEAL:FGMRES::Check %d\t%.17g\n", k, res);
    }
    // back substitution, x += Z y
    for (int i = j - 1; i >= 0; --i) {
      double s = g[i];
      for (int l = i + 1; l < j; ++l) s -= H[(size_t)i * m + l] * y[l];
      y[i] = s / H[(size_t)i * m + i];
    }
    for (int i = 0; i < j; ++i) axpy(N, y[i], Z[i].data(), x);
  } while (st == ITERATE);
  out->outer_iterations = k;
  out->initial_residual = sc.initial;
  out->last_residual = res;
  if (c.log_level >= 1)
    std::printf(st == SUCCESS ? "DEAL:FGMRES::Convergence step %d value %.17g\n"
                              : "DEAL:FGMRES::Failure step %d value %.17g\n",
                k, res);
  if (st != SUCCESS) return std::isnan(res) ? ALFD_E_BREAKDOWN : ALFD_E_NO_CONVERGENCE_OUTER;
  return ALFD_OK;
}

// (n+1) x n Hessenberg least squares by Givens rotations; H row-major with leading dimension m.
static double hessenberg_lsq(const std::vector<double> &H, int m, int n, double beta, std::vector<double> &y) {
  std::vector<double> R((size_t)(n + 1) * n), g(n + 1, 0.0);
  for (int i = 0; i <= n; ++i)
    for (int j = 0; j < n; ++j) R[(size_t)i * n + j] = H[(size_t)i * m + j];
  g[0] = beta;
  for (int j = 0; j < n; ++j) {
    const double a = R[(size_t)j * n + j], b = R[(size_t)(j + 1) * n + j];
    const double denom = std::sqrt(a * a + b * b);
    const double c = a / denom, sn = b / denom;
    for (int l = j; l < n; ++l) {
      const double t = c * R[(size_t)j * n + l] + sn * R[(size_t)(j + 1) * n + l];
      R[(size_t)(j + 1) * n + l] = -sn * R[(size_t)j * n + l] + c * R[(size_t)(j + 1) * n + l];
      R[(size_t)j * n + l] = t;
    }
    const double t = c * g[j];
    g[j + 1] = -sn * g[j];
    g[j] = t;
  }
  for (int i = n - 1; i >= 0; --i) {
    double sum = g[i];
    for (int l = i + 1; l < n; ++l) sum -= R[(size_t)i * n + l] * y[l];
    y[i] = sum / R[(size_t)i * n + i];
  }
  return std::fabs(g[n]);
}

// SolverFGMRES of deal.II <= 9.5 [EXT], written from the published loop (solver_gmres.h of 9.4/9.5):
//   aux = b - A x; beta = |aux|; check(accumulated, beta)            (no increment)
//   for j < m: v_j = aux / a; z_j = P v_j; aux = A z_j;
//              H(0,j) = aux.v_0; H(i+1,j) = aux.add_and_dot(-H(i,j), v_i, v_{i+1});
//              H(j+1,j) = a = sqrt(aux.add_and_dot(-H(j,j), v_j, aux));
//              if j > 0: res = least_squares(H(0:j, 0:j-1)); check(++accumulated, res)
//   x += sum_{i < size(y)} y_i z_i
static int fgmres_dealii95(Problem &P, const double *b, double *x, alfd_result *out, std::vector<double> &history) {
  const alfd_config &c = P.cfg;
  const int m = c.restart;
  const int64_t N = P.ntot();
  std::vector<std::vector<double>> V(m, std::vector<double>(N)), Z(m, std::vector<double>(N));
  std::vector<double> aux(N), H((size_t)(m + 1) * m, 0.0), y(m, 0.0);
  Control sc{c.outer};
  int k = 0;
  State st = ITERATE;
  double res = 0;
  history.clear();
  do {
    int rc = system_apply(P, x, aux.data());
    if (rc != ALFD_OK) return rc;
    sub_from(N, b, aux.data());
    const double beta = std::sqrt(pdot(P, aux.data(), aux.data()));
    res = beta;
    st = sc.check(k, res);
    if (k == 0) history.push_back(res);
    if (c.log_level >= 2) std::printf("DEAL:FGMRES::Check %d\t%.17g\n", k, res);
    if (st != ITERATE) break;
    std::fill(H.begin(), H.end(), 0.0);
    double a = beta;
    int ny = 0;
    for (int j = 0; j < m; ++j) {
      if (a != 0.0) {
        const double ia = 1.0 / a;
        for (int64_t i = 0; i < N; ++i) V[j][i] = ia * aux[i];
      } else {
        std::fill(V[j].begin(), V[j].end(), 0.0);
      }
      rc = precond_apply(P, V[j].data(), Z[j].data());
      if (rc != ALFD_OK) return rc;
      rc = system_apply(P, Z[j].data(), aux.data());
      if (rc != ALFD_OK) return rc;
      H[(size_t)0 * m + j] = pdot(P, aux.data(), V[0].data());
      for (int i = 0; i < j; ++i) {
        axpy(N, -H[(size_t)i * m + j], V[i].data(), aux.data());
        H[(size_t)(i + 1) * m + j] = pdot(P, aux.data(), V[i + 1].data());
      }
      axpy(N, -H[(size_t)j * m + j], V[j].data(), aux.data());
      H[(size_t)(j + 1) * m + j] = a = std::sqrt(pdot(P, aux.data(), aux.data()));
      if (j > 0) {
        res = hessenberg_lsq(H, m, j, beta, y);
        ny = j;
        ++k;
        st = sc.check(k, res);
        history.push_back(res);
        if (c.log_level >= 2) std::printf("DEAL:FGMRES::Check %d\t%.17g\n", k, res);
        if (st != ITERATE) break;
      }
    }
    for (int i = 0; i < ny; ++i) axpy(N, y[i], Z[i].data(), x);
  } while (st == ITERATE);
  out->outer_iterations = k;
  out->initial_residual = sc.initial;
  out->last_residual = res;
  if (st != SUCCESS) return std::isnan(res) ? ALFD_E_BREAKDOWN : ALFD_E_NO_CONVERGENCE_OUTER;
  return ALFD_OK;
}

// deal.II SolverMinRes [EXT] (preconditioned MINRES with the Lanczos three-term
// recurrence; r_l2 is the preconditioned residual estimate the stop rule sees).
// Used at immersed_laplace.cc:629-631 and stokes...:1057-1064.
static int minres(Problem &P, const double *b, double *x, alfd_result *out, std::vector<double> &history) {
  const alfd_config &c = P.cfg;
  const int64_t N = P.ntot();
  std::vector<double> U[3], Mv[3], v(N, 0.0);
  for (int i = 0; i < 3; ++i) U[i].assign(N, 0.0), Mv[i].assign(N, 0.0);
  double *u0 = U[0].data(), *u1 = U[1].data(), *u2 = U[2].data();
  double *m0 = Mv[0].data(), *m1 = Mv[1].data(), *m2 = Mv[2].data();
  double delta[3] = {0, 0, 0}, f[2] = {0, 0}, e[2] = {0, 0};
  double r_l2 = 0, r0 = 0, tau = 0, cc = 0, ss = 0, d_ = 0, phibar = 0;
  int j = 1;
  Control sc{c.outer};
  history.clear();
  int rc = system_apply(P, x, m0);
  if (rc != ALFD_OK) return rc;
  for (int64_t i = 0; i < N; ++i) u1[i] = b[i] - m0[i];
  rc = precond_apply(P, u1, v.data());
  if (rc != ALFD_OK) return rc;
  delta[1] = pdot(P, v.data(), u1);
  if (delta[1] < 0) return ALFD_E_BREAKDOWN;  // ExcPreconditionerNotDefinite
  r0 = std::sqrt(delta[1]);
  r_l2 = r0;
  phibar = r0;
  std::fill(U[0].begin(), U[0].end(), 0.0);
  delta[0] = 1.0;
  for (int i = 0; i < 3; ++i) std::fill(Mv[i].begin(), Mv[i].end(), 0.0);
  State st = sc.check(0, r_l2);
  history.push_back(r_l2);
  if (c.log_level >= 2) std::printf("DEAL:minres::Check 0\t%.17g\n", r_l2);
  while (st == ITERATE) {
    if (delta[1] != 0)
      scale(N, 1.0 / std::sqrt(delta[1]), v.data());
    else
      std::fill(v.begin(), v.end(), 0.0);
    rc = system_apply(P, v.data(), u2);
    if (rc != ALFD_OK) return rc;
    axpy(N, -std::sqrt(delta[1] / delta[0]), u0, u2);
    const double gamma = pdot(P, u2, v.data());
    axpy(N, -gamma / std::sqrt(delta[1]), u1, u2);
    std::memcpy(m0, v.data(), N * sizeof(double));
    rc = precond_apply(P, u2, v.data());
    if (rc != ALFD_OK) return rc;
    delta[2] = pdot(P, v.data(), u2);
    if (delta[2] < 0) return ALFD_E_BREAKDOWN;
    if (j == 1) {
      d_ = gamma;
      e[1] = std::sqrt(delta[2]);
    }
    if (j > 1) {
      d_ = ss * e[0] - cc * gamma;
      e[0] = cc * e[0] + ss * gamma;
      f[1] = ss * std::sqrt(delta[2]);
      e[1] = -cc * std::sqrt(delta[2]);
    }
    const double d = std::sqrt(d_ * d_ + delta[2]);
    // tau_j = c_j * phibar_{j-1}, phibar_j = s_j * phibar_{j-1}, phibar_0 = r0.  (The
    // recurrence tau *= s/c; tau *= c of the textbook form divides by c_{j-1}, which is
    // exactly 0 when the first Lanczos coefficient vanishes -- f = 0 in a saddle-point
    // system with a block-diagonal preconditioner; this product form is identical
    // otherwise.)
    cc = d_ / d;
    ss = std::sqrt(delta[2]) / d;
    tau = cc * phibar;
    phibar = ss * phibar;
    axpy(N, -e[0], m1, m0);
    if (j > 1) axpy(N, -f[0], m2, m0);
    scale(N, 1.0 / d, m0);
    axpy(N, tau, m0, x);
    r_l2 *= std::fabs(ss);
    st = sc.check(j, r_l2);
    history.push_back(r_l2);
    if (c.log_level >= 2) std::printf("DEAL:minres::Check %d\t%.17g\n", j, r_l2);
    ++j;
    double *t = u0;  // u0 <- u1 <- u2 <- (old u0)
    u0 = u1;
    u1 = u2;
    u2 = t;
    t = m2;          // m2 <- m1 <- m0 <- (old m2)
    m2 = m1;
    m1 = m0;
    m0 = t;
    delta[0] = delta[1];
    delta[1] = delta[2];
    f[0] = f[1];
    e[0] = e[1];
  }
  out->outer_iterations = j - 1;
  out->initial_residual = sc.initial;
  out->last_residual = r_l2;
  if (c.log_level >= 1)
    std::printf(st == SUCCESS ? "DEAL:minres::Convergence step %d value %.17g\n"
                              : "DEAL:minres::Failure step %d value %.17g\n",
                j - 1, r_l2);
  if (st != SUCCESS) return std::isnan(r_l2) ? ALFD_E_BREAKDOWN : ALFD_E_NO_CONVERGENCE_OUTER;
  return ALFD_OK;
}

}  // namespace orc

// ------------------------------------------------------------------- C API
extern "C" {

typedef struct orc_csr {
  int64_t nrows, ncols;
  const int64_t *row_ptr;
  const int32_t *col;
  const double *val;
} orc_csr;

typedef struct orc_problem {
  orc_csr mat[ALFD_NSLOTS];
  const double *diag[ALFD_NDIAGS];
  int32_t nblocks;
  int32_t nranks_emulated;
  int64_t n[ALFD_MAX_BLOCKS];
  const int64_t *part_offsets[ALFD_MAX_BLOCKS];  // optional [nranks+1] per block; NULL = even split
  int32_t ml_levels;                             // ALFD_PREC_MULTILEVEL: aggregates per level
  int32_t pad_;
  const int32_t *ml_agg[ALFD_MAX_LEVELS];
  const double *ml_weight[ALFD_MAX_LEVELS];
  int64_t ml_ncoarse[ALFD_MAX_LEVELS];
  const int64_t *ml_offsets[ALFD_MAX_LEVELS];    // emulated ranks: [nranks+1] offsets of each coarse level
  orc_csr ml_prolong[ALFD_MAX_LEVELS];           // CSR prolongator of a level (row_ptr != NULL): replaces ml_agg
} orc_problem;

static int build(const orc_problem *op, const alfd_config *cfg, orc::Problem &P) {
  P.cfg = *cfg;
  P.nblocks = op->nblocks;
  if (P.nblocks < 2 || P.nblocks > 3) return ALFD_E_INVALID;
  for (int b = 0; b < P.nblocks; ++b) {
    P.n[b] = op->n[b];
    P.off[b + 1] = (P.off[b] + P.n[b] + orc::CHUNK - 1) / orc::CHUNK * orc::CHUNK;
  }
  for (int s = 0; s < ALFD_NSLOTS; ++s) {
    orc::Csr &m = P.mat[s];
    m.nrows = op->mat[s].nrows;
    m.ncols = op->mat[s].ncols;
    m.rp = op->mat[s].row_ptr;
    m.col = op->mat[s].col;
    m.val = op->mat[s].val;
  }
  for (int d = 0; d < ALFD_NDIAGS; ++d) P.diag[d] = op->diag[d];
  if (!P.mat[ALFD_A].present() || !P.mat[ALFD_CT].present()) return ALFD_E_INVALID;
  if (!P.diag[ALFD_INVW] && cfg->variant != ALFD_RATIONAL) return ALFD_E_INVALID;
  if (!P.mat[ALFD_C].present()) orc::transpose_into(P.mat[ALFD_CT], P.mat[ALFD_C]);
  const bool ell = cfg->variant == ALFD_AL_ELL_IDEAL || cfg->variant == ALFD_AL_ELL_MODIFIED;
  if (cfg->variant == ALFD_RATIONAL) {
    const orc::Csr &K = P.mat[ALFD_KIMM], &M = P.mat[ALFD_M];
    if (P.nblocks != 2 || !K.present() || !M.present() || K.nnz() != M.nnz() || !(cfg->rho_bound > 0))
      return ALFD_E_INVALID;
    for (int64_t k = 0; k < K.nnz(); ++k)
      if (K.col[k] != M.col[k]) return ALFD_E_INVALID;  // matrix.add() needs one sparsity pattern
  }
  if (ell) {
    if (P.nblocks != 3 || !P.mat[ALFD_A2].present() || !P.mat[ALFD_M].present() || P.n[1] != P.n[2])
      return ALFD_E_INVALID;
  } else if (P.nblocks == 3) {
    if (!P.mat[ALFD_BT].present() || !P.mat[ALFD_MP].present() || !P.diag[ALFD_MP_LUMPED_INV])
      return ALFD_E_INVALID;
    if (!P.mat[ALFD_B].present()) orc::transpose_into(P.mat[ALFD_BT], P.mat[ALFD_B]);
  }
  for (int s = 0; s < ALFD_NSLOTS; ++s)
    if (P.mat[s].present()) orc::choose_lanes(P.mat[s]);
  P.ml_nlev = op->ml_levels;
  for (int l = 0; l < op->ml_levels && l < ALFD_MAX_LEVELS; ++l) {
    P.ml_agg[l] = op->ml_agg[l];
    P.ml_wgt[l] = op->ml_weight[l];
    P.ml_nc[l] = op->ml_ncoarse[l];
    P.ml_off[l] = op->ml_offsets[l];
    if (op->ml_prolong[l].row_ptr) {
      orc::Csr &m = P.ml_P[l];
      m.nrows = op->ml_prolong[l].nrows;
      m.ncols = op->ml_prolong[l].ncols;
      m.rp = op->ml_prolong[l].row_ptr;
      m.col = op->ml_prolong[l].col;
      m.val = op->ml_prolong[l].val;
      P.ml_nc[l] = m.ncols;
      // emulated ranks: the library keeps levels >= 1 and the patch REPLICATED and builds them partition-independently
      // (ml_setup_rep_prolongators), so nothing below level 0 depends on the partition -- plain reductions there
    }
  }
  if (cfg->inner_prec == ALFD_PREC_MULTILEVEL && P.ml_nlev < 1) return ALFD_E_NOT_SETUP;
  P.pt.nranks = op->nranks_emulated > 1 ? op->nranks_emulated : 1;
  if (P.pt.nranks > 1) {
    P.pt.offs.resize(P.nblocks);
    for (int b = 0; b < P.nblocks; ++b) {
      P.pt.offs[b].resize(P.pt.nranks + 1);
      for (int r = 0; r <= P.pt.nranks; ++r)
        P.pt.offs[b][r] = op->part_offsets[b] ? op->part_offsets[b][r] : P.n[b] * r / P.pt.nranks;
    }
  }
  if (cfg->w_inverse != ALFD_W_DIAGONAL) {
    if (cfg->variant == ALFD_RATIONAL) return ALFD_E_UNSUPPORTED;
    if (!P.mat[ALFD_M].present() || P.mat[ALFD_M].nrows != P.n[P.nblocks - 1]) return ALFD_E_NOT_SETUP;
  }
  orc::setup(P);
  return P.status;
}

static void pack(const orc::Problem &P, const double *const *blocks, std::vector<double> &v) {
  v.assign(P.ntot(), 0.0);
  for (int b = 0; b < P.nblocks; ++b) std::memcpy(&v[P.off[b]], blocks[b], P.n[b] * sizeof(double));
}
static void unpack(const orc::Problem &P, const std::vector<double> &v, double *const *blocks) {
  for (int b = 0; b < P.nblocks; ++b) std::memcpy(blocks[b], &v[P.off[b]], P.n[b] * sizeof(double));
}

static void fill_result(const orc::Problem &P, alfd_result *res, int status) {
  res->status = status;
  res->inner_iterations = P.inner_its;
  res->mp_iterations = P.mp_its;
  res->inner_failures = P.inner_failures;
  res->precond_applications = P.precond_applications;
  res->lambda_max = P.lambda_max;
  res->rational_iterations = P.rational_its;
  res->mass_iterations = P.mass_its;
}

int orc_spmv(const orc_csr *m, int lanes, int vec, const double *x, double *y, int mode, double alpha) {
  orc::Csr c;
  c.nrows = m->nrows;
  c.ncols = m->ncols;
  c.rp = m->row_ptr;
  c.col = m->col;
  c.val = m->val;
  if (lanes > 0) {
    c.L = lanes;
    c.V = vec > 0 ? vec : 1;
  } else {
    orc::choose_lanes(c);
  }
  orc::spmv(c, x, y, mode, alpha);
  return c.L;
}

double orc_dot(int64_t n, const double *x, const double *y) { return orc::dot(n, x, y); }

// Persistent handle: setup once (diagonals, lambda_max, multilevel hierarchy), apply many
// times -- used by bench.py's cpu_baseline so that setup is outside the timed sample.
void *orc_open(const orc_problem *op, const alfd_config *cfg, int *status) {
  orc::Problem *P = new orc::Problem;
  const int rc = build(op, cfg, *P);
  if (status) *status = rc;
  if (rc != ALFD_OK) {
    delete P;
    return nullptr;
  }
  return P;
}
void orc_close(void *h) { delete static_cast<orc::Problem *>(h); }
int orc_h_precond_apply(void *h, const alfd_control *inner_override, const double *const *src,
                        double *const *dst, alfd_result *res) {
  orc::Problem &P = *static_cast<orc::Problem *>(h);
  if (inner_override) P.cfg.inner = *inner_override;
  P.inner_its = P.mp_its = P.rational_its = P.mass_its = 0;
  P.inner_its_op[0] = P.inner_its_op[1] = P.inner_its_op[2] = 0;
  P.inner_failures = P.precond_applications = 0;
  std::vector<double> u, v(P.ntot(), 0.0);
  pack(P, src, u);
  const int rc = orc::precond_apply(P, u.data(), v.data());
  unpack(P, v, dst);
  std::memset(res, 0, sizeof(*res));
  fill_result(P, res, rc);
  return rc;
}

// One solve on a persistent handle (setup kept): bench.py's cpu_baseline / parity_prefix at the bench size.
int orc_h_solve(void *h, const double *const *rhs, double *const *x, alfd_result *res, double *history,
                int32_t history_cap, int32_t *history_count) {
  orc::Problem &P = *static_cast<orc::Problem *>(h);
  P.inner_its = P.mp_its = P.rational_its = P.mass_its = 0;
  P.inner_its_op[0] = P.inner_its_op[1] = P.inner_its_op[2] = 0;
  P.inner_failures = P.precond_applications = 0;
  std::vector<double> bb, xx, hist;
  pack(P, rhs, bb);
  pack(P, x, xx);
  std::memset(res, 0, sizeof(*res));
  const auto t0 = std::chrono::steady_clock::now();
  const alfd_config *cfg = &P.cfg;
  int rc = cfg->outer_solver == ALFD_OUTER_MINRES               ? orc::minres(P, bb.data(), xx.data(), res, hist)
           : cfg->fgmres_flavour == ALFD_FGMRES_DEALII_95 ? orc::fgmres_dealii95(P, bb.data(), xx.data(), res, hist)
                                                          : orc::fgmres(P, bb.data(), xx.data(), res, hist);
  res->solve_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  unpack(P, xx, x);
  fill_result(P, res, rc);
  if (history_count) *history_count = (int32_t)hist.size();
  if (history)
    for (int i = 0; i < (int)hist.size() && i < history_cap; ++i) history[i] = hist[i];
  return rc;
}

// Inner CG iterations of the last orc_h_precond_apply / orc_h_solve by alfd_inner_op (alfd_get_inner_iterations).
int orc_h_inner_iterations(void *h, int64_t counts[3]) {
  if (!h || !counts) return ALFD_E_INVALID;
  const orc::Problem &P = *static_cast<orc::Problem *>(h);
  std::copy(P.inner_its_op, P.inner_its_op + 3, counts);
  return ALFD_OK;
}

int orc_h_system_apply(void *h, const double *const *src, double *const *dst) {
  orc::Problem &P = *static_cast<orc::Problem *>(h);
  std::vector<double> u, v(P.ntot(), 0.0);
  pack(P, src, u);
  const int rc = orc::system_apply(P, u.data(), v.data());
  unpack(P, v, dst);
  return rc;
}

// z = M^-1 r: one application of the inner CG's preconditioner on a persistent handle (alfd_inner_prec_apply):
// the dispatch of inner_solve() without the CG.  op: enum alfd_inner_op; r, z as in alfd.h.
int orc_h_inner_prec_apply(void *h, int op, const double *r, double *z) {
  orc::Problem &P = *static_cast<orc::Problem *>(h);
  if (!r || !z) return ALFD_E_INVALID;
  const int v = P.cfg.variant;
  int kind = -1;
  if (op == ALFD_INNER_OP_AUG &&
      (v == ALFD_AL2 || v == ALFD_AL_STOKES || v == ALFD_AL_STOKES_DIAG || v == ALFD_AL_ELL_MODIFIED))
    kind = orc::OP_AUG;
  else if (op == ALFD_INNER_OP_A22 && v == ALFD_AL_ELL_MODIFIED)
    kind = orc::OP_A22;
  else if (op == ALFD_INNER_OP_AUG2 && v == ALFD_AL_ELL_IDEAL)
    kind = orc::OP_AUG2;
  if (kind < 0) return ALFD_E_INVALID;
  orc::InnerOp op2{P, kind, {}};
  const int64_t n = op2.n();
  std::vector<double> rr(n, 0.0), zz(n, 0.0);
  if (kind == orc::OP_AUG2) {          // [r_0 ; r_1] -> [block 0 | pad | block 1]
    std::memcpy(rr.data(), r, P.n[0] * sizeof(double));
    std::memcpy(rr.data() + P.off[1], r + P.n[0], P.n[1] * sizeof(double));
  } else {
    std::memcpy(rr.data(), r, n * sizeof(double));
  }
  if (P.cfg.inner_prec == ALFD_PREC_IDENTITY) {
    orc::IdentityPrec pr;
    pr(rr.data(), zz.data(), n);
  } else if (P.cfg.inner_prec == ALFD_PREC_JACOBI) {
    orc::DiagPrec pr{orc::op_dinv(P, kind)};
    pr(rr.data(), zz.data(), n);
  } else if (P.cfg.inner_prec == ALFD_PREC_MULTILEVEL && kind == orc::OP_AUG) {
    orc::MlPrec pr{P};
    pr(rr.data(), zz.data(), n);
  } else {
    orc::ChebPrec pr{P, op2, orc::op_dinv(P, kind), P.lam_max[kind], P.lam_max[kind] / P.cfg.cheb_eig_ratio, {}, {}, {}};
    pr(rr.data(), zz.data(), n);
  }
  if (kind == orc::OP_AUG2) {
    std::memcpy(z, zz.data(), P.n[0] * sizeof(double));
    std::memcpy(z + P.n[0], zz.data() + P.off[1], P.n[1] * sizeof(double));
  } else {
    std::memcpy(z, zz.data(), n * sizeof(double));
  }
  return ALFD_OK;
}

int orc_precond_apply(const orc_problem *op, const alfd_config *cfg, const double *const *src,
                      double *const *dst, alfd_result *res) {
  orc::Problem P;
  int rc = build(op, cfg, P);
  if (rc != ALFD_OK) return rc;
  std::vector<double> u, v(P.ntot(), 0.0);
  pack(P, src, u);
  rc = orc::precond_apply(P, u.data(), v.data());
  unpack(P, v, dst);
  std::memset(res, 0, sizeof(*res));
  fill_result(P, res, rc);
  return rc;
}

int orc_system_apply(const orc_problem *op, const alfd_config *cfg, const double *const *src,
                     double *const *dst) {
  orc::Problem P;
  int rc = build(op, cfg, P);
  if (rc != ALFD_OK) return rc;
  std::vector<double> u, v(P.ntot(), 0.0);
  pack(P, src, u);
  rc = orc::system_apply(P, u.data(), v.data());
  unpack(P, v, dst);
  return rc;
}

// b0 += gamma Ct (invW .* g)  (stokes...:1012-1018)
int orc_augment_rhs(const orc_problem *op, const alfd_config *cfg, double *const *rhs) {
  orc::Problem P;
  int rc = build(op, cfg, P);
  if (rc != ALFD_OK) return rc;
  const int last = P.nblocks - 1;
  std::vector<double> t(P.n[last]);
  if (cfg->w_inverse != ALFD_W_DIAGONAL) {
    rc = orc::winv_scale(P, 1.0, rhs[last], t.data());
    if (rc != ALFD_OK) return rc;
  } else {
    orc::pmul(P.n[last], P.diag[ALFD_INVW], rhs[last], t.data());
  }
  orc::spmv(P.mat[ALFD_CT], t.data(), rhs[0], 1, cfg->gamma);
  return ALFD_OK;
}

int orc_solve(const orc_problem *op, const alfd_config *cfg, const double *const *rhs,
              double *const *x, alfd_result *res, double *history, int32_t history_cap,
              int32_t *history_count) {
  orc::Problem P;
  int rc = build(op, cfg, P);
  if (rc != ALFD_OK) return rc;
  std::vector<double> bb, xx, hist;
  pack(P, rhs, bb);
  pack(P, x, xx);
  std::memset(res, 0, sizeof(*res));
  const auto t0 = std::chrono::steady_clock::now();
  rc = cfg->outer_solver == ALFD_OUTER_MINRES               ? orc::minres(P, bb.data(), xx.data(), res, hist)
       : cfg->fgmres_flavour == ALFD_FGMRES_DEALII_95 ? orc::fgmres_dealii95(P, bb.data(), xx.data(), res, hist)
                                                      : orc::fgmres(P, bb.data(), xx.data(), res, hist);
  res->solve_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  unpack(P, xx, x);
  fill_result(P, res, rc);
  if (history_count) *history_count = (int32_t)hist.size();
  if (history)
    for (int i = 0; i < (int)hist.size() && i < history_cap; ++i) history[i] = hist[i];
  return rc;
}

// Thread count of the OpenMP loops (results do not depend on it: every row sum
// and every chunk partial is computed by exactly one thread in canonical order).
int orc_set_threads(int n) {
#ifdef _OPENMP
  if (n > 0) omp_set_num_threads(n);
  return omp_get_max_threads();
#else
  (void)n;
  return 1;
#endif
}

int orc_set_row_order(int order) {
  orc::g_row_order = order == 1 ? 1 : 0;
  return orc::g_row_order;
}

// Scalar known-answer hook for a6: evaluates res0 + sum_i res_i / (x - p_i)
// with the constants of rational_preconditioner.h:70-93 passed in by the test.
double orc_rational_eval(int npoles, const double *res, const double *poles, double x) {
  double s = res[0];
  for (int i = 0; i < npoles; ++i) s += res[i + 1] / (x - poles[i]);
  return s;
}

}  // extern "C"
