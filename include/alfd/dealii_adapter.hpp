// dealii_adapter.hpp -- header-only C++17 adapter that presents the C ABI of
// alfd.h as deal.II-shaped classes, so that the reference's solve() functions
// (immersed_laplace.cc:636-949, stokes_immersed_boundary.cc:918-1079) keep
// their call-site shape:
//
//     alfd::dealii_adapter::System sys(/*device*/ 0);
//     sys.set_matrix(ALFD_A,  stokes_matrix.block(0, 0));   // linear_operator(...) captures
//     sys.set_matrix(ALFD_BT, stokes_matrix.block(0, 1));
//     sys.set_matrix(ALFD_CT, coupling_matrix);
//     sys.set_matrix(ALFD_MP, preconditioner_matrix.block(1, 1));
//     sys.set_diag(ALFD_INVW, inverse_squares);             // DiagonalMatrix<Vector<double>>
//     sys.set_diag(ALFD_MP_LUMPED_INV, pressure_diagonal_inv);
//     // `Diagonal mass immersed = false` (stokes...:979-985): cfg.w_inverse = ALFD_W_MASS_INV_SQUARED and
//     // sys.set_matrix(ALFD_M, mass_matrix) -- the UMFPACK solves become CG on M inside the library
//     sys.configure(cfg); sys.setup();
//     BlockPreconditionerAugmentedLagrangianStokes P(sys);  // vmult(v, u) const
//     SolverFGMRES<BlockVector<double>> solver(sys);        // solve(AA, x, b, P)
//     solver.solve(sys.system_operator(), solution_block, system_rhs_block, P);
//     outer_solver_control.last_step()  ->  solver.last_step()
// The other call sites map the same way: elliptic_interface.cc:900-906 / 940-948 ->
// EllipticInterfacePreconditioners::BlockTriangularALPreconditioner{,Modified} + SolverFGMRES;
// immersed_laplace.cc:625-631 -> RationalPreconditioner + SolverMinRes (tests/adapter/adapter_demo.cpp
// runs all three against the golden iteration counts).
//
// It is templated on the matrix / vector types and needs only the members the
// reference uses: SparseMatrix: m(), n(), n_nonzero_elements(), begin(row) /
// end(row) iterators with column() and value(); Vector: size(), begin();
// BlockVector: n_blocks(), block(i).  tests/test_adapter.py compiles it against
// a 60-line mock of those classes (deal.II itself is not installed here).
//
// Errors: a non-zero status from the ABI becomes a C++ exception --
// alfd::dealii_adapter::NoConvergence (mirror of dealii::SolverControl::
// NoConvergence, caught by the reference's main(): stokes...:1233-1254) or
// alfd::dealii_adapter::Error (mirror of ExcMessage).
#ifndef ALFD_DEALII_ADAPTER_HPP
#define ALFD_DEALII_ADAPTER_HPP

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "alfd/alfd.h"

namespace alfd {
namespace dealii_adapter {

struct Error : std::runtime_error {
  int status;
  Error(int s, const std::string &what) : std::runtime_error(what), status(s) {}
};
// dealii::SolverControl::NoConvergence carries last_step / last_residual.
struct NoConvergence : Error {
  unsigned int last_step;
  double last_residual;
  NoConvergence(int s, const std::string &what, unsigned int step, double res)
      : Error(s, what), last_step(step), last_residual(res) {}
};

class System {
 public:
  explicit System(int device_id = 0) {
    const int rc = alfd_create(&ctx_, device_id);
    if (rc != ALFD_OK) throw Error(rc, std::string("alfd_create: ") + alfd_strerror(rc));
  }
  ~System() {
    if (ctx_) alfd_destroy(ctx_);
  }
  System(const System &) = delete;
  System &operator=(const System &) = delete;

  // deal.II stores the diagonal first in each row of a square matrix; the ABI
  // wants ascending columns.  Copies once into CSR, uploads, frees.
  template <class SparseMatrixType>
  void set_matrix(int slot, const SparseMatrixType &M) {
    const int64_t nrows = (int64_t)M.m();
    std::vector<int64_t> rp(nrows + 1, 0);
    std::vector<int32_t> col;
    std::vector<double> val;
    col.reserve(M.n_nonzero_elements());
    val.reserve(M.n_nonzero_elements());
    std::vector<std::pair<int32_t, double>> row;
    for (int64_t r = 0; r < nrows; ++r) {
      row.clear();
      for (auto it = M.begin(r); it != M.end(r); ++it) row.emplace_back((int32_t)it->column(), it->value());
      std::sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
      for (const auto &e : row) {
        col.push_back(e.first);
        val.push_back(e.second);
      }
      rp[r + 1] = (int64_t)col.size();
    }
    check(alfd_set_matrix(ctx_, slot, nrows, (int64_t)M.n(), rp.data(), col.data(), val.data()));
  }

  // Renumbering of the block-0 unknowns (velocity / background space) from one support point per unknown
  // (DoFTools::map_dofs_to_support_points restricted to that block).  The reference numbers its DoFs with
  // Cuthill-McKee, then block-wise (stokes_immersed_boundary.cc:533-541); the batch-major SpMV wants the rows of a
  // mesh brick to read a compact window of x.  This call (BEFORE any set_matrix / set_prolongator) hands the points to
  // alfd_set_numbering_from_points: the library fixes a permutation -- lexicographic order of the points, components
  // of a node together -- and the brick row blocks of A, permutes what is uploaded afterwards and translates every
  // vector that crosses the ABI on the device.  The caller keeps its numbering; nothing is permuted here.
  template <class PointContainer>
  void set_numbering_from_support_points(const PointContainer &points, int dim, const int32_t brick[3] = nullptr) {
    const int64_t n = (int64_t)points.size();
    std::vector<double> xyz((size_t)n * dim);
    int64_t i = 0;
    for (const auto &p : points) {
      for (int d = 0; d < dim; ++d) xyz[(size_t)i * dim + d] = p[d];
      ++i;
    }
    check(alfd_set_numbering_from_points(ctx_, n, dim, xyz.data(), brick));
  }
  bool renumbered() const {
    int64_t n = 0;
    check(alfd_get_numbering(ctx_, nullptr, 0, &n));
    return n > 0;
  }

  // CSR prolongator of a multigrid level (alfd_set_prolongator_block), e.g. from MGTransferPrebuilt or
  // FETools::get_interpolation_matrix.  block = 1: the hierarchy of the immersed block A22 of elliptic_interface.cc
  // (amg_prec_A22, :841-851).
  template <class SparseMatrixType>
  void set_prolongator(int level, const SparseMatrixType &P, int block = 0) {
    const int64_t nrows = (int64_t)P.m();
    std::vector<int64_t> rp(nrows + 1, 0);
    std::vector<int32_t> col;
    std::vector<double> val;
    std::vector<std::pair<int32_t, double>> row;
    for (int64_t r = 0; r < nrows; ++r) {
      row.clear();
      for (auto it = P.begin(r); it != P.end(r); ++it) row.emplace_back((int32_t)it->column(), it->value());
      std::sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
      for (const auto &e : row) {
        col.push_back(e.first);
        val.push_back(e.second);
      }
      rp[r + 1] = (int64_t)col.size();
    }
    check(alfd_set_prolongator_block(ctx_, block, level, nrows, (int64_t)P.n(), rp.data(), col.data(), val.data()));
  }

  template <class VectorType>
  void set_diag(int slot, const VectorType &d) {
    check(alfd_set_diag(ctx_, slot, (int64_t)d.size(), &*d.begin()));
  }

  // Row blocks of the SpMV on `slot` (alfd_set_row_blocks) from one support point per row, e.g.
  //   std::map<types::global_dof_index, Point<dim>> sp;  DoFTools::map_dofs_to_support_points(mapping, dh, sp);
  // restricted to the velocity block.  Call before set_matrix(slot, ...).  A block stages one window of x
  // in LDS: spatially compact blocks (recursive coordinate bisection here) keep that window a third of
  // what a run of consecutive DoF indices needs.  Does not change any result.
  template <class PointContainer>
  void set_row_blocks_from_support_points(int slot, const PointContainer &points, int dim, int max_rows = 192) {
    const int64_t n = (int64_t)points.size();
    std::vector<double> xyz((size_t)n * dim);
    int64_t i = 0;
    for (const auto &p : points) {
      for (int d = 0; d < dim; ++d) xyz[(size_t)i * dim + d] = p[d];
      ++i;
    }
    std::vector<int64_t> ptr((size_t)n + 1);
    std::vector<int32_t> rows((size_t)n);
    int64_t nb = 0;
    check(alfd_host_row_blocks_from_points(n, dim, xyz.data(), max_rows, &nb, ptr.data(), rows.data()));
    check(alfd_set_row_blocks(ctx_, slot, nb, ptr.data(), rows.data()));
  }

  // Aggregates of the multilevel inner preconditioner (ALFD_PREC_MULTILEVEL; replaces the ML
  // aggregation of utilities.h:304-317).  weights may be empty (constant modes).
  void set_aggregates(int level, const std::vector<int32_t> &agg, int64_t n_coarse,
                      const std::vector<double> &weights = {}) {
    check(alfd_set_aggregates(ctx_, level, (int64_t)agg.size(), agg.data(), weights.empty() ? nullptr : weights.data(),
                              n_coarse));
  }
  // Smoothed-aggregation hierarchy built by the library from the uploaded operators (ML's algorithm,
  // utilities.h:304-317; alfd_build_smoothed_aggregation): after set_matrix / configure, before setup.
  // Returns the number of levels; omega (optional) receives the damping of every level.  drop_tolerance /
  // max_row_entries other than 0 truncate every row of the prolongators on the device
  // (alfd_build_smoothed_aggregation_truncated: e.g. 0, 4 keeps the iteration counts at about one eighth of the entries).
  // block = 1: the hierarchy of the immersed block, from (A2, M, W^-1, gamma2) (alfd_build_smoothed_aggregation_block).
  int build_smoothed_aggregation(int32_t block_size = 1, double threshold = 0.02, int32_t max_aggregate_nodes = 8,
                                 double damping = 4.0 / 3.0, int64_t min_coarse = 600, int32_t max_levels = 7,
                                 std::vector<double> *omega = nullptr, double drop_tolerance = 0.0,
                                 int32_t max_row_entries = 0, int block = 0) {
    int32_t levels = 0;
    std::vector<double> w(ALFD_MAX_LEVELS, 0.0);
    if (block != 0)
      check(alfd_build_smoothed_aggregation_block(ctx_, block, block_size, threshold, max_aggregate_nodes, damping,
                                                  drop_tolerance, max_row_entries, min_coarse, max_levels, &levels,
                                                  w.data()));
    else if (drop_tolerance == 0.0 && max_row_entries == 0)
      check(alfd_build_smoothed_aggregation(ctx_, block_size, threshold, max_aggregate_nodes, damping, min_coarse,
                                            max_levels, &levels, w.data()));
    else
      check(alfd_build_smoothed_aggregation_truncated(ctx_, block_size, threshold, max_aggregate_nodes, damping,
                                                      drop_tolerance, max_row_entries, min_coarse, max_levels, &levels,
                                                      w.data()));
    if (omega) omega->assign(w.begin(), w.begin() + levels);
    return levels;
  }
  // Geometric multigrid hierarchy built by the library from one support point per unknown of the block
  // (alfd_build_geometric_from_points; the preconditioner the benchmark measures): after set_matrix, before setup.
  //   std::map<types::global_dof_index, Point<dim>> sp;  DoFTools::map_dofs_to_support_points(mapping, dh, sp);
  // restricted to the block, in the caller's numbering (also under set_numbering_from_support_points).  constrained:
  // one flag per unknown (AffineConstraints::is_constrained, Dirichlet rows included); empty = the rows of the uploaded
  // A that hold nothing but their diagonal, which is what condense() leaves of them.  base: cells per axis of the
  // uniform grid before local refinement (`Initial refinement`), needed when hanging nodes exist; empty on a uniform
  // mesh.  block = 1: the immersed space (rows of A2), no constraints.  Returns the number of levels.
  template <class PointContainer>
  int build_geometric_hierarchy_from_support_points(const PointContainer &points, int dim,
                                                    const std::vector<uint8_t> &constrained = {},
                                                    const std::vector<int32_t> &base = {}, int64_t min_coarse = 400,
                                                    int32_t max_levels = 7, int block = 0) {
    const int64_t n = (int64_t)points.size();
    std::vector<double> xyz((size_t)n * dim);
    int64_t i = 0;
    for (const auto &p : points) {
      for (int d = 0; d < dim; ++d) xyz[(size_t)i * dim + d] = p[d];
      ++i;
    }
    if (!constrained.empty() && (int64_t)constrained.size() != n) check(ALFD_E_INVALID);
    if (!base.empty() && (int)base.size() != dim) check(ALFD_E_INVALID);
    int32_t levels = 0;
    check(alfd_build_geometric_from_points(ctx_, block, n, dim, xyz.data(), nullptr,
                                           constrained.empty() ? nullptr : constrained.data(),
                                           base.empty() ? nullptr : base.data(), min_coarse, max_levels, &levels, nullptr));
    return levels;
  }
  // `Use diagonal inverse = false` / `Diagonal mass immersed = false` (immersed_laplace.cc:859-877,
  // stokes...:979-985, elliptic_interface.cc:713-737): the exact W^-1 = (M^-1)^2 (mode
  // ALFD_W_MASS_INV_SQUARED) or M^-1 (ALFD_W_MASS_INV) from the immersed mass matrix; applied to the
  // config passed to configure() afterwards.
  template <class SparseMatrixType>
  void set_w_inverse(int mode, const SparseMatrixType &mass_matrix) {
    set_matrix(ALFD_M, mass_matrix);
    w_inverse_ = mode;
  }
  // Single-precision operator values inside the inner preconditioner (alfd_set_preconditioner_values; alfd.h has the
  // contract and the caveat): ALFD_PREC_VALUES_FP32 before set_matrix(ALFD_A, ...) or after it, before setup().  For a
  // matrix with general values (locally refined meshes, variable coefficients); dictionary-coded operators ignore it.
  void set_preconditioner_values(int kind) { check(alfd_set_preconditioner_values(ctx_, kind)); }
  // multi-GPU: one System per rank (alfd.h: alfd_comm_init / alfd_set_partition), before any set_matrix
  void comm_init(int rank, int nranks, const void *unique_id, size_t bytes) {
    check(alfd_comm_init(ctx_, rank, nranks, unique_id, bytes));
  }
  void set_partition(const std::vector<std::vector<int64_t>> &offsets) {
    std::vector<const int64_t *> p;
    for (const auto &o : offsets) p.push_back(o.data());
    check(alfd_set_partition(ctx_, (int)p.size(), p.data()));
  }

  void configure(const alfd_config &cfg_in) {
    alfd_config cfg = cfg_in;
    if (w_inverse_ >= 0) cfg.w_inverse = w_inverse_;
    cfg_ = cfg;
    check(alfd_configure(ctx_, &cfg));
  }
  void setup() { check(alfd_setup(ctx_)); }
  // The immersed body moved, the background mesh did not: the new coupling matrix and W^-1 diagonal, then
  // alfd_setup_coupling, which redoes what depends on them and keeps A, the level operators and the transfers of the
  // last setup() (same results as uploading everything into a new System and calling setup(); alfd.h has the contract).
  // A new gamma goes through configure() before this call.  Throws Error with ALFD_E_INVALID / ALFD_E_UNSUPPORTED
  // where only setup() will do (another operator changed, partitioned System, aggregates, rational variant).
  // C: the library derives it from Ct again only while nobody has uploaded slot ALFD_C (the usual case: the call sites
  // upload ALFD_CT alone).  A caller who once called set_matrix(ALFD_C, ...) owns that slot and must upload the new C
  // the same way BEFORE this call, or the old C meets the new Ct.
  template <class SparseMatrixType, class VectorType>
  void update_coupling(const SparseMatrixType &Ct, const VectorType &invW) {
    set_matrix(ALFD_CT, Ct);       // re-derives C unless slot ALFD_C was uploaded explicitly (see above)
    set_diag(ALFD_INVW, invW);
    check(alfd_setup_coupling(ctx_));
  }
  // what the last setup() / update_coupling() ran: indexed by alfd_setup_count
  std::vector<int64_t> setup_counts() const {
    std::vector<int64_t> k(ALFD_SC_NCOUNTS, 0);
    check(alfd_get_setup_counts(ctx_, k.data()));
    return k;
  }
  const alfd_config &config() const { return cfg_; }
  alfd_ctx_t handle() const { return ctx_; }

  // f += gamma Ct invW g  (stokes...:1012-1018)
  template <class BlockVectorType>
  void augment_rhs(BlockVectorType &rhs) {
    std::vector<double *> p = ptrs(rhs);
    check(alfd_augment_rhs(ctx_, p.data()));
  }

  // The sanity block that ends the drivers' solve() (immersed_laplace.cc:987-1010, stokes...:1157-1180,
  // elliptic_interface.cc:973-1009).  estimate_condition_number_CCt replaces the SolverCG on C * Ct with
  // connect_condition_number_slot: .condition is the printed estimate, .converged == 0 the reference's
  // "does not have full rank" verdict (the reference throws there; here the caller decides).  Any other failure
  // throws like every call of this class.  control == nullptr: SolverControl(lambda.size(), 1e-12).
  alfd_spectrum estimate_condition_number_CCt(const alfd_control *control = nullptr) {
    alfd_spectrum s{};
    check(alfd_estimate_spectrum(ctx_, ALFD_SPECTRUM_CCT, control, &s));
    return s;
  }
  // linfty_norm of (last block row of AA) x - g: C u - M u2 for the elliptic variants
  // (difference_constraints, elliptic_interface.cc:973-984), C u - g otherwise.  Shared by all six
  // preconditioner classes through this holder.
  template <class BlockVectorType, class VectorType>
  double constraint_residual(const BlockVectorType &x, const VectorType &g) {
    std::vector<const double *> p = cptrs(x);
    double linf = 0;
    check(alfd_constraint_residual(ctx_, p.data(), &*g.begin(), &linf));
    return linf;
  }
  template <class BlockVectorType>
  double constraint_residual(const BlockVectorType &x) {   // g = 0
    std::vector<const double *> p = cptrs(x);
    double linf = 0;
    check(alfd_constraint_residual(ctx_, p.data(), nullptr, &linf));
    return linf;
  }

  // The block_operator AA (stokes...:1000-1003) as an object with vmult().
  class SystemOperator {
   public:
    explicit SystemOperator(System &s) : sys_(&s) {}
    template <class BlockVectorType>
    void vmult(BlockVectorType &dst, const BlockVectorType &src) const {
      std::vector<const double *> s = cptrs(src);
      std::vector<double *> d = ptrs(dst);
      sys_->check(alfd_system_apply(sys_->ctx_, s.data(), d.data()));
    }
    System *system() const { return sys_; }

   private:
    System *sys_;
  };
  SystemOperator system_operator() { return SystemOperator(*this); }

  void check(int rc, unsigned int step = 0, double res = 0) const {
    if (rc == ALFD_OK) return;
    const std::string msg = std::string(alfd_strerror(rc)) + ": " + alfd_last_error(ctx_);
    if (rc == ALFD_E_NO_CONVERGENCE_OUTER || rc == ALFD_E_NO_CONVERGENCE_INNER)
      throw NoConvergence(rc, msg, step, res);
    throw Error(rc, msg);
  }

  // block pointers for the ABI (the caller's numbering: a renumbering is the library's business)
  template <class BlockVectorType>
  static std::vector<double *> ptrs(BlockVectorType &v) {
    std::vector<double *> p(v.n_blocks());
    for (unsigned int b = 0; b < v.n_blocks(); ++b) p[b] = &*v.block(b).begin();
    return p;
  }
  template <class BlockVectorType>
  static std::vector<const double *> cptrs(const BlockVectorType &v) {
    std::vector<const double *> p(v.n_blocks());
    for (unsigned int b = 0; b < v.n_blocks(); ++b) p[b] = &*v.block(b).begin();
    return p;
  }

 private:
  alfd_ctx_t ctx_ = nullptr;
  alfd_config cfg_{};
  int w_inverse_ = -1;
  friend class SystemOperator;
};

// Common base of the preconditioner classes: depth-1 drop-in, deal.II keeps
// its own SolverFGMRES and calls vmult() once per outer iteration.
template <int Variant>
class ALPreconditioner {
 public:
  explicit ALPreconditioner(System &s) : sys_(&s) {
    if (s.config().variant != Variant) throw Error(ALFD_E_INVALID, "context configured for another variant");
  }
  // void vmult(BlockVector<double>& v, const BlockVector<double>& u) const
  template <class BlockVectorType>
  void vmult(BlockVectorType &v, const BlockVectorType &u) const {
    std::vector<const double *> s = System::cptrs(u);
    std::vector<double *> d = System::ptrs(v);
    alfd_result res{};
    sys_->check(alfd_precond_apply(sys_->handle(), s.data(), d.data(), &res));
    last_ = res;
  }
  const alfd_result &last_result() const { return last_; }
  System *system() const { return sys_; }

 private:
  System *sys_;
  mutable alfd_result last_{};
};

// augmented_lagrangian_preconditioner.h:14-42, :44-79, :81-110
using BlockPreconditionerAugmentedLagrangian = ALPreconditioner<ALFD_AL2>;
using BlockPreconditionerAugmentedLagrangianStokes = ALPreconditioner<ALFD_AL_STOKES>;
using BlockPreconditionerAugmentedLagrangianDiagonal = ALPreconditioner<ALFD_AL_STOKES_DIAG>;

// rational_preconditioner.h:12-99 (used with SolverMinRes, immersed_laplace.cc:625-631)
using RationalPreconditioner = ALPreconditioner<ALFD_RATIONAL>;
// augmented_lagrangian_preconditioner.h:115-164 and :168-238 live in this namespace in the reference
namespace EllipticInterfacePreconditioners {
using BlockTriangularALPreconditioner = ALPreconditioner<ALFD_AL_ELL_IDEAL>;
using BlockTriangularALPreconditionerModified = ALPreconditioner<ALFD_AL_ELL_MODIFIED>;
}  // namespace EllipticInterfacePreconditioners

// Depth-2 drop-ins for SolverFGMRES<BlockVector<double>> (stokes...:1067-1074,
// elliptic_interface.cc:862-906) and SolverMinRes<BlockVector<double>> (immersed_laplace.cc:629-631,
// stokes...:1057-1064): the whole solve runs on the GPU; the stop rule is alfd_config::outer and the
// Krylov method alfd_config::outer_solver, which must match the class used.
template <class BlockVectorType, int OuterSolver>
class GpuKrylovSolver {
 public:
  explicit GpuKrylovSolver(System &s) : sys_(&s) {
    if (s.config().outer_solver != OuterSolver)
      throw Error(ALFD_E_INVALID, "alfd_config::outer_solver does not match this solver class");
  }
  template <class MatrixType, class PreconditionerType>
  void solve(const MatrixType &A, BlockVectorType &x, const BlockVectorType &b, const PreconditionerType &P) {
    if (A.system() != sys_ || P.system() != sys_)
      throw Error(ALFD_E_INVALID, "operator, preconditioner and solver must share one System");
    std::vector<const double *> rhs = System::cptrs(b);
    std::vector<double *> sol = System::ptrs(x);   // x carries the initial guess
    const int rc = alfd_solve(sys_->handle(), rhs.data(), sol.data(), &last_);
    sys_->check(rc, (unsigned int)last_.outer_iterations, last_.last_residual);
  }
  unsigned int last_step() const { return (unsigned int)last_.outer_iterations; }   // SolverControl::last_step()
  double last_value() const { return last_.last_residual; }                        // SolverControl::last_value()
  const alfd_result &last_result() const { return last_; }

 private:
  System *sys_;
  alfd_result last_{};
};
template <class BlockVectorType>
using SolverFGMRES = GpuKrylovSolver<BlockVectorType, ALFD_OUTER_FGMRES>;
template <class BlockVectorType>
using SolverMinRes = GpuKrylovSolver<BlockVectorType, ALFD_OUTER_MINRES>;

}  // namespace dealii_adapter
}  // namespace alfd

#endif  // ALFD_DEALII_ADAPTER_HPP
