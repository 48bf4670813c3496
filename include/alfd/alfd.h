/* alfd.h -- C ABI of the MI355X-native augmented-Lagrangian FGMRES solver.
 *
 * This is the drop-in boundary.  The reference has no FFI:
 * its "operator API" is deal.II's duck-typed concept
 *     void vmult(BlockVector<double>& dst, const BlockVector<double>& src) const
 * implemented by the preconditioner classes of
 * augmented_lagrangian_preconditioner.h:28,62,95,130,186 and
 * rational_preconditioner.h:29, and consumed by
 *     SolverFGMRES<BlockVector<double>>::solve(AA, x, b, P)
 * (immersed_laplace.cc:943-944, stokes_immersed_boundary.cc:1073-1074,
 * elliptic_interface.cc:905-906, 947-948).  Each entry point below says which
 * of those it replaces.  include/alfd/dealii_adapter.hpp wraps this ABI back
 * into deal.II-shaped C++ classes; INTEGRATION.md shows the call-site diff.
 *
 * Conventions: every call returns an int status (never throws across the
 * ABI); all pointers at the ABI are HOST pointers -- device residency is
 * internal -- except the block vectors of the alfd_*_device calls, which are
 * the caller's DEVICE buffers; a context is single-threaded (like the reference, which runs
 * MPI_InitFinalize(argc, argv, 1)); several contexts may coexist.
 * All floating point data is fp64; column indices are int32, row starts int64
 * (deal.II: unsigned int columns, std::size_t rowstart).
 */
#ifndef ALFD_H
#define ALFD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALFD_ABI_VERSION 12
#define ALFD_MAX_BLOCKS 3

/* ------------------------------------------------------------------ status */
enum alfd_status {
  ALFD_OK = 0,
  ALFD_E_INVALID = 1,              /* bad argument / inconsistent sizes */
  ALFD_E_HIP = 2,                  /* a HIP runtime call failed */
  ALFD_E_NO_CONVERGENCE_OUTER = 3, /* SolverControl::NoConvergence from FGMRES */
  ALFD_E_NO_CONVERGENCE_INNER = 4, /* ... from an inner CG (stokes...:1020-1024) */
  ALFD_E_BREAKDOWN = 5,            /* NaN / non-positive curvature */
  ALFD_E_NOT_SETUP = 6,
  ALFD_E_COMM = 7,                 /* RCCL failure */
  ALFD_E_UNSUPPORTED = 8
};

/* ---------------------------------------------------------------- operators
 * Matrix slots (square brackets: which reference object it is).
 *   A    [stokes_matrix.block(0,0) stokes...:923 | stiffness_matrix immersed_laplace.cc:638
 *         | stiffness_matrix_bg elliptic...:680]
 *   BT   [stokes_matrix.block(0,1) stokes...:924]   B [block(1,0) :925]
 *   CT   [coupling_matrix, n_u x n_lambda, stokes...:926, immersed_laplace.cc:640]
 *   C    optional (single rank): when it has not been uploaded explicitly, every
 *        alfd_set_matrix(ALFD_CT) also stores the transpose as C (the reference applies
 *        transpose_operator(Ct), i.e. SparseMatrix::Tvmult -- stokes...:927), so a
 *        re-upload of CT with new values keeps C consistent.  Same for BT -> B.
 *        Multi-rank: the C and B rows of a rank must be uploaded explicitly.
 *   M    [mass_matrix_immersed stokes...:928 | mass_matrix_fg elliptic...:682]
 *   MP   [preconditioner_matrix.block(1,1) stokes...:929]
 *   A2   [stiffness_matrix_fg elliptic...:681]
 *   KIMM [embedded_stiffness_matrix immersed_laplace.cc:639; rational_preconditioner.h:15]
 */
enum alfd_matrix_slot {
  ALFD_A = 0,
  ALFD_BT = 1,
  ALFD_B = 2,
  ALFD_CT = 3,
  ALFD_C = 4,
  ALFD_M = 5,
  ALFD_MP = 6,
  ALFD_A2 = 7,
  ALFD_KIMM = 8,
  ALFD_NSLOTS = 9
};

/* Diagonal operators.
 *   INVW            W^-1 as a vector: 1/M_ii^2 (stokes...:976-978,
 *                   immersed_laplace.cc:866-869), 1/M_ii (operator form, :856-858),
 *                   1/(M^2)_ii (utilities.h:348-374, elliptic...:726)
 *   MP_LUMPED_INV   1/(Mp 1)_i, the preconditioner of the pressure-mass CG
 *                   (stokes...:946-957)
 */
enum alfd_diag_slot { ALFD_INVW = 0, ALFD_MP_LUMPED_INV = 1, ALFD_NDIAGS = 2 };

/* Which preconditioner class / system operator pair is configured. */
enum alfd_variant {
  ALFD_AL2 = 0,            /* BlockPreconditionerAugmentedLagrangian, ...preconditioner.h:14-42;
                              AA = [[Aug,Ct],[C,0]] immersed_laplace.cc:891-892 */
  ALFD_AL_STOKES = 1,      /* ...Stokes, :44-79; AA 3x3 stokes...:1000-1003 */
  ALFD_AL_STOKES_DIAG = 2, /* ...Diagonal, :81-110 (SPD, for MinRes) */
  ALFD_AL_ELL_IDEAL = 3,   /* BlockTriangularALPreconditioner, :115-164 */
  ALFD_AL_ELL_MODIFIED = 4,/* ...Modified, :168-238; system elliptic...:816-819 */
  ALFD_RATIONAL = 5        /* RationalPreconditioner, rational_preconditioner.h:12-99 */
};

/* deal.II stop rules [EXT], SURVEY.md 8(a)-12.
 *   ABS          SolverControl:        success if r <= tol; failure if k >= max_steps or NaN
 *   REDUCTION    ReductionControl:     also success if r < reduce * r0
 *   FIXED_ITERS  IterationNumberControl: success if k >= max_steps (or r <= tol)
 */
enum alfd_control_kind { ALFD_CTRL_ABS = 0, ALFD_CTRL_REDUCTION = 1, ALFD_CTRL_FIXED_ITERS = 2 };

typedef struct alfd_control {
  int32_t kind;
  int32_t max_steps;
  double tol;
  double reduce;
} alfd_control;

/* Preconditioner of the inner CG on the augmented block.  The reference uses
 * Trilinos ML (stokes...:1027-1045); north_star replaces it by a Jacobi /
 * Chebyshev sweep. */
enum alfd_inner_prec {
  ALFD_PREC_IDENTITY = 0,
  ALFD_PREC_JACOBI = 1,
  ALFD_PREC_CHEBYSHEV = 2,
  /* Aggregation multigrid V-cycle with Chebyshev smoothing on every level (the
   * GPU counterpart of the ML smoothed-aggregation AMG the reference initialises
   * in utilities.h:304-317).  Needs alfd_set_aggregates() / alfd_set_prolongator() for the augmented
   * (1,1) block.  The elliptic-interface variants take a second hierarchy, for the immersed block
   * A22 = A2 + gamma2 M invW M (alfd_set_prolongator_block(ctx, 1, ..), amg_prec_A22 of
   * elliptic_interface.cc:824-851): with it the A22 solve of AL_ELL_MODIFIED runs its own V-cycle and the
   * 2-block CG of AL_ELL_IDEAL the block diagonal of the two (elliptic_interface.cc:930-942); without it
   * A22 keeps the CHEBYSHEV sweep and AL_ELL_IDEAL answers ALFD_E_UNSUPPORTED at alfd_setup. */
  ALFD_PREC_MULTILEVEL = 3
};

/* Arnoldi orthogonalisation in FGMRES [EXT]: deal.II <= 9.5 modified
 * Gram-Schmidt; >= 9.6 classical Gram-Schmidt variants. */
enum alfd_orthogonalization { ALFD_ORTH_MGS = 0, ALFD_ORTH_CGS = 1, ALFD_ORTH_CGS2 = 2 };

/* Which deal.II release's SolverFGMRES loop is followed [EXT] (CMakeLists.txt:6 asks for 9.6.0, README.md:45
 * for 9.7): they differ in what last_step() counts.
 *   DEALII_96  >= 9.6: Arnoldi process with Givens rotations; the residual is checked and the counter
 *              incremented after EVERY Arnoldi step; the true residual of a restart is re-checked with the
 *              same counter.  Orthogonalisation: alfd_config::orthogonalization.
 *   DEALII_95  <= 9.5: modified Gram-Schmidt by add_and_dot; within a cycle the projected least-squares
 *              problem is solved with the FIRST j columns after the (j+1)-th Arnoldi vector was built
 *              (no check, no increment at j = 0), so a cycle of m preconditioner applications counts
 *              m - 1 steps and uses m - 1 of its m search directions.  Needs restart >= 2. */
enum alfd_fgmres_flavour { ALFD_FGMRES_DEALII_96 = 0, ALFD_FGMRES_DEALII_95 = 1 };

/* Outer Krylov method: SolverFGMRES (stokes...:1067) or SolverMinRes
 * (stokes...:1057-1064 with the diagonal SPD preconditioner; immersed_laplace.cc:629-631
 * with the rational preconditioner).  MinRes needs a symmetric system and an SPD
 * preconditioner, i.e. ALFD_AL_STOKES_DIAG or ALFD_RATIONAL. */
enum alfd_outer_solver { ALFD_OUTER_FGMRES = 0, ALFD_OUTER_MINRES = 1 };

/* What to do when an inner CG hits max_steps: the reference throws
 * SolverControl::NoConvergence (THROW); ACCEPT keeps the last iterate. */
enum alfd_inner_failure_policy { ALFD_INNER_THROW = 0, ALFD_INNER_ACCEPT = 1 };

/* The weight W^-1 of the AL term gamma Ct W^-1 C.  DIAGONAL: the caller's vector
 * (ALFD_INVW: 1/M_ii^2, or 1/M_ii in operator form) -- `Use diagonal inverse = true`.
 * MASS_INV_SQUARED / MASS_INV: the exact (M^-1)^2 / M^-1 of the reference's
 * `Use diagonal inverse = false` branch (immersed_laplace.cc:866-877, stokes...:979-985,
 * elliptic_interface.cc:713-737; UMFPACK there): every application runs Jacobi-preconditioned CG on the immersed mass
 * matrix (slot ALFD_M) to alfd_config::mass.  The inner preconditioner (Jacobi /
 * Chebyshev / multilevel) keeps using the diagonal weight, as the reference builds its
 * AMG from the diagonal form in either case (utilities.h:218-331). */
enum alfd_w_inverse { ALFD_W_DIAGONAL = 0, ALFD_W_MASS_INV_SQUARED = 1, ALFD_W_MASS_INV = 2 };

typedef struct alfd_config {
  int32_t variant;            /* enum alfd_variant */
  int32_t restart;            /* FGMRES max_basis_size: 30 default, 50 elliptic...:863 */
  int32_t orthogonalization;  /* enum alfd_orthogonalization */
  int32_t grad_div_in_A;      /* 1: A already holds gamma_gd (div,div) (stokes...:991-993).  0 (`Grad-div
                               * stabilization = false`, ALFD_AL_STOKES / _DIAG): A is the 2 eps:eps form and
                               * Aug = A + gamma Ct invW C + gamma_gd Bt Mp^-1 B (stokes...:991-995); every exact
                               * application of Aug (outer system, inner CG) runs a nested lumped-Jacobi CG on Mp to
                               * mp_inner, the inner preconditioner sees Mp^-1 replaced by ALFD_MP_LUMPED_INV.  Inner
                               * preconditioner identity (the reference's), Jacobi or Chebyshev; multilevel is refused
                               * (ALFD_E_UNSUPPORTED), as the reference throws there. */
  double gamma;               /* AL parameter (gamma_1 for elliptic) */
  double gamma_grad_div;      /* stokes...:987 */
  double gamma2;              /* gamma_2, elliptic...:751-752 */
  alfd_control outer;         /* outer_solver_control, stokes...:385-389 */
  alfd_control inner;         /* control_lagrangian, stokes...:1020-1023 */
  alfd_control mp_inner;      /* control_mass(100, 1e-6), stokes...:934 */
  int32_t inner_prec;         /* enum alfd_inner_prec */
  int32_t cheb_degree;        /* polynomial degree k >= 1 */
  int32_t cheb_power_its;     /* power iterations for lambda_max(D^-1 Aug) */
  int32_t on_inner_failure;   /* enum alfd_inner_failure_policy */
  double cheb_eig_ratio;      /* lambda_min = lambda_max / ratio */
  double cheb_safety;         /* lambda_max *= safety (deal.II uses 1.2) */
  int32_t log_level;          /* 0 silent; 1 result lines; 2 per-iteration "Check" lines */
  int32_t outer_solver;       /* enum alfd_outer_solver */
  /* ALFD_RATIONAL only (rational_preconditioner.h): */
  double rho_bound;           /* ||A_Gamma||_inf / min_i M_ii, immersed_laplace.cc:609-614 */
  alfd_control rational;      /* SolverControl(2000, 1e-14) of the 21 immersed solves, :34 */
  /* ALFD_PREC_MULTILEVEL only (ML: smoother_sweeps = 2, utilities.h:312): */
  int32_t ml_smooth_degree;   /* Chebyshev degree of the pre-/post-smoother on every level */
  int32_t ml_coarse_degree;   /* Chebyshev degree that stands in for the coarsest-level solve */
  double ml_smooth_ratio;     /* smoother targets [lambda_max/ratio, lambda_max] */
  double ml_coarse_ratio;     /* same for the coarsest level */
  /* "operator form" (immersed_laplace.cc:653-705, 880-882; `Use operator version = true`):
   * the caller has assembled the AL term into A (gamma/h * int_Gamma phi_i phi_j), so
   * Aug = A and only the preconditioner and the rhs augmentation use gamma and invW. */
  int32_t aug_assembled;
  int32_t w_inverse;          /* enum alfd_w_inverse */
  alfd_control mass;          /* CG on M for the exact W^-1: ReductionControl(1000, 1e-30, 1e-14) */
  int32_t fgmres_flavour;     /* enum alfd_fgmres_flavour */
  int32_t ml_smooth_degree_coarse; /* > 0: smoother degree on levels >= 1 (ml_smooth_degree then applies to level 0
                                      only: the fine operator is the expensive one, the coarse ones are nearly free) */
  /* ALFD_PREC_MULTILEVEL, round 3 (ML in the reference: smoothed prolongators, 2 smoother sweeps, KLU on
   * the coarsest level -- utilities.h:304-317):
   * ml_patch_degree > 0 wraps the V-cycle symmetrically into two corrections on the INTERFACE PATCH, the
   * rows S of the (1,1) block the coupling matrix touches (non-empty rows of Ct): z1 = E q(Aug_SS) E^T r,
   * z2 = z1 + V(r - Aug z1), z = z2 + E q(Aug_SS) E^T (r - Aug z2), q = Chebyshev polynomial of that degree
   * in D^-1 Aug_SS over [lambda_max / ml_patch_ratio, lambda_max].  The penalty gamma Ct W^-1 C is what a
   * multigrid cycle on the background mesh cannot resolve; it lives on S only (a few 10^4 rows at 10^7 DoF).
   * ml_coarse_direct > 0: when the coarsest level has at most that many unknowns its operator is inverted
   * explicitly (dense Cholesky at setup, one dense product per cycle) instead of the Chebyshev sweep; <= 0: off.
   * alfd_setup answers ALFD_E_INVALID for ml_patch_degree < 0 and, with a patch, for an ml_patch_ratio that is not
   * > 1 (the interval [lambda_max / ratio, lambda_max] would be empty), on one rank and on a partitioned context. */
  int32_t ml_patch_degree;
  int32_t ml_coarse_direct;
  double ml_patch_ratio;
} alfd_config;

typedef struct alfd_result {
  int32_t status;             /* enum alfd_status of the solve */
  int32_t outer_iterations;   /* SolverControl::last_step(), stokes...:1087 */
  double initial_residual;
  double last_residual;       /* SolverControl::last_value() */
  int64_t inner_iterations;   /* total CG iterations on the augmented block(s) */
  int64_t mp_iterations;      /* total CG iterations on Mp: the preconditioner's pressure block and, with
                               * grad_div_in_A = 0, the nested solves inside Aug */
  int32_t inner_failures;     /* inner solves that hit max_steps (ACCEPT policy) */
  int32_t precond_applications;
  double solve_seconds;       /* wall time inside alfd_solve, device-synchronised */
  double lambda_max;          /* Chebyshev: estimated lambda_max(D^-1 Aug) incl. safety */
  int64_t rational_iterations;/* total CG iterations of the 21 immersed solves (ALFD_RATIONAL) */
  int64_t mass_iterations;    /* total CG iterations on M (exact W^-1 modes) */
} alfd_result;

typedef struct alfd_ctx *alfd_ctx_t;

/* ---------------------------------------------------------------- lifecycle */
int alfd_abi_version(void);
const char *alfd_strerror(int status);
/* Last error message of a context (HIP error strings etc.). */
const char *alfd_last_error(alfd_ctx_t ctx);

/* One context = one GPU = one rank.  device_id is the HIP ordinal. */
int alfd_create(alfd_ctx_t *ctx, int device_id);
int alfd_destroy(alfd_ctx_t ctx);

/* ------------------------------------------------------- multi-GPU (RCCL)
 * One process per GPU.  Rank 0 obtains an id with alfd_comm_unique_id(), the
 * host launcher broadcasts the bytes (bench.py uses torch.distributed), every
 * rank calls alfd_comm_init().  Without it the context is single-rank.
 * Row partition: every block b of the block vectors is split in contiguous
 * row ranges; offsets[b] has nranks+1 entries (global prefix).  Must be set
 * before matrices are uploaded.  Matrices are then uploaded as LOCAL rows
 * with GLOBAL column indices. */
#define ALFD_UNIQUE_ID_BYTES 128
int alfd_comm_unique_id(void *id_out, size_t bytes);
int alfd_comm_init(alfd_ctx_t ctx, int rank, int nranks, const void *id, size_t bytes);
int alfd_set_partition(alfd_ctx_t ctx, int nblocks, const int64_t *const *offsets /*[nblocks][nranks+1]*/);

/* In-process rank group: N contexts of ONE process (one host thread per rank,
 * typically all on one GPU) exchange through device-to-device copies and a host
 * barrier instead of RCCL.  Test vehicle for the multi-rank path on a single-GPU
 * box; collective calls (alfd_set_matrix, alfd_setup, alfd_solve, ...) must
 * then be issued by all ranks concurrently, one thread each. */
typedef struct alfd_local_group alfd_local_group;
int alfd_local_group_create(int nranks, alfd_local_group **group);
int alfd_local_group_destroy(alfd_local_group *group);
int alfd_comm_init_local(alfd_ctx_t ctx, alfd_local_group *group, int rank);

/* Host-transport rank group: the collectives of the row-partitioned path (one all-gather of a few
 * scalars per reduction, one personalised neighbour exchange per halo) are handed to the caller as
 * HOST buffers -- the library copies device -> host, calls back, copies host -> device.  For
 * launchers whose ranks talk through MPI or gloo instead of RCCL (a deal.II program is an MPI
 * program), and the vehicle of the two-process GPU test.  Both callbacks return 0 on success.
 *   allgather: every rank contributes `bytes` bytes; recv holds nranks * bytes in rank order.
 *   alltoallv: rank r sends send[send_off[p] .. send_off[p+1]) (elements of elem_size bytes) to p and
 *              receives recv[recv_off[p] .. recv_off[p+1]) from p. */
typedef int (*alfd_host_allgather_fn)(void *user, const void *send, void *recv, size_t bytes);
typedef int (*alfd_host_alltoallv_fn)(void *user, const void *send, const int64_t *send_off, void *recv,
                                      const int64_t *recv_off, size_t elem_size);
int alfd_comm_init_host(alfd_ctx_t ctx, int rank, int nranks, alfd_host_allgather_fn allgather,
                        alfd_host_alltoallv_fn alltoallv, void *user);

/* Host-only halo plan of one row-partitioned matrix (no GPU, no communication):
 * rewrites the GLOBAL column indices of this rank's rows into the local index
 * space [owned columns | halo entries], lists the halo's global ids (sorted,
 * hence grouped by owning rank) and the receive prefix per owner
 * (recv_off[nranks+1]).  alfd_set_matrix() runs the same routine internally;
 * it is exported so that the partition logic can be tested on CPU ranks. */
int alfd_host_halo_plan(int64_t nnz, const int32_t *col, const int64_t *col_offsets /*[nranks+1]*/,
                        int nranks, int rank, int32_t *col_local /*[nnz]*/,
                        int32_t *halo_globals /*[halo_capacity] or NULL*/, int64_t halo_capacity,
                        int64_t *n_halo, int64_t *recv_off /*[nranks+1]*/);

/* ------------------------------------------------------------------- upload
 * Replaces: linear_operator(SparseMatrix) captures, stokes...:923-929.
 * Caller keeps ownership of host arrays; the library copies to HBM.
 * Rows in CSR order, columns ascending within a row (the adapter converts
 * deal.II's diagonal-first order).  nrows = local rows, ncols = GLOBAL columns. */
int alfd_set_matrix(alfd_ctx_t ctx, int slot, int64_t nrows, int64_t ncols, const int64_t *row_ptr,
                    const int32_t *col, const double *val);
/* Replaces: DiagonalMatrix<Vector<double>> (stokes...:954, 980). n = local length. */
int alfd_set_diag(alfd_ctx_t ctx, int slot, int64_t n, const double *d);
#define ALFD_MAX_LEVELS 8
/* Aggregates of the multilevel inner preconditioner (replaces ML's aggregation,
 * utilities.h:304-317): level l maps the n_fine unknowns of level l (level 0 = block 0,
 * the velocity / background space) onto n_coarse unknowns of level l+1.  agg[i] in
 * [0, n_coarse) or -1 (not represented on the coarse level, e.g. Dirichlet rows);
 * weight[i] (NULL = 1) is the prolongation entry P_{i,agg[i]} -- pass the near-nullspace
 * vector for non-constant modes.  Coarse operators are the Galerkin products
 * P^T (A + gamma Ct invW C) P, kept factored as (P^T A P) + gamma (C P)^T invW (C P). */
int alfd_set_aggregates(alfd_ctx_t ctx, int level, int64_t n_fine, const int32_t *agg, const double *weight,
                        int64_t n_coarse);
/* General prolongator of level l as a CSR matrix P (n_fine x n_coarse, columns ascending per row):
 * geometric multigrid transfers (e.g. the embedding of Q1 into Q2 on the same mesh followed by trilinear
 * interpolation between nested or non-nested grids -- what deal.II's MGTransfer / FETools interpolation
 * matrices hold), or a smoothed-aggregation prolongator as ML builds it (utilities.h:304-317).  Replaces
 * the aggregates of that level; rows without entries (Dirichlet / constrained unknowns) are not
 * represented on the coarse level.  Coarse operators are the Galerkin products, formed in two steps,
 * (A P) then P^T (A P), each output entry a sequential fma chain in CSR order.
 * Partitioned contexts: level 0 takes the rows of P this rank owns (n_fine = its rows, GLOBAL coarse columns)
 * together with alfd_set_aggregate_partition(ctx, 0, coarse offsets by rank) -- the coarse unknowns whose fine
 * support lies in a rank's rows + halo of A; the prolongators of the levels below are handed over whole on every
 * rank.  The fine level stays partitioned, levels >= 1 (and the interface patch) are replicated; the hierarchy
 * does not depend on the partition.  Aggregates and prolongators cannot be mixed there. */
int alfd_set_prolongator(alfd_ctx_t ctx, int level, int64_t n_fine, int64_t n_coarse, const int64_t *row_ptr,
                         const int32_t *col, const double *val);
/* Multi-rank: agg[] holds this rank's unknowns of level l and GLOBAL coarse ids; the coarse
 * unknowns of each level are numbered rank-major, coarse_offsets[nranks+1] gives the rank
 * ranges.  An aggregate must not span two ranks. */
int alfd_set_aggregate_partition(alfd_ctx_t ctx, int level, const int64_t *coarse_offsets);
/* Algebraic aggregation for callers without grid information (a matrix replayed from an .alfd
 * file, a locally refined mesh with hanging-node rows): builds the aggregates of every level from
 * the uploaded slot A alone and stores them as alfd_set_aggregates would -- the counterpart of
 * ML's uncoupled aggregation (utilities.h:304-317: aggregation_threshold 0.02, one constant mode
 * per component).  Unknowns are node-major with block_size components per node; a node pair is
 * strongly coupled if max |a_ij| >= threshold * sqrt(d_I d_J); rows holding only their diagonal
 * (Dirichlet / constrained rows) are left out; aggregates hold at most max_aggregate_nodes nodes.
 * Coarsening stops at <= min_coarse unknowns or max_levels.  Deterministic (natural order).
 * Single rank.  alfd_get_aggregates returns a level (agg may be NULL to query the sizes), e.g. to
 * hand the same aggregates to another solver instance. */
int alfd_build_aggregates(alfd_ctx_t ctx, int32_t block_size, double threshold, int32_t max_aggregate_nodes,
                          int64_t min_coarse, int32_t max_levels, int32_t *levels_out);
int alfd_get_aggregates(alfd_ctx_t ctx, int level, int32_t *agg, int64_t capacity, int64_t *n_fine,
                        int64_t *n_coarse);
/* Host-only (no device, no context): ONE level of the same aggregation on a CSR matrix; agg[nrows]. */
int alfd_host_aggregate_level(int64_t nrows, const int64_t *row_ptr, const int32_t *col, const double *val,
                              int32_t block_size, double threshold, int32_t max_aggregate_nodes, int32_t *agg,
                              int64_t *n_coarse);
/* The two halves of alfd_host_aggregate_level, host-only (no device, no context); both calls together give its bits.
 * alfd_host_strength_graph: the node graph of one level.  Nodes are block_size consecutive rows; d[n_nodes] = max |a_ii|
 * over the node's rows, fixed[n_nodes] = 1 when the node's rows hold nothing but their diagonals (explicit zeros do not
 * count); node I lists, ascending, the nodes J != I that are not fixed, with weight w_IJ = max |a_ij| > 0 over the
 * bs x bs block and w_IJ >= threshold * sqrt(d_I d_J) (fixed nodes list nothing).  Two-call sizing: with nbr and
 * weight NULL the call returns *nnz (d, fixed, node_ptr[n_nodes + 1] may be NULL too), then capacity >= *nnz.
 * alfd_host_aggregate_graph: the three greedy passes in natural order on such a graph; agg[n_nodes * block_size]. */
int alfd_host_strength_graph(int64_t nrows, const int64_t *row_ptr, const int32_t *col, const double *val,
                             int32_t block_size, double threshold, double *d, int32_t *fixed, int64_t *node_ptr,
                             int32_t *nbr, double *weight, int64_t capacity, int64_t *nnz);
int alfd_host_aggregate_graph(int64_t n_nodes, const int32_t *fixed, const int64_t *node_ptr, const int32_t *nbr,
                              const double *weight, int32_t block_size, int32_t max_aggregate_nodes, int32_t *agg,
                              int64_t *n_coarse);
/* The same node graph from the RESIDENT rows of slot A, formed on the device (max, fabs, one product, one square root
 * and one comparison per edge: the bits of alfd_host_strength_graph), on single-rank and on row-partitioned contexts.
 * Partitioned contexts: collective, every rank calls with the same arguments; a rank forms the graph rows of its own
 * nodes from its rows of A (halo columns included), neighbours are GLOBAL node ids, and the only traffic is one
 * all-gather of d and of the fixed flags (12 bytes per node) plus one status word per phase -- A is not downloaded.
 * The offsets of block 0 in alfd_set_partition must be multiples of block_size (ALFD_E_INVALID on every rank
 * otherwise; the context stays usable).  A failure on one rank is returned by all of them: the ranks exchange a
 * status word after every local phase, so none is left waiting in a collective.  A node with more than 512 neighbour
 * nodes on any rank sends all ranks to the host routine on their own rows (same bits, *on_device = 0).
 * alfd_build_strength_graph keeps the rows of this rank's nodes (*n_nodes of them, *nnz edges) until the next call;
 * alfd_get_strength_graph copies them out: d / fixed [n_nodes], node_ptr [n_nodes + 1], nbr / weight [capacity >= nnz]
 * (any may be NULL).  Gathering the rows of all ranks in rank order and running alfd_host_aggregate_graph on them
 * gives the aggregates of the single-rank alfd_build_aggregates, whatever the partition: the first step of the
 * smoothed-aggregation builders below on a partitioned context.  (alfd_build_aggregates itself stays single-rank.) */
int alfd_build_strength_graph(alfd_ctx_t ctx, int32_t block_size, double threshold, int64_t *n_nodes, int64_t *nnz);
int alfd_get_strength_graph(alfd_ctx_t ctx, double *d, int32_t *fixed, int64_t *node_ptr, int32_t *nbr, double *weight,
                            int64_t capacity, int32_t *on_device);
/* Smoothed aggregation (the algorithm of ML in the reference, utilities.h:304-317) from the uploaded operators alone.
 * Per level l, from A_0 = A (slot A) and C_0 = Ct^T (slot CT):
 *   agg_l   = the aggregation of alfd_build_aggregates on A_l (block_size, threshold, max_aggregate_nodes);
 *   Aug_l   = A_l + gamma C_l^T W^-1 C_l when alfd_configure set an AL variant with w_inverse == ALFD_W_DIAGONAL,
 *             gamma != 0 and aug_assembled == 0 (slot CT and diag slot ALFD_INVW uploaded), else A_l alone;
 *   omega_l = damping / lambda, lambda = lambda_max(D^-1 Aug_l) from cheb_power_its steps of power iteration
 *             (the start vector of alfd_setup, no safety factor), D = diag(Aug_l); ML's default damping is 4/3;
 *   P_l     = P_tent - omega_l D^-1 Aug_l P_tent, P_tent the constant modes of agg_l (one per component), its pattern
 *             the structural union, built on the device (nothing is dropped by value here; ML, hypre and MueLu
 *             truncate the smoothed prolongator: alfd_build_smoothed_aggregation_truncated does);
 *   A_{l+1} = P_l^T A_l P_l, C_{l+1} = C_l P_l.
 * Coarsening stops at <= min_coarse unknowns or max_levels levels.  The levels are stored as alfd_set_prolongator
 * would store them (alfd_setup forms the Galerkin products again), the aggregates as alfd_set_aggregates
 * (alfd_get_aggregates returns them); earlier aggregates / prolongators are cleared.  omega_out (may be NULL) receives
 * omega_l for every built level (room for max_levels entries, ALFD_MAX_LEVELS - 1 when max_levels is out of range).
 * Deterministic, bit for bit.  ALFD_E_NOT_SETUP without slot A, ALFD_E_INVALID on bad arguments (damping <= 0 or not
 * finite, ...).  Canonical order: DESIGN.md section 4.
 * Row-partitioned contexts (alfd_comm_init*, alfd_set_partition; block 0): the call is COLLECTIVE -- every rank calls it
 * with the same arguments -- and builds the single-rank hierarchy of the same global operators bit for bit, whatever
 * the partition: aggregates, omega_l and every P_l.  Slot A holds this rank's rows (slots C / CT and W^-1 its rows of
 * C, Ct and W^-1 when the penalty term applies: on every rank or on none).
 *   partitioned: level 0.  alfd_get_prolongator(0) returns this rank's rows of P_0 with GLOBAL coarse ids,
 *     alfd_get_aggregates(0) this rank's slice; aggregates may hold nodes of several ranks.
 *   replicated: levels >= 1, stored whole on every rank; omega_out is the same on all ranks.
 *   chosen by the library: the coarse offsets of alfd_set_aggregate_partition(0, ...), the rank that forms each row of
 *     A_1: (n_coarse / block_size) * p / nranks * block_size for rank p.  Any contiguous split gives the same bits.
 *   over the wire per build: d and the fixed flags of the nodes and the rows of the node graph (alfd_build_strength_graph),
 *     the rows of C and W^-1, cheb_power_its all-gathers of one velocity vector (the norms of the power iteration are
 *     the one sequential sum over the whole vector on every rank), the remote rows of P_0 and A P_0 in the support of a
 *     rank's coarse unknowns, the rows of A_1 and C_1, and one status word after every rank-local phase.  A is not
 *     downloaded.  Levels >= 1 are built redundantly on every rank.
 * alfd_setup then runs the replicated path of alfd_set_prolongator (interface patch included); for a hierarchy built
 * here it fetches the whole fine support of a rank's coarse unknowns, so the halo condition of caller-supplied
 * prolongators does not apply (it still does once alfd_set_prolongator / alfd_set_aggregates replace a level).
 * A rank group without alfd_set_partition has no rows to build from: ALFD_E_UNSUPPORTED, as before.
 * The offsets of block 0 must be multiples of block_size: ALFD_E_INVALID on every rank otherwise.  A failure on one
 * rank is returned by all of them, and a row with more than 512 candidates on any rank sends all ranks to the host
 * routines (same bits).  The device product holds at most 1024 distinct columns per row of A P_l, P_l^T (A P_l) or
 * C P_l: a wider row sends that product to the host routine (same bits).  On a partitioned context the level-0 product
 * A_r P_0 of a rank's own rows is rank-local, so only the rank that holds the wide row forms it on the host while its
 * peers stay on the device, and every rank goes on to the next collective; the replicated products fall back on all
 * ranks alike.  The same holds at alfd_setup with CSR prolongators.  The context stays usable after an error. */
int alfd_build_smoothed_aggregation(alfd_ctx_t ctx, int32_t block_size, double threshold, int32_t max_aggregate_nodes,
                                    double damping, int64_t min_coarse, int32_t max_levels, int32_t *levels_out,
                                    double *omega_out);
/* The same hierarchy with every row of P_l truncated on the device before it is stored (the untruncated P_l exists
 * nowhere; allocations are sized by kept entries).  For a row i with g = agg_l[i] >= 0 and the entries (J, p_J) of the
 * untruncated row, drop_tolerance tau in [0, 1) and max_row_entries k >= 0 (0: no cap):
 *   m = max |p_J|;  K0 = {J : |p_J| >= tau m} U {g};
 *   if k > 0 and |K0| > k: K = {g} U the first k - 1 members of K0 \ {g} in the order (|p| descending, J ascending),
 *   else K = K0;
 *   per component c (= J mod block_size) with dropped entries D_c and kept ones: t = the sum of p_J over D_c, J
 *   ascending, is added to the kept entry of component c that comes first in that order (so the constant of every
 *   component that keeps an entry is still reproduced); a component that keeps nothing loses D_c;
 *   the row is K, J ascending.
 * omega_l comes from the same power iteration on the untruncated operator; A_{l+1} and C_{l+1} use the truncated P_l.
 * tau == 0 and k == 0 give alfd_build_smoothed_aggregation bit for bit.  Same contract and error codes; ALFD_E_INVALID
 * for tau < 0, tau >= 1, tau not finite or k < 0 also clears the aggregates / prolongators set earlier.
 * Deterministic, bit for bit (selection by counting rank, no ties left open).  Canonical order: DESIGN.md section 4. */
int alfd_build_smoothed_aggregation_truncated(alfd_ctx_t ctx, int32_t block_size, double threshold,
                                              int32_t max_aggregate_nodes, double damping, double drop_tolerance,
                                              int32_t max_row_entries, int64_t min_coarse, int32_t max_levels,
                                              int32_t *levels_out, double *omega_out);
/* The CSR prolongator of a level (built by alfd_build_smoothed_aggregation[_truncated] or set by alfd_set_prolongator):
 * row_ptr[n_fine + 1], col / val [capacity >= nnz].  NULL arrays query the sizes; ALFD_E_INVALID for a level
 * without a CSR prolongator. */
int alfd_get_prolongator(alfd_ctx_t ctx, int level, int64_t *row_ptr, int32_t *col, double *val, int64_t capacity,
                         int64_t *n_fine, int64_t *n_coarse, int64_t *nnz);
/* alfd_set_prolongator, alfd_build_smoothed_aggregation_truncated and alfd_get_prolongator for one of the two
 * hierarchies.  block 0: the augmented (1,1) block, exactly those calls.
 * block 1: the immersed space of the elliptic-interface variants, whose operator is A22 = A2 + gamma2 M invW M -- the
 * roles of (A, C, Ct, gamma) are taken by (A2, M, M, gamma2), n_fine of level 0 is the row count of slot A2, and
 * alfd_setup forms A2_{l+1} = P^T (A2_l P), M_{l+1} = M_l P with the same products, diagonals, power iterations and
 * (alfd_config::ml_coarse_direct) explicit coarsest inverse; the ml_* settings are shared by both hierarchies.  The
 * builder runs the smoothed aggregation above on (A2, M, invW, gamma2), so the immersed hierarchy needs no geometry
 * either (amg_prec_A22.initialize(matrix), elliptic_interface.cc:841-851); drop_tolerance = 0 and max_row_entries = 0
 * truncate nothing.  Block 1 takes CSR prolongators only (there is no alfd_set_aggregates for it), has no interface patch (M touches
 * every row) and is single-rank: ALFD_E_UNSUPPORTED on a partitioned context (block 0 of the builder is collective there,
 * see alfd_build_smoothed_aggregation), ALFD_E_INVALID for another block, for
 * the builder without slot A2, and at alfd_setup for a block-1 hierarchy on a variant without A2 or with sizes that
 * do not match.  alfd_clear_hierarchy forgets what was set or built for a block (the next alfd_setup runs without). */
int alfd_set_prolongator_block(alfd_ctx_t ctx, int block, int level, int64_t n_fine, int64_t n_coarse,
                               const int64_t *row_ptr, const int32_t *col, const double *val);
int alfd_build_smoothed_aggregation_block(alfd_ctx_t ctx, int block, int32_t block_size, double threshold,
                                          int32_t max_aggregate_nodes, double damping, double drop_tolerance,
                                          int32_t max_row_entries, int64_t min_coarse, int32_t max_levels,
                                          int32_t *levels_out, double *omega_out);
int alfd_get_prolongator_block(alfd_ctx_t ctx, int block, int level, int64_t *row_ptr, int32_t *col, double *val,
                               int64_t capacity, int64_t *n_fine, int64_t *n_coarse, int64_t *nnz);
/* The aggregates the builder formed for a level of a block (agg[n_fine], -1: empty row), as alfd_get_aggregates does
 * for block 0; NULL agg queries the sizes.  ALFD_E_INVALID for a level the builder did not form. */
int alfd_get_aggregates_block(alfd_ctx_t ctx, int block, int level, int32_t *agg, int64_t capacity, int64_t *n_fine,
                              int64_t *n_coarse);
int alfd_clear_hierarchy(alfd_ctx_t ctx, int block);
/* Host-only (no device, no context): ONE level's smoothed prolongator with the arithmetic of
 * alfd_build_smoothed_aggregation, from the square CSR A (nrows), optionally Ct (nrows x n_mult, ct_row_ptr == NULL:
 * no penalty term) with the W^-1 diagonal w_inv[n_mult] and gamma, the aggregates agg[nrows] (-1: empty row),
 * n_coarse and omega.  Two calls: p_col == p_val == NULL returns *nnz (and p_row_ptr[nrows + 1] if given), then
 * arrays with capacity >= nnz. */
int alfd_host_smoothed_prolongator(int64_t nrows, const int64_t *row_ptr, const int32_t *col, const double *val,
                                   int64_t n_mult, const int64_t *ct_row_ptr, const int32_t *ct_col, const double *ct_val,
                                   const double *w_inv, double gamma, const int32_t *agg, int64_t n_coarse, double omega,
                                   int64_t *p_row_ptr, int32_t *p_col, double *p_val, int64_t capacity, int64_t *nnz);
/* Host-only (no device, no context): the truncation rule of alfd_build_smoothed_aggregation_truncated applied to a CSR
 * prolongator P (nrows x n_coarse, rows sorted, e.g. from alfd_host_smoothed_prolongator) with the aggregates
 * agg[nrows] (-1: the row comes out empty), same bits as the device.  Two calls as alfd_host_smoothed_prolongator:
 * out_col == out_val == NULL returns *nnz (and out_row_ptr[nrows + 1] if given), then arrays with capacity >= nnz.
 * ALFD_E_INVALID: drop_tolerance < 0, >= 1 or not finite, max_row_entries < 0, block_size < 1, a column outside
 * [0, n_coarse), a row not strictly ascending, agg out of range, a row with agg[i] >= 0 without the column agg[i]. */
int alfd_host_truncate_prolongator(int64_t nrows, int64_t n_coarse, const int64_t *p_row_ptr, const int32_t *p_col,
                                   const double *p_val, const int32_t *agg, int32_t block_size, double drop_tolerance,
                                   int32_t max_row_entries, int64_t *out_row_ptr, int32_t *out_col, double *out_val,
                                   int64_t capacity, int64_t *nnz);
/* Host-only (no device, no context): the sparse product out = A P of the multigrid setup (A P_l, P_l^T (A P_l), C P_l),
 * A a_nrows x a_ncols and P a_ncols x p_ncols in CSR, rows in any order.  Canonical order: entry
 * (i, J) is ONE sequential chain acc = fma(a_ik, p_kJ, acc) from 0 over the entries k of row i of A in CSR order and
 * the entries of row col_k of P in CSR order; the pattern is structural (stored zeros count, an entry that cancels
 * stays, as +0.0) and the rows come out with ascending columns.  Two calls as alfd_host_smoothed_prolongator:
 * out_col == out_val == NULL returns *nnz (and out_row_ptr[a_nrows + 1] if given), then arrays with capacity >= nnz.
 * a_nrows == 0 and operands without entries are valid.  ALFD_E_INVALID: a negative size, a row pointer that does not
 * start at 0 or decreases, a column outside [0, a_ncols) / [0, p_ncols), nnz == NULL, capacity < nnz. */
int alfd_host_sparse_product(int64_t a_nrows, int64_t a_ncols, const int64_t *a_row_ptr, const int32_t *a_col,
                             const double *a_val, int64_t p_ncols, const int64_t *p_row_ptr, const int32_t *p_col,
                             const double *p_val, int64_t *out_row_ptr, int32_t *out_col, double *out_val,
                             int64_t capacity, int64_t *nnz);
/* The same product on the context's device, whatever its size: both operands are uploaded and spgemm_rows_kernel forms
 * the rows (one 64-lane workgroup per row), with the bits of alfd_host_sparse_product.  The kernel holds at most 1024
 * distinct columns per product row; when ANY row has more, the whole product is formed by the host routine instead
 * (same bits) and *on_device (may be NULL) is 0, else 1.  This is the product alfd_setup and the builders run for
 * operators with more than 200 000 entries (tunable "ml_gpu_galerkin"); single-rank, not collective.  Same two-call
 * protocol (each call forms the product) and the same ALFD_E_INVALID cases. */
int alfd_sparse_product(alfd_ctx_t ctx, int64_t a_nrows, int64_t a_ncols, const int64_t *a_row_ptr, const int32_t *a_col,
                        const double *a_val, int64_t p_ncols, const int64_t *p_row_ptr, const int32_t *p_col,
                        const double *p_val, int64_t *out_row_ptr, int32_t *out_col, double *out_val, int64_t capacity,
                        int64_t *nnz, int32_t *on_device);
/* ONE level's smoothed prolongator from the caller's aggregates on the context's device, by the routines of
 * alfd_build_smoothed_aggregation[_truncated]: the arguments of alfd_host_smoothed_prolongator, then block_size,
 * drop_tolerance and max_row_entries of the truncation rule (0 and 0: nothing is truncated; the result then has the
 * bits of alfd_host_smoothed_prolongator, otherwise those of alfd_host_truncate_prolongator applied to it).  The
 * kernels hold at most 512 candidates (distinct aggregates of the row's columns, penalty columns and agg[i]) per row;
 * when ANY row has more, all rows and the truncation are formed by the host routines instead (same bits) and
 * *on_device (may be NULL) is 0, else 1.  Rows of A of any length stay on the device.  Single-rank, not collective;
 * the hierarchy stored in the context is not touched.  Same two-call protocol (each call forms the rows).
 * ALFD_E_INVALID as alfd_host_smoothed_prolongator (a zero diagonal in a row with an aggregate included), and for
 * block_size < 1, drop_tolerance < 0, >= 1 or not finite, max_row_entries < 0. */
int alfd_smoothed_prolongator(alfd_ctx_t ctx, int64_t nrows, const int64_t *row_ptr, const int32_t *col, const double *val,
                              int64_t n_mult, const int64_t *ct_row_ptr, const int32_t *ct_col, const double *ct_val,
                              const double *w_inv, double gamma, const int32_t *agg, int64_t n_coarse, double omega,
                              int32_t block_size, double drop_tolerance, int32_t max_row_entries, int64_t *p_row_ptr,
                              int32_t *p_col, double *p_val, int64_t capacity, int64_t *nnz, int32_t *on_device);
/* Geometric multigrid transfers from support points (DoFTools::map_dofs_to_support_points) and constraint flags: the
 * hierarchy of problems.tensor_prolongators / refined_prolongators / immersed_tensor_prolongators for callers that have
 * points, not the generator's parameters.  ONE rule, so that the results can be compared entry for entry.
 * Lattice.  Per axis d: lo, hi = smallest and largest coordinate; coordinates closer than 1e-9 (hi - lo) count as equal;
 *   delta_d = the smallest gap between distinct coordinates; m_d = round((hi - lo) / delta_d) cells; a point has the lattice
 *   index i_d = round((x_d - lo) / delta_d).  |x_d - lo - i_d delta_d| > 1e-6 delta_d or a non-finite coordinate:
 *   ALFD_E_INVALID (no lattice mesh).  An axis on which all points agree has m_d = 0, delta_d = 0.  The lattice is
 *   COMPLETE when every lattice node carries an unknown.
 * Components.  The unknowns that share a lattice node are its components: component[i] when given, else the rank of i
 *   among them by ascending index (node-major and component-wise block numberings alike).  Every occupied node carries
 *   exactly ncomp unknowns (1 <= ncomp <= 64), each component once, else ALFD_E_INVALID.
 * Level 0: the points onto the Q1 space of a base grid of base_d cells per axis.  Its unknowns are the interior nodes,
 *   lexicographic with x fastest, node-major, ncomp per node; with boundary_unknowns = 1 all base_d + 1 nodes per axis (the
 *   immersed spaces, which have no Dirichlet rows).  Per axis, in integers: num = i_d * base_d, j = num / m_d,
 *   rem = num % m_d; rem == 0 gives weight 1 on node j, else fr = (double)rem / (double)m_d with weight 1.0 - fr on j and
 *   fr on j + 1.  The entry is w_z * (w_y * w_x); entries onto nodes that are no unknowns are dropped (a weight is never
 *   zero); columns ascend within a row.  Rows with constrained[i] != 0 are empty, and with boundary_unknowns = 0 so are
 *   the rows on the lattice boundary (i_d == 0 or i_d == m_d on any axis).
 *   base == NULL needs a complete lattice and takes base_d = (m_d + 1) / 2: for Q2 points the Q1 space of the same mesh, for
 *   Q1 points the next coarser grid.  An incomplete lattice (a locally refined mesh) needs base from the caller, the cells
 *   of its uniform base grid ("Initial refinement"): ALFD_E_INVALID without.  base_d < 2 (< 1 with boundary unknowns) or
 *   base_d > m_d: ALFD_E_INVALID.
 * Levels below: cur_d cells to next_d = (cur_d + 1) / 2 cells by the same integer rule between the two node grids, the same
 *   unknowns on both sides.  While the last n_coarse > min_coarse and fewer than max_levels levels exist a level is added,
 *   provided every next_d >= 2 (interior unknowns) or every cur_d >= 2 (boundary unknowns: a direction down to one cell
 *   ends the hierarchy, level 0 included, so a (2, 1, 1) box gives no level at all).
 * Host-only (no device, no context):
 *   alfd_host_point_lattice     cells[dim] = m_d, lo[dim], delta[dim], index[n * dim] = i_d, *complete (any may be NULL).
 *   alfd_host_point_prolongator level 0 (n x *n_coarse) in the two-call protocol of alfd_host_smoothed_prolongator:
 *                               p_col == p_val == NULL returns *nnz, *n_coarse (and p_row_ptr[n + 1] if given), then
 *                               arrays with capacity >= nnz.  component / constrained / base may be NULL.
 *   alfd_host_grid_prolongator  one lower level between the grids of fine_cells[dim] and coarse_cells[dim] (any
 *                               1 <= coarse_d <= fine_d, 2 <= coarse_d with interior unknowns), same protocol; *n_fine and
 *                               *n_coarse are the unknowns of the two grids.
 *   alfd_host_point_hierarchy_cells
 *                               the level rule alone: from the lattice cells m_d, ncomp, base (NULL: (m_d + 1) / 2),
 *                               min_coarse and max_levels (as alfd_build_geometric_from_points takes them) the number
 *                               of levels and the cells of every level's coarse grid, cells_out[levels * dim] (room
 *                               for ALFD_MAX_LEVELS * dim; may be NULL).  Level 0 of alfd_host_point_prolongator, then
 *                               alfd_host_grid_prolongator between consecutive grids, are the levels the context
 *                               build stores. */
int alfd_host_point_lattice(int64_t n, int32_t dim, const double *points, int32_t *cells, double *lo, double *delta,
                            int32_t *index, int32_t *complete);
int alfd_host_point_prolongator(int64_t n, int32_t dim, const double *points, int32_t ncomp, const int32_t *component,
                                const uint8_t *constrained, const int32_t *base, int32_t boundary_unknowns,
                                int64_t *p_row_ptr, int32_t *p_col, double *p_val, int64_t capacity, int64_t *nnz,
                                int64_t *n_coarse);
int alfd_host_grid_prolongator(int32_t dim, int32_t ncomp, const int32_t *fine_cells, const int32_t *coarse_cells,
                               int32_t boundary_unknowns, int64_t *p_row_ptr, int32_t *p_col, double *p_val,
                               int64_t capacity, int64_t *n_fine, int64_t *n_coarse, int64_t *nnz);
int alfd_host_point_hierarchy_cells(int32_t dim, int32_t ncomp, const int32_t *lattice_cells, const int32_t *base,
                                    int32_t boundary_unknowns, int64_t min_coarse, int32_t max_levels, int32_t *levels_out,
                                    int32_t *cells_out);
/* The whole hierarchy of a block by that rule, stored as alfd_set_prolongator[_block] would store its levels
 * (alfd_get_prolongator[_block] returns them; alfd_setup and alfd_setup_coupling treat them as caller-supplied CSR
 * prolongators); the aggregates and prolongators the block had are cleared, as the smoothed-aggregation builders do.
 *   block 0: interior unknowns; n = the rows of slot A; constrained == NULL takes the rows of the RESIDENT slot A that
 *            hold nothing but their diagonal (explicit zeros do not count: the fixed flags of alfd_host_strength_graph) --
 *            Dirichlet and condensed hanging-node rows as the adapter uploads them.  Under alfd_set_numbering points,
 *            component and constrained are in the caller's numbering, like every level-0 input.
 *   block 1: boundary unknowns, no constraints (constrained must be NULL); n = the rows of slot A2.
 * ncomp is the number of unknowns on the first point's node.  min_coarse >= 1; max_levels outside 1 .. ALFD_MAX_LEVELS - 1
 * means ALFD_MAX_LEVELS - 1.  *levels_out (may be NULL) = the levels built (0 is possible on block 1, see the rule);
 * cells_out (may be NULL; room for ALFD_MAX_LEVELS * dim entries) = the cells of the lattice, then of every level's coarse
 * grid.  ALFD_E_UNSUPPORTED on a partitioned context, ALFD_E_NOT_SETUP without the slot, ALFD_E_INVALID for another block,
 * a bad size or argument and everything the rule refuses.  The levels are formed before the block is touched and the
 * inputs it had are handed back if storing one fails, so after any refusal the context stays usable and keeps the
 * hierarchy it had. */
int alfd_build_geometric_from_points(alfd_ctx_t ctx, int block, int64_t n, int32_t dim, const double *points,
                                     const int32_t *component, const uint8_t *constrained, const int32_t *base,
                                     int64_t min_coarse, int32_t max_levels, int32_t *levels_out, int32_t *cells_out);
int alfd_configure(alfd_ctx_t ctx, const alfd_config *cfg);
/* New stop rules for the following solves WITHOUT a new alfd_setup (alfd_configure invalidates the setup): the
 * reference's SolverControl objects are plain members that a caller may change between two solve() calls
 * (outer_solver_control stokes...:282, control_lagrangian :1020-1023, control_mass :934).  NULL keeps a rule. */
int alfd_set_controls(alfd_ctx_t ctx, const alfd_control *outer, const alfd_control *inner, const alfd_control *mp_inner);
void alfd_default_config(alfd_config *cfg, int variant);
/* Builds transposes, sparse-row views, diag(Aug), lambda_max, halo plans
 * (replaces the setup in stokes...:1027-1045 / utilities.h:112-331). */
int alfd_setup(alfd_ctx_t ctx);
/* Re-setup after a change of the coupling alone (a fictitious-domain run whose immersed body moves over a fixed
 * background mesh): redoes what depends on Ct / C, invW, M and the penalty weights and keeps what depends on A and the
 * transfer operators alone.
 *
 * Contract.  The context was set up by alfd_setup or by an earlier alfd_setup_coupling.  Since then the caller may have
 *   - uploaded any of the slots ALFD_CT, ALFD_C, ALFD_M and the diagonal ALFD_INVW again (same block sizes);
 *   - called alfd_configure with a config that differs from the one of the last setup in gamma and / or gamma2 only
 *     (stop rules go through alfd_set_controls as before).
 * After ALFD_OK the context is in the state alfd_setup produces on a fresh context with the same operators, prolongators
 * and config, bit for bit: solutions, residual histories, every iteration count, alfd_inner_prec_apply,
 * alfd_precond_apply, alfd_system_apply.  A call with nothing changed is valid and leaves the same bits; a context
 * updated many times does not grow (what is replaced is freed).
 *
 * Kept (neither recomputed, re-planned nor uploaded again): slot A and its plans; the level operators A_l (l >= 1); P_l
 * and R_l; everything of B, Bt, Mp; the level vectors; for the elliptic variants A2 and the A2_l of the block-1 hierarchy.
 * Recomputed, by the routines and in the order of alfd_setup: the diagonals and lambda_max of the inner operators; with an
 * upload of CT / C the products C_{l+1} = C_l P_l and their transposes (device product, host fallback); the diagonals and
 * lambda_max of every level; the whole interface patch (S may grow or shrink); the explicit coarsest inverse; the row
 * masks of the fused smoother; the compacted operators of alfd_estimate_spectrum (on its next call); the diagonal of the
 * mass solve (exact W^-1).  The block-1 hierarchy is touched only when M, ALFD_INVW or gamma2 changed, its M_l products
 * only after an upload of M.  An inner preconditioner other than multilevel recomputes its diagonal and lambda_max.
 *
 * FROZEN TRANSFERS: a hierarchy built by alfd_build_smoothed_aggregation[_truncated] counts as CSR prolongators.  The
 * update keeps the P that were built and does not rebuild them, although they were smoothed with the OLD coupling: the
 * result equals alfd_setup on a context that was handed those P through alfd_set_prolongator, not a new build.
 *
 * Refusals are decided before anything is modified; the context is then as before the call (not set up when something
 * was uploaded), and alfd_setup on it succeeds.
 *   ALFD_E_NOT_SETUP    never set up (or the last setup of either kind failed).
 *   ALFD_E_INVALID      with "needs alfd_setup" in alfd_last_error: another slot or diagonal was uploaded since the last
 *                       setup; a prolongator, aggregates or a row-block hint was set; a block size changed; the config
 *                       differs in any other field; aug_assembled = 1 (the coupling lives inside A).  Also, with
 *                       alfd_setup's own message, a gamma / gamma2 that alfd_setup refuses for the variant (modified
 *                       elliptic: gamma2 > 20 or within 0.1 of gamma; ideal elliptic: gamma != gamma2).
 *   ALFD_E_UNSUPPORTED  a partitioned context (the same answer on every rank, before any exchange); the rational
 *                       variant; a hierarchy given as aggregates (alfd_set_aggregates / alfd_build_aggregates), whose
 *                       level products run on the host from a fetched A.  These callers keep using alfd_setup.
 * A failure after the refusals (a HIP error, a coarsest operator that is not positive definite) leaves the context to
 * alfd_setup.  alfd_get_setup_seconds then reports the phases of this call; ALFD_SETUP_UPLOAD keeps its meaning. */
int alfd_setup_coupling(alfd_ctx_t ctx);
/* What the last alfd_setup or alfd_setup_coupling ran, counted rather than timed (one-rank contexts; the replicated
 * levels of a partitioned setup are not counted). */
enum alfd_setup_count {
  ALFD_SC_PRODUCTS_A = 0,        /* sparse products, device or host, with an A_l / A2_l operand, R (A P) included: 2 per
                                  * level, also where an aggregates level forms P^T A P in one pass */
  ALFD_SC_PRODUCTS_C = 1,        /* sparse products with a C_l / M_l operand: 1 per level (C_l P_l; the transpose that
                                  * gives Ct_{l+1}, formed as P^T Ct_l on an aggregates level, is not counted) */
  ALFD_SC_LEVEL_A_UPLOADS = 2,   /* plans + uploads of a level operator A_l / A2_l, l >= 1 */
  ALFD_SC_TRANSFER_UPLOADS = 3,  /* uploads of P_l, R_l */
  ALFD_SC_PATCH_BUILDS = 4,      /* interface patches built */
  ALFD_SC_POWER_ITERATIONS = 5,  /* power iterations for a lambda_max (each alfd_config::cheb_power_its steps) */
  ALFD_SC_NCOUNTS = 6
};
int alfd_get_setup_counts(alfd_ctx_t ctx, int64_t *counts /*[ALFD_SC_NCOUNTS]*/);

/* --------------------------------------------------------------- hot path
 * Depth 1. Replaces <Preconditioner>::vmult(dst, src)
 * (augmented_lagrangian_preconditioner.h:28-34, 62-70, 95-103, 130-156, 185-229).
 * src/dst: one host pointer per block (local rows). */
int alfd_precond_apply(alfd_ctx_t ctx, const double *const *src_blocks, double *const *dst_blocks,
                       alfd_result *res);
/* Replaces AA.vmult(dst, src): the block system operator (stokes...:1000-1003). */
int alfd_system_apply(alfd_ctx_t ctx, const double *const *src_blocks, double *const *dst_blocks);
/* Replaces the rhs augmentation f += gamma Ct invW g (stokes...:1012-1018,
 * immersed_laplace.cc:900-905): rhs_blocks[0] is updated in place from rhs_blocks[last]. */
int alfd_augment_rhs(alfd_ctx_t ctx, double *const *rhs_blocks);
/* Depth 2 (the measured path). Replaces
 * SolverFGMRES<BlockVector<double>>::solve(AA, x, b, P) (stokes...:1067-1074).
 * x_blocks: in = initial guess, out = solution. */
int alfd_solve(alfd_ctx_t ctx, const double *const *rhs_blocks, double *const *x_blocks,
               alfd_result *res);
/* (alfd_precond_apply, alfd_system_apply and alfd_augment_rhs stage their host vectors in buffers of
 * their own: a right-hand side / initial guess uploaded with alfd_upload_rhs stays intact, so the
 * depth-1 calls may be mixed with alfd_solve_resident.) */
/* Same solve with the vectors already resident in HBM (no PCIe in the timed
 * region): alfd_upload_rhs() then alfd_solve_resident() any number of times,
 * alfd_download_solution() at the end.
 * alfd_upload_rhs keeps x0_blocks (NULL: zero) as the initial guess next to the right-hand side.  EVERY
 * alfd_solve_resident starts from that uploaded guess again, not from the previous solution, so repeated calls
 * repeat the same solve; alfd_download_solution returns the solution of the last one.  An upload without
 * x0_blocks replaces an earlier guess by zero. */
int alfd_upload_rhs(alfd_ctx_t ctx, const double *const *rhs_blocks, const double *const *x0_blocks);
int alfd_solve_resident(alfd_ctx_t ctx, alfd_result *res);
int alfd_download_solution(alfd_ctx_t ctx, double *const *x_blocks);
/* ------------------------------------------------- device-resident vectors
 * The six vector calls above on the caller's GPU buffers: a right-hand side
 * assembled on the device, a time-stepping loop, an outer iteration that starts
 * each solve from the previous solution never cross PCIe.  The block tables
 * (rhs_blocks, x_blocks, ...) are HOST arrays of one DEVICE pointer per block,
 * each addressing this rank's rows of the block (n[b] doubles; 8-byte alignment
 * is enough, views such as t[1:] are fine).  `stream` is the caller's
 * hipStream_t (NULL: the null stream).
 *   Same computation.  One kernel launch packs the blocks into the library's
 *     padded vector, one unpacks them; in between runs
 *     the code of the host-pointer call, so the results are bit-identical to
 *     it on the same data.  alfd_solve_device = alfd_upload_rhs_device +
 *     alfd_solve_resident + alfd_download_solution_device; like alfd_solve it
 *     writes x also when the solve returns a no-convergence status.
 *     alfd_precond_apply_device, alfd_system_apply_device and
 *     alfd_augment_rhs_device use the staging of the depth-1 calls: a resident
 *     right-hand side / guess stays intact.
 *   Ordering.  The inputs are awaited ON THE DEVICE: whatever the caller has
 *     enqueued on `stream` before the call (producers of the inputs, earlier
 *     readers of the outputs) completes before the library touches a block;
 *     no host synchronisation is needed before the call.  The call itself is
 *     host-synchronous (the Krylov loops are stepped by the host): on return
 *     the outputs are complete and visible to every stream.  Work on OTHER
 *     streams that touches the blocks is the caller's to order.  The calls
 *     cannot be captured into a HIP graph.
 *   Validation, before anything is launched.  Every block with n[b] > 0 is
 *     looked up with hipPointerGetAttributes and must be device memory
 *     (hipMemoryTypeDevice) of the context's device: a host pointer, a null
 *     pointer, managed memory or memory of another device returns
 *     ALFD_E_INVALID with the block named in alfd_last_error; the runtime's
 *     error state is cleared and the context stays usable.  So does a block
 *     whose n[b] doubles do not end inside its allocation
 *     (hipMemGetAddressRange; where the runtime cannot tell the extent the
 *     block is taken as given, and inside a pooled allocation the check sees
 *     the pool).  A null block pointer is accepted for n[b] == 0 only (a rank
 *     without multiplier rows).  A null ctx, a null block table, a null res of
 *     alfd_solve_device: ALFD_E_INVALID; before alfd_setup: ALFD_E_NOT_SETUP;
 *     alfd_augment_rhs_device on ALFD_RATIONAL: ALFD_E_UNSUPPORTED, as the
 *     host call.
 *   Aliasing.  All inputs are packed before any output is written: dst may
 *     equal src, x blocks may alias rhs blocks, and the blocks may be views
 *     into one allocation.  The OUTPUT blocks of one call must not overlap
 *     each other.
 *   Partitioned contexts.  Collective exactly like the host-pointer calls
 *     (every rank calls, one thread / process each); the pointers address the
 *     rank's own rows.  A refusal on one rank leaves the others waiting, as
 *     with any collective whose arguments are wrong on one side.
 * x0_blocks == NULL: zero guess.  res of alfd_precond_apply_device may be
 * NULL. */
int alfd_upload_rhs_device(alfd_ctx_t ctx, const double *const *rhs_blocks, const double *const *x0_blocks,
                           void *stream);
int alfd_download_solution_device(alfd_ctx_t ctx, double *const *x_blocks, void *stream);
/* x_blocks: in = initial guess, out = solution. */
int alfd_solve_device(alfd_ctx_t ctx, const double *const *rhs_blocks, double *const *x_blocks, alfd_result *res,
                      void *stream);
int alfd_precond_apply_device(alfd_ctx_t ctx, const double *const *src_blocks, double *const *dst_blocks,
                              alfd_result *res, void *stream);
int alfd_system_apply_device(alfd_ctx_t ctx, const double *const *src_blocks, double *const *dst_blocks, void *stream);
/* rhs_blocks[0] is updated in place from rhs_blocks[last]. */
int alfd_augment_rhs_device(alfd_ctx_t ctx, double *const *rhs_blocks, void *stream);
/* Inner CG iterations of the last solve (or alfd_precond_apply) by inner operator, counts[alfd_inner_op]: the
 * augmented (1,1) block, A22, the 2-block operator.  alfd_result::inner_iterations is their sum (plus the K solves of
 * the rational variant). */
int alfd_get_inner_iterations(alfd_ctx_t ctx, int64_t counts[3]);
/* Residual history of the last solve: out[k] = residual checked at step k. */
int alfd_get_history(alfd_ctx_t ctx, double *out, int32_t capacity, int32_t *count);

/* ------------------------------------------------------------- primitives
 * The kernels under the solver, callable on host data for parity tests
 * (SURVEY.md 8(a) a13/a14).  y = A x (mode 0) or y += alpha A x (mode 1).  On a partitioned context
 * alfd_spmv is collective: x holds this rank's owned columns of the slot's column block, y its rows. */
int alfd_spmv(alfd_ctx_t ctx, int slot, const double *x, double *y, int mode, double alpha);
/* The two diagonal-scaled epilogues of the same kernels, which carry the augmented-Lagrangian and the nested
 * grad-div terms of the solver (t = W^-1 .* (C x), q = Mp_lumped^-1 .* (B u)): with y2 == NULL y = d .* (A x); with
 * y2 != NULL y = A x and y2 = d .* (A x).  d, y and y2 have the slot's (this rank's) row count.  Goes through the
 * solver's own dispatch (storage form, halo overlap, tunables); collective on a partitioned context like alfd_spmv.
 * y and y2 are uploaded as given before the launch.  ALFD_E_INVALID for a null ctx, x, d or y, an unset slot, and
 * y2 == y (the kernels take both as restrict pointers). */
int alfd_spmv_scaled(alfd_ctx_t ctx, int slot, const double *x, const double *d, double *y, double *y2);
/* The pair launch of the factored operators (tunable "ml_fuse" >= 2), callable on host data: y = A x for slot_a and
 * t = d .* (C x) for slot_c out of ONE launch, C as extra workgroups of A's grid.  Same bits as alfd_spmv (mode 0) on
 * slot_a and alfd_spmv_scaled (y2 == NULL) on slot_c.  x has the common column count, y slot_a's row count, d and t
 * slot_c's.  ALFD_E_UNSUPPORTED, with y and t untouched, when the pair does not qualify whatever "ml_fuse" says:
 * slot_a not on the long-row batch-major kernel (4 waves, narrow codes) or the streaming kernel (R = 2, U = 8), slot_c
 * not resident as plain CSR rows with 16, 32 or 64 lanes per row, different column counts, a partitioned context,
 * w_inverse != diagonal, aug_assembled, grad_div_in_A = 0.  ALFD_E_INVALID for a null ctx, x, d, y or t, an unset
 * slot, and t == y. */
int alfd_spmv_pair(alfd_ctx_t ctx, int slot_a, int slot_c, const double *x, const double *d, double *y, double *t);
/* One smoother step of a factored operator A + gamma Ct invW C on host data, in either of its two forms (tunable
 * "ml_tail_in_spmv" below), so that the block-end epilogue of the batch-major kernel can be run at shapes no solver
 * case reaches.  mode: 0 STEP (res = rin - y, d = fma(c1, din, c2 (dinv res)), z = zin + d; stores res, d, z), 1 LAST
 * (stores z), 2 LAST_ADD (stores zout = fma(1, z, zout)), 3 RES (stores res), 4 RES_INIT (z = c1 (dinv res); stores z,
 * and res when store_res), 5 RES_INIT_ADD (stores zout); y stands for A x + gamma Ct t of the row.  Ct is the caller's
 * CSR (ct_nrows = rows of slot_a, ct_ncols >= 1 columns; it may have no entries), t has ct_ncols entries.  slot_c < 0:
 * t is read.  slot_c >= 0: t = w .* (C x) is formed beside A x (w, t: the slot's row count = ct_ncols) and returned.
 * Vectors a mode does not use may be null; all others have the row count of slot_a (x: its column count).  Every vector
 * is staged on the device once per distinct address, so vectors passed at one address are one device vector.
 * Outputs are uploaded as given and written back; y receives A x on the rows Ct lists, and on the others only in
 * form 1 (form 0 never stores it there). */
typedef struct alfd_tail_step {
  int32_t mode, store_res, slot_c, reserved;
  double gamma, c1, c2;
  int64_t ct_nrows, ct_ncols;
  const int64_t *ct_rp;
  const int32_t *ct_col;
  const double *ct_val;
  const double *x, *w;
  double *t;
  const double *dinv, *rin, *din, *zin;
  double *y, *res, *d, *z, *zout;
} alfd_tail_step;
/* form 0: the A launch with the block-end epilogue, then the rows party of the tail launch.  form 1: y = A x (with
 * slot_c: the solver's pair launch or its two launches), then the whole tail launch.  Same bits.  Form 0 does not ask
 * the tunable; it returns ALFD_E_UNSUPPORTED when slot_a has no epilogue instantiation (not on the long-row batch-major
 * kernel with 4 waves, its largest block beyond 20 KB of LDS with the row buffer, half or more of the rows in Ct,
 * side rows while the tunable "ml_tail_side_rows" is 0 -- that one it does obey, like the solver; with 1 the side rows
 * get their tails from spmv_side_rows_tail_kernel behind the A launch -- or mode 5), and ALFD_E_INVALID, with nothing launched, when a vector the mode stores (y included) was passed at x's
 * address: inside one launch that would be a race.  Both forms: ALFD_E_UNSUPPORTED on a partitioned context, with
 * w_inverse != diagonal, aug_assembled, grad_div_in_A = 0, or a Ct that does not stay plain CSR rows. */
int alfd_spmv_tail_step(alfd_ctx_t ctx, int slot_a, int form, const alfd_tail_step *s);
/* The number of A launches with the block-end epilogue since alfd_create (solver and alfd_spmv_tail_step alike). */
int alfd_get_fused_tail_launches(alfd_ctx_t ctx, int64_t *count);
/* What the last SpMV launch of this context instantiated: written on the host beside every kernel launch of the SpMV
 * launchers, from the template arguments of that launch (not from the settings that chose it), so that a test or a
 * measuring session can tell which kernel a setting reached -- a shape no dispatch list names falls through to another
 * family without a word ("Launch shapes from the environment").  The split launch of a partitioned
 * long-row batch-major operator records its second half; a pair launch records A's family.  A call that launches
 * nothing (no entries on this rank) leaves the record as it was.
 *   lanes        lanes per row (64 for the long-row families)
 *   R, U         rows per batch and 64-entry chunks in flight of the stream / window / group kernels; R and J of
 *                WINDOW_VI; BATCH_MAJOR: R = waves per workgroup, U = 1 with wide codes; else 0
 *   nontemporal  1: the stream kernel with non-temporal loads
 *   epilogue     0 y = s, 1 y = fma(alpha, s, y), 2 y = d .* s, 3 y = s and y2 = d .* s
 *   xcd_order    the block-order argument the window / class-batched / batch-major kernel was launched with; else 0
 *   grid         workgroups launched (a pair launch: both parties); lds_bytes: dynamic LDS of one workgroup
 * ALFD_E_NOT_SETUP before the first SpMV launch of the context, ALFD_E_INVALID for a null ctx or out. */
enum alfd_spmv_family {
  ALFD_SPMV_PLAIN = 0,              /* spmv_kernel<L>: one row per group of L lanes */
  ALFD_SPMV_SPARSE_ROWS = 1,        /* the same on the list of non-empty rows */
  ALFD_SPMV_STREAM = 2,             /* spmv_stream_kernel<R, U> */
  ALFD_SPMV_WINDOW = 3,             /* spmv_window_kernel<R, U> */
  ALFD_SPMV_WINDOW_VI = 4,          /* spmv_window_vi_kernel<R, J>: dictionary-coded values, in-order batches */
  ALFD_SPMV_WINDOW_VIB = 5,         /* spmv_window_vib_kernel: dictionary-coded values, class-sorted batches */
  ALFD_SPMV_WINDOW_GROUP = 6,       /* spmv_window_group_kernel<L, R, U>: short rows */
  ALFD_SPMV_BATCH_MAJOR = 7,        /* spmv_vs_kernel: long rows */
  ALFD_SPMV_BATCH_MAJOR_SHORT = 8,  /* spmv_vss_kernel<L>: short rows */
  ALFD_SPMV_PLAIN_F32 = 9,          /* the single-precision copy of slot A on the three families it has */
  ALFD_SPMV_STREAM_F32 = 10,
  ALFD_SPMV_WINDOW_F32 = 11,
  ALFD_SPMV_ROW_LANE = 12,          /* spmv_rowlane_kernel<L>: one thread per row, rows of at most 2 L entries, L 4 or 8 */
  ALFD_SPMV_NFAMILIES = 13
};
typedef struct alfd_spmv_launch {
  int32_t family;   /* enum alfd_spmv_family */
  int32_t lanes, R, U, nontemporal, epilogue, xcd_order;
  int64_t grid, lds_bytes;
} alfd_spmv_launch;
int alfd_get_last_spmv_launch(alfd_ctx_t ctx, alfd_spmv_launch *out);
int alfd_dot(alfd_ctx_t ctx, int64_t n, const double *x, const double *y, double *result);
/* z = M^-1 r: ONE application of the preconditioner of the inner CG, with no CG around it -- exactly the operator
 * the configured variant's inner solve calls once per iteration (alfd_config::inner_prec: identity, Jacobi, the
 * Chebyshev sweep, the multilevel cycle incl. patch and coarsest inverse), after alfd_setup.  Unlike
 * alfd_precond_apply with one fixed CG step, which returns alpha(r) M^-1 r, this keeps the scale, so linearity,
 * symmetry and the operator itself can be compared with an independent reference.  `op` selects the inner operator:
 *   ALFD_INNER_OP_AUG   the augmented (1,1) block: AL2, AL_STOKES, AL_STOKES_DIAG, AL_ELL_MODIFIED; r, z have the
 *                       length of block 0
 *   ALFD_INNER_OP_A22   the second block A22_aug of AL_ELL_MODIFIED; r, z have the length of block 1
 *                       (ALFD_PREC_MULTILEVEL: the V-cycle of the block-1 hierarchy when one is set, else the sweep)
 *   ALFD_INNER_OP_AUG2  the coupled 2-block operator of AL_ELL_IDEAL; r, z hold block 0 followed by block 1
 *                       (ALFD_PREC_MULTILEVEL: the block diagonal of the two hierarchies, patch included on block 0)
 * An op the configured variant does not solve with: ALFD_E_INVALID; before alfd_setup: ALFD_E_NOT_SETUP.  Stages
 * through the buffers of the depth-1 calls (a resident right-hand side stays intact).  On a partitioned context the
 * call is collective like alfd_spmv: r, z hold this rank's rows. */
enum alfd_inner_op { ALFD_INNER_OP_AUG = 0, ALFD_INNER_OP_A22 = 1, ALFD_INNER_OP_AUG2 = 2 };
int alfd_inner_prec_apply(alfd_ctx_t ctx, int op, const double *r, double *z);
/* ------------------------------------------------------------ sanity checks
 * The diagnostic block that ends every driver's solve (immersed_laplace.cc:987-1010,
 * stokes_immersed_boundary.cc:1157-1180, elliptic_interface.cc:973-1009, `Perform sanity checks`).
 *
 * alfd_estimate_spectrum replaces the unpreconditioned SolverCG on C Ct with connect_condition_number_slot [EXT]:
 * right-hand side all ones, zero start, SolverControl(lambda.size(), 1e-12) when ctrl == NULL.  The arithmetic is
 * the inner CG's with ALFD_PREC_IDENTITY on y = C (Ct x), run on the compacted operators
 * C[:,S], Ct[S,:] (S = non-empty rows of Ct), so an iteration costs O(nnz(C) + n_lambda) whatever n_u is; on one
 * rank the stop rule runs on the device and the host reads the state once per group of iterations (tunables
 * "spectrum_group", "spectrum_host_stepped").  With alpha_j = r_{j-1}.r_{j-1} / p_j.(C Ct p_j) and
 * beta_j = r_j.r_j / r_{j-1}.r_{j-1} the Lanczos matrix T_k of k CG steps is tridiagonal with the diagonal
 * delta_1 = 1/alpha_1, delta_j = 1/alpha_j + beta_{j-1}/alpha_{j-1} and the off-diagonal
 * eta_j = sqrt(beta_j)/alpha_j, j < k; its extreme eigenvalues (Ritz values) estimate those of C Ct, which is what
 * SolverCG's condition-number slot reports [EXT].
 *   After alfd_setup, every variant (all have C and CT); before it ALFD_E_NOT_SETUP.  Unknown op or
 *   ctrl->max_steps < 1: ALFD_E_INVALID.  Partitioned context: ALFD_E_UNSUPPORTED (single rank only).
 *   ALFD_OK whenever an estimate was produced, also when the CG did not converge -- the reference catches that
 *   exception and keeps the number; `converged` carries the "C Ct does not have full rank" verdict.  A step with
 *   p.Ap <= 0 (or NaN) ends the solve at the step before it; if that was the first step there is nothing to
 *   estimate from: ALFD_E_BREAKDOWN.  A start that already meets the stop rule gives steps = 0 and NaN estimates.
 *   Touches neither a resident right-hand side / solution nor the staging of the depth-1 calls: a solve after it
 *   gives the same bits as before.  log_level >= 1 prints "Condition number estimate: <kappa>" and, when the CG did
 *   not converge, the reference's "***CCt solve not successfull (see condition number above)***" to stderr. */
typedef struct alfd_spectrum {
  int32_t converged;        /* 1: the CG met its stop rule; 0: it hit max_steps, broke down (p.Ap <= 0) or met a NaN */
  int32_t steps;            /* CG steps taken = order k of the tridiagonal matrix */
  double initial_residual, last_residual;
  double lambda_min, lambda_max, condition;   /* extreme Ritz values of T_k and their ratio */
} alfd_spectrum;
enum alfd_spectrum_op { ALFD_SPECTRUM_CCT = 0 };   /* C Ct on the multiplier block */
int alfd_estimate_spectrum(alfd_ctx_t ctx, int op, const alfd_control *ctrl /* NULL: ABS, max_steps = n_lambda, tol 1e-12 */,
                           alfd_spectrum *out);
/* alpha_1..alpha_k and beta_1..beta_{k-1} of the last estimate: *count = k, at most `capacity` entries are written,
 * beta[k-1] never.  ALFD_E_NOT_SETUP before the first estimate. */
int alfd_get_cg_coefficients(alfd_ctx_t ctx, double *alpha, double *beta, int32_t capacity, int32_t *count);
/* Host-only (no device, no context): the smallest and largest eigenvalue of T_k above by Sturm-count bisection down
 * to neighbouring doubles (no LAPACK); k = 1 gives 1/alpha_1 twice (beta may be NULL).  ALFD_E_INVALID for k < 1, a
 * non-finite or non-positive alpha, a negative or non-finite beta.  alfd_estimate_spectrum calls this routine. */
int alfd_host_tridiagonal_extremes(int32_t k, const double *alpha, const double *beta, double *lambda_min, double *lambda_max);
/* || (last block row of AA) x - g ||_inf for host vectors x_blocks (one pointer per block, as alfd_system_apply);
 * g == NULL: zero.  The row is C x0 for ALFD_AL2, the Stokes variants and ALFD_RATIONAL, C x0 - M x1 for the elliptic
 * variants (the "L infty norm of constraints residual" of elliptic_interface.cc:973-984, up to its sign).  The
 * product is the last block of alfd_system_apply, same bits; a NaN entry makes the result NaN.  Stages through the
 * buffers of the depth-1 calls.  Single rank: ALFD_E_UNSUPPORTED on a partitioned context. */
int alfd_constraint_residual(alfd_ctx_t ctx, const double *const *x_blocks, const double *g /* may be NULL */, double *linf);
/* Lanes per row the canonical SpMV order uses for this slot (after setup). */
int alfd_matrix_lanes(alfd_ctx_t ctx, int slot, int32_t *lanes);
/* Benchmark hook: run `reps` back-to-back y = A x launches of `slot` on resident
 * device data and return the mean kernel time in ms measured with HIP events on
 * the library's stream, plus the algorithmic bytes of one launch. */
int alfd_bench_spmv(alfd_ctx_t ctx, int slot, int32_t reps, double *ms_per_launch,
                    double *algorithmic_bytes);
/* Device storage format chosen for a matrix slot at upload:
 * lanes per row, LDS-window blocks, and -- for matrices whose row blocks repeat
 * <= 256 distinct entry values, as finite-element matrices on the reference's
 * uniformly refined hyper_cube grids do (stokes_immersed_boundary.cc:355-372) --
 * dictionary-coded values.  streamed_bytes is what one SpMV launch of the kernel
 * in use moves by format; algorithmic_bytes is the plain-CSR figure of SURVEY 8(d). */
typedef struct alfd_matrix_info {
  int32_t lanes, windowed, value_indexed;
  int32_t batch_major;   /* 0: no; 1: batch-major format on runs of the numbering; 2: on the caller's row blocks */
  int64_t nnz, window_blocks, window_fallback_blocks;
  int64_t value_indexed_blocks, value_indexed_nnz, dictionary_entries, value_wide_nnz;
  double algorithmic_bytes, streamed_bytes;
  int64_t shared_nnz;    /* batch-major forms: entries of rows stored as translates of a template row */
  int64_t batch_major_blocks;
  int64_t batch_major_wide;  /* 1: 10-bit dictionary codes / 11-bit window columns (blocks with > 512 distinct values) */
  int64_t batch_major_interior_blocks; /* partitioned contexts: leading row blocks that read no halo column -- launched
                                        * before the halo exchange is started (the rest after it has arrived); else 0 */
} alfd_matrix_info;
int alfd_get_matrix_info(alfd_ctx_t ctx, int slot, alfd_matrix_info *out);
/* The shape of a batch-major operator: what alfd_matrix_info has no room for.  rows / waves: rows per block the long-row
 * form was planned with and waves per workgroup of its launches; small = 1 when the small-operator rule chose them
 * (tunable "batch_major_small") and not the context-wide defaults; lds_bytes: dynamic LDS of one workgroup (dictionary
 * + largest x window).  alfd_get_matrix_shape: a matrix slot.  alfd_get_operator_shape: the operators the library
 * builds at alfd_setup -- A_l of level `level` >= 1 of the velocity hierarchy, A[S,S] / A[S,:] of the interface patch
 * (level ignored); ALFD_E_INVALID when the context has no such operator. */
typedef struct alfd_batch_major_shape {
  int32_t batch_major, lanes;     /* as in alfd_matrix_info */
  int64_t nrows, nnz, shared_nnz;
  int64_t rows, waves, small;
  int64_t blocks, batches, lds_bytes;
  int64_t compute_units;          /* of the context's device: what the small-operator rule sizes against */
} alfd_batch_major_shape;
enum alfd_operator { ALFD_OPERATOR_LEVEL = 0, ALFD_OPERATOR_PATCH_SS = 1, ALFD_OPERATOR_PATCH_S = 2 };
int alfd_get_matrix_shape(alfd_ctx_t ctx, int slot, alfd_batch_major_shape *out);
int alfd_get_operator_shape(alfd_ctx_t ctx, int op, int level, alfd_batch_major_shape *out);
/* Measurement hook (one rank): `reps` back-to-back y = A x launches of such an operator in its long-row batch-major form,
 * timed with HIP events on the library's stream after one warm-up launch.  rows = 0: the operator as the solver holds
 * it; rows in 4..250 and waves in {1, 2, 4}: a second copy planned at that shape for the call (the solver's stays as it
 * is).  info, if not NULL, describes what was timed. */
int alfd_bench_operator(alfd_ctx_t ctx, int op, int level, int32_t rows, int32_t waves, int32_t reps,
                        double *us_per_launch, alfd_batch_major_shape *info);
/* Host-only: the shape the small-operator rule gives an operator of nrows rows whose default plan (rows per block,
 * waves per workgroup) has `blocks` blocks and `batches` batches, on a device of compute_units CUs. */
int alfd_host_small_shape(int64_t nrows, int64_t blocks, int64_t batches, int32_t rows, int32_t waves,
                          int32_t compute_units, int32_t *rows_out, int32_t *waves_out);
/* Host-only (no device, no context): plans the LDS-window / value-indexed storage of
 * a CSR matrix exactly as alfd_set_matrix would (default tunables), decodes the plan
 * back -- window columns through the segment table, values through the block
 * dictionaries, every row through the class-sorted batch descriptors -- and reports
 * the number of entries / rows that do not reproduce the input (must be 0).
 * lanes: the canonical lanes-per-row of the matrix (alfd_matrix_lanes). */
typedef struct alfd_window_plan_info {
  int32_t windowed, value_indexed, row_block, max_window;
  int64_t blocks, fallback_blocks, segments;
  int64_t value_indexed_blocks, value_indexed_nnz, value_wide_nnz, dictionary_entries;
  int64_t batches, decode_mismatches;
} alfd_window_plan_info;
int alfd_host_window_plan(int64_t nrows, const int64_t *row_ptr, const int32_t *col, const double *val,
                          int32_t lanes, int32_t want_value_index, alfd_window_plan_info *out);
/* Host-only: plans the batch-major format (tunable "batch_major") of a CSR matrix as
 * alfd_set_matrix would -- row blocks = runs of `row_block` rows, or the caller's blocks as in
 * alfd_set_row_blocks when n_blocks > 0 -- and decodes it back (rows through the batch
 * descriptors, columns through the window segments, values through the dictionaries). */
typedef struct alfd_stream_plan_info {
  int32_t ok, max_window, max_rows, max_batches;
  int64_t blocks, batches, segments, dictionary_entries, stream_bytes;
  int64_t decode_mismatches, rows_covered;
  int64_t shared_nnz;   /* entries of rows stored as translates of a template row (one stored row per batch) */
} alfd_stream_plan_info;
int alfd_host_stream_plan(int64_t nrows, const int64_t *row_ptr, const int32_t *col, const double *val,
                          int32_t row_block, int64_t n_blocks, const int64_t *block_ptr, const int32_t *rows,
                          alfd_stream_plan_info *out);
/* The same with side rows (tunable "batch_major_side_rows" = 1): plans as alfd_set_matrix would with the tunable on and
 * decodes the blocks as alfd_host_stream_plan does; rows_covered counts the rows of the blocks only.  *n_side_out rows
 * went to the side list, side_rows_out (capacity nrows) names them in the order of the list, *side_nnz_out is the number
 * of their entries; a side row whose compact CSR copy does not reproduce the input row, and a row that is in both or in
 * neither of blocks and list, count into decode_mismatches.  Where the variant is refused (no row beyond 384 entries,
 * more than 1/8 of the entries in such rows, a row beyond 65 535 entries) the result is alfd_host_stream_plan's. */
int alfd_host_stream_plan_side(int64_t nrows, const int64_t *row_ptr, const int32_t *col, const double *val,
                               int32_t row_block, int64_t n_blocks, const int64_t *block_ptr, const int32_t *rows,
                               int64_t *n_side_out, int32_t *side_rows_out, int64_t *side_nnz_out,
                               alfd_stream_plan_info *out);
/* The side list of a matrix slot in the long-row batch-major form (all fields 0 for a matrix without one): its rows,
 * their entries, the longest of them, how many of them read no halo column (partitioned contexts, where these go with
 * the interior blocks; else 0) and the workgroups of the side launch over the whole list. */
typedef struct alfd_side_rows_info {
  int64_t rows, nnz, longest, interior_rows, grid;
} alfd_side_rows_info;
int alfd_get_side_rows(alfd_ctx_t ctx, int slot, alfd_side_rows_info *out);
/* The same for a short-row matrix (lanes = 8, 16 or 32, see alfd_matrix_lanes): the batch-major form of
 * spmv_vss_kernel -- one stored template row per batch of translate rows -- planned on runs of the numbering and
 * decoded back.  stream_bytes includes the batch descriptors. */
int alfd_host_stream_plan_short(int64_t nrows, const int64_t *row_ptr, const int32_t *col, const double *val,
                                int32_t lanes, alfd_stream_plan_info *out);
/* alfd_bench_spmv with the value-indexed kernel switched on (1) or off (0: the same
 * matrix through the 10 B/nnz window kernel); streamed_bytes as in alfd_matrix_info. */
int alfd_bench_spmv_format(alfd_ctx_t ctx, int slot, int32_t reps, int use_value_index,
                           double *ms_per_launch, double *streamed_bytes);
/* ---------------------------------------- single-precision operator values inside the inner preconditioner
 * (DESIGN.md section 6).  Opt-in, default ALFD_PREC_VALUES_FP64: nothing changes until the setter is called.
 *
 * With ALFD_PREC_VALUES_FP32 the library keeps, next to the 8-byte values of slot ALFD_A, the operator
 *   A~ = fl32(A) entry by entry: round to nearest even to IEEE binary32; an image that would be subnormal
 *   (0 < |fl32(a)| < 2^-126) is stored as a zero with the sign of a; an entry without a finite image (|a| beyond
 *   FLT_MAX, or a not finite) makes the whole copy ineligible and nothing is stored.
 * A kernel on A~ loads a float, widens it (exact) and forms the fma chains of the 8-byte kernels in the canonical
 * order, so A~ x has, bit for bit, the value alfd_spmv gives on a matrix that holds the rounded values.  The copy costs
 * 4 B per entry of device memory and is made on the device from the resident values (no second upload).  Row pointers,
 * columns and window tables are shared; one launch streams 6 instead of 10 B per entry on the window kernel, 8
 * instead of 12 on the streaming and plain kernels.
 *
 * The copy exists ("stored") when the request is on and slot ALFD_A uses 64 lanes per row, is not in the sparse-row
 * form, holds no dictionary-coded entries (batch-major or value-indexed: those stream fewer bytes already and stay
 * exact), lives on a single-rank context, and every image is finite.  It is made at alfd_set_matrix(ALFD_A), or by the
 * setter when A is resident, and released when the request is dropped or A is replaced.
 *
 * It is "used", decided at alfd_setup, when it is stored and alfd_config::inner_prec is
 *   ALFD_PREC_MULTILEVEL: every application of the level-0 operator of the block-0 hierarchy inside the cycle (smoother
 *     steps, the residual before the restriction, the residual before the post-smoothing), also as the block-0 half
 *     of AL_ELL_IDEAL's block-diagonal preconditioner;
 *   ALFD_PREC_CHEBYSHEV on the augmented (1,1) block (cheb_degree > 1): the A product inside the sweep.
 * Everything else stays as it is: alfd_setup computes what it computes without the option (diagonals, every
 * lambda_max -- alfd_result::lambda_max is bit-equal -- and all Galerkin products come from the 8-byte values); the
 * patch operators, the levels >= 1, A2 and its hierarchy, C, Ct, B, Bt, M, Mp, the operator of the inner CG and the
 * outer system keep their 8-byte values.  The inner preconditioner stays a fixed symmetric linear operator
 * (fl32(a_ij) = fl32(a_ji)); the residuals and the Krylov vectors are those of the exact operator, so the accuracy of
 * the solve is unchanged -- only iteration counts may move.  Caveat: A~ differs from A by up to 2^-24 relative per
 * entry; for an A whose condition number approaches 1e7 the smoother's operator may lose definiteness in its lowest
 * modes.  The option is meant for operators well below that (the finite-element blocks here: 1e4 .. 1e5).
 *
 * alfd_set_preconditioner_values: an unknown kind is ALFD_E_INVALID.  A call that changes the request on a set-up
 *   context un-sets it up like alfd_configure (solves answer ALFD_E_NOT_SETUP, alfd_setup_coupling ALFD_E_INVALID with
 *   "needs alfd_setup"); a call that changes nothing leaves the setup alone.  On a partitioned context the request is
 *   accepted and stays ineligible (PARTITIONED): decided locally, the same answer on every rank, no exchange.
 * alfd_get_preconditioner_values: see the struct.  alfd_setup_coupling keeps the copy, like the rest of slot A.
 * alfd_spmv_preconditioner: y = A~ x (mode 0) or y = fma(alpha, A~ x, y) (mode 1) on host data through the dispatch the
 *   cycle uses; needs no setup.  ALFD_E_UNSUPPORTED, y untouched, when the copy is not stored.
 * alfd_bench_spmv_preconditioner: alfd_bench_spmv on the copy; streamed_bytes = streamed_bytes_fp32 of the struct.
 * Null ctx, out, x or y: ALFD_E_INVALID. */
enum alfd_prec_values { ALFD_PREC_VALUES_FP64 = 0, ALFD_PREC_VALUES_FP32 = 1 };
enum alfd_prec_values_reason {
  ALFD_PREC_VALUES_NONE = 0,            /* stored and used */
  ALFD_PREC_VALUES_NOT_REQUESTED = 1,
  ALFD_PREC_VALUES_NO_MATRIX = 2,       /* slot A not set yet */
  ALFD_PREC_VALUES_SHORT_ROWS = 3,      /* fewer than 64 lanes per row */
  ALFD_PREC_VALUES_SPARSE_ROWS = 4,
  ALFD_PREC_VALUES_DICTIONARY_FORM = 5, /* batch-major or value-indexed entries */
  ALFD_PREC_VALUES_PARTITIONED = 6,
  ALFD_PREC_VALUES_OUT_OF_RANGE = 7,    /* an entry without a finite binary32 image */
  ALFD_PREC_VALUES_NOT_APPLIED = 8      /* stored, but the configured variant / inner_prec never applies slot A inside
                                         * the inner preconditioner; also before a setup */
};
typedef struct alfd_prec_values_info {
  int32_t requested, stored, used;
  int32_t reason;                       /* alfd_prec_values_reason */
  int32_t family;                       /* kernel family of the copy: 0 plain, 1 stream, 2 window (stored only) */
  int32_t reserved;
  int64_t nnz;                          /* of slot A (0 without a matrix) */
  int64_t flushed_to_zero;              /* entries whose image would be subnormal */
  int64_t copy_bytes;                   /* device memory of the copy */
  double streamed_bytes_fp64, streamed_bytes_fp32;   /* format bytes of one launch on the 8-byte values / on the copy */
} alfd_prec_values_info;
int alfd_set_preconditioner_values(alfd_ctx_t ctx, int kind);
int alfd_get_preconditioner_values(alfd_ctx_t ctx, alfd_prec_values_info *out);
int alfd_spmv_preconditioner(alfd_ctx_t ctx, const double *x, double *y, int mode, double alpha);
int alfd_bench_spmv_preconditioner(alfd_ctx_t ctx, int32_t reps, double *ms_per_launch, double *streamed_bytes);

/* Row-block hint for the batch-major SpMV format of a long-row matrix (tunable "batch_major" = 1):
 * a partition of the rows of `slot` into blocks of at most 250 rows -- rows[block_ptr[b] .. block_ptr[b+1])
 * -- whose columns are close together, e.g. bricks of the mesh (all components of the nodes of a
 * 4 x 4 x 4 patch).  A block stages ONE window of x in LDS, so the fewer distinct columns a block
 * touches the better; the result of the SpMV does not depend on the blocks (each row keeps the
 * canonical summation order).  Takes effect at the next alfd_set_matrix of that slot; n_blocks = 0
 * removes the hint (blocks are then runs of the row numbering). */
int alfd_set_row_blocks(alfd_ctx_t ctx, int slot, int64_t n_blocks, const int64_t *block_ptr, const int32_t *rows);

/* Host-only helper for alfd_set_row_blocks when the caller has no grid metadata: recursive coordinate
 * bisection of one support point per matrix row (deal.II: DoFTools::map_dofs_to_support_points) into
 * blocks of at most max_rows (<= 250) rows.  block_ptr_out needs room for nrows + 1 entries, rows_out
 * for nrows; *n_blocks_out receives the number of blocks. */
int alfd_host_row_blocks_from_points(int64_t nrows, int32_t dim, const double *points, int32_t max_rows,
                                     int64_t *n_blocks_out, int64_t *block_ptr_out, int32_t *rows_out);

/* Host-only helpers for callers whose DoF numbering is not the one the SpMV formats like (a deal.II program numbers
 * with Cuthill-McKee and then block-wise, stokes_immersed_boundary.cc:533-541; the batch-major form wants the rows of a
 * mesh brick to read a compact set of columns).  From one support point per unknown of a block
 * (DoFTools::map_dofs_to_support_points):
 *   alfd_host_numbering_from_points: new_to_old[nrows] = the unknowns in lexicographic order of their points (last
 *     coordinate slowest), unknowns with the same point -- the components of a node -- kept together in their order.
 *     alfd_set_numbering (below) takes it: the library then permutes the operators at upload and the vectors on the
 *     device, and the caller keeps its own numbering.
 *   alfd_host_brick_blocks_from_points: row blocks for alfd_set_row_blocks = bricks of brick[0] x brick[1] x brick[2]
 *     grid nodes, a node's grid index along an axis being the rank of its coordinate among the distinct coordinates
 *     of that axis (exact on tensor grids, consistent on locally refined ones); blocks above max_rows rows are split.
 *   alfd_host_permute_csr: out = in with rows taken in the order row_new_to_old (NULL: unchanged) and column j renamed
 *     col_old_to_new[j] (NULL: unchanged), the entries of a row re-sorted by the new column.  out_row_ptr[nrows + 1],
 *     out_col / out_val [nnz]. */
int alfd_host_numbering_from_points(int64_t nrows, int32_t dim, const double *points, int64_t *new_to_old);
int alfd_host_brick_blocks_from_points(int64_t nrows, int32_t dim, const double *points, const int32_t *brick,
                                       int32_t max_rows, int64_t *n_blocks_out, int64_t *block_ptr_out, int32_t *rows_out);
int alfd_host_permute_csr(int64_t nrows, const int64_t *row_ptr, const int32_t *col, const double *val,
                          const int64_t *row_new_to_old, const int64_t *col_old_to_new, int64_t *out_row_ptr,
                          int32_t *out_col, double *out_val);

/* ------------------------------------------------ numbering of block 0 (additive within ABI 12)
 * A caller whose block-0 unknowns (velocity / background space) are not numbered the way the SpMV formats like declares
 * a permutation ONCE and keeps its own numbering for everything it hands in or gets back; the library permutes the
 * operators at upload and the vectors on the device, inside the pack / unpack launch that moves the caller's blocks
 * into the padded internal vector.  Internal index k of block 0 is the caller's index new_to_old[k].
 *
 *   alfd_host_check_numbering: host only.  ALFD_E_INVALID unless new_to_old is a bijection of [0, n) (an entry out of
 *     range or repeated, a null pointer with n > 0, n < 0); old_to_new (may be NULL) receives the inverse.
 *   alfd_set_numbering: fixes the permutation (n == 0 clears it).  It must precede every upload it affects: with slot
 *     A, BT, B, CT or C, a level-0 prolongator or aggregates of block 0, or a row-block hint for A / BT / CT present it
 *     returns ALFD_E_INVALID and alfd_last_error names what is in the way -- clearing included.  ALFD_E_UNSUPPORTED on a
 *     partitioned context (nranks > 1), and alfd_comm_init* / alfd_set_partition refuse the same way after it.  n must
 *     be the size of block 0 at every later use: a mismatch at an upload, at alfd_setup or at a vector call is
 *     ALFD_E_INVALID.  n < 2^31 (columns are int32; the device copy is 32-bit).
 *   alfd_set_numbering_from_points: from one support point per block-0 unknown ([n][dim], dim 1..3; a non-finite
 *     coordinate is ALFD_E_INVALID): the numbering of alfd_host_numbering_from_points, and as the row-block hint of A
 *     the blocks alfd_host_brick_blocks_from_points(.., brick, 250, ..) forms of the points sorted by it (brick NULL:
 *     16, 4, 1).
 *   alfd_get_numbering: *n = entries (0: none); new_to_old != NULL: the permutation, ALFD_E_INVALID when capacity < *n.
 *
 * THE RULE: with a numbering, whatever crosses the calls below is in the CALLER's numbering.
 *   alfd_set_matrix: rows of A, BT, CT are taken in the new order, columns of A, B, C renamed and a row's entries
 *     sorted by new column (the arithmetic of alfd_host_permute_csr); the derived transposes follow from the permuted
 *     operand; every later re-upload (the new CT of alfd_setup_coupling) is permuted the same way.
 *   alfd_set_prolongator / alfd_set_prolongator_block(block 0) at level 0: rows; alfd_set_aggregates at level 0: agg[]
 *     and weight[].  alfd_get_prolongator[_block] / alfd_get_aggregates[_block] (block 0, level 0) answer in the
 *     caller's numbering, whoever made the level.
 *   alfd_set_row_blocks for A, BT, CT: row ids are mapped; the order inside a block stays.
 *   Block vectors -- alfd_solve, alfd_precond_apply, alfd_system_apply, alfd_augment_rhs, alfd_upload_rhs,
 *     alfd_download_solution, alfd_constraint_residual and the six *_device calls: block 0 is translated on the way in
 *     and on the way out (the *_device calls keep their aliasing rules: all inputs are packed before any output).
 * NOT translated -- these speak the internal numbering, alfd_get_numbering is the key: the single-vector primitives and
 * diagnostics (alfd_spmv*, alfd_spmv_tail_step, alfd_inner_prec_apply, alfd_spmv_preconditioner, alfd_bench_*), the
 * strength-graph getters, and everything the alfd_build_* builders produce below level 0.
 * Without a numbering every call behaves as before and launches the same kernels. */
int alfd_host_check_numbering(int64_t n, const int64_t *new_to_old, int64_t *old_to_new /* may be NULL */);
int alfd_set_numbering(alfd_ctx_t ctx, int64_t n, const int64_t *new_to_old);
int alfd_set_numbering_from_points(alfd_ctx_t ctx, int64_t n, int32_t dim, const double *points,
                                   const int32_t *brick /* [3], NULL: 16,4,1 */);
int alfd_get_numbering(alfd_ctx_t ctx, int64_t *new_to_old, int64_t capacity, int64_t *n);

/* Free / total bytes of the context's device (hipMemGetInfo): leak checks, capacity planning. */
int alfd_get_device_memory(alfd_ctx_t ctx, int64_t *free_bytes, int64_t *total_bytes);
/* Run-time switches of a context (measurement and A/B comparison; results never change):
 *   "value_index"  1 (default): matrices whose row blocks were dictionary-coded at upload use the
 *                  3 B/nnz kernel; 0: every windowed matrix goes through the general 10 B/nnz kernel
 *                  (8-byte values + 16-bit window columns), as a matrix with unrelated values would.
 *   "batch_major"  1 (default): long-row matrices with repeating values, and short-row (8 / 16 / 32 lanes per
 *                  row) matrices whose rows are mostly translates of one another, use the batch-major forms of
 *                  csrc/kernels_vs.hpp (decided at alfd_set_matrix; also switches the kernel at launch); 0: the
 *                  round-1 window formats.  "batch_major_rows" (4..250, default 96): rows per block of the long-row
 *                  form when no alfd_set_row_blocks hint is given; "batch_major_waves" (1, 2, 4, 8): waves per workgroup;
 *                  "batch_major_xcd" (0/1): XCD-contiguous block order (measured slower); "batch_major_share" (0/1):
 *                  store rows that are translates of one another once (0: every row stored, ~3.1 B/nnz -- what a
 *                  matrix with repeating values but no translate structure gets; at the next alfd_set_matrix);
 *                  "batch_major_wide" (0/1, default 1): blocks with more than 512 distinct values are re-planned with
 *                  10-bit codes / 11-bit window columns instead of being halved (cell-wise assembled matrices).
 *                  "batch_major_small" (0/1; environment ALFD_SPMV_SMALL_SHAPES, read at alfd_create): 1: the level and
 *                  patch operators the library builds whose default plan gives fewer blocks x waves than half the resident
 *                  wave slots of the device (16 per compute unit) are planned with smaller row blocks, down to one batch
 *                  per wave; 0: rows / waves above for every operator.  At the next alfd_setup.
 *                  "batch_major_side_rows" (0/1, default 0; other values are refused with ALFD_E_INVALID; at the next
 *                  alfd_set_matrix / alfd_setup): 1: the long-row form, which takes rows of at most 384 entries and
 *                  otherwise refuses the whole matrix, keeps longer rows out of its row blocks and stores them in a
 *                  side list (plain CSR, longest row first) that spmv_side_rows_kernel computes in a launch of its
 *                  own behind every batch-major launch, timed with it; alfd_get_last_spmv_launch keeps describing the
 *                  batch-major launch, alfd_get_side_rows the list.  Same bits.  Not used when no row is that long
 *                  (the plan is then the one of 0), when such rows hold more than 1/8 of the entries, or when one has
 *                  more than 65 535.  A side row has no block end: what "ml_tail_in_spmv" does with such an operator is
 *                  the subject of "ml_tail_side_rows" below.
 *   "short_rows_per_thread" (0/1, default 1; other values are refused with ALFD_E_INVALID; at the next launch): 1: an
 *                  operator with 4 or 8 lanes per row that would run on spmv_kernel<L> (no window or batch-major form,
 *                  not the sparse-row list) and whose longest row has at most 2 L entries runs y = A x and
 *                  y = fma(alpha, A x, y) on spmv_rowlane_kernel<L>, one thread per row (the prolongators of a tensor
 *                  grid hierarchy); the longest row is counted at alfd_set_matrix.  0: spmv_kernel<L>.
 *                  Same bits; alfd_get_last_spmv_launch says which ran (ALFD_SPMV_ROW_LANE).
 *   "nested_mp_host_stepped" (0/1, default 0): grad_div_in_A = 0, one rank: the nested CG on Mp inside Aug is
 *                  device-stepped (stop rule on the device, one state read per group); 1 steps it on the host (one
 *                  synchronisation per iteration), as partitioned contexts always do.  Same bits either way.
 *                  "nested_mp_group" (1..1000, default 16): device-stepped iterations enqueued per state read.
 *   "spectrum_host_stepped" (0/1, default 0): alfd_estimate_spectrum steps its CG on the host (one synchronisation
 *                  per iteration, through the inner CG's own loop) instead of on the device.  Same bits either way.
 *                  "spectrum_group" (1..1000, default 16): device-stepped iterations enqueued per state read.
 *   "numbering_unpack_scatter" (0/1, default 0): under alfd_set_numbering block 0 leaves the internal vector through
 *                  the scatter form of the unpack kernel (coalesced reads, writes at new_to_old[k]) instead of the
 *                  gather form (reads at old_to_new[i], coalesced writes).  Same bits; the gather form measured
 *                  faster (profiles/numbering/).
 *   "ml_fuse"      0..3 (default 2; environment ALFD_ML_FUSE, read at alfd_create): how many launches one application
 *                  of a factored operator A + gamma Ct invW C takes inside ALFD_PREC_MULTILEVEL.  0: separate
 *                  launches.  1: the product y += gamma Ct t that ends it and the element-wise kernel after it
 *                  (Chebyshev step, residual, residual + first direction, final z += correction) are one launch
 *                  (aug_tail_kernel).  2: also t = invW .* (C x) rides as extra workgroups of the launch of y = A x
 *                  (alfd_spmv_pair above) on the levels l >= 1, on the patch and for A[S,:] / C of the patch
 *                  correction.  3: also on the fine level, which includes the operator of the inner CG.  Same bits at
 *                  every value; takes effect at the next apply.  Values outside 0..3 take the nearest level, here
 *                  and in the environment (before the levels, every non-zero value meant 1).  The first step needs Ct in the plain
 *                  row-per-lane-group form, the second the forms alfd_spmv_pair names; partitioned contexts,
 *                  grad_div_in_A = 0, w_inverse != diagonal and aug_assembled always use the separate launches.
 *   "ml_tail_in_spmv" (0/1, default 1; environment ALFD_ML_TAIL_IN_SPMV, read at alfd_create, where every non-zero
 *                  value means 1; here other values are refused with ALFD_E_INVALID): with "ml_fuse" >= 1, the
 *                  element-wise part of aug_tail_kernel for the rows Ct does NOT list runs at the block end of the
 *                  launch that forms y = A x (spmv_vs_kernel keeps the row sums of a block in LDS and applies the tail
 *                  to them; y is neither stored nor read back for those rows), and the tail launch shrinks to the rows
 *                  of Ct.  Same bits either way; takes effect at the next apply.  Used on a level only when A runs the
 *                  long-row batch-major kernel with 4 waves, dictionary + window + row buffer of its largest block
 *                  stay within 20 KB of LDS, and fewer than half of the rows are in Ct; never with the
 *                  single-precision values of the preconditioner, nor where "ml_fuse" keeps the separate launches.
 *                  A sweep step that has to deliver into the vector its own product reads (the only step of a
 *                  degree-2 sweep without a target to add to) keeps the two launches.  Costs two more vectors per
 *                  level that qualifies.
 *   "ml_tail_side_rows" (0/1, default 0; other values are refused with ALFD_E_INVALID): what "ml_tail_in_spmv" does with
 *                  an operator that has side rows ("batch_major_side_rows" = 1 and rows beyond 384 entries; one rank).
 *                  1: the launch with the block-end tail is followed, on the same stream and timed with it, by
 *                  spmv_side_rows_tail_kernel: one wave per side row forms the row sum of spmv_side_rows_kernel and
 *                  lane 0 stores y for a row of Ct, or applies the tail and stores no y, as the block end does for the
 *                  other rows.  0: such an operator keeps the two-launch tail (the launch with the block-end tail
 *                  refuses it).  Same bits either way.  A level qualifies at alfd_setup / alfd_setup_coupling (its two
 *                  extra vectors are allocated there) with the value of that moment; afterwards 0 / 1 switch the form
 *                  of a level that qualified at the next apply.  No launch of a context without side rows depends on it.
 *   "ml_gpu_galerkin" (0/1, default 1; environment ALFD_ML_GPU_GALERKIN, read at alfd_create): the Galerkin products of
 *                  alfd_setup with CSR prolongators and of the builders run on the device (alfd_sparse_product; inside
 *                  the builders and on replicated levels only for operators with more than 200 000 entries).  0: all
 *                  of them on the host.  Same bits either way; takes effect at the next alfd_setup / build.  The
 *                  level-0 product of a partitioned context runs on the device at either value.
 *   "ml_tail_rows" (>= 0, default 0 = off): the levels l >= 1 of the block-1 (immersed) hierarchy from the first one
 *                  with at most this many unknowns down to the coarsest run their part of the V-cycle in ONE launch
 *                  (ml_tail_kernel: one workgroup, a barrier where the launches were) instead of 15-21 launches per
 *                  level.  Same bits either way; takes effect at the next apply.  Used only when every operator of
 *                  those levels is stored as plain CSR rows, on one rank, with the diagonal W^-1 and the factored
 *                  operator; otherwise the launches.  Off by default: every level keeps all multiplier rows of M_l,
 *                  so at sizes where the launches matter one workgroup is slower.
 * Returns ALFD_E_INVALID for an unknown name. */
int alfd_set_tunable(alfd_ctx_t ctx, const char *name, int value);
/* Kernel-class timing of the last solve, accumulated with HIP events when
 * alfd_enable_timing(ctx, 1) was called before: class ids in alfd_timing_class. */
enum alfd_timing_class {
  ALFD_T_SPMV_A = 0,
  ALFD_T_SPMV_OTHER = 1,
  ALFD_T_DOT = 2,
  ALFD_T_VEC = 3,
  ALFD_T_NCLASSES = 4
};
int alfd_enable_timing(alfd_ctx_t ctx, int on); /* 0 off, 1 = A-SpMV launches only, 2 = all classes */
int alfd_get_timing(alfd_ctx_t ctx, double *ms /*[ALFD_T_NCLASSES]*/, int64_t *launches /*[..]*/,
                    double *algorithmic_bytes /*[..]*/);
/* The same launches priced by the bytes of the storage format each kernel reads (alfd_matrix_info::streamed_bytes for
 * the SpMV classes; equal to the algorithmic bytes for vector kernels): what a perfect cache would still move. */
int alfd_get_timing_streamed(alfd_ctx_t ctx, double *streamed_bytes /*[ALFD_T_NCLASSES]*/);
/* Wall seconds of the last uploads + alfd_setup by phase (host clock, device-synchronised at the phase ends): what
 * the reference's "Solve system" timer also contains (AMG setup, factorisations: stokes...:827, immersed_laplace.cc:504). */
enum alfd_setup_phase {
  ALFD_SETUP_UPLOAD = 0,        /* alfd_set_matrix calls since the last alfd_setup: format planning + copies to HBM */
  ALFD_SETUP_DIAG_LAMBDA = 1,   /* diag(Aug), lambda_max of the inner operators */
  ALFD_SETUP_ML_FETCH = 2,      /* multilevel: host copies of the level-0 operators */
  ALFD_SETUP_ML_GALERKIN = 3,   /* Galerkin products of all levels */
  ALFD_SETUP_ML_UPLOAD = 4,     /* level operators, transfers: format planning + copies */
  ALFD_SETUP_ML_LAMBDA = 5,     /* per-level diagonals and lambda_max */
  ALFD_SETUP_ML_PATCH = 6,      /* interface-patch operators + lambda_max */
  ALFD_SETUP_ML_COARSE = 7,     /* explicit coarsest inverse */
  ALFD_SETUP_NPHASES = 8
};
int alfd_get_setup_seconds(alfd_ctx_t ctx, double *seconds /*[ALFD_SETUP_NPHASES]*/);

#ifdef __cplusplus
}
#endif
#endif /* ALFD_H */
