// alfd.hip -- host side of libalfd.so: context, HBM-resident operators, the
// inner PCG, the AL preconditioner vmult()s, FGMRES, and the C ABI of
// include/alfd/alfd.h.  All arithmetic runs in the kernels of kernels.hpp; the
// host only sequences launches and does the O(m^2) Hessenberg/Givens algebra.
//
// Reference objects replaced (file:line in /root/reference):
//   * Aug = A + gamma Ct invW C                stokes_immersed_boundary.cc:991-993,
//                                              immersed_laplace.cc:880-884
//   * Aug_inv = inverse_operator(Aug, CG, prec) stokes...:1020-1045, immersed_laplace.cc:907-916
//   * Mp_inv  = inverse_operator(Mp, CG(100,1e-6), lumped diag)   stokes...:931-957
//   * BlockPreconditionerAugmentedLagrangian{,Stokes,Diagonal}::vmult
//                                              augmented_lagrangian_preconditioner.h:28-34,62-70,95-103
//   * AA = block_operator<..>                  stokes...:1000-1003, immersed_laplace.cc:891-892
//   * SolverFGMRES<BlockVector<double>>::solve stokes...:1067-1074 ([EXT] deal.II 9.6 flavour)
//   * SolverControl / ReductionControl / IterationNumberControl stop rules [EXT]
// There is NO CPU fallback: without a HIP device every entry point fails.

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <climits>
#include <condition_variable>
#include <functional>
#include <limits>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_set>
#include <utility>
#include <vector>

#include "alfd/alfd.h"
#include "kernels.hpp"
#include "kernels_vs.hpp"
#include "point_hierarchy.hpp"

namespace alfd {


// ------------------------------------------------------------------ helpers
#define HIPC(call)                                                                          \
  do {                                                                                      \
    hipError_t e__ = (call);                                                                \
    if (e__ != hipSuccess) {                                                                \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(e__) + " (" + __FILE__ + ":" + \
                 std::to_string(__LINE__) + ")";                                            \
      return ALFD_E_HIP;                                                                    \
    }                                                                                       \
  } while (0)
#define RC(call)                  \
  do {                            \
    int rc__ = (call);            \
    if (rc__ != ALFD_OK) return rc__; \
  } while (0)

static inline int64_t pad_chunk(int64_t n) { return (n + kChunk - 1) / kChunk * kChunk; }

struct DevCsr {
  bool present = false;
  int64_t nrows = 0, ncols = 0, nnz = 0;  // local rows, global cols
  int64_t n_list = 0;                     // rows the kernel iterates over (== nrows unless sparse)
  bool sparse = false;
  bool rep = false;  // replicated on every rank (coarse multigrid levels): never exchanges a halo
  bool derived = false;  // C / B built by the library as the transpose of an uploaded CT / BT
  int L = 64;
  int64_t longest = -1;                   // entries of the longest row, counted at upload (-1: not counted)
  int32_t n_local_cols = 0;               // columns < n_local_cols read x, others the halo
  int64_t *rp = nullptr;
  int32_t *col = nullptr;
  double *val = nullptr;
  int32_t *rows = nullptr;
  // multi-rank halo plan
  std::vector<int64_t> send_off, recv_off;  // per peer prefix (size nranks+1)
  std::vector<int32_t> halo_globals;        // global column id of every halo entry (host)
  int32_t *send_idx = nullptr;              // local indices to pack
  double *send_buf = nullptr, *halo = nullptr;
  int64_t n_halo = 0;
  std::vector<void *> owned;  // device arrays of this matrix (released on re-upload / destroy)
  // LDS-window format (long-row matrices): see spmv_window_kernel
  bool win = false;
  bool win_deferred = false, win_user = true;   // window plan not built yet (the batch-major form holds the matrix)
  int tag = 0;  // 1 = multigrid level matrix (separate kernel instantiation for profiling)
  int32_t win_RB = 0, win_maxW = 0;
  int64_t win_nblocks = 0, win_fallback_blocks = 0, win_nseg = 0;
  uint16_t *lcol = nullptr;
  // value-indexed blocks (see spmv_window_kernel): 8-bit dictionary index per entry
  bool vi = false;
  uint8_t *vidx = nullptr;
  int32_t *blk_dict_off = nullptr, *blk_dict_n = nullptr;
  double *dict = nullptr;
  int64_t vi_blocks = 0, vi_nnz = 0, vi_dict_total = 0, vi_wide_nnz = 0;
  uint16_t *vidw = nullptr;  // 16-bit value codes of the blocks with 257..512 distinct values
  uint64_t *vib_tab = nullptr;  // class-sorted row batches per block (spmv_window_vib_kernel)
  int32_t *vib_cnt = nullptr;
  int32_t vib_stride = 0;
  int32_t *blk_seg_begin = nullptr, *blk_W = nullptr, *seg_col = nullptr, *seg_off = nullptr;
  // batch-major format (spmv_vs_kernel, kernels_vs.hpp)
  struct Vs {
    bool on = false, bricks = false;
    int64_t nb = 0, nseg = 0, stream_bytes = 0, nbatch = 0, dict_total = 0, shared_nnz = 0;
    int32_t stride = 0, maxW = 0;
    int32_t tail_lds = 0;          // long rows: max over the blocks of vs_tail_lds_need, the LDS behind the dictionary region that a launch with the block-end epilogue asks for
    int32_t L = 64, tab_u64 = 16;  // lanes per row of the format; descriptor words per batch
    int32_t wide = 0;              // 10-bit codes / 11-bit window columns (VsFmt<1>)
    int32_t RB = 0, NW = 4;        // long rows: rows per block the plan was made with, waves per workgroup of its launches
    bool small = false;            // RB / NW chosen by vs_small_shape ("batch_major_small"), not the context's defaults
    uint8_t *stream = nullptr;
    int64_t *sb = nullptr;
    uint64_t *tab = nullptr;
    int32_t *cnt = nullptr, *seg_begin = nullptr, *blkW = nullptr, *seg_col = nullptr,
            *seg_off = nullptr, *doff = nullptr, *dn = nullptr;
    // long rows (spmv_vs_kernel): everything a block needs first is addressable from its index alone -- an 8-dword
    // header {batches, window slots, segments, dictionary size, dictionary offset, stream offset lo / hi, 0} and the
    // segment table with a fixed stride per block ((column, slot) pairs) -- so that the x window is requested after ONE
    // dependent round trip instead of two (header -> segment table -> x)
    int32_t *hdrb = nullptr, *segx = nullptr;
    int32_t seg_stride = 0;
    int64_t nb_interior = 0;     // partitioned contexts: the first nb_interior blocks read no halo column
    double *dict = nullptr;
    // side rows ("batch_major_side_rows", spmv_side_rows_kernel): the rows beyond kVsMaxLen entries, which no block
    // lists.  Every launch of the blocks is followed by launch_side on the same stream (VsPlan has the order of the list)
    int64_t side_n = 0, side_nnz = 0, side_longest = 0, side_interior = 0;
    int32_t *side_rows = nullptr, *side_col = nullptr;
    int64_t *side_rp = nullptr;
    double *side_val = nullptr;
  } vs;
  // bytes the kernel in use moves per launch (format bytes, x read once)
  double streamed_bytes(bool use_vi, bool use_vs = false) const {
    const double vec = (double)(n_list + 1) * 8.0 + (double)n_list * 8.0 + (double)(sparse ? n_list : ncols) * 8.0;
    if (vs.on && use_vs && use_vi)
      return (double)vs.stream_bytes + 8.0 * vs.tab_u64 * (double)vs.nbatch + 28.0 * (double)vs.nb +
             8.0 * (double)vs.nseg + 8.0 * (double)vs.dict_total + 8.0 * (double)nrows +
             8.0 * (double)(sparse ? n_list : ncols) + 12.0 * (double)(vs.side_nnz + vs.side_n);
    if (!win) return (double)nnz * 12.0 + vec;
    const double meta = (double)win_nblocks * 8.0 + (double)win_nseg * 8.0;
    if (!(vi && use_vi)) return (double)nnz * 10.0 + vec + meta;
    return (double)(vi_nnz - vi_wide_nnz) * 3.0 + (double)vi_wide_nnz * 4.0 + (double)(nnz - vi_nnz) * 10.0 + vec + meta + (double)vi_dict_total * 8.0 +
           (double)win_nblocks * (8.0 + (vib_tab ? 32.0 * vib_stride + 4.0 : 0.0));
  }
  // single-precision copy of val (slot A only, alfd_set_preconditioner_values): what the level-0 products inside the
  // inner preconditioner stream instead of val.  Not in `owned`: dropped with the request, too (a32_release)
  float *val32 = nullptr;
  int64_t val32_flushed = 0;   // entries whose binary32 image would be subnormal: stored as signed zeros
  // ... and the bytes of one launch on it: 4-byte values + 16-bit window columns, or + 32-bit columns
  double streamed_bytes32() const {
    const double vec = (double)(n_list + 1) * 8.0 + (double)n_list * 8.0 + (double)ncols * 8.0;
    if (!win) return (double)nnz * 8.0 + vec;
    return (double)nnz * 6.0 + vec + (double)win_nblocks * 8.0 + (double)win_nseg * 8.0;
  }
  double algorithmic_bytes() const {
    // nnz*(8+4) + (nrows+1)*8 + nrows*8 + ncols*8  (x read once)
    return (double)nnz * 12.0 + (double)(n_list + 1) * 8.0 + (double)n_list * 8.0 +
           (double)(sparse ? n_list : ncols) * 8.0;
  }
};

struct HostCsr {
  int64_t nrows = 0, ncols = 0;
  std::vector<int64_t> rp;
  std::vector<int32_t> col;
  std::vector<double> val;
  int64_t nnz() const { return rp.empty() ? 0 : rp.back(); }
};

constexpr int kScratchSlot = ALFD_NSLOTS;  // internal upload target (level matrices, batched systems)

// The operators and vectors of one multigrid level in ONE index space.  P / R connect the record to the record of the
// next finer level that the V-cycle pairs it with: loc to loc, rep to rep, and the loc pair of the first replicated level
// to the finer level's loc (MlLevel).
struct LevelStore {
  DevCsr A, C, Ct;   // operator pieces of this level (levels >= 1; level 0 uses the slots)
  DevCsr P, R;       // prolongation from this level to the next finer one, and R = P^T
  int64_t n = 0, npad = 0;
  double *dinv = nullptr, *r = nullptr, *z = nullptr, *t = nullptr, *cd = nullptr, *cres = nullptr, *ctmp = nullptr;
};

// One level of the aggregation multigrid hierarchy (level 0 = the augmented block itself).  loc holds this rank's rows.
// Multi-rank: levels from alfd_ctx::ml_rep_level on are REPLICATED on every rank (global operators and vectors, no halo
// exchanges) and run on rep, the whole level; rep.P / rep.R connect two replicated levels, loc.P / loc.R above stay
// rank-local.  A replicated level of the aggregate path keeps loc as well: its dinv and the restricted residual are
// gathered from there.
struct MlLevel {
  LevelStore loc, rep;
  double lmax = 0;
  uint8_t *tail_mask = nullptr;   // loc.npad bytes, 1 = row listed in Ct (aug_tail_kernel); null: this level runs unfused
  double *tail_z2 = nullptr, *tail_d2 = nullptr;   // second iterate / direction vector of a sweep whose tails run inside the A launch (build_tail_vectors); null: they do not
  bool P_global_cols = false;     // loc.P addresses the replicated coarse vector by GLOBAL ids (CSR prolongators)
  // the all-gather of the restricted residual from loc.r into rep.r (first replicated level)
  std::vector<int64_t> offs;      // rank offsets of this level's unknowns (size nranks + 1)
  int64_t maxpiece = 0;
  double *send = nullptr, *stage = nullptr;
};

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

struct TimedLaunch {
  int cls;
  hipEvent_t a, b;
};

}  // namespace alfd

using namespace alfd;

struct alfd_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t xstream = nullptr;                  // halo exchanges that run beside the interior row blocks of an SpMV
  hipEvent_t ev_x = nullptr, ev_halo = nullptr;
  hipEvent_t ev_in = nullptr;                     // *_device calls: the caller's stream up to the call (made on first use)
  int overlap_halo = -1;                          // ALFD_SPMV_OVERLAP_HALO: 1 on, 0 off, -1 (default): on for the in-process and
                                                  // host transports, off over RCCL until that path has run on hardware once
                                                  // (one communicator driven from two streams)
  std::string err;
  // partition / comm
  int rank = 0, nranks = 1;
  ncclComm_t nccl = nullptr;
  struct alfd_local_group *local = nullptr;  // in-process rank group (single-GPU emulation of N ranks)
  alfd_host_allgather_fn host_allgather = nullptr;   // host-transport rank group (MPI / gloo launchers)
  alfd_host_alltoallv_fn host_alltoallv = nullptr;
  void *host_user = nullptr;
  std::vector<char> host_send, host_recv;
  std::vector<std::vector<int64_t>> part;  // [block][nranks+1] global offsets
  // layout
  int nblocks = 0;
  int64_t n[ALFD_MAX_BLOCKS] = {0, 0, 0};        // local block lengths
  int64_t off[ALFD_MAX_BLOCKS + 1] = {0, 0, 0, 0};  // padded local offsets
  int64_t nmax = 0;                               // max padded block length
  int64_t diag_cap = 0;                           // length of the dA / s_aug scratch vectors
  DevCsr mat[ALFD_NSLOTS + 1];
  double *diag[ALFD_NDIAGS] = {nullptr, nullptr};
  int64_t diag_n[ALFD_NDIAGS] = {0, 0};
  alfd_config cfg;
  bool configured = false, is_setup = false;
  // alfd_set_preconditioner_values: a32_reason says why slot A holds no single-precision copy (NONE: it does);
  // a32_used, decided by alfd_setup: the inner preconditioner applies A through it; a32_view: the launches of slot A
  // between here and the end of the scope read it (A32Scope)
  int prec_values = ALFD_PREC_VALUES_FP64, a32_reason = ALFD_PREC_VALUES_NOT_REQUESTED;
  bool a32_used = false, a32_view = false;
  int a32_R = 4, a32_U = 16;                  // launch shape of the window kernel on the copy (ALFD_SPMV_PREC32_R / _U)
  unsigned long long *a32_counts = nullptr;   // device: {flushed to zero, without a finite image} of the last conversion
  // device workspace
  double *sc = nullptr;        // device scalar table
  double *sc_host = nullptr;   // pinned mirror
  double *partial = nullptr;   // dot partials [(kMaxBasis+2) * pstride]
  int64_t pstride = 0;
  double *gather = nullptr;    // multi-rank scalar all-gather buffer
  double *dinv_aug = nullptr, *dA = nullptr, *s_aug = nullptr;
  double *dinv_a22 = nullptr, *dinv_aug2 = nullptr;   // elliptic: 1/diag(A22_aug), [dinv_aug | dinv_a22]
  double lam_max[7] = {0, 0, 0, 0, 0, 0, 0};              // per inner operator kind
  double *dinv_k = nullptr;                            // rational: 1/diag(K)
  // exact W^-1 (alfd_config::w_inverse != 0): Jacobi CG on M nested inside the operator the
  // outer inner-CG runs on, so it owns a second set of CG vectors / scalar tables
  double *dinv_m = nullptr, *m_tmp = nullptr, *m_tmp2 = nullptr;
  double *n_r = nullptr, *n_z = nullptr, *n_p = nullptr, *n_Ap = nullptr;
  double *n_sc = nullptr, *n_sc_host = nullptr, *n_partial = nullptr, *n_gather = nullptr;
  int64_t mass_its = 0;
  // grad_div_in_A = 0 (Stokes): Aug = A + gamma Ct invW C + gamma_gd Bt Mp^-1 B.  The nested Mp solve shares the
  // n_* set with the mass solve above (n_owner: which of the two holds it, 0 = free); gd_bx / gd_q hold B x and q
  int n_owner = 0;
  double *gd_bx = nullptr, *gd_q = nullptr;
  int nmp_group = 16;               // iterations the host enqueues per state read ("nested_mp_group")
  int nmp_host_stepped = 0;         // "nested_mp_host_stepped" = 1: host-stepped pcg() on one rank too
  // alfd_estimate_spectrum: CG on C Ct over the compacted interface operators Ct[S,:], C[:,S] (S = non-empty rows of
  // Ct) -- the patch's when it is on, else extractions of its own (built on first use, released by the next setup)
  struct Spectrum {
    DevCsr own_Cs, own_Cts;
    DevCsr *Cs = nullptr, *Cts = nullptr;
    int64_t m = 0;                              // |S|
    double *t = nullptr, *ones = nullptr, *x = nullptr, *coef = nullptr, *linf = nullptr;
    int64_t coef_cap = 0;
    std::vector<void *> owned;                  // the vectors above
    std::vector<double> alpha, beta;            // coefficients of the last estimate
    bool have = false;
  } spec;
  int spec_group = 16;              // "spectrum_group": device-stepped iterations enqueued per state read
  int spec_host_stepped = 0;        // "spectrum_host_stepped" = 1: the same CG through the host-stepped pcg()
  // RationalPreconditioner state (batched CG over the 21 immersed systems)
  HostCsr h_M, h_K;                                    // host copies of the (tiny) immersed matrices
  // multilevel inner preconditioner: hier[0] on the augmented (1,1) block (A, C, Ct, gamma), hier[1] on the immersed
  // block A22 = A2 + gamma2 M invW M of the elliptic variants (A2, M, M, gamma2; CSR prolongators, one rank)
  struct Hierarchy {
    std::vector<int32_t> agg[ALFD_MAX_LEVELS];
    std::vector<double> wgt[ALFD_MAX_LEVELS];
    int64_t ncoarse[ALFD_MAX_LEVELS] = {0, 0, 0, 0, 0, 0, 0, 0};
    HostCsr P[ALFD_MAX_LEVELS];                // CSR prolongator of a level (alfd_set_prolongator), replaces its aggregates
    DevCsr inv;                                // explicit inverse of the coarsest operator (alfd_config::ml_coarse_direct)
    HostCsr coarse_A, coarse_C, coarse_Ct;     // host copies of the coarsest level of a CSR-prolongator hierarchy: what
                                               // coarse_inverse reads (alfd_setup_coupling replaces the last two only)
    std::vector<MlLevel> ml;
    TailTable *tail_tab = nullptr;             // level descriptors of ml_tail_kernel (hierarchy 1; setup workspace)
    bool built_partitioned = false;            // made by alfd_build_smoothed_aggregation on a partitioned context:
                                               // level 0 = local rows, alfd_setup fetches the whole fine support
    void clear_input() {
      for (int l = 0; l < ALFD_MAX_LEVELS; ++l) agg[l].clear(), wgt[l].clear(), P[l] = HostCsr(), ncoarse[l] = 0;
      built_partitioned = false;
    }
  } hier[2];
  // interface patch (alfd_config::ml_patch_degree > 0): S = non-empty rows of Ct, vectors of length |S|
  struct Patch {
    bool on = false;
    int64_t m = 0, mpad = 0;
    DevCsr Ass, As, Ats, Cs, Cts;              // A[S,S], A[S,:], A[:,S] (sparse rows), C[:,S], Ct[S,:]
    int32_t *S = nullptr;
    double *dinv = nullptr, *rS = nullptr, *zS = nullptr, *uS = nullptr, *eS = nullptr, *cd = nullptr,
           *cres = nullptr, *ctmp = nullptr, *rr = nullptr;
    double lmax = 0;
    uint8_t *tail_mask = nullptr;              // rows of Cts (aug_tail_kernel), as MlLevel::tail_mask
    // partitioned context: the patch is REPLICATED (Ass, Cs, Cts whole on every rank); S[] = this rank's rows
    // (m_loc of them, patch ids soff[rank] ..), Cts_loc / Ctg = Ct[S_loc, :] / Ct[owned rows, :] over GLOBAL
    // multiplier ids, As / Ats = this rank's rows of A[S, :] (halo on the fine vector) / A[:, S]
    bool rep = false;
    int64_t m_loc = 0, piece = 1, lam_piece = 1;
    std::vector<int64_t> soff;
    DevCsr Cts_loc, Ctg;
    double *send = nullptr, *stage = nullptr, *lam_send = nullptr, *lam_stage = nullptr, *loc = nullptr;
  } patch;
  // alfd_build_strength_graph: the node-graph rows of this rank's nodes (neighbours as GLOBAL node ids)
  struct StrengthGraph {
    bool have = false, on_device = false;     // on_device: sa_node_graph_kernel formed it (false: the joint host fallback)
    int64_t n_nodes = 0, node0 = 0;
    std::vector<int64_t> gp;
    std::vector<int32_t> gc, fixed;
    std::vector<double> gw, d;
  } sg;
  int ml_rep_level = -1;                      // first replicated level (multi-rank), -1: none
  bool dots_replicated = false;               // reductions over REPLICATED vectors (every rank holds the whole vector): no exchange
  int64_t ml_rep_threshold = 300000;          // replicate levels with at most this many unknowns (ALFD_ML_REPLICATE)
  int ml_fuse = 2;                            // fused smoother steps: aug_tail_kernel, pair launches ("ml_fuse", ALFD_ML_FUSE)
  int short_rows_per_thread = 1;              // "short_rows_per_thread": 4- and 8-lane operators with rows of at most 2 L entries run on spmv_rowlane_kernel (0: spmv_kernel<L>)
  int ml_tail_in_spmv = 1;                    // "ml_tail_in_spmv", ALFD_ML_TAIL_IN_SPMV: the element-wise tails at the block end of the batch-major A launch
  int ml_tail_side_rows = 0;                  // "ml_tail_side_rows" = 1: an operator with side rows runs that form too, its side rows' tails in spmv_side_rows_tail_kernel
  int64_t fused_tail_launches = 0;            // launches of that form since alfd_create (alfd_get_fused_tail_launches)
  int ml_tail_rows = 0;                       // "ml_tail_rows": levels >= 1 of hierarchy 1 with at most this many unknowns
                                              // run in one launch (ml_tail_kernel); 0 = off (the measured default)
  int ml_gpu_galerkin = 1;                    // Galerkin products of CSR-prolongator levels on the device (ALFD_ML_GPU_GALERKIN)
  double *g_w = nullptr, *g_tlam = nullptr;   // global W^-1 diagonal and multiplier work vector of the replicated levels
  std::vector<int64_t> ml_coff[ALFD_MAX_LEVELS];       // rank offsets of the coarse dofs of each level
  const int64_t *up_col_offsets = nullptr;             // upload_matrix overrides (level matrices)
  bool up_local_only = false;
  DevCsr rat_mat;                                      // block-diagonal [S_1 .. S_20, M]
  double *rt_r = nullptr, *rt_z = nullptr, *rt_p = nullptr, *rt_Ap = nullptr, *rt_x = nullptr;
  double *rt_dinv = nullptr, *rt_partial = nullptr, *rt_scb = nullptr, *rt_coef = nullptr;
  double *rt_scb_host = nullptr;
  int64_t rational_its = 0;
  int64_t wmax = 0;                                    // length of the inner-solve work vectors
  std::vector<void *> ws_allocs;                       // workspace of the current setup()
  double *w_r = nullptr, *w_z = nullptr, *w_p = nullptr, *w_Ap = nullptr;  // PCG
  double *c_d = nullptr, *c_res = nullptr, *c_tmp = nullptr;               // Chebyshev
  double *t_lam = nullptr;                                                 // invW .* (C x)
  double *q_tmp = nullptr, *rhs_tmp = nullptr;                             // precond scratch
  double *V = nullptr, *Z = nullptr, *xb = nullptr, *bb = nullptr, *io = nullptr;
  double *st_in = nullptr, *st_out = nullptr;   // staging of the depth-1 calls (the resident rhs / guess stay intact)
  double lambda_max = 0, lambda_min = 0;
  // stats of the current solve
  int64_t inner_its = 0, mp_its = 0;
  int64_t inner_its_op[3] = {0, 0, 0};            // inner_its by alfd_inner_op (alfd_get_inner_iterations)
  int inner_failures = 0, precond_applications = 0;
  std::vector<double> history;
  // timing
  int timing = 0;  // 0 off, 1 = A-SpMV launches only (cheap), 2 = every kernel class
  std::vector<TimedLaunch> timed;
  double t_ms[ALFD_T_NCLASSES] = {0, 0, 0, 0};
  int64_t t_launches[ALFD_T_NCLASSES] = {0, 0, 0, 0};
  double t_bytes[ALFD_T_NCLASSES] = {0, 0, 0, 0};
  double t_fbytes[ALFD_T_NCLASSES] = {0, 0, 0, 0};   // the same launches priced by format bytes
  double setup_s[ALFD_SETUP_NPHASES] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool upload_since_setup = false;
  // alfd_setup_coupling: what the last successful setup of either kind saw.  gen / dgen count the uploads per slot and
  // diagonal; needs_full names an input (prolongator, aggregates, row-block hint) set since then, which only alfd_setup
  // takes in; coupling_ready = 0 until an alfd_setup succeeds and again after a setup of either kind fails half way.
  uint64_t gen[ALFD_NSLOTS + 1] = {}, gen_setup[ALFD_NSLOTS + 1] = {};
  uint64_t dgen[ALFD_NDIAGS] = {}, dgen_setup[ALFD_NDIAGS] = {};
  alfd_config cfg_setup;
  const char *needs_full = nullptr;
  bool coupling_ready = false;
  int64_t setup_counts[ALFD_SC_NCOUNTS] = {};
  std::vector<void *> cp_allocs[2];                    // the setup workspace that alfd_setup_coupling replaces, per hierarchy
  std::vector<void *> allocs;
  int spmv_stream_R = 2, spmv_stream_U = 8, spmv_nt = 0, spmv_grid_mult = 8;  // tunables (env ALFD_SPMV_*)
  int spmv_group_R = 4, spmv_group_U = 4;  // batch shape of the short-row window kernel
  bool vi_off = false;                      // alfd_bench_spmv_format: time the plain 10 B/nnz kernel on a value-indexed matrix
  int vi_rows_R = 4, vi_rows_J = 2;         // row-batched VI kernel shape (ALFD_SPMV_VI_R=0: stream-ordered VI kernel)
  int vi_xcd = 0;                           // XCD-contiguous row-block order in the class-batched kernel
  int vi_levels = 1;                        // also dictionary-code multigrid level matrices
                        // waves per workgroup of the class-batched kernel (4 or 8)
  int vi_batched = 1;                       // class-batched VI kernel (ALFD_SPMV_VI_BATCHED=0: in-order batches)
  int win_RB_vi = 96;                       // row block of value-indexed matrices (ALFD_SPMV_WINDOW_RB_VI)
  int win_vi = 1;                           // dictionary-coded values in window blocks (ALFD_SPMV_VALUE_INDEX)
  int win_short_scale = 2;                  // short-row block = min(512, win_RB * scale * 64 / L) rows; 0 = off
  int vs_enable = 1, vs_NW = 4, vs_RB = 96, vs_xcd = 0, vs_share = 1, vs_wide = 1;
  int vs_side = 0;                          // "batch_major_side_rows": rows beyond kVsMaxLen entries go to a side list (build_vs)
  int vs_small = 1;                         // "batch_major_small": level / patch operators that leave the chip under-filled get smaller row blocks (vs_small_shape)
  int vs_cus = 0;                           // compute units of the device (hipDeviceProp_t::multiProcessorCount)
  int vs_force_RB = 0, vs_force_NW = 0;     // alfd_bench_operator: the shape of the next build_vs, whatever the rule says
  int vs_lds_base_ok = -1;                  // -1 unknown; the absolute LDS addressing of kernels_vs.hpp needs base 0   // batch-major format (alfd_set_tunable "batch_major")
  std::vector<int64_t> rb_ptr[ALFD_NSLOTS + 1];   // row-block hint per slot (alfd_set_row_blocks)
  std::vector<int32_t> rb_rows[ALFD_NSLOTS + 1];
  // alfd_set_numbering: internal index k of block 0 is the caller's index n2o[k] (empty: none).  The device copies are
  // int32, padded with zeros to whole chunks (the index loads of pack / unpack); stage: one block-0 vector in the
  // caller's order, the stop of the host-pointer calls on their way through the same kernels.
  struct Numbering {
    std::vector<int64_t> n2o, o2n;
    int32_t *perm = nullptr, *inv = nullptr;
    double *stage = nullptr;
    int64_t n() const { return (int64_t)n2o.size(); }
    bool on() const { return !n2o.empty(); }
  } num;
  int num_unpack_scatter = 0;               // "numbering_unpack_scatter": unpack_blocks_perm_scatter_kernel instead of the gather form
  int win_short_min_blocks = 256;           // the same for short-row matrices (ALFD_SPMV_WINDOW_SHORT_MIN_BLOCKS; 64 costs cfg 3 30 %, 1024 leaves its 262 k-row level operator out)
  int win_min_blocks = 256;                 // long-row window formats need this many row blocks (ALFD_SPMV_WINDOW_MIN_BLOCKS; 1 per CU: the level-2 operator of the bench, 152 k rows, gains 2 % of the solve, the 36.7 k-row patch matrix another 1 %; 128: slower)
  int win_enable = 1, win_RB = 96, win_maxW = 4096, win_gap = 8, win_xcd = 0;  // win_xcd: XCD-contiguous block order (measured neutral on MI355X)
  alfd_spmv_launch last_spmv = {};          // what the last SpMV launch instantiated (note_spmv, alfd_get_last_spmv_launch)
  bool has_last_spmv = false;
  int64_t ntot() const { return off[nblocks]; }
};

// ---------------------------------------------------------------------------
// In-process rank group: N contexts in ONE process (one host thread per rank)
// exchange through device-to-device copies and a host barrier instead of RCCL.
// It exists so that everything of the multi-rank path except the literal RCCL
// calls (halo plans, pack kernels, halo SpMV, ordered reductions, setup
// protocol) can be executed on a single-GPU box; one process per GPU over
// RCCL remains the production configuration.
struct alfd_local_group {
  int n = 0;
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  long generation = 0;
  std::vector<const void *> buf;            // per rank: published buffer
  std::vector<const int64_t *> off;         // per rank: published prefix (alltoallv)
  void barrier() {
    std::unique_lock<std::mutex> lk(mu);
    const long g = generation;
    if (++arrived == n) {
      arrived = 0;
      ++generation;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return generation != g; });
    }
  }
};

namespace alfd {

// all-gather of `bytes` per rank, device buffers, result ordered by rank
static int comm_allgather(alfd_ctx *ctx, const void *send, void *recv, size_t bytes) {
  if (ctx->local) {
    alfd_local_group *g = ctx->local;
    HIPC(hipStreamSynchronize(ctx->stream));
    g->buf[ctx->rank] = send;
    g->barrier();
    for (int p = 0; p < g->n; ++p)
      HIPC(hipMemcpyAsync((char *)recv + (size_t)p * bytes, g->buf[p], bytes, hipMemcpyDeviceToDevice,
                          ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    g->barrier();
    return ALFD_OK;
  }
  if (ctx->host_allgather) {
    ctx->host_send.resize(bytes);
    ctx->host_recv.resize(bytes * (size_t)ctx->nranks);
    HIPC(hipMemcpyAsync(ctx->host_send.data(), send, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    if (ctx->host_allgather(ctx->host_user, ctx->host_send.data(), ctx->host_recv.data(), bytes) != 0)
      return ctx->err = "host all-gather callback failed", ALFD_E_COMM;
    HIPC(hipMemcpyAsync(recv, ctx->host_recv.data(), ctx->host_recv.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));   // the staging buffer is reused by the next collective
    return ALFD_OK;
  }
  if (ncclAllGather(send, recv, bytes, ncclChar, ctx->nccl, ctx->stream) != ncclSuccess)
    return ctx->err = "ncclAllGather failed", ALFD_E_COMM;
  return ALFD_OK;
}

// personalised exchange: rank r sends sendbuf[send_off[p] .. send_off[p+1]) to p and
// receives recvbuf[recv_off[p] .. recv_off[p+1]) from p (element size `es` bytes)
static int comm_alltoallv(alfd_ctx *ctx, const void *sendbuf, const int64_t *send_off, void *recvbuf,
                          const int64_t *recv_off, size_t es, hipStream_t st = nullptr) {
  if (!st) st = ctx->stream;
  if (ctx->local) {
    alfd_local_group *g = ctx->local;
    HIPC(hipStreamSynchronize(st));
    g->buf[ctx->rank] = sendbuf;
    g->off[ctx->rank] = send_off;
    g->barrier();
    for (int p = 0; p < g->n; ++p) {
      const int64_t nr = recv_off[p + 1] - recv_off[p];
      if (nr > 0)  // what p sends to me starts at p's send_off[my rank]
        HIPC(hipMemcpyAsync((char *)recvbuf + (size_t)recv_off[p] * es,
                            (const char *)g->buf[p] + (size_t)g->off[p][ctx->rank] * es, (size_t)nr * es,
                            hipMemcpyDeviceToDevice, st));
    }
    HIPC(hipStreamSynchronize(st));
    g->barrier();
    return ALFD_OK;
  }
  if (ctx->host_alltoallv) {
    const size_t ns = (size_t)send_off[ctx->nranks] * es, nr = (size_t)recv_off[ctx->nranks] * es;
    ctx->host_send.resize(std::max<size_t>(ns, 1));
    ctx->host_recv.resize(std::max<size_t>(nr, 1));
    if (ns) HIPC(hipMemcpyAsync(ctx->host_send.data(), sendbuf, ns, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    if (ctx->host_alltoallv(ctx->host_user, ctx->host_send.data(), send_off, ctx->host_recv.data(), recv_off, es) != 0)
      return ctx->err = "host all-to-all callback failed", ALFD_E_COMM;
    if (nr) HIPC(hipMemcpyAsync(recvbuf, ctx->host_recv.data(), nr, hipMemcpyHostToDevice, st));
    HIPC(hipStreamSynchronize(st));
    return ALFD_OK;
  }
  if (ncclGroupStart() != ncclSuccess) return ctx->err = "ncclGroupStart", ALFD_E_COMM;
  const char *failed = nullptr;  // the group is closed on every path: an open group would strand the peers
  for (int p = 0; p < ctx->nranks && !failed; ++p) {
    const int64_t ns = send_off[p + 1] - send_off[p], nr = recv_off[p + 1] - recv_off[p];
    if (ns > 0 && ncclSend((const char *)sendbuf + (size_t)send_off[p] * es, (size_t)ns * es, ncclChar, p,
                           ctx->nccl, st) != ncclSuccess)
      failed = "ncclSend";
    if (!failed && nr > 0 &&
        ncclRecv((char *)recvbuf + (size_t)recv_off[p] * es, (size_t)nr * es, ncclChar, p, ctx->nccl,
                 st) != ncclSuccess)
      failed = "ncclRecv";
  }
  if (ncclGroupEnd() != ncclSuccess && !failed) failed = "ncclGroupEnd";
  if (failed) return ctx->err = failed, ALFD_E_COMM;
  return ALFD_OK;
}

}  // namespace alfd

namespace alfd {

template <class T>
static int dev_alloc(alfd_ctx *ctx, T **p, int64_t count) {
  void *q = nullptr;
  HIPC(hipMalloc(&q, std::max<int64_t>(count, 1) * sizeof(T)));
  ctx->allocs.push_back(q);
  *p = static_cast<T *>(q);
  return ALFD_OK;
}
static int dev_alloc_zero(alfd_ctx *ctx, double **p, int64_t count) {
  RC(dev_alloc(ctx, p, count));
  HIPC(hipMemsetAsync(*p, 0, std::max<int64_t>(count, 1) * sizeof(double), ctx->stream));
  return ALFD_OK;
}

template <class T>
static int csr_alloc(alfd_ctx *ctx, DevCsr &m, T **p, int64_t count) {
  void *q = nullptr;
  HIPC(hipMalloc(&q, std::max<int64_t>(count, 1) * sizeof(T)));
  m.owned.push_back(q);
  *p = static_cast<T *>(q);
  return ALFD_OK;
}
static void csr_free(DevCsr &m) {
  for (void *q : m.owned) hipFree(q);
  if (m.val32) hipFree(m.val32);
  m = DevCsr();
}

// the compacted operators and vectors of alfd_estimate_spectrum (the coefficients of the last estimate go with them)
static void spectrum_release(alfd_ctx *ctx) {
  csr_free(ctx->spec.own_Cs);
  csr_free(ctx->spec.own_Cts);
  for (void *q : ctx->spec.owned) hipFree(q);
  ctx->spec = alfd_ctx::Spectrum();
}

static inline int grid_for_rows(int64_t nrows, int L) {
  const int64_t groups = (nrows + (kBlock / L) - 1) / (kBlock / L);
  // 256 CUs x 8 resident 256-thread workgroups; grid-stride beyond that
  return (int)std::max<int64_t>(1, std::min<int64_t>(groups, 256 * 8));
}

struct Timer {
  alfd_ctx *ctx;
  int cls;
  hipEvent_t a = nullptr, b = nullptr;
  bool on;
  Timer(alfd_ctx *c, int cl, double bytes, double fbytes = -1.0) : ctx(c), cls(cl) {
    on = ctx->timing >= 2 || (ctx->timing == 1 && cl == ALFD_T_SPMV_A);
    if (on) {
      hipEventCreate(&a);
      hipEventCreate(&b);
      hipEventRecord(a, ctx->stream);
      ctx->t_bytes[cls] += bytes;
      ctx->t_fbytes[cls] += fbytes < 0.0 ? bytes : fbytes;
      ctx->t_launches[cls]++;
    }
  }
  ~Timer() {
    if (on) {
      hipEventRecord(b, ctx->stream);
      ctx->timed.push_back({cls, a, b});
    }
  }
};

// accumulates the wall time of a setup phase (device-synchronised at its end)
struct PhaseClock {
  alfd_ctx *ctx;
  int phase;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  PhaseClock(alfd_ctx *c, int ph) : ctx(c), phase(ph) {}
  ~PhaseClock() {
    hipStreamSynchronize(ctx->stream);
    ctx->setup_s[phase] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
};

static void flush_timers(alfd_ctx *ctx) {
  for (auto &t : ctx->timed) {
    hipEventSynchronize(t.b);
    float ms = 0;
    hipEventElapsedTime(&ms, t.a, t.b);
    ctx->t_ms[t.cls] += ms;
    hipEventDestroy(t.a);
    hipEventDestroy(t.b);
  }
  ctx->timed.clear();
}

// ------------------------------------------------------------------- SpMV
// ---- a run-time value as a template argument.  with_const<Vs...>(v, f) hands f the one of Vs... that v equals, as a
// std::integral_constant (f reads it as decltype(c)::value), and answers whether there was one.  with_const_or_last gives
// whatever is not listed to the last listed value: the `else` / `default:` of a hand-written ladder.  Every launcher
// turns its epilogue, matrix tag, lane count, wave count and tail mode into template arguments with these.
template <int... Vs, class F>
static inline bool with_const(int v, F &&f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>()), true) : false) || ...);
}
template <int V, int... Vs, class F>
static inline void with_const_or_last(int v, F &&f) {
  if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V>());
  else if (v == V) f(std::integral_constant<int, V>());
  else with_const_or_last<Vs...>(v, f);
}
template <class F> static inline void with_epi(int epi, F &&f) { with_const_or_last<0, 1, 2, 3>(epi, f); }
template <class F> static inline void with_flag(int flag, F &&f) { with_const_or_last<0, 1>(flag, f); }   // matrix tag, bool
template <class F> static inline void with_lanes(int L, F &&f) { with_const_or_last<4, 8, 16, 32, 64>(L, f); }

// ---- the (R, U) launch shapes the ALFD_SPMV_* variables select ("Launch shapes from the environment"):
// each list once, in the order it is searched.  with_shape looks (R, U) up in one of them and hands f the pair as two
// constants.  A pair the list lacks answers false, and the caller falls through to the next kernel family; with or_last
// it runs the last entry instead.
struct Shape { int R, U; };
constexpr Shape kStreamShapes[] = {{2, 2}, {2, 4}, {4, 2}, {4, 4}, {4, 8}, {8, 4}, {8, 8}, {1, 4}, {2, 8}, {8, 2}};
constexpr Shape kWindowShapes[] = {{1, 4}, {2, 4}, {2, 8}, {4, 2}, {4, 4}, {4, 8}, {8, 4}, {1, 8}, {1, 16}, {2, 16}};
constexpr Shape kGroupShapes[] = {{4, 4}, {2, 4}, {4, 2}, {8, 4}, {8, 2}};
// (R, J) of the in-order value-indexed kernel; the last one is the default
constexpr Shape kViShapes[] = {{4, 3}, {2, 4}, {4, 4}, {4, 2}};
// the window kernel on the single-precision copy of A.  (4, 16), the last, is the measured choice (profiles/prec_values/:
// 0.90 of the 8-byte kernel's time per launch at N = 56, where (2, 8), the shape of the 8-byte kernel, takes 1.18 of it);
// the other candidates stay selectable for re-measuring
constexpr Shape kWindow32Shapes[] = {{2, 8}, {4, 8}, {2, 16}, {4, 16}};

template <const auto &Tab, class F, size_t... I>
static inline bool with_shape_at(size_t i, F &&f, std::index_sequence<I...>) {
  return ((i == I ? (f(std::integral_constant<int, Tab[I].R>(), std::integral_constant<int, Tab[I].U>()), true) : false) || ...);
}
template <const auto &Tab, class F>
static inline bool with_shape(int R, int U, bool or_last, F &&f) {
  constexpr size_t N = sizeof(Tab) / sizeof(Shape);
  size_t i = 0;
  while (i < N && (Tab[i].R != R || Tab[i].U != U)) ++i;
  if (i == N && or_last) i = N - 1;
  return with_shape_at<Tab>(i, f, std::make_index_sequence<N>());
}

// The record of alfd_get_last_spmv_launch: every launcher below calls this beside its hipLaunchKernelGGL, inside the lambda
// that holds the template arguments as constants, with those constants and the grid / LDS / block-order arguments it
// passes, so that the record cannot disagree with the launch.  Host side, a few stores.
static inline void note_spmv(alfd_ctx *ctx, int family, int lanes, int R, int U, bool nt, int epi, int xcd, int64_t grid,
                             size_t lds) {
  ctx->last_spmv = alfd_spmv_launch{family, lanes, R, U, nt ? 1 : 0, epi, xcd, grid, (int64_t)lds};
  ctx->has_last_spmv = true;
}

template <int L>
static void launch_spmv_L(alfd_ctx *ctx, const DevCsr &m, const double *x, double *y, int epi, double alpha,
                          const double *d, double *y2) {
  const int grid = grid_for_rows(m.n_list, L);
  with_epi(epi, [&](auto e) {
    with_flag(m.sparse, [&](auto sp) {
      constexpr int EPI = decltype(e)::value;
      constexpr bool SP = decltype(sp)::value != 0;
      note_spmv(ctx, SP ? ALFD_SPMV_SPARSE_ROWS : ALFD_SPMV_PLAIN, L, 0, 0, false, EPI, 0, grid, 0);
      hipLaunchKernelGGL((spmv_kernel<L, EPI, SP>), dim3(grid), dim3(kBlock), 0, ctx->stream, m.n_list, m.rp, m.col, m.val,
                         m.rows, x, m.halo, m.n_local_cols, y, alpha, d, y2);
    });
  });
}
// spmv_kernel at the lane count of m, whatever other forms m has
static void launch_spmv(alfd_ctx *ctx, const DevCsr &m, const double *x, double *y, int epi, double alpha, const double *d,
                        double *y2) {
  with_lanes(m.L, [&](auto l) { launch_spmv_L<decltype(l)::value>(ctx, m, x, y, epi, alpha, d, y2); });
}

// ---- one thread per row (spmv_rowlane_kernel): taken exactly where spmv_launch_local would launch
// spmv_kernel<L, EPI, false> with L 4 or 8 and EPI 0 or 1, when no row has more than 2 L entries.  Same bits.
static inline bool rowlane_form(const alfd_ctx *ctx, const DevCsr &m, int epi) {
  return ctx->short_rows_per_thread && !m.sparse && (m.L == 4 || m.L == 8) && (epi == 0 || epi == 1) && m.longest >= 0 &&
         m.longest <= 2 * m.L && m.n_list <= (int64_t)INT32_MAX * kBlock;
}
static void launch_rowlane(alfd_ctx *ctx, const DevCsr &m, const double *x, double *y, int epi, double alpha) {
  const int64_t grid = (m.n_list + kBlock - 1) / kBlock;   // one row per thread
  with_const<4, 8>(m.L, [&](auto l) {
    with_flag(epi, [&](auto e) {
      constexpr int L = decltype(l)::value, EPI = decltype(e)::value;
      note_spmv(ctx, ALFD_SPMV_ROW_LANE, L, 0, 0, false, EPI, 0, grid, 0);
      hipLaunchKernelGGL((spmv_rowlane_kernel<L, EPI>), dim3((unsigned)grid), dim3(kBlock), 0, ctx->stream, m.n_list, m.rp, m.col,
                         m.val, x, m.halo, m.n_local_cols, y, alpha);
    });
  });
}

// workgroups of the stream kernel: 4 waves, a batch of R rows per wave and pass
static inline int stream_grid(const alfd_ctx *ctx, int64_t nrows, int R) {
  const int64_t nbatches = (nrows + R - 1) / R;
  return (int)std::max<int64_t>(1, std::min<int64_t>((nbatches + 3) / 4, 256 * ctx->spmv_grid_mult));
}

template <bool NT>
static bool launch_stream_RU(alfd_ctx *ctx, const DevCsr &m, const double *x, double *y, int epi,
                             double alpha, const double *d, double *y2) {
  return with_shape<kStreamShapes>(ctx->spmv_stream_R, ctx->spmv_stream_U, false, [&](auto r, auto u) {
    with_epi(epi, [&](auto e) {
      constexpr int R = decltype(r)::value, U = decltype(u)::value, EPI = decltype(e)::value;
      const int grid = stream_grid(ctx, m.nrows, R);
      note_spmv(ctx, ALFD_SPMV_STREAM, 64, R, U, NT, EPI, 0, grid, 0);
      hipLaunchKernelGGL((spmv_stream_kernel<R, U, EPI, NT>), dim3(grid), dim3(kBlock), 0, ctx->stream, m.nrows, m.rp,
                         m.col, m.val, x, m.halo, m.n_local_cols, y, alpha, d, y2, NoPair());
    });
  });
}

// the windowed 64-lane kernels: class-batched value-indexed, in-order value-indexed, general
template <int R, int U>
static void launch_window(alfd_ctx *ctx, const DevCsr &m, const double *x, double *y, int epi, double alpha,
                          const double *d, double *y2) {
  const bool vi = m.vi && !ctx->vi_off;
  const size_t lds = (size_t)(m.win_maxW + (vi ? kDictMaxEntries : 0)) * sizeof(double);
  const dim3 grid((unsigned)m.win_nblocks);
  with_epi(epi, [&](auto e) {
    constexpr int EPI = decltype(e)::value;
    if (vi && ctx->vi_batched && m.vib_tab) {
      with_flag(m.tag, [&](auto t) {
        constexpr int TAG = decltype(t)::value;
        note_spmv(ctx, ALFD_SPMV_WINDOW_VIB, 64, 0, 0, false, EPI, ctx->vi_xcd, m.win_nblocks, lds);
        hipLaunchKernelGGL((spmv_window_vib_kernel<EPI, TAG>), grid, dim3(kBlock), lds, ctx->stream, m.nrows, m.win_RB,
                           m.rp, m.col, m.lcol, m.val, m.blk_seg_begin, m.blk_W, m.seg_col, m.seg_off, x, m.halo,
                           m.n_local_cols, y, alpha, d, y2, m.vidx, m.vidw, m.blk_dict_off, m.blk_dict_n, m.dict,
                           m.win_maxW, m.vib_tab, m.vib_cnt, m.vib_stride, ctx->vi_xcd);
      });
    } else if (vi && ctx->vi_rows_R > 0) {
      with_shape<kViShapes>(ctx->vi_rows_R, ctx->vi_rows_J, true, [&](auto rv, auto jv) {
        constexpr int RV = decltype(rv)::value, JV = decltype(jv)::value;
        note_spmv(ctx, ALFD_SPMV_WINDOW_VI, 64, RV, JV, false, EPI, 0, m.win_nblocks, lds);
        hipLaunchKernelGGL((spmv_window_vi_kernel<RV, JV, EPI>), grid, dim3(kBlock), lds, ctx->stream, m.nrows, m.win_RB,
                           m.rp, m.col, m.lcol, m.val, m.blk_seg_begin, m.blk_W, m.seg_col, m.seg_off, x, m.halo,
                           m.n_local_cols, y, alpha, d, y2, m.vidx, m.vidw, m.blk_dict_off, m.blk_dict_n, m.dict,
                           m.win_maxW);
      });
    } else {
      with_flag(m.tag, [&](auto t) {
        constexpr int TAG = decltype(t)::value;
        note_spmv(ctx, ALFD_SPMV_WINDOW, 64, R, U, false, EPI, ctx->win_xcd, m.win_nblocks, lds);
        hipLaunchKernelGGL((spmv_window_kernel<R, U, EPI, TAG>), grid, dim3(kBlock), lds, ctx->stream, m.nrows, m.win_RB,
                           m.rp, m.col, m.lcol, m.val, m.blk_seg_begin, m.blk_W, m.seg_col, m.seg_off, x, m.halo,
                           m.n_local_cols, y, alpha, d, y2, ctx->win_xcd);
      });
    }
  });
}

// the windowed kernel of L-lane rows, L < 64
template <int L>
static bool launch_window_group_RU(alfd_ctx *ctx, const DevCsr &m, const double *x, double *y, int epi,
                                   double alpha, const double *d, double *y2) {
  const size_t lds = (size_t)m.win_maxW * sizeof(double);
  return with_shape<kGroupShapes>(ctx->spmv_group_R, ctx->spmv_group_U, false, [&](auto r, auto u) {
    with_epi(epi, [&](auto e) {
      with_flag(m.tag, [&](auto t) {
        constexpr int R = decltype(r)::value, U = decltype(u)::value, EPI = decltype(e)::value, TAG = decltype(t)::value;
        note_spmv(ctx, ALFD_SPMV_WINDOW_GROUP, L, R, U, false, EPI, 0, m.win_nblocks, lds);
        hipLaunchKernelGGL((spmv_window_group_kernel<L, R, U, EPI, TAG>), dim3((unsigned)m.win_nblocks), dim3(kBlock), lds,
                           ctx->stream, m.nrows, m.win_RB, m.rp, m.col, m.lcol, m.val, m.blk_seg_begin, m.blk_W, m.seg_col,
                           m.seg_off, x, m.halo, m.n_local_cols, y, alpha, d, y2);
      });
    });
  });
}

static bool launch_window_RU(alfd_ctx *ctx, const DevCsr &m, const double *x, double *y, int epi,
                             double alpha, const double *d, double *y2) {
  bool ok = false;
  if (with_const<32, 16, 8>(m.L, [&](auto l) { ok = launch_window_group_RU<decltype(l)::value>(ctx, m, x, y, epi, alpha, d, y2); }))
    return ok;
  if (m.L != 64) return false;
  return with_shape<kWindowShapes>(ctx->spmv_stream_R, ctx->spmv_stream_U, false, [&](auto r, auto u) {
    launch_window<decltype(r)::value, decltype(u)::value>(ctx, m, x, y, epi, alpha, d, y2);
  });
}
// ---- the single-precision copy of slot A (alfd_set_preconditioner_values): the float instantiations
// of the three kernel families a 64-lane operator with 8-byte values runs on, epilogues 0 and 1 (all that level 0 of the
// cycle uses).  A kernel loads a float, widens it (exact) and forms the canonical sums, so the shape of the launch does
// not show in the result: one shape per family, whatever ALFD_SPMV_STREAM_R / _U name for the 8-byte kernels (the window
// kernel keeps its measured candidates behind ALFD_SPMV_PREC32_R / _U).
struct A32Scope {   // launches of slot A inside the scope read the copy
  alfd_ctx *ctx;
  bool was;
  A32Scope(alfd_ctx *c, bool on) : ctx(c), was(c->a32_view) { if (on) c->a32_view = true; }
  ~A32Scope() { ctx->a32_view = was; }
};
static inline bool a32_active(const alfd_ctx *ctx, const DevCsr &m) {
  return ctx->a32_view && &m == &ctx->mat[ALFD_A] && m.val32;
}
// 2 window, 1 stream, 0 plain: the family spmv_launch_local's choice for the 8-byte values belongs to
static inline int a32_family(const alfd_ctx *ctx, const DevCsr &m) { return m.win ? 2 : ctx->spmv_stream_R > 0 ? 1 : 0; }

static int spmv_launch_a32(alfd_ctx *ctx, const DevCsr &m, const double *x, double *y, int epi, double alpha) {
  if (epi != 0 && epi != 1) return ctx->err = "the single-precision copy of A has epilogues 0 and 1 only", ALFD_E_UNSUPPORTED;
  const int family = a32_family(ctx, m);
  const double *no_d = nullptr;
  double *no_y2 = nullptr;
  with_flag(epi, [&](auto e) {
    constexpr int EPI = decltype(e)::value;
    if (family == 2) {
      const size_t lds = (size_t)m.win_maxW * sizeof(double);
      with_shape<kWindow32Shapes>(ctx->a32_R, ctx->a32_U, true, [&](auto r, auto u) {
        constexpr int R = decltype(r)::value, U = decltype(u)::value;
        note_spmv(ctx, ALFD_SPMV_WINDOW_F32, 64, R, U, false, EPI, ctx->win_xcd, m.win_nblocks, lds);
        hipLaunchKernelGGL((spmv_window_kernel<R, U, EPI, 0, float>), dim3((unsigned)m.win_nblocks), dim3(kBlock), lds,
                           ctx->stream, m.nrows, m.win_RB, m.rp, m.col, m.lcol, m.val32, m.blk_seg_begin, m.blk_W, m.seg_col,
                           m.seg_off, x, m.halo, m.n_local_cols, y, alpha, no_d, no_y2, ctx->win_xcd);
      });
    } else if (family == 1) {   // one shape, (2, 8)
      const int grid = stream_grid(ctx, m.nrows, 2);
      note_spmv(ctx, ALFD_SPMV_STREAM_F32, 64, 2, 8, false, EPI, 0, grid, 0);
      hipLaunchKernelGGL((spmv_stream_kernel<2, 8, EPI, false, false, float>), dim3(grid), dim3(kBlock), 0, ctx->stream,
                         m.nrows, m.rp, m.col, m.val32, x, m.halo, m.n_local_cols, y, alpha, no_d, no_y2, NoPair());
    } else {
      const int grid = grid_for_rows(m.n_list, 64);
      note_spmv(ctx, ALFD_SPMV_PLAIN_F32, 64, 0, 0, false, EPI, 0, grid, 0);
      hipLaunchKernelGGL((spmv_kernel<64, EPI, false, float>), dim3(grid), dim3(kBlock), 0, ctx->stream, m.n_list, m.rp,
                         m.col, m.val32, m.rows, x, m.halo, m.n_local_cols, y, alpha, no_d, no_y2);
    }
  });
  HIPC(hipGetLastError());
  return ALFD_OK;
}

template <int L>
static void launch_vss(alfd_ctx *ctx, const DevCsr &m, const double *x, double *y, int epi, double alpha,
                       const double *d, double *y2) {
  const DevCsr::Vs &v = m.vs;
  const size_t lds = (size_t)kVsWinOff + (size_t)v.maxW * sizeof(double);
  with_epi(epi, [&](auto e) {
    with_flag(m.tag, [&](auto t) {
      constexpr int EPI = decltype(e)::value, TAG = decltype(t)::value;
      note_spmv(ctx, ALFD_SPMV_BATCH_MAJOR_SHORT, L, 0, 0, false, EPI, 0, v.nb, lds);
      hipLaunchKernelGGL((spmv_vss_kernel<L, EPI, TAG>), dim3((unsigned)v.nb), dim3(256), lds, ctx->stream, v.stream, v.sb,
                         v.tab, v.cnt, v.stride, v.seg_begin, v.blkW, v.seg_col, v.seg_off, v.doff, v.dn, v.dict, x, m.halo,
                         m.n_local_cols, y, alpha, d, y2);
    });
  });
}

// does dynamic LDS start at offset 0 (vs_lds_base_probe_kernel)?  Asked once per context, at its first batch-major launch
static bool vs_lds_base_ok(alfd_ctx *ctx) {
  if (ctx->vs_lds_base_ok < 0) {   // not asked yet
    uint32_t *probe = nullptr, base = 1;
    if (hipMalloc((void **)&probe, sizeof(uint32_t)) == hipSuccess) {
      hipLaunchKernelGGL(vs_lds_base_probe_kernel, dim3(1), dim3(64), 4096, ctx->stream, probe);
      hipMemcpyAsync(&base, probe, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
      hipStreamSynchronize(ctx->stream);
      hipFree(probe);
    }
    ctx->vs_lds_base_ok = base == 0 ? 1 : 0;
    if (!ctx->vs_lds_base_ok)
      std::fprintf(stderr, "[alfd] dynamic LDS does not start at offset 0 (%u): batch-major SpMV formats disabled\n", base);
  }
  return ctx->vs_lds_base_ok != 0;
}

// ---- the one launch of spmv_vs_kernel, for the plain product (launch_vs), the pair launch (launch_pair) and the launch
// with the block-end tail (launch_vs_tail): its argument list, its dynamic LDS and its record.
// LDS: the x window of the widest block behind the dictionary region; with the tail, what the neediest block takes for
// window and row buffer (DevCsr::Vs::tail_lds)
static inline size_t vs_lds(const DevCsr::Vs &v, bool tail) {
  return (size_t)(v.wide ? VsFmt<1>::kWinOff : VsFmt<0>::kWinOff) + (tail ? (size_t)v.tail_lds : (size_t)v.maxW * sizeof(double));
}
// grid: the workgroups of both parties; base: the first row block of this launch.  The record has R = waves, U = wide codes.
template <int EPI, int TAG, int NW, int WD = 0, bool PAIR = false, int TM = -1>
static void launch_vs_kernel(alfd_ctx *ctx, const DevCsr &m, const double *x, double *y, double alpha, const double *d,
                             double *y2, unsigned grid, int32_t base, PairArg<PAIR> pc = {}, TailArg<TM> ta = {}) {
  const DevCsr::Vs &v = m.vs;
  const size_t lds = vs_lds(v, TM >= 0);
  note_spmv(ctx, ALFD_SPMV_BATCH_MAJOR, 64, NW, WD, false, EPI, ctx->vs_xcd, grid, lds);
  hipLaunchKernelGGL((spmv_vs_kernel<EPI, TAG, NW, WD, PAIR, TM>), dim3(grid), dim3(64 * NW), lds, ctx->stream, v.stream,
                     v.tab, v.stride, v.hdrb, v.segx, v.seg_stride, v.dict, x, m.halo, m.n_local_cols, y, alpha, d, y2,
                     ctx->vs_xcd, base, pc, ta);
}

// ---- the side rows of a long-row batch-major operator (spmv_side_rows_kernel): behind every launch of its blocks, on
// the same stream with the same epilogue arguments, inside the Timer of that launch.  No record: alfd_get_last_spmv_launch
// keeps describing the batch-major launch.  part: kSideAll, or one of the two groups of a partitioned operator (the
// rows that read no halo column, which go with the interior blocks, and the others).
enum { kSideAll = 0, kSideInterior = 1, kSideBoundary = 2 };
static inline int64_t side_grid(int64_t n) { return std::min<int64_t>((n + 3) / 4, 256 * 8); }   // one wave per row, grid-stride beyond
static void launch_side(alfd_ctx *ctx, const DevCsr &m, const double *x, double *y, int epi, double alpha, const double *d,
                        double *y2, int part = kSideAll) {
  const DevCsr::Vs &v = m.vs;
  const int64_t first = part == kSideBoundary ? v.side_interior : 0;
  const int64_t n = (part == kSideInterior ? v.side_interior : v.side_n) - first;
  if (n <= 0) return;
  with_epi(epi, [&](auto e) {
    hipLaunchKernelGGL((spmv_side_rows_kernel<decltype(e)::value>), dim3((unsigned)side_grid(n)), dim3(kBlock), 0, ctx->stream, n,
                       v.side_rows + first, v.side_rp + first, v.side_col, v.side_val, x, m.halo, m.n_local_cols, y, alpha, d, y2);
  });
}

static bool launch_vs(alfd_ctx *ctx, const DevCsr &m, const double *x, double *y, int epi, double alpha,
                      const double *d, double *y2, int64_t first_block = 0, int64_t n_blocks = -1, int side_part = kSideAll) {
  const DevCsr::Vs &v = m.vs;
  if (!vs_lds_base_ok(ctx)) return false;
  if (with_const<32, 16, 8>(v.L, [&](auto l) { launch_vss<decltype(l)::value>(ctx, m, x, y, epi, alpha, d, y2); })) return true;
  if (n_blocks < 0) n_blocks = v.nb - first_block;
  const unsigned grid = (unsigned)std::max<int64_t>(n_blocks, 0);
  const int32_t base = (int32_t)first_block;
  if (grid > 0) with_epi(epi, [&](auto e) {
    constexpr int EPI = decltype(e)::value;
    if (v.wide)   // 10-bit codes: one instantiation per epilogue (4 waves, tag 0)
      return launch_vs_kernel<EPI, 0, 4, 1>(ctx, m, x, y, alpha, d, y2, grid, base);
    with_const_or_last<8, 2, 1, 4>(v.NW, [&](auto nw) {
      with_flag(m.tag, [&](auto t) {
        // tag 1, a multigrid level matrix: its own instantiation, so that profiles keep the two apart (8 waves: 4)
        constexpr int TAG = decltype(t)::value, NW = TAG && decltype(nw)::value > 4 ? 4 : decltype(nw)::value;
        launch_vs_kernel<EPI, TAG, NW>(ctx, m, x, y, alpha, d, y2, grid, base);
      });
    });
  });
  launch_side(ctx, m, x, y, epi, alpha, d, y2, side_part);
  return true;
}

static int halo_exchange(alfd_ctx *ctx, DevCsr &m, const double *x, hipStream_t st = nullptr);
static int spmv_launch_local(alfd_ctx *ctx, DevCsr &m, const double *x, double *y, int epi, double alpha, const double *d,
                             double *y2);

// epi 0: y = A x; 1: y = fma(alpha, A x, y); 2: y = d .* (A x); 3: y = A x, y2 = d .* y
static int spmv_m(alfd_ctx *ctx, DevCsr &m, int cls, const double *x, double *y, int epi, double alpha = 0.0,
                  const double *d = nullptr, double *y2 = nullptr) {
  if (!m.present) return ctx->err = "matrix not set", ALFD_E_NOT_SETUP;
  if (a32_active(ctx, m)) {   // one rank, every row listed: no exchange, no memset
    if (m.n_list == 0) return ALFD_OK;
    Timer tm(ctx, cls, m.algorithmic_bytes(), m.streamed_bytes32());
    return spmv_launch_a32(ctx, m, x, y, epi, alpha);
  }
  // RCCL send/recv pairs can be skipped by ranks with nothing to exchange; the
  // barrier-based in-process group needs every rank in every exchange.
  const bool exchange = ctx->nranks > 1 && !m.rep && (ctx->local || ctx->host_alltoallv || m.n_halo > 0 || m.send_off.back() > 0);
  // Long-row batch-major operators on a partitioned context: the row blocks that read no halo column come first in the
  // plan, so they are launched BEFORE the exchange is started (on a stream of its own: pack, send / receive); the
  // blocks along the partition boundary follow when the halo has arrived.  Row sums do not depend on the order of the
  // blocks: same bits as the one-launch form.
  const bool overlap = exchange && (ctx->overlap_halo > 0 || (ctx->overlap_halo < 0 && (ctx->local || ctx->host_alltoallv))) && ctx->xstream && m.vs.on && m.vs.L == 64 && ctx->vs_enable && !ctx->vi_off &&
                       m.vs.nb_interior > 0 && !m.sparse && m.n_list > 0;
  if (overlap) {
    Timer tm(ctx, cls, m.algorithmic_bytes(), m.streamed_bytes(true, true));
    HIPC(hipEventRecord(ctx->ev_x, ctx->stream));          // x is complete here
    if (!launch_vs(ctx, m, x, y, epi, alpha, d, y2, 0, m.vs.nb_interior, kSideInterior)) return ctx->err = "batch-major launch failed", ALFD_E_HIP;
    HIPC(hipStreamWaitEvent(ctx->xstream, ctx->ev_x, 0));
    RC(halo_exchange(ctx, m, x, ctx->xstream));
    HIPC(hipEventRecord(ctx->ev_halo, ctx->xstream));
    HIPC(hipStreamWaitEvent(ctx->stream, ctx->ev_halo, 0));
    launch_vs(ctx, m, x, y, epi, alpha, d, y2, m.vs.nb_interior, m.vs.nb - m.vs.nb_interior, kSideBoundary);   // with the side rows that read the halo
    HIPC(hipGetLastError());
    return ALFD_OK;
  }
  if (exchange) RC(halo_exchange(ctx, m, x));
  if (m.sparse && epi != 1) {
    // rows outside the list are structurally empty: their result is 0
    HIPC(hipMemsetAsync(y, 0, m.nrows * sizeof(double), ctx->stream));
    if (epi == 3) HIPC(hipMemsetAsync(y2, 0, m.nrows * sizeof(double), ctx->stream));
  }
  if (m.n_list == 0) return ALFD_OK;
  Timer tm(ctx, cls, m.algorithmic_bytes(), m.streamed_bytes(!ctx->vi_off, ctx->vs_enable != 0 && !ctx->vi_off));
  return spmv_launch_local(ctx, m, x, y, epi, alpha, d, y2);
}

// the kernel of the storage form in use, on this rank's rows (halo already in place)
static int spmv_launch_local(alfd_ctx *ctx, DevCsr &m, const double *x, double *y, int epi, double alpha, const double *d,
                             double *y2) {
  if (m.vs.on && ctx->vs_enable && !ctx->vi_off && launch_vs(ctx, m, x, y, epi, alpha, d, y2)) {   // vi_off: alfd_bench_spmv_format(…, 0)
    HIPC(hipGetLastError());
    return ALFD_OK;
  }
  if (m.win && launch_window_RU(ctx, m, x, y, epi, alpha, d, y2)) {
    HIPC(hipGetLastError());
    return ALFD_OK;
  }
  if (m.L == 64 && !m.sparse && ctx->spmv_stream_R > 0) {
    const bool ok = ctx->spmv_nt ? launch_stream_RU<true>(ctx, m, x, y, epi, alpha, d, y2)
                                 : launch_stream_RU<false>(ctx, m, x, y, epi, alpha, d, y2);
    if (ok) {
      HIPC(hipGetLastError());
      return ALFD_OK;
    }
  }
  if (rowlane_form(ctx, m, epi))
    launch_rowlane(ctx, m, x, y, epi, alpha);
  else
    launch_spmv(ctx, m, x, y, epi, alpha, d, y2);
  HIPC(hipGetLastError());
  return ALFD_OK;
}

// A short-row operator that took the batch-major form (spmv_vss_kernel) also has the windowed group kernel to fall back
// on, and which of the two is faster depends on the operator: the 27-point stencils of cfg 2 run 3x faster batch-major,
// the 9.9 M x 0.42 M gradient block Bt of the Stokes system (15 entries per row, few translates) 1.5x SLOWER (0.66 against
// 0.44 ms).  Large operators are therefore timed once at upload, five launches of each on a zero vector, and keep the
// faster form; results do not depend on the choice (same canonical sums).
static int pick_short_row_format(alfd_ctx *ctx, DevCsr &m) {
  if (!m.vs.on || m.vs.L == 64 || m.nnz < 20000000 || ctx->vi_off || !ctx->vs_enable || m.sparse) return ALFD_OK;
  double *x = nullptr, *y = nullptr;
  const int64_t nx = std::max<int64_t>(ctx->nranks > 1 && !m.rep ? m.n_local_cols : m.ncols, 1);
  HIPC(hipMalloc((void **)&x, nx * sizeof(double)));
  HIPC(hipMalloc((void **)&y, std::max<int64_t>(m.nrows, 1) * sizeof(double)));
  HIPC(hipMemsetAsync(x, 0, nx * sizeof(double), ctx->stream));
  hipEvent_t e0, e1;
  HIPC(hipEventCreate(&e0));
  HIPC(hipEventCreate(&e1));
  float t[2] = {0.f, 0.f};
  bool ok = true;
  const alfd_spmv_launch rec = ctx->last_spmv;   // the timing launches of an upload are nobody's SpMV: the record stays
  const bool has_rec = ctx->has_last_spmv;
  for (int f = 0; f < 2 && ok; ++f) {
    for (int it = 0; it < 6 && ok; ++it) {   // the first launch of each form is a warm-up
      if (it == 1) hipEventRecord(e0, ctx->stream);
      m.vs.on = f == 0;   // f = 1: whatever the operator runs on without the batch-major form
      ok = spmv_launch_local(ctx, m, x, y, 0, 0.0, nullptr, nullptr) == ALFD_OK;
    }
    m.vs.on = true;
    hipEventRecord(e1, ctx->stream);
    hipEventSynchronize(e1);
    hipEventElapsedTime(&t[f], e0, e1);
  }
  ctx->last_spmv = rec;
  ctx->has_last_spmv = has_rec;
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  hipFree(x);
  hipFree(y);
  HIPC(hipGetLastError());
  if (ok && t[1] < 0.9f * t[0]) {
    m.vs.on = false;
    if (ctx->cfg.log_level > 0 || std::getenv("ALFD_LOG_UPLOAD"))
      std::fprintf(stderr, "[alfd] short-row operator (%lld rows, %lld nnz): without the batch-major form %.3f ms, with it %.3f ms per launch "
                   "-> batch-major form dropped\n", (long long)m.nrows, (long long)m.nnz, t[1] / 5.0, t[0] / 5.0);
  }
  return ALFD_OK;
}

// ---- the single-precision copy of slot A: made when the request and the storage form of A allow it, else released
static void a32_release(alfd_ctx *ctx) {
  DevCsr &m = ctx->mat[ALFD_A];
  if (m.val32) hipFree(m.val32);
  m.val32 = nullptr;
  m.val32_flushed = 0;
  ctx->a32_used = false;
}

// Why slot A holds no copy, as far as the request and the storage form say.  The partition is asked first: every rank
// gives the same answer whatever its piece of A looks like.
static int a32_form_reason(const alfd_ctx *ctx) {
  const DevCsr &m = ctx->mat[ALFD_A];
  if (ctx->prec_values != ALFD_PREC_VALUES_FP32) return ALFD_PREC_VALUES_NOT_REQUESTED;
  if (ctx->nranks > 1) return ALFD_PREC_VALUES_PARTITIONED;
  if (!m.present) return ALFD_PREC_VALUES_NO_MATRIX;
  if (m.sparse) return ALFD_PREC_VALUES_SPARSE_ROWS;
  if (m.L != 64) return ALFD_PREC_VALUES_SHORT_ROWS;
  if (m.vs.on || m.vi) return ALFD_PREC_VALUES_DICTIONARY_FORM;
  return ALFD_PREC_VALUES_NONE;
}

// After a change of the request or of slot A: a32_reason, and the copy when nothing speaks against it (converted on the
// device from the resident values, which also counts the flushed entries and those without a finite image)
static int a32_sync(alfd_ctx *ctx) {
  DevCsr &m = ctx->mat[ALFD_A];
  a32_release(ctx);
  ctx->a32_reason = a32_form_reason(ctx);
  if (ctx->a32_reason != ALFD_PREC_VALUES_NONE) return ALFD_OK;
  if (!ctx->a32_counts) RC(dev_alloc(ctx, &ctx->a32_counts, 2));
  HIPC(hipMalloc((void **)&m.val32, std::max<int64_t>(m.nnz, 1) * sizeof(float)));
  HIPC(hipMemsetAsync(ctx->a32_counts, 0, 2 * sizeof(unsigned long long), ctx->stream));
  if (m.nnz > 0) {
    const unsigned grid = (unsigned)std::min<int64_t>((m.nnz + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(round_values_kernel, dim3(grid), dim3(256), 0, ctx->stream, m.nnz, m.val, m.val32, ctx->a32_counts);
    HIPC(hipGetLastError());
  }
  unsigned long long counts[2] = {0, 0};
  HIPC(hipMemcpyAsync(counts, ctx->a32_counts, sizeof(counts), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  if (counts[1] > 0) {
    a32_release(ctx);
    ctx->a32_reason = ALFD_PREC_VALUES_OUT_OF_RANGE;
    return ALFD_OK;
  }
  m.val32_flushed = (int64_t)counts[0];
  ctx->a32_reason = ALFD_PREC_VALUES_NOT_APPLIED;   // until a setup says otherwise
  return ALFD_OK;
}

// alfd_setup / alfd_setup_coupling succeeded: does the configured inner preconditioner apply slot A?  The multilevel
// cycle on level 0 of hierarchy 0 (not when that level is the coarsest one with an explicit inverse), the Chebyshev
// sweep on Aug of the variants whose inner solve runs on the (1,1) block alone.
static void a32_decide_used(alfd_ctx *ctx) {
  const alfd_config &c = ctx->cfg;
  ctx->a32_used = false;
  if (!ctx->mat[ALFD_A].val32) return;
  const alfd_ctx::Hierarchy &H = ctx->hier[0];
  if (c.inner_prec == ALFD_PREC_MULTILEVEL)
    ctx->a32_used = c.variant != ALFD_RATIONAL && !H.ml.empty() && (H.ml.size() > 1 || !H.inv.present);
  else if (c.inner_prec == ALFD_PREC_CHEBYSHEV)
    ctx->a32_used = c.cheb_degree > 1 && (c.variant == ALFD_AL2 || c.variant == ALFD_AL_STOKES ||
                                          c.variant == ALFD_AL_STOKES_DIAG || c.variant == ALFD_AL_ELL_MODIFIED);
  ctx->a32_reason = ctx->a32_used ? ALFD_PREC_VALUES_NONE : ALFD_PREC_VALUES_NOT_APPLIED;
}

static int spmv(alfd_ctx *ctx, int slot, const double *x, double *y, int epi, double alpha = 0.0,
                const double *d = nullptr, double *y2 = nullptr) {
  DevCsr &m = ctx->mat[slot];
  if (!m.present) return ctx->err = "matrix slot " + std::to_string(slot) + " not set", ALFD_E_NOT_SETUP;
  return spmv_m(ctx, m, slot == ALFD_A ? ALFD_T_SPMV_A : ALFD_T_SPMV_OTHER, x, y, epi, alpha, d, y2);
}

// ml_tail_kernel and the second party of a pair launch walk the CSR arrays of m: everything spmv_launch_local runs on spmv_kernel or, for 64-lane rows, on
// the streaming kernel (which reads the same arrays and forms the canonical sums)
static bool tail_form(const DevCsr &m) { return m.present && !m.vs.on && !m.win; }

// ---- pair launch ("ml_fuse" >= 2): y = A x and t = w .* (C x) of a factored operator read the same x and
// write different vectors, and the C product is a latency-bound kernel of a few microseconds.  Where A runs on the
// long-row batch-major kernel (1, 2 or 4 waves, narrow codes) or on spmv_stream_kernel<2, 8>, C rides as extra workgroups of
// that grid (PairC, kernels.hpp).  Same sums, same bits; one launch, timed as A's.

// which PAIR instantiation spmv_launch_local's choice for A has: 1 batch-major, 2 stream, 0 none
static int pair_form_A(alfd_ctx *ctx, const DevCsr &A) {
  if (!A.present || A.sparse || A.n_list == 0) return 0;
  if (a32_active(ctx, A)) return 0;   // the single-precision copy has no PAIR instantiation (speed only)
  if (A.vs.on && ctx->vs_enable && !ctx->vi_off)
    return A.vs.L == 64 && !A.vs.wide && A.vs.NW <= 4 && A.vs.nb > 0 && vs_lds_base_ok(ctx) ? 1 : 0;
  if (A.win) return 0;
  return A.L == 64 && ctx->spmv_stream_R == 2 && ctx->spmv_stream_U == 8 && !ctx->spmv_nt ? 2 : 0;
}

// Partitioned contexts (halo exchanges, the overlap path of spmv_m), the exact W^-1, the assembled operator and the
// nested grad-div term keep the two launches
static inline bool gd_nested(const alfd_ctx *ctx);
// the PAIR instantiation (pair_form_A) that takes A and C together, 0: none
static int pair_forms(alfd_ctx *ctx, const DevCsr &A, const DevCsr &C) {
  const bool ok = ctx->nranks == 1 && ctx->cfg.w_inverse == ALFD_W_DIAGONAL && !ctx->cfg.aug_assembled && !gd_nested(ctx) &&
                  tail_form(C) && !C.sparse && C.nrows > 0 && (C.L == 16 || C.L == 32 || C.L == 64) && A.ncols == C.ncols;
  return ok ? pair_form_A(ctx, A) : 0;
}
// ... and so does the fine level below ml_fuse 3
static int pair_ok(alfd_ctx *ctx, const DevCsr &A, const DevCsr &C) {
  const bool fine = &A == &ctx->mat[ALFD_A] || &A == &ctx->mat[ALFD_A2];
  return ctx->ml_fuse >= (fine ? 3 : 2) ? pair_forms(ctx, A, C) : 0;
}

// The second party t = w .* (C x) behind the nA workgroups of A, in workgroups of `threads` threads (64 NW of the
// batch-major kernel, kBlock of the stream kernel): threads / L rows per pass, as many workgroups as cover its rows once,
// grid-stride beyond.  The launch with the block-end tail always has 4 waves, 256 threads.
static PairC pair_c(const DevCsr &C, const double *w, double *t, uint32_t nA, int threads) {
  PairC pc{};
  pc.nrows = C.n_list, pc.rp = C.rp, pc.col = C.col, pc.val = C.val, pc.x_halo = C.halo, pc.d = w, pc.t = t;
  pc.n_local = C.n_local_cols, pc.L = C.L;
  const int64_t rpb = threads / C.L;
  pc.nA = nA;
  pc.nC = (uint32_t)std::max<int64_t>(1, std::min<int64_t>((C.n_list + rpb - 1) / rpb, 256 * 8));
  return pc;
}

// form: what pair_forms(ctx, A, C) answered, not 0
static int launch_pair(alfd_ctx *ctx, int form, const DevCsr &A, int clsA, const DevCsr &C, const double *w,
                       const double *x, double *y, double *t) {
  const bool vi = !ctx->vi_off, vs = ctx->vs_enable != 0 && !ctx->vi_off;
  Timer tm(ctx, clsA, A.algorithmic_bytes() + C.algorithmic_bytes(), A.streamed_bytes(vi, vs) + C.streamed_bytes(vi, vs));
  if (form == 1) {
    const PairC pc = pair_c(C, w, t, (uint32_t)A.vs.nb, 64 * A.vs.NW);
    with_flag(A.tag, [&](auto tg) {
      with_const_or_last<1, 2, 4>(A.vs.NW, [&](auto nw) {
        launch_vs_kernel<0, decltype(tg)::value, decltype(nw)::value, 0, true>(ctx, A, x, y, 0.0, nullptr, nullptr,
                                                                                 pc.nA + pc.nC, 0, pc);
      });
    });
    launch_side(ctx, A, x, y, 0, 0.0, nullptr, nullptr);
  } else {   // the stream kernel at (2, 8), kBlock threads
    const PairC pc = pair_c(C, w, t, (uint32_t)stream_grid(ctx, A.nrows, 2), kBlock);
    note_spmv(ctx, ALFD_SPMV_STREAM, 64, 2, 8, false, 0, 0, (int64_t)pc.nA + pc.nC, 0);
    hipLaunchKernelGGL((spmv_stream_kernel<2, 8, 0, false, true>), dim3(pc.nA + pc.nC), dim3(kBlock), 0, ctx->stream,
                       A.nrows, A.rp, A.col, A.val, x, A.halo, A.n_local_cols, y, 0.0, (const double *)nullptr,
                       (double *)nullptr, pc);
  }
  HIPC(hipGetLastError());
  return ALFD_OK;
}

// y = A x and t = w .* (C x): the pair launch where it applies, else the two launches
static int spmv_AC(alfd_ctx *ctx, DevCsr &A, int clsA, DevCsr &C, const double *w, const double *x, double *y, double *t) {
  if (const int form = pair_ok(ctx, A, C)) return launch_pair(ctx, form, A, clsA, C, w, x, y, t);
  RC(spmv_m(ctx, A, clsA, x, y, 0));
  return spmv_m(ctx, C, ALFD_T_SPMV_OTHER, x, t, 2, 0.0, w);
}

// ------------------------------------------------------------ reductions
// count dots whose chunk partials sit at partial[j*pstride ..]; results land in
// sc[out+j] (single rank) with optional PCG post-op.
static int finish_dots(alfd_ctx *ctx, int64_t nb, int count, int out, int fin) {
  if (ctx->nranks == 1 || ctx->dots_replicated) {
    hipLaunchKernelGGL(dot_final_kernel, dim3(count), dim3(kBlock), 0, ctx->stream, ctx->partial, nb,
                       ctx->pstride, ctx->sc, out, fin);
    HIPC(hipGetLastError());
    return ALFD_OK;
  }
  // multi-rank: local sums -> all-gather -> ordered sum (rank 0 first); the
  // PCG post-ops are applied by a tiny follow-up kernel on every rank.
  hipLaunchKernelGGL(dot_final_kernel, dim3(count), dim3(kBlock), 0, ctx->stream, ctx->partial, nb,
                     ctx->pstride, ctx->sc, (int)S_STAGE, (int)FIN_STORE);
  HIPC(hipGetLastError());
  RC(comm_allgather(ctx, ctx->sc + S_STAGE, ctx->gather, (size_t)count * sizeof(double)));
  const int tgt = fin == FIN_STORE ? out : (int)S_TMP;
  hipLaunchKernelGGL(rank_sum_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->gather, ctx->nranks, count,
                     ctx->sc, tgt);
  if (fin != FIN_STORE) {
    // re-run the post-op on the summed value: a 1-chunk "partial" == the value
    hipLaunchKernelGGL(dot_final_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, ctx->sc + S_TMP,
                       (int64_t)1, (int64_t)0, ctx->sc, out, fin);
  }
  HIPC(hipGetLastError());
  return ALFD_OK;
}

static int dot_async(alfd_ctx *ctx, int64_t npad, const double *x, const double *y, int out,
                     int fin = FIN_STORE) {
  const int64_t nb = npad / kChunk;
  if (nb > 0) {
    Timer tm(ctx, ALFD_T_DOT, 16.0 * npad);
    hipLaunchKernelGGL(dot_partial_kernel, dim3((unsigned)nb), dim3(kBlock), 0, ctx->stream, x, y,
                       ctx->partial);
  }
  HIPC(hipGetLastError());
  return finish_dots(ctx, nb, 1, out, fin);
}

static int read_scalars(alfd_ctx *ctx, int first, int count) {
  // The mirror is mapped pinned host memory: a one-workgroup kernel stores the scalars
  // there directly (a D2H hipMemcpyAsync goes through the runtime's blit kernels, which
  // cost far more than this launch at one readback per CG iteration).
  hipLaunchKernelGGL(mirror_scalars_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, ctx->sc + first,
                     ctx->sc_host + first, count);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(ctx->stream));
  return ALFD_OK;
}

// A rank may own zero rows of a block (e.g. the multiplier rows of a localised immersed body):
// its vectors are empty and the launch is skipped; collectives are still entered by every rank.
#define VEC_LAUNCH(kernel, npad, bytes_per_elem, ...)                                              \
  do {                                                                                             \
    if ((npad) > 0) {                                                                              \
      Timer tm__(ctx, ALFD_T_VEC, (double)(bytes_per_elem) * (double)(npad));                      \
      hipLaunchKernelGGL(kernel, dim3((unsigned)((npad) / kChunk)), dim3(kBlock), 0, ctx->stream,  \
                         __VA_ARGS__);                                                             \
    }                                                                                              \
  } while (0)

// ------------------------------------------------------------- operators
// Inner operators (SPD) the CG runs on:
//   OP_AUG   y = A x + gamma Ct (invW .* (C x))         stokes...:991-993; A11_aug elliptic...:807
//   OP_MP    y = Mp x                                   stokes...:929
//   OP_A22   y = A2 x + gamma2 M (invW .* (M x))        A22_aug, elliptic_interface.cc:810
//   OP_AUG2  2x2 [[A11_aug, A12_aug],[A21_aug, A22_aug]] on [x0 | pad | x1] (elliptic...:927-929):
//            s = C x0 - M x1, t = invW .* s, y0 = A x0 + gamma Ct t, y1 = A2 x1 - gamma2 M t
//   OP_K     y = A x  (K_inv of the rational branch: UMFPACK in the reference,
//            immersed_laplace.cc:617-620; here CG to alfd_config::inner)
//   OP_MASS  y = M x  (the immersed mass matrix of the exact W^-1 = (M^-1)^2, stokes...:979-985)
//   OP_CCT   y = C[:,S] (Ct[S,:] x) = C Ct x on the multiplier block (the sanity check of the drivers,
//            elliptic_interface.cc:986-1009; alfd_estimate_spectrum)
enum OpKind { OP_AUG = 0, OP_MP = 1, OP_A22 = 2, OP_AUG2 = 3, OP_K = 4, OP_MASS = 5, OP_CCT = 6 };

static inline int64_t op_npad(const alfd_ctx *ctx, int op) {
  if (op == OP_MASS || op == OP_CCT) return pad_chunk(ctx->n[ctx->nblocks - 1]);
  return (op == OP_AUG || op == OP_K) ? pad_chunk(ctx->n[0]) : op == OP_AUG2 ? ctx->off[2] : pad_chunk(ctx->n[1]);
}

static int winv_scale(alfd_ctx *ctx, double alpha, const double *src, double *dst);
static int nested_mp_solve(alfd_ctx *ctx, const double *b, double *x);

// grad_div_in_A = 0 on a Stokes variant: Aug carries the term gamma_gd Bt Mp^-1 B (stokes...:991-995)
static inline bool gd_nested(const alfd_ctx *ctx) {
  return !ctx->cfg.grad_div_in_A && (ctx->cfg.variant == ALFD_AL_STOKES || ctx->cfg.variant == ALFD_AL_STOKES_DIAG);
}

// exact_w: apply the configured W^-1 (the operator the inner CG and the outer system see);
// false: the diagonal weight (everything inside the inner preconditioner).  The same split holds for
// the grad-div-off term: exact_w solves q = Mp^-1 (B x), otherwise q = l .* (B x), l = ALFD_MP_LUMPED_INV.
static int op_apply(alfd_ctx *ctx, int op, const double *x, double *y, bool exact_w = false) {
  const double *w = ctx->diag[ALFD_INVW];
  switch (op) {
    case OP_AUG:
      if (ctx->cfg.aug_assembled) return spmv(ctx, ALFD_A, x, y, 0);  // operator form: A already holds the AL term
      if (exact_w && ctx->cfg.w_inverse != ALFD_W_DIAGONAL) {
        RC(spmv(ctx, ALFD_A, x, y, 0));
        RC(spmv(ctx, ALFD_C, x, ctx->t_lam, 0));
        RC(winv_scale(ctx, 1.0, ctx->t_lam, ctx->t_lam));
      } else {
        if (!ctx->mat[ALFD_A].present || !ctx->mat[ALFD_C].present) return ctx->err = "matrix not set", ALFD_E_NOT_SETUP;
        RC(spmv_AC(ctx, ctx->mat[ALFD_A], ALFD_T_SPMV_A, ctx->mat[ALFD_C], w, x, y, ctx->t_lam));
      }
      RC(spmv(ctx, ALFD_CT, ctx->t_lam, y, 1, ctx->cfg.gamma));
      if (!gd_nested(ctx)) return ALFD_OK;
      if (exact_w) {
        RC(spmv(ctx, ALFD_B, x, ctx->gd_bx, 0));
        RC(nested_mp_solve(ctx, ctx->gd_bx, ctx->gd_q));
      } else {
        RC(spmv(ctx, ALFD_B, x, ctx->gd_q, 2, 0.0, ctx->diag[ALFD_MP_LUMPED_INV]));
      }
      return spmv(ctx, ALFD_BT, ctx->gd_q, y, 1, ctx->cfg.gamma_grad_div);
    case OP_MASS:
      return spmv(ctx, ALFD_M, x, y, 0);
    case OP_CCT:
      RC(spmv_m(ctx, *ctx->spec.Cts, ALFD_T_SPMV_OTHER, x, ctx->spec.t, 0));
      return spmv_m(ctx, *ctx->spec.Cs, ALFD_T_SPMV_OTHER, ctx->spec.t, y, 0);
    case OP_MP:
      return spmv(ctx, ALFD_MP, x, y, 0);
    case OP_K:
      return spmv(ctx, ALFD_A, x, y, 0);
    case OP_A22:
      RC(spmv(ctx, ALFD_A2, x, y, 0));
      if (exact_w && ctx->cfg.w_inverse != ALFD_W_DIAGONAL) {
        RC(spmv(ctx, ALFD_M, x, ctx->t_lam, 0));
        RC(winv_scale(ctx, 1.0, ctx->t_lam, ctx->t_lam));
      } else {
        RC(spmv(ctx, ALFD_M, x, ctx->t_lam, 2, 0.0, w));
      }
      return spmv(ctx, ALFD_M, ctx->t_lam, y, 1, ctx->cfg.gamma2);
    default: {
      const double *x1 = x + ctx->off[1];
      double *y1 = y + ctx->off[1];
      const int64_t nlp = pad_chunk(ctx->n[2]);
      RC(spmv(ctx, ALFD_C, x, ctx->t_lam, 0));
      RC(spmv(ctx, ALFD_M, x1, ctx->t_lam, 1, -1.0));
      if (exact_w) RC(winv_scale(ctx, 1.0, ctx->t_lam, ctx->t_lam));  // diagonal weight unless w_inverse says otherwise
      else VEC_LAUNCH(pmul_scale_kernel, nlp, 24, 1.0, w, ctx->t_lam, ctx->t_lam);
      RC(spmv(ctx, ALFD_A, x, y, 0));
      RC(spmv(ctx, ALFD_CT, ctx->t_lam, y, 1, ctx->cfg.gamma));
      RC(spmv(ctx, ALFD_A2, x1, y1, 0));
      return spmv(ctx, ALFD_M, ctx->t_lam, y1, 1, -ctx->cfg.gamma2);
    }
  }
}

static const double *op_dinv(const alfd_ctx *ctx, int op) {
  return op == OP_AUG ? ctx->dinv_aug : op == OP_A22 ? ctx->dinv_a22 : op == OP_AUG2 ? ctx->dinv_aug2
         : op == OP_K ? ctx->dinv_k : op == OP_MASS ? ctx->dinv_m : ctx->diag[ALFD_MP_LUMPED_INV];
}

// Chebyshev coefficients for the spectrum [lmax / ratio, lmax]: the first direction is (1 / theta) D^-1 r,
// step() gives c1, c2 of the next one (d = c1 d + c2 D^-1 res)
struct ChebCoef {
  double theta, delta, sigma, rho;
  ChebCoef(double lmax, double ratio) {
    const double lmin = lmax / ratio;
    theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin);
    sigma = theta / delta;
    rho = 1.0 / sigma;
  }
  void step(double &c1, double &c2) {
    const double rho_new = 1.0 / (2.0 * sigma - rho);
    c1 = rho_new * rho, c2 = 2.0 * rho_new / delta;
    rho = rho_new;
  }
};

// Chebyshev sweep z = p_k(D^-1 Op) D^-1 r from a zero start, k = degree; apply(x, y): y = Op x.
// cd / cres / ctmp: direction, residual and product vectors of the sweep.
template <class Apply>
static int cheb_sweep(alfd_ctx *ctx, int64_t npad, const double *dinv, double lmax, double ratio, int degree, double *cd,
                      double *cres, double *ctmp, const double *r, double *z, Apply apply) {
  ChebCoef k(lmax, ratio);
  VEC_LAUNCH(cheb_init_kernel, npad, degree > 1 ? 40 : 32, 1.0 / k.theta, dinv, r, cd, z, cres, degree > 1 ? 1 : 0);
  for (int j = 1; j < degree; ++j) {
    RC(apply(cd, ctmp));
    double c1, c2;
    k.step(c1, c2);
    VEC_LAUNCH(cheb_step_kernel, npad, 64, c1, c2, dinv, ctmp, cres, cd, z);
  }
  HIPC(hipGetLastError());
  return ALFD_OK;
}

static int cheb_apply(alfd_ctx *ctx, int op, const double *r, double *z, int64_t npad) {
  const int k = ctx->cfg.cheb_degree;
  const A32Scope a32(ctx, op == OP_AUG && ctx->a32_used);   // the A product of the sweep on Aug
  // SpMV writes rows only: padding of the product vector must be zero
  if (k > 1) HIPC(hipMemsetAsync(ctx->c_tmp, 0, npad * sizeof(double), ctx->stream));
  return cheb_sweep(ctx, npad, op_dinv(ctx, op), ctx->lam_max[op], ctx->cfg.cheb_eig_ratio, k, ctx->c_d, ctx->c_res,
                    ctx->c_tmp, r, z, [&](const double *x, double *y) { return op_apply(ctx, op, x, y); });
}

// deal.II SolverCG via inverse_operator (zero initial guess) [EXT]; b and x are
// padded device vectors of the operator's span.
static int ml_cycle(alfd_ctx *ctx, int h, int l, const double *r, double *z);
static int ml_apply(alfd_ctx *ctx, const double *r, double *z);
// ALFD_PREC_MULTILEVEL on the inner operator op: the augmented (1,1) block always; A22 and the 2-block operator of the ideal
// variant when the immersed hierarchy is set up (setup() refuses the ideal variant without it), else the Chebyshev sweep
static bool ml_covers(const alfd_ctx *ctx, int op) {
  return op == OP_AUG || ((op == OP_A22 || op == OP_AUG2) && !ctx->hier[1].ml.empty());
}
// z = M^-1 r there: the V-cycle of the block, and for the 2-block operator the block diagonal z = [ml_apply(r0); V1(r1)]
// ({{AMG_A1, 0}, {0, AMG_A2}}, elliptic_interface.cc:930-942)
static int ml_prec(alfd_ctx *ctx, int op, const double *r, double *z) {
  if (op == OP_A22) return ml_cycle(ctx, 1, 0, r, z);
  RC(ml_apply(ctx, r, z));
  return op == OP_AUG2 ? ml_cycle(ctx, 1, 0, r + ctx->off[1], z + ctx->off[1]) : ALFD_OK;
}
// rec (alfd_estimate_spectrum only): the CG coefficients alpha_j, beta_j come back with the readback of r.r, and a
// step with p.Ap <= 0 (or NaN) ends the solve as FAILURE at the step before it.
struct CgRecord {
  std::vector<double> alpha, beta;
};
static int pcg(alfd_ctx *ctx, int op, int prec, const alfd_control &ctrl, const double *b, double *x,
               int *its_out, State *st_out, double *res_out, CgRecord *rec = nullptr) {
  const int64_t npad = op_npad(ctx, op);
  const int64_t nb = npad / kChunk;
  const double *dinv = op_dinv(ctx, op);
  double *r = ctx->w_r, *z = ctx->w_z, *p = ctx->w_p, *Ap = ctx->w_Ap;
  VEC_LAUNCH(scale_copy_kernel, npad, 16, 1.0, b, r);   // r = b
  HIPC(hipMemsetAsync(x, 0, npad * sizeof(double), ctx->stream));
  // SpMV writes rows only: the padding of Ap may hold data of a previous, longer
  // solve and must be zero for the fused r-update / dot kernels.
  HIPC(hipMemsetAsync(Ap, 0, npad * sizeof(double), ctx->stream));
  Control sc{ctrl};
  RC(dot_async(ctx, npad, r, r, S_RR));
  RC(read_scalars(ctx, S_RR, 1));
  double res = std::sqrt(ctx->sc_host[S_RR]);
  State st = sc.check(0, res);
  int its = 0;
  while (st == ITERATE) {
    ++its;
    const double *zz = z;
    if (prec == ALFD_PREC_IDENTITY) {
      zz = r;
      RC(dot_async(ctx, npad, r, r, 0, FIN_RZ));
    } else if (prec == ALFD_PREC_JACOBI) {
      VEC_LAUNCH(jacobi_dot_kernel, npad, 24, dinv, r, z, ctx->partial);
      RC(finish_dots(ctx, nb, 1, 0, FIN_RZ));
    } else if (prec == ALFD_PREC_MULTILEVEL && ml_covers(ctx, op)) {
      RC(ml_prec(ctx, op, r, z));
      RC(dot_async(ctx, npad, r, z, 0, FIN_RZ));
    } else {
      RC(cheb_apply(ctx, op, r, z, npad));
      RC(dot_async(ctx, npad, r, z, 0, FIN_RZ));
    }
    VEC_LAUNCH(p_update_kernel, npad, its == 1 ? 16 : 24, ctx->sc, its == 1 ? 1 : 0, zz, p);
    RC(op_apply(ctx, op, p, Ap, true));
    RC(dot_async(ctx, npad, p, Ap, 0, FIN_ALPHA));
    VEC_LAUNCH(xr_update_dot_kernel, npad, 48, ctx->sc, p, Ap, x, r, ctx->partial);
    RC(finish_dots(ctx, nb, 1, S_RR, FIN_STORE));
    if (rec) {
      RC(read_scalars(ctx, S_PAP, S_RR - S_PAP + 1));
      if (!(ctx->sc_host[S_PAP] > 0.0)) {
        --its;
        st = FAILURE;
        break;
      }
      rec->alpha.push_back(ctx->sc_host[S_ALPHA]);
      if (its > 1) rec->beta.push_back(ctx->sc_host[S_BETA]);
    } else {
      RC(read_scalars(ctx, S_RR, 1));
    }
    res = std::sqrt(ctx->sc_host[S_RR]);
    st = sc.check(its, res);
  }
  *its_out = its;
  *st_out = st;
  *res_out = res;
  return ALFD_OK;
}

static int inner_solve(alfd_ctx *ctx, int op, const double *b, double *x) {
  int its = 0;
  State st;
  double res;
  const bool mp = op == OP_MP;
  RC(pcg(ctx, op, mp ? (int)ALFD_PREC_JACOBI : ctx->cfg.inner_prec, mp ? ctx->cfg.mp_inner : ctx->cfg.inner, b,
         x, &its, &st, &res));
  (mp ? ctx->mp_its : ctx->inner_its) += its;
  if (op == OP_AUG || op == OP_A22 || op == OP_AUG2)
    ctx->inner_its_op[op == OP_AUG ? ALFD_INNER_OP_AUG : op == OP_A22 ? ALFD_INNER_OP_A22 : ALFD_INNER_OP_AUG2] += its;
  if (ctx->cfg.log_level >= 3 && ctx->rank == 0)
    std::printf("DEAL:%s:cg::%s step %d value %.17g\n", mp ? "mp" : "aug",
                st == SUCCESS ? "Convergence" : "Failure", its, res);
  if (st == FAILURE) {
    if (std::isnan(res)) return ctx->err = "inner CG breakdown (NaN)", ALFD_E_BREAKDOWN;
    if (ctx->cfg.on_inner_failure == ALFD_INNER_THROW)
      return ctx->err = "inner CG did not converge (SolverControl::NoConvergence)",
             ALFD_E_NO_CONVERGENCE_INNER;
    ctx->inner_failures++;
  }
  return ALFD_OK;
}

static inline bool is_elliptic(int v) { return v == ALFD_AL_ELL_IDEAL || v == ALFD_AL_ELL_MODIFIED; }

// The nested solves -- the exact-W^-1 mass solve and the Mp solve of the grad-div-off Aug -- may start in
// the middle of an inner-CG iteration (inside Aug p) or of the outer system_apply, so they run on their own
// CG vectors, scalar table and reduction buffers, the n_* set, swapped in for the w_* set pcg() works on.
// The two share that set because they are never live at the same time: mass_solve runs to completion inside
// winv_scale, before op_apply / system_apply reach the Bt Mp^-1 B term, and neither solve's operator (M, Mp)
// applies W^-1 or Aug.  n_owner records the holder; a second claim is an internal error.
enum { NESTED_FREE = 0, NESTED_MASS = 1, NESTED_MP = 2, NESTED_CCT = 3 };
static int nested_claim(alfd_ctx *ctx, int who) {
  if (ctx->n_owner != NESTED_FREE)
    return ctx->err = "nested solve started while another holds its work vectors", ALFD_E_INVALID;
  ctx->n_owner = who;
  return ALFD_OK;
}
static void nested_swap_ws(alfd_ctx *ctx) {
  std::swap(ctx->w_r, ctx->n_r);
  std::swap(ctx->w_z, ctx->n_z);
  std::swap(ctx->w_p, ctx->n_p);
  std::swap(ctx->w_Ap, ctx->n_Ap);
  std::swap(ctx->sc, ctx->n_sc);
  std::swap(ctx->sc_host, ctx->n_sc_host);
  std::swap(ctx->partial, ctx->n_partial);
  std::swap(ctx->gather, ctx->n_gather);
}

// x = M^-1 b by Jacobi-preconditioned CG to alfd_config::mass (UMFPACK in the reference,
// stokes...:966-968).
static int mass_solve(alfd_ctx *ctx, const double *b, double *x) {
  int its = 0;
  State st = FAILURE;
  double res = 0;
  RC(nested_claim(ctx, NESTED_MASS));
  nested_swap_ws(ctx);
  const int rc = pcg(ctx, OP_MASS, ALFD_PREC_JACOBI, ctx->cfg.mass, b, x, &its, &st, &res);
  nested_swap_ws(ctx);
  ctx->n_owner = NESTED_FREE;
  if (rc != ALFD_OK) return rc;
  ctx->mass_its += its;
  if (st == FAILURE) {
    if (std::isnan(res)) return ctx->err = "mass-matrix CG breakdown (NaN)", ALFD_E_BREAKDOWN;
    return ctx->err = "mass-matrix CG (exact W^-1) did not converge", ALFD_E_NO_CONVERGENCE_INNER;
  }
  return ALFD_OK;
}

// Device-stepped form of pcg(ctx, OP_MP, ALFD_PREC_JACOBI, mp_inner, ..) on one rank: the stop rule runs
// on the device (nmp_finish_kernel), the host enqueues nmp_group iterations at a time and reads the state
// once per group through the mapped scalar mirror: 5 launches per iteration plus one mirror launch per group.
// Same arithmetic as pcg(): same bits, same step.  Works on the n_* set (the caller holds it).
static int pcg_mp_device(alfd_ctx *ctx, const double *b, double *x, int *its_out, State *st_out, double *res_out) {
  const alfd_control &ctrl = ctx->cfg.mp_inner;
  const DevCsr &m = ctx->mat[ALFD_MP];
  const int64_t npad = op_npad(ctx, OP_MP), nb = npad / kChunk;
  const double *l = ctx->diag[ALFD_MP_LUMPED_INV];
  double *r = ctx->n_r, *z = ctx->n_z, *p = ctx->n_p, *Ap = ctx->n_Ap, *sc = ctx->n_sc;
  double *part_rr = ctx->n_partial, *part_rz = ctx->n_partial + ctx->pstride, *part_pap = ctx->n_partial + 2 * ctx->pstride;
  const unsigned grid = (unsigned)nb;
  const int sgrid = grid_for_rows(m.nrows, m.L);
  auto update = [&](int first) {
    Timer tm(ctx, ALFD_T_VEC, first ? 40.0 * npad : 72.0 * npad);
    hipLaunchKernelGGL(nmp_update_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, sc, first, part_pap, nb, b, l, p,
                       Ap, x, r, z, part_rr, part_rz);
  };
  auto finish = [&](int step) {
    Timer tm(ctx, ALFD_T_DOT, 16.0 * nb);
    hipLaunchKernelGGL(nmp_finish_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, part_rr, part_rz, nb, sc, step,
                       ctrl.kind, ctrl.max_steps, ctrl.tol, ctrl.reduce);
  };
  if (nb > 0) update(1);
  finish(0);
  HIPC(hipGetLastError());
  int enq = 0;   // iterations enqueued so far
  for (;;) {
    const int group = std::max(1, ctx->nmp_group);
    for (int g = 0; g < group && nb > 0 && enq < std::max(ctrl.max_steps, 0); ++g) {
      const int it = ++enq;
      {
        Timer tm(ctx, ALFD_T_VEC, it == 1 ? 16.0 * npad : 24.0 * npad);
        hipLaunchKernelGGL(nmp_p_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, sc, it == 1 ? 1 : 0, z, p);
      }
      {
        Timer tm(ctx, ALFD_T_SPMV_OTHER, m.algorithmic_bytes());
        with_lanes(m.L, [&](auto l) {
          hipLaunchKernelGGL((nmp_spmv_kernel<decltype(l)::value>), dim3(sgrid), dim3(kBlock), 0, ctx->stream, sc, m.nrows,
                             m.rp, m.col, m.val, p, Ap);
        });
      }
      {
        Timer tm(ctx, ALFD_T_DOT, 16.0 * npad);
        hipLaunchKernelGGL(nmp_dot_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, sc, p, Ap, part_pap);
      }
      update(0);
      finish(it);
    }
    HIPC(hipGetLastError());
    {
      Timer tm(ctx, ALFD_T_DOT, 8.0 * (S_NRTOL + 1));
      hipLaunchKernelGGL(mirror_scalars_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, sc, ctx->n_sc_host, (int)(S_NRTOL + 1));
    }
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(ctx->stream));
    const double *h = ctx->n_sc_host;
    if (h[S_NSTATE] != 0.0) {
      *its_out = (int)h[S_NSTEP];
      *st_out = h[S_NSTATE] == 1.0 ? SUCCESS : FAILURE;
      *res_out = std::sqrt(h[S_RR]);
      return ALFD_OK;
    }
    if (enq >= ctrl.max_steps) return ctx->err = "nested Mp CG: the device stop rule did not end the solve", ALFD_E_INVALID;
  }
}

// q = Mp^-1 b: the same solve as the preconditioner's pressure block (lumped-Jacobi CG to alfd_config::mp_inner,
// zero start), for the gamma_gd Bt Mp^-1 B term of Aug when grad_div_in_A = 0 (stokes...:933-956, 991-995).
// Device-stepped on one rank; partitioned contexts (dots through the host or an all-gather) and the tunable
// "nested_mp_host_stepped" take the host-stepped pcg().  Its iterations count as mp_iterations.
static int nested_mp_solve(alfd_ctx *ctx, const double *b, double *x) {
  int its = 0;
  State st = FAILURE;
  double res = 0;
  RC(nested_claim(ctx, NESTED_MP));
  int rc;
  if (ctx->nranks == 1 && !ctx->nmp_host_stepped && !ctx->mat[ALFD_MP].sparse) {
    rc = pcg_mp_device(ctx, b, x, &its, &st, &res);
  } else {
    nested_swap_ws(ctx);
    rc = pcg(ctx, OP_MP, ALFD_PREC_JACOBI, ctx->cfg.mp_inner, b, x, &its, &st, &res);
    nested_swap_ws(ctx);
  }
  ctx->n_owner = NESTED_FREE;
  if (rc != ALFD_OK) return rc;
  ctx->mp_its += its;
  if (ctx->cfg.log_level >= 3 && ctx->rank == 0)
    std::printf("DEAL:mp_aug:cg::%s step %d value %.17g\n", st == SUCCESS ? "Convergence" : "Failure", its, res);
  if (st == FAILURE) {
    if (std::isnan(res)) return ctx->err = "nested Mp CG breakdown (NaN)", ALFD_E_BREAKDOWN;
    if (ctx->cfg.on_inner_failure == ALFD_INNER_THROW)
      return ctx->err = "nested Mp CG (Bt Mp^-1 B of Aug) did not converge (SolverControl::NoConvergence)",
             ALFD_E_NO_CONVERGENCE_INNER;
    ctx->inner_failures++;
  }
  return ALFD_OK;
}

// dst = alpha * W^-1 src on the multiplier block (padded vectors; dst may alias src)
static int winv_scale(alfd_ctx *ctx, double alpha, const double *src, double *dst) {
  const int64_t nlp = pad_chunk(ctx->n[ctx->nblocks - 1]);
  if (ctx->cfg.w_inverse == ALFD_W_DIAGONAL) {
    VEC_LAUNCH(pmul_scale_kernel, nlp, 24, alpha, ctx->diag[ALFD_INVW], src, dst);
    return ALFD_OK;
  }
  RC(mass_solve(ctx, src, ctx->m_tmp));
  const double *z = ctx->m_tmp;
  if (ctx->cfg.w_inverse == ALFD_W_MASS_INV_SQUARED) {
    RC(mass_solve(ctx, ctx->m_tmp, ctx->m_tmp2));
    z = ctx->m_tmp2;
  }
  VEC_LAUNCH(scale_copy_kernel, nlp, 16, alpha, z, dst);
  return ALFD_OK;
}

// ---- RationalPreconditioner (rational_preconditioner.h:29-63) ----------------
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
constexpr int kRatSystems = 21;  // 20 shifted systems + the mass system

// v1 = sum_i rho res_i (A_Gamma - rho p_i M)^-1 u1 + res_0 M^-1 u1 : the 21 CG solves
// (Jacobi-preconditioned; the mass solve unpreconditioned, :54-56) run in lock step.
static int rational_apply(alfd_ctx *ctx, const double *u1, double *v1) {
  const int64_t npl = pad_chunk(ctx->n[1]);
  const int cps = (int)(npl / kChunk);
  const int64_t ntot = npl * kRatSystems;
  const unsigned grid = (unsigned)(ntot / kChunk);
  const alfd_control &ctl = ctx->cfg.rational;
  double *sh = ctx->rt_scb_host;
  hipLaunchKernelGGL(b_replicate_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, cps, u1, ctx->rt_r);
  HIPC(hipMemsetAsync(ctx->rt_x, 0, ntot * sizeof(double), ctx->stream));
  HIPC(hipMemsetAsync(ctx->rt_Ap, 0, ntot * sizeof(double), ctx->stream));
  for (int s = 0; s < kRatSystems; ++s) {
    for (int k = 0; k < kBS; ++k) sh[s * kBS + k] = 0.0;
    sh[s * kBS + B_ACTIVE] = 1.0;
  }
  HIPC(hipMemcpyAsync(ctx->rt_scb, sh, kRatSystems * kBS * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  // initial residuals
  hipLaunchKernelGGL(dot_partial_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, ctx->rt_r, ctx->rt_r,
                     ctx->rt_partial);
  hipLaunchKernelGGL(b_final_kernel, dim3(kRatSystems), dim3(kBlock), 0, ctx->stream, ctx->rt_partial, cps,
                     ctx->rt_scb, (int)FIN_STORE);
  HIPC(hipMemcpyAsync(sh, ctx->rt_scb, kRatSystems * kBS * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  Control sc[kRatSystems];
  State st[kRatSystems];
  int its[kRatSystems];
  int nactive = 0;
  for (int s = 0; s < kRatSystems; ++s) {
    sc[s] = Control{ctl};
    its[s] = 0;
    st[s] = sc[s].check(0, std::sqrt(sh[s * kBS + B_RR]));
    nactive += st[s] == ITERATE;
  }
  int it = 0;
  while (nactive > 0) {
    ++it;
    // freeze the systems that have stopped
    for (int s = 0; s < kRatSystems; ++s) sh[s * kBS + B_ACTIVE] = st[s] == ITERATE ? 1.0 : 0.0;
    for (int s = 0; s < kRatSystems; ++s)
      HIPC(hipMemcpyAsync(ctx->rt_scb + s * kBS + B_ACTIVE, sh + s * kBS + B_ACTIVE, sizeof(double),
                          hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(b_jacobi_dot_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, ctx->rt_scb, cps,
                       ctx->rt_dinv, ctx->rt_r, ctx->rt_z, ctx->rt_partial);
    hipLaunchKernelGGL(b_final_kernel, dim3(kRatSystems), dim3(kBlock), 0, ctx->stream, ctx->rt_partial, cps,
                       ctx->rt_scb, (int)FIN_RZ);
    hipLaunchKernelGGL(b_p_update_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, ctx->rt_scb, cps,
                       it == 1 ? 1 : 0, ctx->rt_z, ctx->rt_p);
    launch_spmv(ctx, ctx->rat_mat, ctx->rt_p, ctx->rt_Ap, 0, 0.0, nullptr, nullptr);
    hipLaunchKernelGGL(dot_partial_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, ctx->rt_p, ctx->rt_Ap,
                       ctx->rt_partial);
    hipLaunchKernelGGL(b_final_kernel, dim3(kRatSystems), dim3(kBlock), 0, ctx->stream, ctx->rt_partial, cps,
                       ctx->rt_scb, (int)FIN_ALPHA);
    hipLaunchKernelGGL(b_xr_update_dot_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, ctx->rt_scb, cps,
                       ctx->rt_p, ctx->rt_Ap, ctx->rt_x, ctx->rt_r, ctx->rt_partial);
    hipLaunchKernelGGL(b_final_kernel, dim3(kRatSystems), dim3(kBlock), 0, ctx->stream, ctx->rt_partial, cps,
                       ctx->rt_scb, (int)FIN_STORE);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(sh, ctx->rt_scb, kRatSystems * kBS * sizeof(double), hipMemcpyDeviceToHost,
                        ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    nactive = 0;
    for (int s = 0; s < kRatSystems; ++s)
      if (st[s] == ITERATE) {
        its[s] = it;
        st[s] = sc[s].check(it, std::sqrt(sh[s * kBS + B_RR]));
        nactive += st[s] == ITERATE;
      }
  }
  for (int s = 0; s < kRatSystems; ++s) {
    ctx->rational_its += its[s];
    if (st[s] == FAILURE) {
      if (std::isnan(sc[s].last_value)) return ctx->err = "rational CG breakdown (NaN)", ALFD_E_BREAKDOWN;
      if (ctx->cfg.on_inner_failure == ALFD_INNER_THROW)
        return ctx->err = "rational-preconditioner CG did not converge", ALFD_E_NO_CONVERGENCE_INNER;
      ctx->inner_failures++;
    }
  }
  hipLaunchKernelGGL(b_combine_kernel, dim3((unsigned)cps), dim3(kBlock), 0, ctx->stream, kRatSystems, npl,
                     ctx->rt_coef, ctx->rt_x, v1);
  HIPC(hipGetLastError());
  return ALFD_OK;
}

// Preconditioner vmult on padded device block vectors.
static int precond_apply(alfd_ctx *ctx, const double *u, double *v) {
  ctx->precond_applications++;
  const alfd_config &c = ctx->cfg;
  const double *w = ctx->diag[ALFD_INVW];
  const int64_t *off = ctx->off;
  const int64_t n0p = pad_chunk(ctx->n[0]), n1p = pad_chunk(ctx->n[1]), n2p = pad_chunk(ctx->n[2]);
  if (c.variant == ALFD_AL2) {
    // augmented_lagrangian_preconditioner.h:28-34
    RC(winv_scale(ctx, -c.gamma, u + off[1], v + off[1]));
    VEC_LAUNCH(scale_copy_kernel, n0p, 16, 1.0, u + off[0], ctx->rhs_tmp);
    RC(spmv(ctx, ALFD_CT, v + off[1], ctx->rhs_tmp, 1, -1.0));
    return inner_solve(ctx, OP_AUG, ctx->rhs_tmp, v + off[0]);
  }
  if (c.variant == ALFD_AL_STOKES || c.variant == ALFD_AL_STOKES_DIAG) {
    // :62-70 (block triangular) / :95-103 (block diagonal SPD)
    const bool tri = c.variant == ALFD_AL_STOKES;
    const double sgn = tri ? -1.0 : 1.0;
    RC(winv_scale(ctx, sgn * c.gamma, u + off[2], v + off[2]));
    RC(inner_solve(ctx, OP_MP, u + off[1], ctx->q_tmp));
    VEC_LAUNCH(scale_copy_kernel, n1p, 16, sgn * c.gamma_grad_div, ctx->q_tmp, v + off[1]);
    VEC_LAUNCH(scale_copy_kernel, n0p, 16, 1.0, u + off[0], ctx->rhs_tmp);
    if (tri) {
      RC(spmv(ctx, ALFD_BT, v + off[1], ctx->rhs_tmp, 1, -1.0));
      RC(spmv(ctx, ALFD_CT, v + off[2], ctx->rhs_tmp, 1, -1.0));
    }
    return inner_solve(ctx, OP_AUG, ctx->rhs_tmp, v + off[0]);
  }
  if (c.variant == ALFD_AL_ELL_MODIFIED) {
    // BlockTriangularALPreconditionerModified::vmult, ...preconditioner.h:225-228
    double *d0 = v + off[0], *d1 = v + off[1], *d2 = v + off[2];
    RC(winv_scale(ctx, -c.gamma, u + off[2], d2));                              // d2 = -gamma invW lambda
    HIPC(hipMemcpyAsync(ctx->q_tmp, u + off[1], n1p * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    RC(spmv(ctx, ALFD_M, d2, ctx->q_tmp, 1, 1.0));                              // u2 + M d2
    RC(inner_solve(ctx, OP_A22, ctx->q_tmp, d1));                               // d1 = A22_inv (...)
    if (c.w_inverse != ALFD_W_DIAGONAL) {                                        // t = invW M d1
      RC(spmv(ctx, ALFD_M, d1, ctx->t_lam, 0));
      RC(winv_scale(ctx, 1.0, ctx->t_lam, ctx->t_lam));
    } else {
      RC(spmv(ctx, ALFD_M, d1, ctx->t_lam, 2, 0.0, w));
    }
    VEC_LAUNCH(scale_copy_kernel, n0p, 16, 1.0, u + off[0], ctx->rhs_tmp);
    RC(spmv(ctx, ALFD_CT, ctx->t_lam, ctx->rhs_tmp, 1, c.gamma));               // u + gamma Ct t
    RC(spmv(ctx, ALFD_CT, d2, ctx->rhs_tmp, 1, -1.0));                          //   - Ct d2
    return inner_solve(ctx, OP_AUG, ctx->rhs_tmp, d0);                          // d0 = A11_inv (...)
  }
  if (c.variant == ALFD_AL_ELL_IDEAL) {
    // BlockTriangularALPreconditioner::vmult, ...preconditioner.h:130-156
    RC(winv_scale(ctx, -c.gamma, u + off[2], v + off[2]));
    HIPC(hipMemcpyAsync(ctx->rhs_tmp, u, off[2] * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    RC(spmv(ctx, ALFD_CT, v + off[2], ctx->rhs_tmp, 1, -1.0));                  // u0 - Ct v2
    RC(spmv(ctx, ALFD_M, v + off[2], ctx->rhs_tmp + off[1], 1, 1.0));           // u1 + M v2
    return inner_solve(ctx, OP_AUG2, ctx->rhs_tmp, v);                          // [v0;v1] = Aug_inv (...)
  }
  if (c.variant == ALFD_RATIONAL) {
    // RationalPreconditioner::vmult (block diagonal, SPD): v0 = K_inv u0, v1 = rational(u1)
    RC(inner_solve(ctx, OP_K, u + off[0], v + off[0]));
    return rational_apply(ctx, u + off[1], v + off[1]);
  }
  return ctx->err = "preconditioner variant not implemented yet", ALFD_E_UNSUPPORTED;
}

// AA.vmult on padded device block vectors.
static int system_apply(alfd_ctx *ctx, const double *x, double *y) {
  const alfd_config &c = ctx->cfg;
  const int64_t *off = ctx->off;
  const int last = ctx->nblocks - 1;
  const double *w = ctx->diag[ALFD_INVW];
  if (c.variant == ALFD_AL2 || c.variant == ALFD_AL_STOKES || c.variant == ALFD_AL_STOKES_DIAG) {
    const double *x0 = x + off[0];
    double *y0 = y + off[0];
    RC(spmv(ctx, ALFD_A, x0, y0, 0));
    if (c.aug_assembled) {
      RC(spmv(ctx, ALFD_C, x0, y + off[last], 0));
    } else {
      if (c.w_inverse != ALFD_W_DIAGONAL) {
        RC(spmv(ctx, ALFD_C, x0, y + off[last], 0));
        RC(winv_scale(ctx, 1.0, y + off[last], ctx->t_lam));
      } else {
        RC(spmv(ctx, ALFD_C, x0, y + off[last], 3, 0.0, w, ctx->t_lam));
      }
      RC(spmv(ctx, ALFD_CT, ctx->t_lam, y0, 1, c.gamma));
    }
    if (gd_nested(ctx)) {
      // y0 = fma(gamma_gd, (Bt q)_i, y0), q = Mp^-1 (B x0), before + Bt x1; B x0 is block 1 of y
      RC(spmv(ctx, ALFD_B, x0, y + off[1], 0));
      RC(nested_mp_solve(ctx, y + off[1], ctx->gd_q));
      RC(spmv(ctx, ALFD_BT, ctx->gd_q, y0, 1, c.gamma_grad_div));
      RC(spmv(ctx, ALFD_BT, x + off[1], y0, 1, 1.0));
    } else if (ctx->nblocks == 3) {
      RC(spmv(ctx, ALFD_BT, x + off[1], y0, 1, 1.0));
      RC(spmv(ctx, ALFD_B, x0, y + off[1], 0));
    }
    RC(spmv(ctx, ALFD_CT, x + off[last], y0, 1, 1.0));
    return ALFD_OK;
  }
  if (c.variant == ALFD_RATIONAL) {
    // AA = [[K, Ct],[C, 0]] (immersed_laplace.cc:596-597)
    RC(spmv(ctx, ALFD_A, x + off[0], y + off[0], 0));
    RC(spmv(ctx, ALFD_CT, x + off[1], y + off[0], 1, 1.0));
    return spmv(ctx, ALFD_C, x + off[0], y + off[1], 0);
  }
  if (is_elliptic(c.variant)) {
    // elliptic_interface.cc:810-819
    const double *x0 = x + off[0], *x1 = x + off[1], *x2 = x + off[2];
    double *y0 = y + off[0], *y1 = y + off[1], *y2 = y + off[2];
    RC(spmv(ctx, ALFD_C, x0, y2, 0));
    RC(spmv(ctx, ALFD_M, x1, y2, 1, -1.0));                                     // y2 = C x0 - M x1
    RC(winv_scale(ctx, 1.0, y2, ctx->t_lam));
    RC(spmv(ctx, ALFD_A, x0, y0, 0));
    RC(spmv(ctx, ALFD_CT, ctx->t_lam, y0, 1, c.gamma));
    RC(spmv(ctx, ALFD_CT, x2, y0, 1, 1.0));
    RC(spmv(ctx, ALFD_A2, x1, y1, 0));
    RC(spmv(ctx, ALFD_M, ctx->t_lam, y1, 1, -c.gamma2));
    return spmv(ctx, ALFD_M, x2, y1, 1, -1.0);
  }
  return ctx->err = "system operator variant not implemented yet", ALFD_E_UNSUPPORTED;
}

// ---------------------------------------------------------------- FGMRES
static int block_dots(alfd_ctx *ctx, const double *Vb, int count, const double *w, int out) {
  const int64_t N = ctx->ntot(), nb = N / kChunk;
  if (nb > 0) {
    Timer tm(ctx, ALFD_T_DOT, 8.0 * N * (count + 1));
    hipLaunchKernelGGL(multi_dot_partial_kernel, dim3((unsigned)nb), dim3(kBlock), 0, ctx->stream, Vb, N,
                       count, w, ctx->partial, ctx->pstride);
  }
  HIPC(hipGetLastError());
  return finish_dots(ctx, nb, count, out, FIN_STORE);
}

static int fgmres(alfd_ctx *ctx, alfd_result *out) {
  const alfd_config &c = ctx->cfg;
  const int m = c.restart;
  const int64_t N = ctx->ntot();
  double *x = ctx->xb, *b = ctx->bb;
  std::vector<double> H((size_t)(m + 1) * m, 0.0), cs(m), sn(m), g(m + 1), h(m + 2), h2(m + 2), y(m);
  Control sc{c.outer};
  int k = 0;
  State st = ITERATE;
  double res = 0;
  ctx->history.clear();
  auto Vj = [&](int j) { return ctx->V + (int64_t)j * N; };
  auto Zj = [&](int j) { return ctx->Z + (int64_t)j * N; };
  do {
    RC(system_apply(ctx, x, Vj(0)));
    VEC_LAUNCH(sub_from_kernel, N, 24, b, Vj(0));
    RC(dot_async(ctx, N, Vj(0), Vj(0), S_TMP));
    RC(read_scalars(ctx, S_TMP, 1));
    res = std::sqrt(ctx->sc_host[S_TMP]);
    st = sc.check(k, res);
    if (k == 0) ctx->history.push_back(res);
    if (c.log_level >= 2 && ctx->rank == 0) std::printf("DEAL:FGMRES::Check %d\t%.17g\n", k, res);
    if (st != ITERATE) break;
    if (res != 0.0) VEC_LAUNCH(scale_kernel, N, 16, (const double *)nullptr, 0, 0, 1.0 / res, Vj(0));
    g[0] = res;
    int j = 0;
    for (; j < m && st == ITERATE; ++j) {
      RC(precond_apply(ctx, Vj(j), Zj(j)));
      double *wv = Vj(j + 1);
      RC(system_apply(ctx, Zj(j), wv));
      if (c.orthogonalization == ALFD_ORTH_MGS) {
        for (int i = 0; i <= j; ++i) {
          RC(dot_async(ctx, N, Vj(i), wv, S_H + i));
          VEC_LAUNCH(multi_axpy_neg_kernel, N, 24, Vj(i), N, 1, ctx->sc, (int)S_H + i, wv);
        }
        RC(read_scalars(ctx, S_H, j + 1));
        for (int i = 0; i <= j; ++i) h[i] = ctx->sc_host[S_H + i];
      } else {
        RC(block_dots(ctx, ctx->V, j + 1, wv, S_H));
        VEC_LAUNCH(multi_axpy_neg_kernel, N, 8.0 * (j + 3), ctx->V, N, j + 1, ctx->sc, (int)S_H, wv);
        if (c.orthogonalization == ALFD_ORTH_CGS2) {
          RC(block_dots(ctx, ctx->V, j + 1, wv, S_H + kMaxBasis));
          VEC_LAUNCH(multi_axpy_neg_kernel, N, 8.0 * (j + 3), ctx->V, N, j + 1, ctx->sc,
                     (int)S_H + kMaxBasis, wv);
          RC(read_scalars(ctx, S_H, 2 * kMaxBasis));
          for (int i = 0; i <= j; ++i) h[i] = ctx->sc_host[S_H + i] + ctx->sc_host[S_H + kMaxBasis + i];
        } else {
          RC(read_scalars(ctx, S_H, j + 1));
          for (int i = 0; i <= j; ++i) h[i] = ctx->sc_host[S_H + i];
        }
      }
      RC(dot_async(ctx, N, wv, wv, S_TMP));
      RC(read_scalars(ctx, S_TMP, 1));
      h[j + 1] = std::sqrt(ctx->sc_host[S_TMP]);
      if (h[j + 1] != 0.0)
        VEC_LAUNCH(scale_kernel, N, 16, (const double *)nullptr, 0, 0, 1.0 / h[j + 1], wv);
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
      ctx->history.push_back(res);
      if (c.log_level >= 2 && ctx->rank == 0) std::printf("DEAL:FGMRES::Check %d\t%.17g\n", k, res);
    }
    for (int i = j - 1; i >= 0; --i) {
      double s = g[i];
      for (int l = i + 1; l < j; ++l) s -= H[(size_t)i * m + l] * y[l];
      y[i] = s / H[(size_t)i * m + i];
    }
    for (int i = 0; i < j; ++i) ctx->sc_host[S_H + i] = y[i];
    HIPC(hipMemcpyAsync(ctx->sc + S_H, ctx->sc_host + S_H, j * sizeof(double), hipMemcpyHostToDevice,
                        ctx->stream));
    VEC_LAUNCH(multi_axpy_kernel, N, 8.0 * (j + 2), ctx->Z, N, j, ctx->sc, (int)S_H, x);
    HIPC(hipStreamSynchronize(ctx->stream));  // sc_host is reused next cycle
  } while (st == ITERATE);
  out->outer_iterations = k;
  out->initial_residual = sc.initial;
  out->last_residual = res;
  if (c.log_level >= 1 && ctx->rank == 0)
    std::printf(st == SUCCESS ? "DEAL:FGMRES::Convergence step %d value %.17g\n"
                              : "DEAL:FGMRES::Failure step %d value %.17g\n",
                k, res);
  if (st != SUCCESS) {
    ctx->err = "FGMRES did not converge (SolverControl::NoConvergence)";
    return std::isnan(res) ? ALFD_E_BREAKDOWN : ALFD_E_NO_CONVERGENCE_OUTER;
  }
  return ALFD_OK;
}

// Least squares min || beta e1 - H(0:n, 0:n-1) y || of the (n+1) x n leading Hessenberg block by
// Givens rotations (deal.II <= 9.5 uses Householder::least_squares: the same minimiser).  H is
// stored row-major with leading dimension m.  Returns the residual norm, y[0..n).
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

// SolverFGMRES of deal.II <= 9.5 [EXT] (alfd_fgmres_flavour): modified Gram-Schmidt, delayed
// least-squares check, no counter increment at j = 0 of a cycle.
static int fgmres_dealii95(alfd_ctx *ctx, alfd_result *out) {
  const alfd_config &c = ctx->cfg;
  const int m = c.restart;
  const int64_t N = ctx->ntot();
  double *x = ctx->xb, *b = ctx->bb;
  std::vector<double> H((size_t)(m + 1) * m, 0.0), y(m, 0.0);
  Control sc{c.outer};
  int k = 0;
  State st = ITERATE;
  double res = 0;
  ctx->history.clear();
  auto Vj = [&](int j) { return ctx->V + (int64_t)j * N; };
  auto Zj = [&](int j) { return ctx->Z + (int64_t)j * N; };
  double *aux = Vj(m);
  auto dotv = [&](const double *p, const double *q, double *r) -> int {
    RC(dot_async(ctx, N, p, q, S_TMP));
    RC(read_scalars(ctx, S_TMP, 1));
    *r = ctx->sc_host[S_TMP];
    return ALFD_OK;
  };
  do {
    RC(system_apply(ctx, x, aux));
    VEC_LAUNCH(sub_from_kernel, N, 24, b, aux);                  // aux = b - AA x
    double bb2 = 0;
    RC(dotv(aux, aux, &bb2));
    const double beta = std::sqrt(bb2);
    res = beta;
    st = sc.check(k, res);
    if (k == 0) ctx->history.push_back(res);
    if (c.log_level >= 2 && ctx->rank == 0) std::printf("DEAL:FGMRES::Check %d\t%.17g\n", k, res);
    if (st != ITERATE) break;
    std::fill(H.begin(), H.end(), 0.0);
    double a = beta;
    int ny = 0;
    for (int j = 0; j < m; ++j) {
      if (a != 0.0) VEC_LAUNCH(scale_copy_kernel, N, 16, 1.0 / a, aux, Vj(j));   // v_j = aux / a
      else HIPC(hipMemsetAsync(Vj(j), 0, N * sizeof(double), ctx->stream));
      RC(precond_apply(ctx, Vj(j), Zj(j)));
      RC(system_apply(ctx, Zj(j), aux));
      double h = 0;
      RC(dotv(aux, Vj(0), &h));
      H[(size_t)0 * m + j] = h;
      for (int i = 0; i < j; ++i) {                              // H(i+1,j) = (aux -= H(i,j) v_i) . v_{i+1}
        VEC_LAUNCH(axpy_kernel, N, 24, (const double *)nullptr, 0, -H[(size_t)i * m + j], Vj(i), aux);
        RC(dotv(aux, Vj(i + 1), &h));
        H[(size_t)(i + 1) * m + j] = h;
      }
      VEC_LAUNCH(axpy_kernel, N, 24, (const double *)nullptr, 0, -H[(size_t)j * m + j], Vj(j), aux);
      RC(dotv(aux, aux, &h));
      H[(size_t)(j + 1) * m + j] = a = std::sqrt(h);
      if (j > 0) {
        res = hessenberg_lsq(H, m, j, beta, y);
        ny = j;
        ++k;
        st = sc.check(k, res);
        ctx->history.push_back(res);
        if (c.log_level >= 2 && ctx->rank == 0) std::printf("DEAL:FGMRES::Check %d\t%.17g\n", k, res);
        if (st != ITERATE) break;
      }
    }
    for (int i = 0; i < ny; ++i) ctx->sc_host[S_H + i] = y[i];
    if (ny > 0) {
      HIPC(hipMemcpyAsync(ctx->sc + S_H, ctx->sc_host + S_H, ny * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
      VEC_LAUNCH(multi_axpy_kernel, N, 8.0 * (ny + 2), ctx->Z, N, ny, ctx->sc, (int)S_H, x);
    }
    HIPC(hipStreamSynchronize(ctx->stream));
  } while (st == ITERATE);
  out->outer_iterations = k;
  out->initial_residual = sc.initial;
  out->last_residual = res;
  if (c.log_level >= 1 && ctx->rank == 0)
    std::printf(st == SUCCESS ? "DEAL:FGMRES::Convergence step %d value %.17g\n"
                              : "DEAL:FGMRES::Failure step %d value %.17g\n",
                k, res);
  if (st != SUCCESS) {
    ctx->err = "FGMRES did not converge (SolverControl::NoConvergence)";
    return std::isnan(res) ? ALFD_E_BREAKDOWN : ALFD_E_NO_CONVERGENCE_OUTER;
  }
  return ALFD_OK;
}

// deal.II SolverMinRes [EXT] on device vectors (immersed_laplace.cc:629-631,
// stokes...:1057-1064).  Vectors: u0,u1,u2 | m0,m1,m2 | v live in the Krylov arenas.
static int minres(alfd_ctx *ctx, alfd_result *out) {
  const alfd_config &c = ctx->cfg;
  const int64_t N = ctx->ntot();
  double *x = ctx->xb, *b = ctx->bb;
  double *u0 = ctx->V, *u1 = ctx->V + N, *u2 = ctx->V + 2 * N;
  double *m0 = ctx->Z, *m1 = ctx->Z + N, *m2 = ctx->Z + 2 * N;
  double *v = ctx->V + 3 * N;
  double delta[3] = {0, 0, 0}, f[2] = {0, 0}, e[2] = {0, 0};
  double r_l2 = 0, r0 = 0, tau = 0, cc = 0, ss = 0, d_ = 0, phibar = 0;
  int j = 1;
  Control sc{c.outer};
  ctx->history.clear();
  auto dotv = [&](const double *a, const double *bb_, double *res) -> int {
    RC(dot_async(ctx, N, a, bb_, S_TMP));
    RC(read_scalars(ctx, S_TMP, 1));
    *res = ctx->sc_host[S_TMP];
    return ALFD_OK;
  };
  RC(system_apply(ctx, x, m0));
  HIPC(hipMemcpyAsync(u1, m0, N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  VEC_LAUNCH(sub_from_kernel, N, 24, b, u1);                       // u1 = b - A x
  HIPC(hipMemsetAsync(v, 0, N * sizeof(double), ctx->stream));
  RC(precond_apply(ctx, u1, v));
  RC(dotv(v, u1, &delta[1]));
  if (delta[1] < 0) return ctx->err = "MinRes: preconditioner not positive definite", ALFD_E_BREAKDOWN;
  r0 = std::sqrt(delta[1]);
  r_l2 = r0;
  phibar = r0;
  HIPC(hipMemsetAsync(u0, 0, N * sizeof(double), ctx->stream));
  delta[0] = 1.0;
  HIPC(hipMemsetAsync(ctx->Z, 0, 3 * N * sizeof(double), ctx->stream));
  State st = sc.check(0, r_l2);
  ctx->history.push_back(r_l2);
  if (c.log_level >= 2 && ctx->rank == 0) std::printf("DEAL:minres::Check 0\t%.17g\n", r_l2);
  while (st == ITERATE) {
    if (delta[1] != 0)
      VEC_LAUNCH(scale_kernel, N, 16, (const double *)nullptr, 0, 0, 1.0 / std::sqrt(delta[1]), v);
    else
      HIPC(hipMemsetAsync(v, 0, N * sizeof(double), ctx->stream));
    RC(system_apply(ctx, v, u2));
    VEC_LAUNCH(axpy_kernel, N, 24, (const double *)nullptr, 0, -std::sqrt(delta[1] / delta[0]), u0, u2);
    double gamma = 0;
    RC(dotv(u2, v, &gamma));
    VEC_LAUNCH(axpy_kernel, N, 24, (const double *)nullptr, 0, -gamma / std::sqrt(delta[1]), u1, u2);
    HIPC(hipMemcpyAsync(m0, v, N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    RC(precond_apply(ctx, u2, v));
    RC(dotv(v, u2, &delta[2]));
    if (delta[2] < 0) return ctx->err = "MinRes: preconditioner not positive definite", ALFD_E_BREAKDOWN;
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
    // tau_j = c_j phibar_{j-1}, phibar_j = s_j phibar_{j-1}: division-free form of deal.II's
    // "tau *= s/c; tau *= c" (which is 0*inf when the first Lanczos coefficient is 0)
    cc = d_ / d;
    ss = std::sqrt(delta[2]) / d;
    tau = cc * phibar;
    phibar = ss * phibar;
    VEC_LAUNCH(axpy_kernel, N, 24, (const double *)nullptr, 0, -e[0], m1, m0);
    if (j > 1) VEC_LAUNCH(axpy_kernel, N, 24, (const double *)nullptr, 0, -f[0], m2, m0);
    VEC_LAUNCH(scale_kernel, N, 16, (const double *)nullptr, 0, 0, 1.0 / d, m0);
    VEC_LAUNCH(axpy_kernel, N, 24, (const double *)nullptr, 0, tau, m0, x);
    r_l2 *= std::fabs(ss);
    st = sc.check(j, r_l2);
    ctx->history.push_back(r_l2);
    if (c.log_level >= 2 && ctx->rank == 0) std::printf("DEAL:minres::Check %d\t%.17g\n", j, r_l2);
    ++j;
    double *t = u0;
    u0 = u1;
    u1 = u2;
    u2 = t;
    t = m2;
    m2 = m1;
    m1 = m0;
    m0 = t;
    delta[0] = delta[1];
    delta[1] = delta[2];
    f[0] = f[1];
    e[0] = e[1];
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  out->outer_iterations = j - 1;
  out->initial_residual = sc.initial;
  out->last_residual = r_l2;
  if (c.log_level >= 1 && ctx->rank == 0)
    std::printf(st == SUCCESS ? "DEAL:minres::Convergence step %d value %.17g\n"
                              : "DEAL:minres::Failure step %d value %.17g\n",
                j - 1, r_l2);
  if (st != SUCCESS) {
    ctx->err = "MinRes did not converge (SolverControl::NoConvergence)";
    return std::isnan(r_l2) ? ALFD_E_BREAKDOWN : ALFD_E_NO_CONVERGENCE_OUTER;
  }
  return ALFD_OK;
}

// ---------------------------------------------------------------- halo
static int halo_exchange(alfd_ctx *ctx, DevCsr &m, const double *x, hipStream_t st) {
  if (!st) st = ctx->stream;
  const int64_t nsend = m.send_off.back();
  if (nsend > 0) {
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)((nsend + 255) / 256)), dim3(256), 0, st,
                       nsend, m.send_idx, x, m.send_buf);
    HIPC(hipGetLastError());
  }
  RC(comm_alltoallv(ctx, m.send_buf, m.send_off.data(), m.halo, m.recv_off.data(), sizeof(double), st));
  return ALFD_OK;
}

// Which vector blocks a slot maps between: {row block, col block}; -1 = last.
static void slot_blocks(const alfd_ctx *ctx, int slot, int *rb, int *cb) {
  const int last = ctx->nblocks - 1;
  switch (slot) {
    case ALFD_A: *rb = 0, *cb = 0; break;
    case ALFD_BT: *rb = 0, *cb = 1; break;
    case ALFD_B: *rb = 1, *cb = 0; break;
    case ALFD_CT: *rb = 0, *cb = last; break;
    case ALFD_C: *rb = last, *cb = 0; break;
    case ALFD_M: *rb = last, *cb = last; break;
    case ALFD_MP: *rb = 1, *cb = 1; break;
    case ALFD_A2: *rb = 1, *cb = 1; break;
    default: *rb = last, *cb = last; break;
  }
}

static void choose_lanes(DevCsr &m, int64_t nonempty) {
  const double avg = nonempty ? (double)m.nnz / (double)nonempty : 0.0;
  if (avg > 48) m.L = 64;
  else if (avg > 24) m.L = 32;
  else if (avg > 12) m.L = 16;
  else if (avg > 6) m.L = 8;
  else m.L = 4;
}

// Host-only part of the halo plan of one row-partitioned matrix (no HIP, no
// communication): off-rank columns sorted unique (ascending global index =>
// grouped by owner), columns rewritten to the local index space
// [owned | halo], and the receive counts per owner.  Exposed through the ABI
// as alfd_host_halo_plan so it can be exercised without a GPU.
static void host_halo_plan(int64_t nnz, const int32_t *col, const int64_t *col_offsets, int nranks, int rank,
                           int32_t *col_local, std::vector<int32_t> &halo_globals, int64_t *recv_off) {
  const int64_t c0 = col_offsets[rank], c1 = col_offsets[rank + 1];
  halo_globals.clear();
  for (int64_t k = 0; k < nnz; ++k)
    if (col[k] < c0 || col[k] >= c1) halo_globals.push_back(col[k]);
  std::sort(halo_globals.begin(), halo_globals.end());
  halo_globals.erase(std::unique(halo_globals.begin(), halo_globals.end()), halo_globals.end());
  const int32_t n_local = (int32_t)(c1 - c0);
  for (int64_t k = 0; k < nnz; ++k) {
    const int32_t c = col[k];
    if (c >= c0 && c < c1)
      col_local[k] = (int32_t)(c - c0);
    else
      col_local[k] = n_local + (int32_t)(std::lower_bound(halo_globals.begin(), halo_globals.end(), c) -
                                         halo_globals.begin());
  }
  for (int p = 0; p <= nranks; ++p) recv_off[p] = 0;
  for (int32_t c : halo_globals) {
    const int owner =
        (int)(std::upper_bound(col_offsets, col_offsets + nranks + 1, (int64_t)c) - col_offsets) - 1;
    recv_off[owner + 1]++;
  }
  for (int p = 0; p < nranks; ++p) recv_off[p + 1] += recv_off[p];
}

// Build the LDS-window format of a long-row matrix (host, multi-threaded).
// col: column indices in the LOCAL index space [local | halo].
// ---- window / value-index format: pure host planning (also exported as
// alfd_host_window_plan so that CPU tests can decode and check it), then upload.
struct WindowParams {
  int RB_long = 96, short_scale = 2, RB_vi = 96, maxW = 4096, gap = 8;
  bool want_vi = true;
};
struct WindowPlan {
  bool win = false, vi = false;
  int RB = 0;
  int32_t maxW = 0;
  int64_t nb = 0, fallback = 0;
  std::vector<uint16_t> lcol;
  std::vector<int32_t> blkW, seg_begin, seg_col, seg_off;
  std::vector<uint8_t> vidx;
  std::vector<uint16_t> vidw;
  std::vector<int32_t> blk_dn, doff;
  std::vector<double> dict;
  int64_t vi_blocks = 0, vi_nnz = 0, wide_nnz = 0;
  std::vector<uint64_t> tab;
  std::vector<int32_t> cnt;
  int stride = 0;
};
static int window_row_block(const WindowParams &wp, int L) {
  // short rows: larger row blocks, so a window serves about as many entries as for L = 64
  return L == 64 ? wp.RB_long : std::min(512, wp.RB_long * wp.short_scale * 64 / L);
}

static void plan_window(int64_t nrows, int L, const int64_t *rp, const int32_t *col, const double *val,
                        const WindowParams &wp, WindowPlan &pl) {
  const int64_t nnz = rp[nrows];
  int RB = window_row_block(wp, L);
  const bool want_vi = wp.want_vi && L == 64;
  if (want_vi && wp.RB_vi > 0 && wp.RB_vi != RB) {
    // The value-indexed kernel has its own best block size.  Sample a few blocks: if their
    // values look dictionary-codable, build the window format with that block.
    const int64_t nb0 = (nrows + RB - 1) / RB;
    int good = 0, seen = 0;
    for (int64_t q = 0; q < 32 && q < nb0; ++q) {
      const int64_t b = nb0 * q / std::min<int64_t>(32, nb0);
      const int64_t k0 = rp[b * RB], k1 = rp[std::min<int64_t>((b + 1) * RB, nrows)];
      std::unordered_set<uint64_t> u;
      for (int64_t k = k0; k < k1 && u.size() <= 1024; ++k) {
        uint64_t bits;
        std::memcpy(&bits, &val[k], 8);
        u.insert(bits);
      }
      ++seen;
      good += u.size() <= 1024;
    }
    if (good * 4 >= seen * 3) RB = wp.RB_vi;
  }
  const int maxW = wp.maxW, GAP = wp.gap;
  const int64_t nb = (nrows + RB - 1) / RB;
  if (nb == 0 || nb > 2147483000LL) return;
  pl.RB = RB;
  pl.nb = nb;
  pl.lcol.assign(nnz, 0);
  pl.blkW.assign(nb, 0);
  std::vector<int32_t> blk_nseg(nb, 0);
  pl.vidx.assign(want_vi ? nnz : 0, 0);
  pl.vidw.assign(want_vi ? nnz : 0, 0);  // 16-bit codes (uploaded only if some block needs them)
  pl.blk_dn.assign(nb, -1);
  std::vector<std::vector<double>> t_dict(want_vi ? nb : 0);
  std::vector<int64_t> t_wide(64, 0);
  const int T = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::vector<int32_t>> t_seg_col(T), t_seg_off(T);
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t]() {
      const int64_t b0 = nb * t / T, b1 = nb * (t + 1) / T;
      std::vector<uint8_t> mark;
      std::vector<int32_t> pos;
      for (int64_t b = b0; b < b1; ++b) {
        const int64_t r0 = b * RB, r1 = std::min<int64_t>(r0 + RB, nrows);
        const int64_t k0 = rp[r0], k1 = rp[r1];
        if (k1 == k0) continue;
        int32_t clo = INT32_MAX, chi = -1;
        for (int64_t k = k0; k < k1; ++k) {
          clo = std::min(clo, col[k]);
          chi = std::max(chi, col[k]);
        }
        const int64_t range = (int64_t)chi - clo + 1;
        if (range > (int64_t)(1 << 22)) {
          pl.blkW[b] = -1;
          continue;
        }
        mark.assign(range, 0);
        for (int64_t k = k0; k < k1; ++k) mark[col[k] - clo] = 1;
        pos.assign(range, -1);
        int32_t W = 0, nseg = 0;
        const size_t seg_base = t_seg_col[t].size();
        int64_t c = 0;
        while (c < range) {
          if (!mark[c]) {
            ++c;
            continue;
          }
          // segment starts at c; extend over gaps shorter than GAP
          int64_t e = c, last = c;
          while (e < range) {
            if (mark[e]) last = e;
            else if (e - last >= GAP) break;
            ++e;
          }
          t_seg_col[t].push_back((int32_t)(clo + c));
          t_seg_off[t].push_back(W);
          for (int64_t q = c; q <= last; ++q) pos[q] = W++;
          ++nseg;
          c = last + 1;
        }
        if (W > maxW || W > 65535) {
          t_seg_col[t].resize(seg_base);
          t_seg_off[t].resize(seg_base);
          pl.blkW[b] = -1;
          continue;
        }
        pl.blkW[b] = W;
        blk_nseg[b] = nseg;
        for (int64_t k = k0; k < k1; ++k) pl.lcol[k] = (uint16_t)pos[col[k] - clo];
        if (want_vi) {
          // open-addressing table over the 64-bit patterns.  Up to 256 distinct values:
          // 8-bit codes; up to kDictMaxEntries: 16-bit codes; beyond that: raw block.
          constexpr int kTab = 2048;
          std::vector<uint64_t> keys(kTab);
          std::vector<int16_t> ids(kTab, (int16_t)-1);
          std::vector<double> &dv = t_dict[b];
          bool ok = true;
          for (int64_t k = k0; k < k1 && ok; ++k) {
            uint64_t bits;
            std::memcpy(&bits, &val[k], 8);
            uint32_t h = (uint32_t)((bits * 0x9E3779B97F4A7C15ull) >> 53);
            for (;;) {
              if (ids[h] < 0) {
                if ((int)dv.size() == kDictMaxEntries) {
                  ok = false;
                  break;
                }
                keys[h] = bits;
                ids[h] = (int16_t)dv.size();
                dv.push_back(val[k]);
                break;
              }
              if (keys[h] == bits) break;
              h = (h + 1) & (kTab - 1);
            }
            if (ok) pl.vidw[k] = (uint16_t)ids[h];
          }
          if (!ok) {
            dv.clear();
          } else if (dv.size() <= 256) {
            for (int64_t k = k0; k < k1; ++k) pl.vidx[k] = (uint8_t)pl.vidw[k];
            pl.blk_dn[b] = (int32_t)dv.size();
          } else {
            pl.blk_dn[b] = (int32_t)dv.size() | kDictWide;
            t_wide[t] += k1 - k0;
          }
        }
      }
    });
  for (auto &x : th) x.join();
  pl.seg_begin.assign(nb + 1, 0);
  for (int64_t b = 0; b < nb; ++b) pl.seg_begin[b + 1] = pl.seg_begin[b] + blk_nseg[b];
  for (int t = 0; t < T; ++t) {
    pl.seg_col.insert(pl.seg_col.end(), t_seg_col[t].begin(), t_seg_col[t].end());
    pl.seg_off.insert(pl.seg_off.end(), t_seg_off[t].begin(), t_seg_off[t].end());
  }
  int32_t mw = 0;
  for (int64_t b = 0; b < nb; ++b) {
    mw = std::max(mw, pl.blkW[b]);
    pl.fallback += pl.blkW[b] < 0;
  }
  pl.maxW = std::max(mw, 1);
  if (pl.fallback * 2 > nb) return;  // windows do not pay for this matrix: keep the plain kernels
  pl.win = true;
  if (!want_vi) return;
  pl.doff.assign(nb, 0);
  for (int64_t b = 0; b < nb; ++b) {
    pl.doff[b] = (int32_t)pl.dict.size();
    if (pl.blk_dn[b] < 0) continue;
    pl.dict.insert(pl.dict.end(), t_dict[b].begin(), t_dict[b].end());
    ++pl.vi_blocks;
    pl.vi_nnz += rp[std::min<int64_t>((b + 1) * RB, nrows)] - rp[b * RB];
  }
  for (int64_t e : t_wide) pl.wide_nnz += e;
  if (!(pl.vi_blocks * 2 > nb && pl.dict.size() < 2000000000ull)) return;  // worthwhile only if most blocks are coded
  pl.vi = true;
  int64_t longest = 0;
  for (int64_t r = 0; r < nrows; ++r) longest = std::max(longest, rp[r + 1] - rp[r]);
  if (RB > 250 || longest > 65535) return;
  // class-sorted batches of 4 rows per block
  const int stride = (RB + 3) / 4 + kVibMaxClass + 2;
  pl.stride = stride;
  pl.tab.assign((size_t)nb * stride * 4, 0);
  pl.cnt.assign(nb, 0);
  std::vector<std::thread> th2;
  for (int t = 0; t < T; ++t)
    th2.emplace_back([&, t]() {
      std::vector<int> ids[kVibMaxClass + 2];
      for (int64_t b = nb * t / T; b < nb * (t + 1) / T; ++b) {
        const int64_t r0 = b * RB, r1 = std::min<int64_t>(r0 + RB, nrows);
        for (auto &v : ids) v.clear();
        for (int64_t r = r0; r < r1; ++r) {
          const int64_t len = rp[r + 1] - rp[r];
          const int64_t cls = (len + 63) / 64;
          ids[cls > kVibMaxClass ? kVibMaxClass + 1 : cls].push_back((int)(r - r0));
        }
        int nbt = 0;
        for (int cls = 0; cls <= kVibMaxClass + 1; ++cls)
          for (size_t q = 0; q < ids[cls].size(); q += 4) {
            uint64_t *dst = &pl.tab[((size_t)b * stride + nbt++) * 4];
            for (int i = 0; i < 4; ++i) {
              const bool real = q + i < ids[cls].size();
              const int id = ids[cls][real ? q + i : q];  // filler: repeat the batch's first row
              const uint64_t ks = (uint64_t)(rp[r0 + id] - rp[r0]);
              const uint64_t len = (uint64_t)(rp[r0 + id + 1] - rp[r0 + id]);
              dst[i] = ks | (len << 32) | ((uint64_t)(real ? id : 0xff) << 48) | ((uint64_t)cls << 56);
            }
          }
        pl.cnt[b] = nbt;
      }
    });
  for (auto &x : th2) x.join();
}

template <class T>
static int upload_vec(alfd_ctx *ctx, DevCsr &m, T **dst, const std::vector<T> &v) {
  RC(csr_alloc(ctx, m, dst, (int64_t)v.size()));
  HIPC(hipMemcpyAsync(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
  return ALFD_OK;
}

static int build_window(alfd_ctx *ctx, DevCsr &m, const int64_t *rp, const int32_t *col, const double *val,
                        bool slot_is_user, bool skip_vi = false) {
  WindowParams wp;
  wp.RB_long = ctx->win_RB;
  wp.short_scale = ctx->win_short_scale;
  wp.RB_vi = ctx->win_RB_vi;
  wp.maxW = ctx->win_maxW;
  wp.gap = ctx->win_gap;
  // skip_vi: the batch-major form already holds the matrix with dictionaries of its own; the window plan then only
  // provides the 16-bit columns of the general 10 B/nnz kernel (a third of the planning time at N = 74)
  wp.want_vi = !skip_vi && ctx->win_vi && (slot_is_user || ctx->vi_levels);
  WindowPlan pl;
  plan_window(m.nrows, m.L, rp, col, val, wp, pl);
  if (!pl.win) return ALFD_OK;
  m.win_RB = pl.RB;
  m.win_maxW = pl.maxW;
  m.win_nblocks = pl.nb;
  m.win_fallback_blocks = pl.fallback;
  m.win_nseg = (int64_t)pl.seg_col.size();
  RC(upload_vec(ctx, m, &m.lcol, pl.lcol));
  RC(upload_vec(ctx, m, &m.blk_seg_begin, pl.seg_begin));
  RC(upload_vec(ctx, m, &m.blk_W, pl.blkW));
  RC(upload_vec(ctx, m, &m.seg_col, pl.seg_col));
  RC(upload_vec(ctx, m, &m.seg_off, pl.seg_off));
  HIPC(hipStreamSynchronize(ctx->stream));
  m.win = true;
  if (!pl.vi) return ALFD_OK;
  RC(upload_vec(ctx, m, &m.vidx, pl.vidx));
  if (pl.wide_nnz > 0) RC(upload_vec(ctx, m, &m.vidw, pl.vidw));
  RC(upload_vec(ctx, m, &m.blk_dict_off, pl.doff));
  RC(upload_vec(ctx, m, &m.blk_dict_n, pl.blk_dn));
  RC(upload_vec(ctx, m, &m.dict, pl.dict));
  if (pl.stride > 0) {
    RC(upload_vec(ctx, m, &m.vib_tab, pl.tab));
    RC(upload_vec(ctx, m, &m.vib_cnt, pl.cnt));
    m.vib_stride = pl.stride;
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  m.vi = true;
  m.vi_blocks = pl.vi_blocks;
  m.vi_nnz = pl.vi_nnz;
  m.vi_wide_nnz = pl.wide_nnz;
  m.vi_dict_total = (int64_t)pl.dict.size();
  if (ctx->cfg.log_level > 0)
    std::fprintf(stderr, "[alfd] value-indexed %s matrix: %lld rows, %lld of %lld blocks coded, dict %zu\n",
                 slot_is_user ? "user" : "level", (long long)m.nrows, (long long)pl.vi_blocks, (long long)pl.nb,
                 pl.dict.size());
  return ALFD_OK;
}


// ---- batch-major format (kernels_vs.hpp): host planning, then upload.
// Row blocks are lists of rows: runs of RB rows of the numbering, or the caller's blocks
// (alfd_set_row_blocks: bricks of the mesh graph).  The format is all-or-nothing: every block
// needs an x window of at most maxW slots, at most 256 distinct values, rows of at most
// kVsMaxLen entries; otherwise the matrix keeps the formats of plan_window.
struct VsPlan {
  bool ok = false;
  int64_t nb = 0, nbatch = 0, shared_nnz = 0, nb_interior = 0;
  bool dict_split = false;   // blocks were halved for their dictionaries (or row counts): wide codes may pay
  int rbs = 0, stride = 0;
  int32_t maxW = 0;
  std::vector<int32_t> blkW, seg_begin, seg_col, seg_off, doff, dn, cnt;
  std::vector<double> dict;
  std::vector<int64_t> sb;
  std::vector<uint8_t> stream;
  std::vector<uint64_t> tab;
  int wide = 0;       // 1: 10-bit codes / 11-bit window columns (VsFmt<1>)
  int64_t nb_in = 0;  // blocks before the dictionary limit halved any
  // side rows ("batch_major_side_rows"): the rows beyond kVsMaxLen entries, kept out of the blocks.  Global row numbers,
  // longest row first, ties by row number (partitioned operators: the side_interior rows that read no halo column
  // first, each group in that order), and their compact CSR, the entries in the row's own order
  std::vector<int32_t> side_rows, side_col;
  std::vector<int64_t> side_rp;
  std::vector<double> side_val;
  int64_t side_interior = 0;
};

// The share of a matrix's entries that side rows may hold.  Not a tuned number: a condition that keeps a matrix MADE of
// long rows on the window forms, where the one-wave-per-row side kernel would be the whole product.
constexpr double kVsSideMaxShare = 1.0 / 8;   // a power of two: the comparison below is exact

// The rows longer than kVsMaxLen entries, or false: there are none, they hold more than kVsSideMaxShare of the entries,
// or one has more than kSideMaxLen.  Fills the side list of pl and the row lists (optr / orows) without those rows:
// runs of RB rows of the numbering or the caller's blocks, a block left empty dropped.
static bool vs_take_side_rows(int64_t nrows, const int64_t *rp, const int32_t *col, const double *val, int RB, int64_t nb_in,
                              const int64_t *bptr, const int32_t *brows, int64_t n_local_cols, VsPlan &pl,
                              std::vector<int64_t> &optr, std::vector<int32_t> &orows) {
  std::vector<int32_t> side;
  int64_t side_nnz = 0;
  for (int64_t r = 0; r < nrows; ++r) {
    const int64_t n = rp[r + 1] - rp[r];
    if (n <= kVsMaxLen) continue;
    if (n > kSideMaxLen) return false;
    side.push_back((int32_t)r);
    side_nnz += n;
  }
  if (side.empty() || (double)side_nnz > kVsSideMaxShare * (double)rp[nrows]) return false;
  auto halo = [&](int32_t r) {
    if (n_local_cols < 0) return false;
    for (int64_t k = rp[r]; k < rp[r + 1]; ++k)
      if (col[k] >= n_local_cols) return true;
    return false;
  };
  std::vector<uint8_t> bnd(side.size(), 0);
  std::vector<size_t> order(side.size());
  for (size_t i = 0; i < side.size(); ++i) bnd[i] = halo(side[i]), order[i] = i;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    if (bnd[a] != bnd[b]) return bnd[a] < bnd[b];
    const int64_t la = rp[side[a] + 1] - rp[side[a]], lb = rp[side[b] + 1] - rp[side[b]];
    return la != lb ? la > lb : side[a] < side[b];
  });
  pl.side_rp.assign(1, 0);
  pl.side_col.reserve((size_t)side_nnz);
  pl.side_val.reserve((size_t)side_nnz);
  for (size_t i : order) {
    const int32_t r = side[i];
    pl.side_rows.push_back(r);
    pl.side_col.insert(pl.side_col.end(), col + rp[r], col + rp[r + 1]);
    pl.side_val.insert(pl.side_val.end(), val + rp[r], val + rp[r + 1]);
    pl.side_rp.push_back((int64_t)pl.side_col.size());
    pl.side_interior += (n_local_cols >= 0 && !bnd[i]) ? 1 : 0;   // 0 where there is no halo
  }
  const bool nat = bptr == nullptr;
  const int64_t nb = nat ? (nrows + RB - 1) / RB : nb_in;
  optr.assign(1, 0);
  orows.clear();
  orows.reserve((size_t)nrows - side.size());
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t lo = nat ? b * RB : bptr[b], hi = nat ? std::min<int64_t>((b + 1) * RB, nrows) : bptr[b + 1];
    for (int64_t i = lo; i < hi; ++i) {
      const int32_t r = nat ? (int32_t)i : brows[i];
      if (rp[r + 1] - rp[r] <= kVsMaxLen) orows.push_back(r);
    }
    if ((int64_t)orows.size() > optr.back()) optr.push_back((int64_t)orows.size());
  }
  return true;
}

constexpr int kVsBatchRows = 16;   // rows a batch descriptor names (16 x uint64 = 128 bytes)
constexpr int kVsRefineW = 2048;   // window a block halved for its window may keep (slots): 8 workgroups per CU; B at N = 74: 0.129 ms (4096: 0.138, 1536: 0.170, general kernel 0.414)
struct VsBatch {
  int cls, nreal, id[kVsBatchRows];   // plain: up to 4 rows; shared: up to 16
  bool shared;                        // the rows are translates of one another: one template + a window shift per row
  int32_t shift[kVsBatchRows];        // window slots, relative to row id[0]
};

// x window of a row block: maximal runs of used columns, gaps shorter than GAP bridged, cut into pieces
// of at most 64 slots (one wave-load each).  slot(c) = window slot of column c.
struct VsWindow {
  int32_t clo = 0, W = 0, nseg = 0;
  // the window as runs of consecutive columns: run i holds columns run_col[i] .. run_col[i] + run_len[i] - 1 in the
  // slots run_slot[i] ..  (sparse: a block of an operator whose rows reach far -- the divergence block of a Taylor-Hood
  // pair -- spans 300 k columns with 2 k of them used; dense per-column tables made planning such operators cost more
  // than planning A)
  std::vector<int32_t> run_col, run_slot, run_len;
  std::vector<uint8_t> mark;       // scratch, all zero between calls, grown on demand
  std::vector<int32_t> ucol;       // scratch
  int32_t slot(int32_t c) const {  // window slot of a column of the block
    size_t lo = 0, hi = run_col.size();
    while (hi - lo > 1) {
      const size_t mid = (lo + hi) / 2;
      if (run_col[mid] <= c) lo = mid;
      else hi = mid;
    }
    return run_slot[lo] + (c - run_col[lo]);
  }
};
static bool vs_window(const std::vector<int32_t> &rows, const int64_t *rp, const int32_t *col, int GAP, int maxW,
                      VsWindow &w, std::vector<int32_t> *seg_col, std::vector<int32_t> *seg_off) {
  w.ucol.clear();
  for (int32_t r : rows)
    for (int64_t k = rp[r]; k < rp[r + 1]; ++k) {
      const int32_t c = col[k];
      if ((size_t)c >= w.mark.size()) w.mark.resize((size_t)c + 1 + w.mark.size() / 2, 0);
      if (!w.mark[c]) {
        w.mark[c] = 1;
        w.ucol.push_back(c);
      }
    }
  for (int32_t c : w.ucol) w.mark[c] = 0;
  std::sort(w.ucol.begin(), w.ucol.end());
  w.clo = w.ucol.empty() ? 0 : w.ucol.front();
  w.run_col.clear();
  w.run_slot.clear();
  w.run_len.clear();
  w.W = 0;
  w.nseg = 0;
  size_t i = 0;
  while (i < w.ucol.size()) {
    const int32_t c = w.ucol[i];
    int32_t last = c;
    size_t j = i + 1;
    while (j < w.ucol.size() && w.ucol[j] - last <= GAP) last = w.ucol[j++];   // gaps shorter than GAP are bridged
    const int32_t len = last - c + 1;
    for (int32_t q0 = 0; q0 < len; q0 += 64) {   // pieces of at most 64 slots (one wave-load each)
      if (seg_col) {
        seg_col->push_back(c + q0);
        seg_off->push_back(w.W + q0);
      }
      ++w.nseg;
    }
    w.run_col.push_back(c);
    w.run_slot.push_back(w.W);
    w.run_len.push_back(len);
    w.W += len;
    if (w.W > 4096 && !seg_col) return false;   // hopeless already (the planner's callers pass no segment lists when probing)
    i = j;
  }
  if (w.run_col.empty()) {
    w.run_col.push_back(0);
    w.run_slot.push_back(0);
    w.run_len.push_back(0);
  }
  return w.W <= maxW && w.W <= 4096;
}

// Batches of one block.  Rows are grouped by chunk count (class); inside a class, rows that are
// translates of one another -- same length, same values entry by entry, window columns differing by one
// constant -- form SHARED batches (one stored template, a shift per row: what a uniform mesh gives for
// the rows of one node type inside a brick); the rest form plain batches, longest rows first.
static bool vs_batches(const std::vector<int32_t> &rows, const int64_t *rp, const int32_t *col, const double *val,
                       const VsWindow &w, std::vector<VsBatch> &out, bool share = true) {
  const int nr = (int)rows.size();
  out.clear();
  std::vector<int64_t> len(nr);
  std::vector<uint64_t> key(nr);
  std::vector<int32_t> first(nr, 0);
  for (int i = 0; i < nr; ++i) {
    const int64_t k0 = rp[rows[i]], n = rp[rows[i] + 1] - k0;
    if (n > kVsMaxLen) return false;
    len[i] = n;
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
    const int32_t p0 = n ? w.slot(col[k0]) : 0;
    first[i] = p0;
    for (int64_t k = 0; k < n; ++k) {
      uint64_t bits;
      std::memcpy(&bits, &val[k0 + k], 8);
      h = (h ^ bits) * 0xff51afd7ed558ccdull;
      h = (h ^ (uint64_t)(uint32_t)(w.slot(col[k0 + k]) - p0)) * 0xc4ceb9fe1a85ec53ull;
      h ^= h >> 29;
    }
    key[i] = h;
  }
  auto same = [&](int a, int b) {   // exact test behind the hash
    if (len[a] != len[b]) return false;
    const int64_t ka = rp[rows[a]], kb = rp[rows[b]];
    for (int64_t k = 0; k < len[a]; ++k) {
      if (std::memcmp(&val[ka + k], &val[kb + k], 8) != 0) return false;
      if (w.slot(col[ka + k]) - first[a] != w.slot(col[kb + k]) - first[b]) return false;
    }
    return true;
  };
  std::vector<int> ids, plain;
  for (int cls = 0; cls <= 6; ++cls) {
    ids.clear();
    plain.clear();
    for (int i = 0; i < nr; ++i)
      if ((int)((len[i] + 63) / 64) == cls) ids.push_back(i);
    if (cls == 0) {
      plain = ids;
    } else {
      std::stable_sort(ids.begin(), ids.end(), [&](int a, int b) { return key[a] < key[b]; });
      size_t g0 = 0;
      while (g0 < ids.size()) {
        size_t g1 = g0 + 1;
        while (share && g1 < ids.size() && key[ids[g1]] == key[ids[g0]] && same(ids[g0], ids[g1])) ++g1;
        size_t q = g0;
        while (g1 - q >= 2) {   // 2..16 rows per shared batch (never a lone leftover if it can be avoided)
          const size_t left = g1 - q;
          const size_t take = left == kVsBatchRows + 1 ? kVsBatchRows / 2 + 1 : std::min<size_t>(kVsBatchRows, left);
          VsBatch bt{cls, 0, {}, true, {}};
          for (size_t i = q; i < q + take; ++i) {
            bt.id[bt.nreal] = ids[i];
            bt.shift[bt.nreal] = first[ids[i]] - first[ids[q]];
            ++bt.nreal;
          }
          out.push_back(bt);
          q += take;
        }
        for (; q < g1; ++q) plain.push_back(ids[q]);
        g0 = g1;
      }
    }
    // plain batches: longest first, so that the rows of a batch have equal or close remainders in the last chunk
    std::stable_sort(plain.begin(), plain.end(), [&](int a, int b) { return len[a] != len[b] ? len[a] > len[b] : a < b; });
    for (size_t q = 0; q < plain.size(); q += 4) {
      VsBatch bt{cls, 0, {}, false, {}};
      for (size_t i = q; i < std::min(q + 4, plain.size()); ++i) bt.id[bt.nreal++] = plain[i];
      out.push_back(bt);
    }
  }
  return true;
}

// 16-byte units a batch occupies.  Plain: 12 bytes (4 row slots x 24 bits) per lane and chunk; shared: 4 bytes
// (one 24-bit field in a dword).  Of the last chunk only the lanes below the longest remainder (rounded up to 4).
static int64_t vs_batch_units(const VsBatch &q, const std::vector<int32_t> &rows, const int64_t *rp) {
  if (q.cls == 0) return 0;
  const int64_t full = 64 * (q.cls - 1);
  int64_t mr = 1;
  for (int i = 0; i < q.nreal; ++i) mr = std::max(mr, rp[rows[q.id[i]] + 1] - rp[rows[q.id[i]]] - full);
  const int64_t lanes = full + (mr + 3) / 4 * 4;
  return q.shared ? lanes / 4 : 3 * lanes / 4;
}

// Blocks whose entries take more than kVsMaxDict distinct values (9-bit codes), or that list more than
// kVsMaxRows rows, are halved until they fit; false if a single row does not fit.
static bool vs_refine_blocks(int64_t nrows, const int64_t *rp, const double *val, int RB, int64_t nb_in,
                             const int64_t *bptr, const int32_t *brows, std::vector<int64_t> &optr,
                             std::vector<int32_t> &orows, int max_rows = kVsMaxRows, int max_dict = kVsMaxDict) {
  const bool nat = bptr == nullptr;
  const int64_t nb = nat ? (nrows + RB - 1) / RB : nb_in;
  const int T = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::vector<int64_t>> t_sizes(T);
  std::atomic<bool> bad(false);
  orows.resize(nrows);
  if (nat) {
    for (int64_t r = 0; r < nrows; ++r) orows[r] = (int32_t)r;
  } else {
    std::copy(brows, brows + nrows, orows.begin());
  }
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t]() {
      constexpr int kTab = 4096;   // open addressing over the 64-bit patterns; stamps avoid clearing
      std::vector<uint64_t> keys(kTab);
      std::vector<uint32_t> stamp(kTab, 0);
      uint32_t gen = 0;
      std::vector<std::pair<int64_t, int64_t>> stack;
      for (int64_t b = nb * t / T; b < nb * (t + 1) / T && !bad; ++b) {
        const int64_t lo = nat ? b * RB : bptr[b], hi = nat ? std::min<int64_t>((b + 1) * RB, nrows) : bptr[b + 1];
        stack.clear();
        stack.emplace_back(lo, hi);
        while (!stack.empty() && !bad) {   // depth-first, left half first: pieces come out in row-list order
          const auto [a, e] = stack.back();
          stack.pop_back();
          bool fits = e - a <= max_rows;
          if (fits) {
            ++gen;
            int distinct = 0;
            for (int64_t i = a; i < e && fits; ++i) {
              const int32_t r = orows[i];
              for (int64_t k = rp[r]; k < rp[r + 1] && fits; ++k) {
                uint64_t bits;
                std::memcpy(&bits, &val[k], 8);
                uint32_t h = (uint32_t)((bits * 0x9E3779B97F4A7C15ull) >> 52);
                while (stamp[h] == gen && keys[h] != bits) h = (h + 1) & (kTab - 1);
                if (stamp[h] != gen) {
                  stamp[h] = gen;
                  keys[h] = bits;
                  fits = ++distinct <= max_dict;
                }
              }
            }
          }
          if (fits) {
            t_sizes[t].push_back(e - a);
          } else if (e - a <= 1) {
            bad = true;
          } else {
            const int64_t mid = a + (e - a) / 2;
            stack.emplace_back(mid, e);
            stack.emplace_back(a, mid);
          }
        }
      }
    });
  for (auto &x : th) x.join();
  if (bad) return false;
  optr.assign(1, 0);
  for (int t = 0; t < T; ++t)
    for (int64_t sz : t_sizes[t]) optr.push_back(optr.back() + sz);
  // blocks that had to be cut to a quarter of their size on average: the values do not repeat
  // enough for this format (a window per handful of rows costs more than the codes save)
  return (int64_t)optr.size() - 1 <= 4 * nb + 16;
}

static void plan_vs(int64_t nrows, const int64_t *rp, const int32_t *col, const double *val, int RB, int maxW,
                    int GAP, int64_t nb_in, const int64_t *bptr_in, const int32_t *brows_in, VsPlan &pl,
                    bool share = true, int wide = 0, int64_t n_local_cols = -1, bool side = false) {
  std::vector<int64_t> r_ptr, s_ptr;
  std::vector<int32_t> r_rows, s_rows;
  int64_t n_listed = nrows;   // rows the blocks list
  if (side && nrows > 0 && vs_take_side_rows(nrows, rp, col, val, RB, nb_in, bptr_in, brows_in, n_local_cols, pl, s_ptr, s_rows)) {
    // the blocks without the side rows, as a caller's blocks; where the variant is refused the plan is today's
    nb_in = (int64_t)s_ptr.size() - 1, bptr_in = s_ptr.data(), brows_in = s_rows.data();
    n_listed = (int64_t)s_rows.size();
    if (nb_in == 0) return;
  }
  const int max_dict = wide ? VsFmt<1>::kMaxDict : VsFmt<0>::kMaxDict, code_shift = wide ? VsFmt<1>::kCodeShift : VsFmt<0>::kCodeShift;
  maxW = std::min(maxW, wide ? VsFmt<1>::kMaxSlots : VsFmt<0>::kMaxSlots);
  pl.wide = wide;
  pl.nb_in = nb_in > 0 ? nb_in : (nrows + RB - 1) / RB;
  if (nrows == 0 || !vs_refine_blocks(n_listed, rp, val, RB, nb_in, bptr_in, brows_in, r_ptr, r_rows, kVsMaxRows, max_dict)) return;
  pl.dict_split = (int64_t)r_ptr.size() - 1 > pl.nb_in;
  if (n_local_cols >= 0) {
    // partitioned operator: the blocks that read no halo column (columns >= n_local_cols) first, so that they can run
    // while the halo is still on its way (spmv_m); the order of the blocks is free, every row names its own result
    const int64_t nb0 = (int64_t)r_ptr.size() - 1;
    std::vector<uint8_t> bnd(nb0, 0);
    for (int64_t b = 0; b < nb0; ++b)
      for (int64_t i = r_ptr[b]; i < r_ptr[b + 1] && !bnd[b]; ++i) {
        const int32_t r = r_rows[i];
        for (int64_t k = rp[r]; k < rp[r + 1] && !bnd[b]; ++k) bnd[b] = col[k] >= n_local_cols;   // halo columns sit anywhere in a row
      }
    std::vector<int64_t> np(1, 0);
    std::vector<int32_t> nr;
    nr.reserve(r_rows.size());
    for (int pass = 0; pass < 2; ++pass)
      for (int64_t b = 0; b < nb0; ++b)
        if (bnd[b] == pass) {
          nr.insert(nr.end(), r_rows.begin() + r_ptr[b], r_rows.begin() + r_ptr[b + 1]);
          np.push_back((int64_t)nr.size());
        }
    r_ptr.swap(np);
    r_rows.swap(nr);
  }
  const int T = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::vector<VsBatch>> batches;
  std::vector<int64_t> blk_units;
  std::atomic<bool> bad(false), too_wide(false);
  std::atomic<int64_t> n_shared_nnz(0);
  int64_t nb = 0;
  const int64_t *bptr = nullptr;
  const int32_t *brows = nullptr;
  for (int attempt = 0; attempt < 3; ++attempt) {
    if (attempt == 1) {
      // cheap first: how often do a few sample blocks have to be halved?  Split every block that often, untested (the
      // pass below tests all of them; what still does not fit goes through the exact refinement of attempt 2)
      if (!too_wide) return;
      int k = 0;
      std::vector<int32_t> rows;
      VsWindow w;
      for (int64_t b : {(int64_t)0, nb / 2, nb - 1}) {
        int64_t len = bptr[b + 1] - bptr[b];
        int kb = 0;
        for (; len > 1; ++kb, len = (len + 1) / 2) {
          rows.assign(brows + bptr[b], brows + bptr[b] + len);
          if (vs_window(rows, rp, col, GAP, std::min(maxW, kVsRefineW), w, nullptr, nullptr)) break;
        }
        k = std::max(k, kb);
      }
      if (k == 0) continue;   // the samples fit: straight to the exact refinement
      std::vector<int64_t> np(1, 0);
      for (int64_t b = 0; b < nb; ++b) {
        const int64_t a = bptr[b], len = bptr[b + 1] - a, pieces = std::min<int64_t>((int64_t)1 << k, std::max<int64_t>(len, 1));
        for (int64_t q = 1; q <= pieces; ++q)
          if (a + len * q / pieces > np.back()) np.push_back(a + len * q / pieces);
      }
      r_ptr.swap(np);
      bad = false;
      too_wide = false;
      n_shared_nnz = 0;
    }
    if (attempt == 2) {
      // A block's x window did not fit the LDS budget (operators whose rows reach far, e.g. the divergence block B of a
      // Taylor-Hood pair: 96 pressure rows touch 15 000 velocity columns): halve such blocks until their windows fit.
      // Only paid by operators that need it -- the first attempt is the plan of everything else.
      if (!too_wide) return;
      std::vector<std::vector<int64_t>> t_sizes(T);
      std::atomic<bool> hopeless(false);
      const int64_t nb0 = nb;
      std::vector<std::thread> th;
      for (int t = 0; t < T; ++t)
        th.emplace_back([&, t]() {
          std::vector<int32_t> rows;
          VsWindow w;
          std::vector<std::pair<int64_t, int64_t>> stack;
          for (int64_t b = nb0 * t / T; b < nb0 * (t + 1) / T && !hopeless; ++b) {
            stack.clear();
            stack.emplace_back(bptr[b], bptr[b + 1]);
            while (!stack.empty() && !hopeless) {   // depth-first, left half first: pieces come out in row-list order
              const auto [a, e] = stack.back();
              stack.pop_back();
              rows.assign(brows + a, brows + e);
              if (vs_window(rows, rp, col, GAP, std::min(maxW, kVsRefineW), w, nullptr, nullptr)) {
                t_sizes[t].push_back(e - a);
              } else if (e - a <= 1) {
                hopeless = true;
              } else {
                const int64_t mid = a + (e - a) / 2;
                stack.emplace_back(mid, e);
                stack.emplace_back(a, mid);
              }
            }
          }
        });
      for (auto &x : th) x.join();
      if (hopeless) return;
      std::vector<int64_t> np(1, 0);
      for (int t = 0; t < T; ++t)
        for (int64_t sz : t_sizes[t]) np.push_back(np.back() + sz);
      r_ptr.swap(np);
      bad = false;
      n_shared_nnz = 0;
    }
  bptr = r_ptr.data();
  brows = r_rows.data();
  nb = (int64_t)r_ptr.size() - 1;
  if (nb == 0 || nb > 2147483000LL) return;
  // pass 1: windows, batches (kept), stream extents
  batches.assign(nb, std::vector<VsBatch>());
  blk_units.assign(nb, 0);
  {
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
      th.emplace_back([&, t]() {
        std::vector<int32_t> rows;
        VsWindow w;
        int64_t sh = 0;
        for (int64_t b = nb * t / T; b < nb * (t + 1) / T && !bad; ++b) {
          rows.assign(brows + bptr[b], brows + bptr[b + 1]);
          if (rows.size() <= (size_t)kVsMaxRows && !vs_window(rows, rp, col, GAP, maxW, w, nullptr, nullptr)) {
            too_wide = true;
            bad = true;
            break;
          }
          if (rows.size() > (size_t)kVsMaxRows || !vs_batches(rows, rp, col, val, w, batches[b], share)) {
            bad = true;
            break;
          }
          int64_t e = 0;
          for (const VsBatch &q : batches[b]) {
            e += vs_batch_units(q, rows, rp);
            if (q.shared)
              for (int i = 0; i < q.nreal; ++i) sh += rp[rows[q.id[i]] + 1] - rp[rows[q.id[i]]];
          }
          blk_units[b] = e;
        }
        n_shared_nnz += sh;
      });
    for (auto &x : th) x.join();
  }
    if (!bad) break;
  }
  if (bad) return;
  pl.nb = nb;
  pl.nb_interior = 0;
  if (n_local_cols >= 0) {   // leading blocks without a halo column (splits for the window keep the order)
    bool interior = true;
    for (int64_t b = 0; b < nb && interior; ++b) {
      for (int64_t i = bptr[b]; i < bptr[b + 1] && interior; ++i) {
        const int32_t r = brows[i];
        for (int64_t k = rp[r]; k < rp[r + 1] && interior; ++k) interior = col[k] < n_local_cols;
      }
      if (interior) pl.nb_interior = b + 1;
    }
  }
  pl.shared_nnz = n_shared_nnz;
  pl.sb.assign(nb, 0);
  int64_t tot = 0;
  int maxb = 1, maxr = 1;
  for (int64_t b = 0; b < nb; ++b) {
    pl.sb[b] = tot;
    tot += 16 * blk_units[b];
    if (blk_units[b] > 0xfffffLL) return;
    maxb = std::max(maxb, (int)batches[b].size());
    maxr = std::max(maxr, (int)(bptr[b + 1] - bptr[b]));
    pl.nbatch += (int64_t)batches[b].size();
  }
  if (maxb > 0xffff) return;
  pl.stride = maxb;
  pl.rbs = maxr;
  pl.stream.assign((size_t)tot + 4096, 0);
  pl.tab.assign((size_t)nb * maxb * kVsBatchRows, 0);
  pl.cnt.assign(nb, 0);
  pl.blkW.assign(nb, 0);
  pl.dn.assign(nb, 0);
  std::vector<int32_t> blk_nseg(nb, 0);
  std::vector<std::vector<double>> t_dict(T);
  std::vector<std::vector<int32_t>> t_seg_col(T), t_seg_off(T), t_doff(T);
  {
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
      th.emplace_back([&, t]() {
        std::vector<int32_t> rows;
        VsWindow w;
        constexpr int kTab = 4096;
        std::vector<uint64_t> keys(kTab);
        std::vector<int16_t> ids(kTab);
        for (int64_t b = nb * t / T; b < nb * (t + 1) / T && !bad; ++b) {
          rows.assign(brows + bptr[b], brows + bptr[b + 1]);
          const std::vector<VsBatch> &bts = batches[b];
          pl.cnt[b] = (int32_t)bts.size();
          t_doff[t].push_back((int32_t)t_dict[t].size());
          vs_window(rows, rp, col, GAP, maxW, w, &t_seg_col[t], &t_seg_off[t]);
          pl.blkW[b] = w.W;
          blk_nseg[b] = w.nseg;
          // dictionary (<= kVsMaxDict bit patterns) and the batch-major stream
          std::fill(ids.begin(), ids.end(), (int16_t)-1);
          const size_t d0 = t_dict[t].size();
          uint8_t *sp = pl.stream.data() + pl.sb[b];
          uint32_t eoff = 0;  // 16-byte units from the block's first byte
          auto field_of = [&](int64_t k) -> int64_t {   // (code << 15) | (window slot << 3) of CSR entry k; -1: dictionary full
            uint64_t bits;
            std::memcpy(&bits, &val[k], 8);
            uint32_t h = (uint32_t)((bits * 0x9E3779B97F4A7C15ull) >> 52);
            for (;;) {
              if (ids[h] < 0) {
                if (t_dict[t].size() - d0 == (size_t)max_dict) return -1;
                keys[h] = bits;
                ids[h] = (int16_t)(t_dict[t].size() - d0);
                t_dict[t].push_back(val[k]);
                break;
              }
              if (keys[h] == bits) break;
              h = (h + 1) & (kTab - 1);
            }
            return ((int64_t)ids[h] << code_shift) | ((int64_t)w.slot(col[k]) << 3);
          };
          for (size_t q = 0; q < bts.size() && !bad; ++q) {
            const VsBatch &bt = bts[q];
            uint8_t *fb = sp + 16 * (size_t)eoff;
            uint64_t *dst = &pl.tab[((size_t)b * maxb + q) * kVsBatchRows];
            for (int i = 0; i < kVsBatchRows && !bad; ++i) {
              const int src = i < bt.nreal ? i : 0;     // fillers repeat the batch's first row
              const int32_t r = rows[bt.id[src]];
              const int64_t k0 = rp[r], n = rp[r + 1] - k0;
              if (bt.shared ? i == 0 : i < 4)
                for (int64_t k = 0; k < n; ++k) {   // entry k: chunk k / 64, lane k % 64 (row slot i of a plain batch)
                  const int64_t f = field_of(k0 + k);
                  if (f < 0) { bad = true; break; }
                  if (bt.shared) {
                    const uint32_t f32 = (uint32_t)f;
                    std::memcpy(fb + 256 * (size_t)(k / 64) + 4 * (size_t)(k % 64), &f32, 4);
                  } else {
                    uint8_t *cell = fb + 768 * (size_t)(k / 64) + 12 * (size_t)(k % 64) + 3 * i;
                    cell[0] = (uint8_t)f;
                    cell[1] = (uint8_t)(f >> 8);
                    cell[2] = (uint8_t)(f >> 16);
                  }
                }
              // low dword: offset | count | class; rows 1.. of a shared batch: their window shift in bytes (signed)
              const uint64_t low = (bt.shared && i > 0) ? (uint64_t)(uint32_t)(i < bt.nreal ? bt.shift[i] * 8 : 0)
                                                        : ((uint64_t)eoff | ((uint64_t)n << 20) | ((uint64_t)bt.cls << 29));
              dst[i] = low | ((uint64_t)(i < bt.nreal ? (uint32_t)r : 0xffffffffu) << 32);
            }
            if (bt.shared) dst[0] |= 1ull << 63;
            eoff += (uint32_t)vs_batch_units(bt, rows, rp);
          }
          pl.dn[b] = (int32_t)(t_dict[t].size() - d0);
        }
      });
    for (auto &x : th) x.join();
  }
  if (bad) return;
  pl.seg_begin.assign(nb + 1, 0);
  for (int64_t b = 0; b < nb; ++b) pl.seg_begin[b + 1] = pl.seg_begin[b] + blk_nseg[b];
  pl.doff.reserve(nb);
  for (int t = 0; t < T; ++t) {
    const int32_t base = (int32_t)pl.dict.size();
    for (int32_t o : t_doff[t]) pl.doff.push_back(base + o);
    pl.dict.insert(pl.dict.end(), t_dict[t].begin(), t_dict[t].end());
    pl.seg_col.insert(pl.seg_col.end(), t_seg_col[t].begin(), t_seg_col[t].end());
    pl.seg_off.insert(pl.seg_off.end(), t_seg_off[t].begin(), t_seg_off[t].end());
  }
  if (pl.dict.size() > 2000000000ull) return;
  int32_t mw = 1;
  for (int64_t b = 0; b < nb; ++b) mw = std::max(mw, pl.blkW[b]);
  pl.maxW = mw;
  pl.ok = true;
}

// ---- the same idea for SHORT rows (canonical L = 8, 16 or 32 lanes per row: Q1 stencils, the level operators of
// scalar problems).  A 64-lane wave holds G = 64 / L rows side by side, a batch is ONE stored template row (a dword
// per entry: 9-bit value code, 12-bit window column, ready-shifted) shared by up to 4 G translate rows -- on a
// uniform mesh every interior row of a run is a translate of its neighbour, so the matrix stream all but vanishes
// (27-point Laplace: 12 B/nnz CSR -> ~0.6 B/nnz incl. descriptors) and what is left is one LDS gather and one fma
// per entry.  Rows without a translate partner are batches of one.  Descriptor per batch (uint64 words):
//   [0] eb (20 bits, 16-byte units) | entry count (9) | class = ceil(count / L) (3) | rows in the batch (32)
//   [1 + i] global row (32, low) | window shift in bytes (32, high, signed)      i = 0 .. 4 G - 1
constexpr int kVssMaxClass = 4;   // rows of at most 4 L entries
constexpr int kVssMaxRows = 512;  // rows per block
struct VssBatch {
  int cls, nreal;
  std::vector<int> id;
  std::vector<int32_t> shift;
};

static void plan_vss(int64_t nrows, int L, const int64_t *rp, const int32_t *col, const double *val, int RB, int maxW,
                     int GAP, VsPlan &pl) {
  const int RBb = 4 * (64 / L);   // rows per batch
  std::vector<int64_t> r_ptr;
  std::vector<int32_t> r_rows;
  if (nrows == 0 || !vs_refine_blocks(nrows, rp, val, RB, 0, nullptr, nullptr, r_ptr, r_rows, kVssMaxRows)) return;
  {
    // blocks whose x window would not fit (operators whose rows reach far: the restriction from the Q2 grid, 384 coarse
    // rows touch 7 000 fine columns): how often do three sample blocks have to be halved?  Every block is split that often.
    int k = 0;
    std::vector<int32_t> rows;
    VsWindow w;
    const int64_t nb0 = (int64_t)r_ptr.size() - 1;
    for (int64_t b : {(int64_t)0, nb0 / 2, nb0 - 1}) {
      int64_t len = r_ptr[b + 1] - r_ptr[b];
      int kb = 0;
      for (; len > 1; ++kb, len = (len + 1) / 2) {
        rows.assign(r_rows.begin() + r_ptr[b], r_rows.begin() + r_ptr[b] + len);
        if (vs_window(rows, rp, col, GAP, maxW, w, nullptr, nullptr)) break;
      }
      k = std::max(k, kb);
    }
    if (k > 0) {
      std::vector<int64_t> np(1, 0);
      for (int64_t b = 0; b < nb0; ++b) {
        const int64_t a = r_ptr[b], len = r_ptr[b + 1] - a, pieces = std::min<int64_t>((int64_t)1 << k, std::max<int64_t>(len, 1));
        for (int64_t q = 1; q <= pieces; ++q)
          if (a + len * q / pieces > np.back()) np.push_back(a + len * q / pieces);
      }
      r_ptr.swap(np);
    }
  }
  const int64_t *bptr = r_ptr.data();
  const int32_t *brows = r_rows.data();
  const int64_t nb = (int64_t)r_ptr.size() - 1;
  if (nb == 0 || nb > 2147483000LL) return;
  const int T = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::vector<VssBatch>> batches(nb);
  std::vector<int64_t> blk_units(nb, 0);
  std::atomic<bool> bad(false);
  std::atomic<int64_t> n_shared_nnz(0);
  auto units_of = [&](const VssBatch &q) { return (int64_t)(q.cls * L + 3) / 4; };   // cls * L dwords, 16-byte units
  {
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
      th.emplace_back([&, t]() {
        std::vector<int32_t> rows, first;
        std::vector<int64_t> len;
        std::vector<uint64_t> key;
        std::vector<int> ids;
        VsWindow w;
        int64_t sh = 0;
        for (int64_t b = nb * t / T; b < nb * (t + 1) / T && !bad; ++b) {
          rows.assign(brows + bptr[b], brows + bptr[b + 1]);
          if (!vs_window(rows, rp, col, GAP, maxW, w, nullptr, nullptr)) { bad = true; break; }
          const int nr = (int)rows.size();
          len.assign(nr, 0);
          key.assign(nr, 0);
          first.assign(nr, 0);
          for (int i = 0; i < nr && !bad; ++i) {
            const int64_t k0 = rp[rows[i]], n = rp[rows[i] + 1] - k0;
            if (n > (int64_t)kVssMaxClass * L) { bad = true; break; }
            len[i] = n;
            uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
            const int32_t p0 = n ? w.slot(col[k0]) : 0;
            first[i] = p0;
            for (int64_t k = 0; k < n; ++k) {
              uint64_t bits;
              std::memcpy(&bits, &val[k0 + k], 8);
              h = (h ^ bits) * 0xff51afd7ed558ccdull;
              h = (h ^ (uint64_t)(uint32_t)(w.slot(col[k0 + k]) - p0)) * 0xc4ceb9fe1a85ec53ull;
              h ^= h >> 29;
            }
            key[i] = h;
          }
          if (bad) break;
          auto same = [&](int a, int c) {
            if (len[a] != len[c]) return false;
            const int64_t ka = rp[rows[a]], kc = rp[rows[c]];
            for (int64_t k = 0; k < len[a]; ++k) {
              if (std::memcmp(&val[ka + k], &val[kc + k], 8) != 0) return false;
              if (w.slot(col[ka + k]) - first[a] != w.slot(col[kc + k]) - first[c]) return false;
            }
            return true;
          };
          std::vector<VssBatch> &out = batches[b];
          for (int cls = 0; cls <= kVssMaxClass; ++cls) {
            ids.clear();
            for (int i = 0; i < nr; ++i)
              if ((int)((len[i] + L - 1) / L) == cls) ids.push_back(i);
            std::stable_sort(ids.begin(), ids.end(), [&](int a, int c) { return key[a] < key[c]; });
            size_t g0 = 0;
            while (g0 < ids.size()) {
              size_t g1 = g0 + 1;
              while (cls > 0 && g1 < ids.size() && key[ids[g1]] == key[ids[g0]] && same(ids[g0], ids[g1])) ++g1;
              if (cls == 0) g1 = ids.size();   // empty rows: any number per batch
              for (size_t q = g0; q < g1; q += RBb) {
                VssBatch bt{cls, 0, {}, {}};
                for (size_t i = q; i < std::min(q + (size_t)RBb, g1); ++i) {
                  bt.id.push_back(ids[i]);
                  bt.shift.push_back(first[ids[i]] - first[ids[q]]);
                  ++bt.nreal;
                }
                if (bt.nreal > 1) sh += (int64_t)bt.nreal * len[bt.id[0]];
                out.push_back(std::move(bt));
              }
              g0 = g1;
            }
          }
          int64_t e = 0;
          for (const VssBatch &q : out) e += units_of(q);
          blk_units[b] = e;
        }
        n_shared_nnz += sh;
      });
    for (auto &x : th) x.join();
  }
  if (bad) return;
  pl.nb = nb;
  pl.shared_nnz = n_shared_nnz;
  pl.sb.assign(nb, 0);
  int64_t tot = 0;
  int maxb = 1, maxr = 1;
  for (int64_t b = 0; b < nb; ++b) {
    pl.sb[b] = tot;
    tot += 16 * blk_units[b];
    if (blk_units[b] > 0xfffffLL) return;
    maxb = std::max(maxb, (int)batches[b].size());
    maxr = std::max(maxr, (int)(bptr[b + 1] - bptr[b]));
    pl.nbatch += (int64_t)batches[b].size();
  }
  if (maxb > 0xffff) return;
  const int W64 = 1 + RBb;   // descriptor words per batch
  pl.stride = maxb;
  pl.rbs = maxr;
  pl.stream.assign((size_t)tot + 4096, 0);
  pl.tab.assign((size_t)nb * maxb * W64, 0);
  pl.cnt.assign(nb, 0);
  pl.blkW.assign(nb, 0);
  pl.dn.assign(nb, 0);
  std::vector<int32_t> blk_nseg(nb, 0);
  std::vector<std::vector<double>> t_dict(T);
  std::vector<std::vector<int32_t>> t_seg_col(T), t_seg_off(T), t_doff(T);
  {
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
      th.emplace_back([&, t]() {
        std::vector<int32_t> rows;
        VsWindow w;
        constexpr int kTab = 1024;
        std::vector<uint64_t> keys(kTab);
        std::vector<int16_t> ids(kTab);
        for (int64_t b = nb * t / T; b < nb * (t + 1) / T && !bad; ++b) {
          rows.assign(brows + bptr[b], brows + bptr[b + 1]);
          const std::vector<VssBatch> &bts = batches[b];
          pl.cnt[b] = (int32_t)bts.size();
          t_doff[t].push_back((int32_t)t_dict[t].size());
          vs_window(rows, rp, col, GAP, maxW, w, &t_seg_col[t], &t_seg_off[t]);
          pl.blkW[b] = w.W;
          blk_nseg[b] = w.nseg;
          std::fill(ids.begin(), ids.end(), (int16_t)-1);
          const size_t d0 = t_dict[t].size();
          uint8_t *sp = pl.stream.data() + pl.sb[b];
          uint32_t eoff = 0;
          for (size_t q = 0; q < bts.size() && !bad; ++q) {
            const VssBatch &bt = bts[q];
            uint64_t *dst = &pl.tab[((size_t)b * maxb + q) * W64];
            const int32_t r0 = rows[bt.id[0]];
            const int64_t k0 = rp[r0], n = rp[r0 + 1] - k0;
            for (int64_t k = 0; k < n; ++k) {
              uint64_t bits;
              std::memcpy(&bits, &val[k0 + k], 8);
              uint32_t h = (uint32_t)((bits * 0x9E3779B97F4A7C15ull) >> 54);
              for (;;) {
                if (ids[h] < 0) {
                  if (t_dict[t].size() - d0 == (size_t)kVsMaxDict) { bad = true; break; }
                  keys[h] = bits;
                  ids[h] = (int16_t)(t_dict[t].size() - d0);
                  t_dict[t].push_back(val[k0 + k]);
                  break;
                }
                if (keys[h] == bits) break;
                h = (h + 1) & (kTab - 1);
              }
              if (bad) break;
              const uint32_t f = ((uint32_t)ids[h] << 15) | ((uint32_t)w.slot(col[k0 + k]) << 3);
              std::memcpy(sp + 16 * (size_t)eoff + 4 * (size_t)k, &f, 4);
            }
            dst[0] = (uint64_t)eoff | ((uint64_t)n << 20) | ((uint64_t)bt.cls << 29) | ((uint64_t)bt.nreal << 32);
            for (int i = 0; i < RBb; ++i) {
              const uint32_t row = i < bt.nreal ? (uint32_t)rows[bt.id[i]] : 0xffffffffu;
              const int32_t shb = i < bt.nreal ? bt.shift[i] * 8 : 0;
              dst[1 + i] = (uint64_t)row | ((uint64_t)(uint32_t)shb << 32);
            }
            eoff += (uint32_t)units_of(bt);
          }
          pl.dn[b] = (int32_t)(t_dict[t].size() - d0);
        }
      });
    for (auto &x : th) x.join();
  }
  if (bad) return;
  pl.seg_begin.assign(nb + 1, 0);
  for (int64_t b = 0; b < nb; ++b) pl.seg_begin[b + 1] = pl.seg_begin[b] + blk_nseg[b];
  pl.doff.reserve(nb);
  for (int t = 0; t < T; ++t) {
    const int32_t base = (int32_t)pl.dict.size();
    for (int32_t o : t_doff[t]) pl.doff.push_back(base + o);
    pl.dict.insert(pl.dict.end(), t_dict[t].begin(), t_dict[t].end());
    pl.seg_col.insert(pl.seg_col.end(), t_seg_col[t].begin(), t_seg_col[t].end());
    pl.seg_off.insert(pl.seg_off.end(), t_seg_off[t].begin(), t_seg_off[t].end());
  }
  if (pl.dict.size() > 2000000000ull) return;
  int32_t mw = 1;
  for (int64_t b = 0; b < nb; ++b) mw = std::max(mw, pl.blkW[b]);
  pl.maxW = mw;
  pl.ok = true;
}

// ---- row blocks of SMALL long-row operators ("batch_major_small").  A launch of spmv_vs_kernel is one
// workgroup of NW waves per row block, and a wave walks its share of the block's batches one after another.  An operator
// of a few ten thousand rows planned with the context-wide block (96 rows) gives a few hundred workgroups: most of the
// chip's wave slots stay empty while every wave that does run works through a queue of batches.  The rule below shrinks
// the block of such an operator until blocks x waves reaches HALF the resident wave slots of the device (4 of the 8
// waves a SIMD holds) or every wave is down to one batch, whichever comes first.  Half, not all: every block pays its
// frame (dictionary and x window into LDS) again, and in the sweep of profiles/small_operator_shapes the two patch
// operators of the N = 74 system gain down to 56 % of the slots and lose beyond, while A_2, at 71 % with the default
// block, loses at every smaller one.  The waves per workgroup stay: 4 beat 2 and 1 at every block size there.  It is a
// function of the operator (rows, and blocks / batches of its default plan) and of the device (compute units) alone:
// two setups of one problem plan the same blocks.  Results do not depend on the blocks (every row keeps its canonical sum).
constexpr int kVsFillWavesPerCu = 16;   // 4 SIMDs x 4 of the 8 resident waves (amdgpu_waves_per_eu(8, 8))
constexpr int kVsSmallMinRows = 16;     // never below one full shared batch
static void vs_small_shape(int64_t nrows, int64_t blocks, int64_t batches, int rows, int waves, int cus, int *rows_out,
                           int *waves_out) {
  *rows_out = rows;
  *waves_out = waves;
  const int64_t slots = (int64_t)std::max(cus, 1) * kVsFillWavesPerCu;
  if (nrows <= 0 || blocks <= 0 || batches <= 0 || blocks * waves >= slots) return;   // the default plan fills the chip
  // whole 16-row shared batches: the floor -- one batch per wave, a block of `waves` batches holds waves * nrows /
  // batches rows on average -- rounded up, the block that gives blocks x waves = slots rounded down (so that it does)
  const int64_t floor_rows = ((nrows * waves + batches - 1) / batches + 15) / 16 * 16;
  const int64_t fill_rows = (nrows * waves + slots - 1) / slots / 16 * 16;
  const int64_t r = std::max<int64_t>(std::max(floor_rows, fill_rows), kVsSmallMinRows);
  if (r < rows) *rows_out = (int)r;
}

static int build_vs(alfd_ctx *ctx, DevCsr &m, int slot, const int64_t *rp, const int32_t *col, const double *val) {
  VsPlan pl;
  int RB = ctx->vs_RB, NW = ctx->vs_NW;
  const bool forced = slot == kScratchSlot && ctx->vs_force_RB > 0;
  if (forced) RB = ctx->vs_force_RB, NW = ctx->vs_force_NW;
  const bool side = ctx->vs_side != 0;
  const int64_t nlc = (ctx->nranks > 1 && !m.rep) ? (int64_t)m.n_local_cols : -1;   // columns >= nlc are halo columns
  bool hint = slot >= 0 && slot < ALFD_NSLOTS && !ctx->rb_ptr[slot].empty();
  if (hint && ctx->rb_ptr[slot].back() != m.nrows) {
    // the hint was given for a matrix of another size (a re-upload of the slot): it no longer applies
    if (ctx->cfg.log_level > 0)
      std::fprintf(stderr, "[alfd] row-block hint of slot %d dropped: it lists %lld rows, the matrix has %lld\n", slot,
                   (long long)ctx->rb_ptr[slot].back(), (long long)m.nrows);
    ctx->rb_ptr[slot].clear();
    ctx->rb_rows[slot].clear();
    hint = false;
  }
  if (hint) {
    // the hint must list every row exactly once
    const auto &bp = ctx->rb_ptr[slot];
    const auto &br = ctx->rb_rows[slot];
    bool good = bp.front() == 0 && bp.back() == m.nrows && (int64_t)br.size() == m.nrows;
    std::vector<uint8_t> seen(good ? m.nrows : 0, 0);
    for (size_t i = 0; good && i < br.size(); ++i) {
      good = br[i] >= 0 && br[i] < m.nrows && !seen[br[i]];
      if (good) seen[br[i]] = 1;
    }
    for (size_t i = 0; good && i + 1 < bp.size(); ++i) good = bp[i] <= bp[i + 1];
    if (!good) return ctx->err = "alfd_set_row_blocks: the blocks are not a partition of the matrix rows", ALFD_E_INVALID;
    plan_vs(m.nrows, rp, col, val, RB, ctx->win_maxW, ctx->win_gap, (int64_t)bp.size() - 1, bp.data(),
            br.data(), pl, ctx->vs_share != 0, 0, nlc, side);
  } else {
    plan_vs(m.nrows, rp, col, val, RB, ctx->win_maxW, ctx->win_gap, 0, nullptr, nullptr, pl, ctx->vs_share != 0, 0, nlc, side);
  }
  if (ctx->vs_wide && (!pl.ok || pl.dict_split)) {
    // blocks with more than 512 distinct values had to be halved (or the plan failed): the same blocks with 10-bit
    // codes and 11-bit window columns, kept if the stream gets smaller
    VsPlan pw;
    if (hint)
      plan_vs(m.nrows, rp, col, val, RB, ctx->win_maxW, ctx->win_gap, (int64_t)ctx->rb_ptr[slot].size() - 1,
              ctx->rb_ptr[slot].data(), ctx->rb_rows[slot].data(), pw, ctx->vs_share != 0, 1, nlc, side);
    else
      plan_vs(m.nrows, rp, col, val, RB, ctx->win_maxW, ctx->win_gap, 0, nullptr, nullptr, pw, ctx->vs_share != 0, 1, nlc, side);
    if (pw.ok && (!pl.ok || pw.stream.size() + 128 * (size_t)pw.nbatch < pl.stream.size() + 128 * (size_t)pl.nbatch)) pl = std::move(pw);
  }
  if (!pl.ok) return ALFD_OK;
  bool small = false;
  if (ctx->vs_small && !forced && !hint && slot == kScratchSlot && !pl.wide) {
    // the library's own operators (multigrid levels, the interface patch; replicated ones on partitioned contexts
    // included): re-planned ONCE at the shape of vs_small_shape when the default plan leaves the chip under-filled.
    // Narrow codes only: the wide instantiations exist for 4 waves, and no level or patch operator needs them.
    int rs = RB, ws = NW;
    vs_small_shape(m.nrows, pl.nb, pl.nbatch, RB, NW, ctx->vs_cus, &rs, &ws);
    if (rs != RB || ws != NW) {
      VsPlan ps;
      plan_vs(m.nrows, rp, col, val, rs, ctx->win_maxW, ctx->win_gap, 0, nullptr, nullptr, ps, ctx->vs_share != 0, 0, nlc, side);
      if (ps.ok && !ps.dict_split) {
        pl = std::move(ps);
        RB = rs, NW = ws, small = true;
      }
    }
  }
  DevCsr::Vs &v = m.vs;
  v.RB = RB;
  v.NW = pl.wide ? 4 : NW;
  v.small = small;
  // block headers and the fixed-stride segment table (the kernel reads one segment past a block's last, and its first
  // round of 8 x 4 segments unconditionally; the descriptor table is read up to 16 batches past a block's last)
  int32_t max_nseg = 0, tail_lds = 0, tail_W = 0, tail_cnt = 0, tail_nd = 0;
  for (int64_t b = 0; b < pl.nb; ++b) max_nseg = std::max(max_nseg, pl.seg_begin[b + 1] - pl.seg_begin[b]);
  const int32_t S = std::max(max_nseg + 1, 33);
  if ((double)pl.nb * S * 8.0 > 2.0e9) return ALFD_OK;   // a block with thousands of window pieces: not this format
  std::vector<int32_t> hdrb((size_t)pl.nb * 8, 0), segx((size_t)pl.nb * S * 2 + 16, 0);   // + the reads past the last block
  for (int64_t b = 0; b < pl.nb; ++b) {
    const int32_t s0 = pl.seg_begin[b], ns = pl.seg_begin[b + 1] - s0;
    int32_t *h = &hdrb[(size_t)b * 8];
    h[0] = pl.cnt[b];
    h[1] = pl.blkW[b];
    h[2] = ns;
    h[3] = pl.dn[b];
    h[4] = pl.doff[b];
    h[5] = (int32_t)(uint32_t)((uint64_t)pl.sb[b] & 0xffffffffull);
    h[6] = (int32_t)((uint64_t)pl.sb[b] >> 32);
    const int32_t need = vs_tail_lds_need(pl.wide ? VsFmt<1>::kWinOff : VsFmt<0>::kWinOff, pl.dn[b], pl.blkW[b], pl.cnt[b]);
    if (need > tail_lds) tail_lds = need, tail_W = pl.blkW[b], tail_cnt = pl.cnt[b], tail_nd = pl.dn[b];
    for (int32_t q = 0; q < ns; ++q) {
      segx[((size_t)b * S + q) * 2] = pl.seg_col[s0 + q];
      segx[((size_t)b * S + q) * 2 + 1] = pl.seg_off[s0 + q];
    }
  }
  pl.tab.resize(pl.tab.size() + (size_t)16 * kVsBatchRows, 0);
  RC(upload_vec(ctx, m, &v.stream, pl.stream));
  RC(upload_vec(ctx, m, &v.tab, pl.tab));
  RC(upload_vec(ctx, m, &v.hdrb, hdrb));
  RC(upload_vec(ctx, m, &v.segx, segx));
  RC(upload_vec(ctx, m, &v.dict, pl.dict));
  if (!pl.side_rows.empty()) {
    RC(upload_vec(ctx, m, &v.side_rows, pl.side_rows));
    RC(upload_vec(ctx, m, &v.side_rp, pl.side_rp));
    RC(upload_vec(ctx, m, &v.side_col, pl.side_col));
    RC(upload_vec(ctx, m, &v.side_val, pl.side_val));
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  v.side_n = (int64_t)pl.side_rows.size();
  v.side_nnz = (int64_t)pl.side_col.size();
  v.side_longest = 0;
  for (int64_t i = 0; i < v.side_n; ++i) v.side_longest = std::max(v.side_longest, pl.side_rp[i + 1] - pl.side_rp[i]);   // the boundary group has its own longest
  v.side_interior = pl.side_interior;
  v.seg_stride = S;
  v.nb_interior = pl.nb_interior;
  v.nb = pl.nb;
  v.nseg = (int64_t)pl.seg_col.size();
  v.stream_bytes = (int64_t)pl.stream.size() - 4096;
  v.nbatch = pl.nbatch;
  v.shared_nnz = pl.shared_nnz;
  v.dict_total = (int64_t)pl.dict.size();
  v.stride = pl.stride;
  v.maxW = pl.maxW;
  v.tail_lds = tail_lds;
  v.wide = pl.wide;
  v.bricks = hint;
  v.on = true;
  if (ctx->cfg.log_level > 0 || std::getenv("ALFD_LOG_UPLOAD"))
    std::fprintf(stderr, "[alfd] batch-major format, %lld rows: with the row buffer of the block-end epilogue the largest block asks for "
                 "%d bytes of LDS (dictionary region %d with %d values, %d window slots, %d batches)\n", (long long)m.nrows,
                 (pl.wide ? VsFmt<1>::kWinOff : VsFmt<0>::kWinOff) + tail_lds, pl.wide ? VsFmt<1>::kWinOff : VsFmt<0>::kWinOff,
                 tail_nd, tail_W, tail_cnt);
  if (ctx->cfg.log_level > 0)
    std::fprintf(stderr,
                 "[alfd] batch-major format%s: %lld blocks (%s), %lld batches, window <= %d slots, %.2f B/nnz, %.1f %% of the "
                 "entries in template-shared batches\n", pl.wide ? " (10-bit codes)" : "",
                 (long long)pl.nb, hint ? "caller's row blocks" : "runs of the numbering", (long long)pl.nbatch, pl.maxW,
                 (double)v.stream_bytes / (double)std::max<int64_t>(m.nnz, 1),
                 100.0 * (double)pl.shared_nnz / (double)std::max<int64_t>(m.nnz, 1));
  return ALFD_OK;
}

static int build_vss(alfd_ctx *ctx, DevCsr &m, const int64_t *rp, const int32_t *col, const double *val) {
  VsPlan pl;
  const int RB = std::min(kVssMaxRows, std::max(64, ctx->win_RB * std::max(1, ctx->win_short_scale) * 64 / m.L));
  plan_vss(m.nrows, m.L, rp, col, val, RB, ctx->win_maxW, ctx->win_gap, pl);
  // worthwhile only if rows do share templates (otherwise a dword per entry + descriptors buys nothing over the
  // 10 B/nnz window format... it still halves the stream, but the L-lane window kernel is the tested default)
  if (!pl.ok || pl.shared_nnz * 2 < m.nnz) return ALFD_OK;
  DevCsr::Vs &v = m.vs;
  RC(upload_vec(ctx, m, &v.stream, pl.stream));
  RC(upload_vec(ctx, m, &v.sb, pl.sb));
  RC(upload_vec(ctx, m, &v.tab, pl.tab));
  RC(upload_vec(ctx, m, &v.cnt, pl.cnt));
  RC(upload_vec(ctx, m, &v.seg_begin, pl.seg_begin));
  RC(upload_vec(ctx, m, &v.blkW, pl.blkW));
  RC(upload_vec(ctx, m, &v.seg_col, pl.seg_col));
  RC(upload_vec(ctx, m, &v.seg_off, pl.seg_off));
  RC(upload_vec(ctx, m, &v.doff, pl.doff));
  RC(upload_vec(ctx, m, &v.dn, pl.dn));
  RC(upload_vec(ctx, m, &v.dict, pl.dict));
  HIPC(hipStreamSynchronize(ctx->stream));
  v.nb = pl.nb;
  v.nseg = (int64_t)pl.seg_col.size();
  v.stream_bytes = (int64_t)pl.stream.size() - 4096;
  v.nbatch = pl.nbatch;
  v.shared_nnz = pl.shared_nnz;
  v.dict_total = (int64_t)pl.dict.size();
  v.stride = pl.stride;
  v.maxW = pl.maxW;
  v.L = m.L;
  v.tab_u64 = 1 + 4 * (64 / m.L);
  v.bricks = false;
  v.on = true;
  if (ctx->cfg.log_level > 0)
    std::fprintf(stderr, "[alfd] batch-major format (L = %d): %lld blocks, %lld batches, window <= %d slots, %.2f B/nnz, "
                 "%.1f %% of the entries in shared batches\n", m.L, (long long)pl.nb, (long long)pl.nbatch, pl.maxW,
                 (double)(v.stream_bytes + 8.0 * v.tab_u64 * v.nbatch) / (double)std::max<int64_t>(m.nnz, 1),
                 100.0 * (double)pl.shared_nnz / (double)std::max<int64_t>(m.nnz, 1));
  return ALFD_OK;
}

static int upload_matrix(alfd_ctx *ctx, int slot, int64_t nrows, int64_t ncols, const int64_t *rp,
                         const int32_t *col, const double *val) {
  DevCsr &m = ctx->mat[slot];
  csr_free(m);  // a re-upload releases the previous arrays of this slot
  const auto t_up0 = std::chrono::steady_clock::now();
  m.nrows = nrows;
  m.ncols = ncols;
  m.nnz = rp[nrows];
  int64_t nonempty = 0;
  m.longest = 0;
  for (int64_t r = 0; r < nrows; ++r) {
    nonempty += rp[r + 1] > rp[r];
    m.longest = std::max(m.longest, rp[r + 1] - rp[r]);
  }
  m.sparse = nonempty * 2 < nrows;
  if (ctx->nranks > 1) {
    // lanes-per-row follows the GLOBAL matrix (so every rank, and the oracle, use one L)
    int64_t mine[2] = {m.nnz, nonempty};
    std::vector<int64_t> all(2 * (size_t)ctx->nranks);
    int64_t *d_m = nullptr, *d_a = nullptr;
    HIPC(hipMalloc((void **)&d_m, 2 * sizeof(int64_t)));
    HIPC(hipMalloc((void **)&d_a, 2 * sizeof(int64_t) * ctx->nranks));
    HIPC(hipMemcpyAsync(d_m, mine, sizeof(mine), hipMemcpyHostToDevice, ctx->stream));
    RC(comm_allgather(ctx, d_m, d_a, sizeof(mine)));
    HIPC(hipMemcpyAsync(all.data(), d_a, all.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    hipFree(d_m);
    hipFree(d_a);
    int64_t gn = 0, ge = 0;
    for (int p = 0; p < ctx->nranks; ++p) gn += all[2 * p], ge += all[2 * p + 1];
    DevCsr tmp;
    tmp.nnz = gn;
    choose_lanes(tmp, ge);
    m.L = tmp.L;
  } else {
    choose_lanes(m, nonempty);
  }
  const int32_t *col_up = col;
  std::vector<int32_t> remap;
  m.n_local_cols = (int32_t)ncols;
  if (ctx->nranks > 1 && ctx->up_local_only) {
    // rank-local operator (multigrid transfers): no halo, but the plan arrays must exist
    m.send_off.assign(ctx->nranks + 1, 0);
    m.recv_off.assign(ctx->nranks + 1, 0);
  } else if (ctx->nranks > 1) {
    if (ctx->part.empty()) return ctx->err = "alfd_set_partition must precede alfd_set_matrix", ALFD_E_INVALID;
    int rb, cb;
    slot_blocks(ctx, slot, &rb, &cb);
    const int64_t *po = ctx->up_col_offsets ? ctx->up_col_offsets : ctx->part[cb].data();
    const int64_t c0 = po[ctx->rank], c1 = po[ctx->rank + 1];
    m.n_local_cols = (int32_t)(c1 - c0);
    std::vector<int32_t> hal;
    remap.resize(m.nnz);
    m.recv_off.assign(ctx->nranks + 1, 0);
    host_halo_plan(m.nnz, col, po, ctx->nranks, ctx->rank, remap.data(), hal, m.recv_off.data());
    m.n_halo = (int64_t)hal.size();
    m.halo_globals = hal;
    col_up = remap.data();
    // counts all-to-all through an all-gather of the nranks x nranks matrix
    std::vector<int32_t> cnt_local(ctx->nranks), cnt_all((size_t)ctx->nranks * ctx->nranks);
    for (int p = 0; p < ctx->nranks; ++p) cnt_local[p] = (int32_t)(m.recv_off[p + 1] - m.recv_off[p]);
    int32_t *d_cl = nullptr, *d_ca = nullptr;
    HIPC(hipMalloc((void **)&d_cl, sizeof(int32_t) * ctx->nranks));
    HIPC(hipMalloc((void **)&d_ca, sizeof(int32_t) * ctx->nranks * ctx->nranks));
    HIPC(hipMemcpyAsync(d_cl, cnt_local.data(), ctx->nranks * 4, hipMemcpyHostToDevice, ctx->stream));
    RC(comm_allgather(ctx, d_cl, d_ca, (size_t)ctx->nranks * 4));
    HIPC(hipMemcpyAsync(cnt_all.data(), d_ca, cnt_all.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    m.send_off.assign(ctx->nranks + 1, 0);
    for (int p = 0; p < ctx->nranks; ++p)
      m.send_off[p + 1] = m.send_off[p] + cnt_all[(size_t)p * ctx->nranks + ctx->rank];
    const int64_t nsend = m.send_off.back();
    // exchange requested ids: I send my halo id list slices, receive what peers want from me
    int32_t *d_req = nullptr, *d_want = nullptr;
    HIPC(hipMalloc((void **)&d_req, sizeof(int32_t) * std::max<int64_t>(m.n_halo, 1)));
    HIPC(hipMalloc((void **)&d_want, sizeof(int32_t) * std::max<int64_t>(nsend, 1)));
    HIPC(hipMemcpyAsync(d_req, hal.data(), m.n_halo * 4, hipMemcpyHostToDevice, ctx->stream));
    // I send my wanted-id list slices (grouped by owner), I receive what peers want from me
    RC(comm_alltoallv(ctx, d_req, m.recv_off.data(), d_want, m.send_off.data(), sizeof(int32_t)));
    std::vector<int32_t> want(nsend);
    HIPC(hipMemcpyAsync(want.data(), d_want, nsend * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    hipFree(d_cl);
    hipFree(d_ca);
    hipFree(d_req);
    hipFree(d_want);
    // the column space of this matrix is block cb; my owned range there starts at c0
    for (auto &g : want) g = (int32_t)(g - c0);
    RC(csr_alloc(ctx, m, &m.send_idx, nsend));
    HIPC(hipMemcpyAsync(m.send_idx, want.data(), nsend * 4, hipMemcpyHostToDevice, ctx->stream));
    RC(csr_alloc(ctx, m, &m.send_buf, nsend));
    RC(csr_alloc(ctx, m, &m.halo, m.n_halo));
    HIPC(hipStreamSynchronize(ctx->stream));
  }
  RC(csr_alloc(ctx, m, &m.col, m.nnz));
  RC(csr_alloc(ctx, m, &m.val, m.nnz));
  // The CSR copy of a large operator (21 GB at N = 74, 0.9 s of PCIe time from pageable memory) runs on a helper thread
  // while this one plans the storage formats from the host arrays; joined before the call returns (the guard also joins
  // on the error paths).
  struct CopyJob {
    std::thread th;
    hipError_t rc = hipSuccess;
    ~CopyJob() { if (th.joinable()) th.join(); }
  } copy_job;
  if (m.nnz > 50000000) {
    const int dev = ctx->device;
    int32_t *dcol = m.col;
    double *dval = m.val;
    const int64_t nn = m.nnz;
    copy_job.th = std::thread([&copy_job, dev, dcol, dval, col_up, val, nn] {
      hipStream_t st = nullptr;   // a stream of its own: nothing here orders against the plan uploads on the context's
      hipError_t e = hipSetDevice(dev);
      if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
      if (e == hipSuccess) e = hipMemcpyAsync(dcol, col_up, nn * sizeof(int32_t), hipMemcpyHostToDevice, st);
      if (e == hipSuccess) e = hipMemcpyAsync(dval, val, nn * sizeof(double), hipMemcpyHostToDevice, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (st) hipStreamDestroy(st);
      copy_job.rc = e;
    });
  } else {
    HIPC(hipMemcpyAsync(m.col, col_up, m.nnz * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipMemcpyAsync(m.val, val, m.nnz * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  }
  if (m.sparse) {
    std::vector<int32_t> rows;
    std::vector<int64_t> crp(1, 0);
    for (int64_t r = 0; r < nrows; ++r)
      if (rp[r + 1] > rp[r]) {
        rows.push_back((int32_t)r);
        crp.push_back(rp[r + 1]);
      }
    // compact row pointer: entries of non-empty rows are contiguous in CSR order
    for (size_t i = 0; i < rows.size(); ++i) crp[i] = rp[rows[i]];
    crp[rows.size()] = m.nnz;
    m.n_list = (int64_t)rows.size();
    RC(csr_alloc(ctx, m, &m.rows, m.n_list));
    RC(csr_alloc(ctx, m, &m.rp, m.n_list + 1));
    HIPC(hipMemcpyAsync(m.rows, rows.data(), m.n_list * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipMemcpyAsync(m.rp, crp.data(), (m.n_list + 1) * sizeof(int64_t), hipMemcpyHostToDevice,
                        ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
  } else {
    m.n_list = nrows;
    RC(csr_alloc(ctx, m, &m.rp, nrows + 1));
    HIPC(hipMemcpyAsync(m.rp, rp, (nrows + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  // the windowed kernel launches one workgroup per row block: only for matrices with
  // enough row blocks to fill the chip (256 CUs x several workgroups)
  const bool win_long = m.L == 64 && m.nrows >= (int64_t)ctx->win_RB * ctx->win_min_blocks;
  const bool win_short = ctx->win_short_scale > 0 && m.L >= 8 && m.L < 64 &&
                         m.nrows >= (int64_t)std::min(512, ctx->win_RB * ctx->win_short_scale * 64 / m.L) * ctx->win_short_min_blocks;
  const bool windows = ctx->win_enable && (win_long || win_short) && !m.sparse && m.nnz > 0;
  const auto t_plan0 = std::chrono::steady_clock::now();
  // long rows: the batch-major form first -- it has dictionaries of its own (per row block, up to 1024 values with wide
  // codes) and is tried even when 96-row window blocks cannot be coded (cell-wise assembled operators)
  if (windows && ctx->vs_enable && ctx->win_vi && m.L == 64 && (slot != kScratchSlot || ctx->vi_levels))
    RC(build_vs(ctx, m, slot, rp, col_up, val));
  const auto t_plan1 = std::chrono::steady_clock::now();
  // a matrix the batch-major form holds needs the window plan (16-bit columns of the general 10 B/nnz kernel) only
  // when that kernel is asked for (tunables "value_index" / "batch_major" = 0, alfd_bench_spmv_format(..., 0)):
  // planned then, from the device copy (ensure_window_plan) -- 1.5 s of the upload at N = 74 otherwise
  m.win_deferred = windows && m.vs.on && m.L == 64;
  m.win_user = slot != kScratchSlot;
  if (windows && !m.win_deferred) RC(build_window(ctx, m, rp, col_up, val, slot != kScratchSlot, m.vs.on));
  if ((ctx->cfg.log_level > 0 || std::getenv("ALFD_LOG_UPLOAD")) && m.nnz > 50000000)
    std::fprintf(stderr, "[alfd] upload of a %lld-nnz matrix: CSR copy %.2f s, batch-major plan + copy %.2f s, window plan + copy %.2f s\n",
                 (long long)m.nnz, std::chrono::duration<double>(t_plan0 - t_up0).count(),
                 std::chrono::duration<double>(t_plan1 - t_plan0).count(),
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - t_plan1).count());
  // (also when the 10 B/nnz window plan did not fit its row blocks: plan_vss halves blocks whose x window is too wide --
  // transfer operators, whose rows reach across two grids)
  if (ctx->vs_enable && windows && !m.sparse && (m.L == 32 || m.L == 16 || m.L == 8)) RC(build_vss(ctx, m, rp, col_up, val));
  if (copy_job.th.joinable()) {
    copy_job.th.join();
    if (copy_job.rc != hipSuccess) return ctx->err = hipGetErrorString(copy_job.rc), ALFD_E_HIP;
  }
  m.present = true;
  RC(pick_short_row_format(ctx, m));
  return ALFD_OK;
}

static int upload_transpose(alfd_ctx *ctx, int slot, int64_t nrows, int64_t ncols, const int64_t *rp,
                            const int32_t *col, const double *val) {
  const int64_t nnz = rp[nrows];
  std::vector<int64_t> trp(ncols + 1, 0);
  std::vector<int32_t> tcol(nnz);
  std::vector<double> tval(nnz);
  for (int64_t k = 0; k < nnz; ++k) trp[col[k] + 1]++;
  for (int64_t r = 0; r < ncols; ++r) trp[r + 1] += trp[r];
  std::vector<int64_t> cur(trp.begin(), trp.end() - 1);
  for (int64_t r = 0; r < nrows; ++r)
    for (int64_t k = rp[r]; k < rp[r + 1]; ++k) {
      const int64_t p = cur[col[k]]++;
      tcol[p] = (int32_t)r;
      tval[p] = val[k];
    }
  return upload_matrix(ctx, slot, ncols, nrows, trp.data(), tcol.data(), tval.data());
}

static int nblocks_of(int variant) { return variant == ALFD_AL2 || variant == ALFD_RATIONAL ? 2 : 3; }

static int ws_alloc_zero(alfd_ctx *ctx, double **p, int64_t count, std::vector<void *> *list = nullptr) {
  void *q = nullptr;
  HIPC(hipMalloc(&q, std::max<int64_t>(count, 1) * sizeof(double)));
  (list ? *list : ctx->ws_allocs).push_back(q);
  *p = static_cast<double *>(q);
  HIPC(hipMemsetAsync(q, 0, std::max<int64_t>(count, 1) * sizeof(double), ctx->stream));
  return ALFD_OK;
}
// workspace whose size or content follows the coupling (the patch, the row masks, the tail table): released by both kinds
// of setup, where ws_alloc_zero's is released by alfd_setup alone
static int cp_alloc_zero(alfd_ctx *ctx, int h, double **p, int64_t count) {
  return ws_alloc_zero(ctx, p, count, &ctx->cp_allocs[h]);
}
static void cp_release(alfd_ctx *ctx, int h) {
  for (void *p : ctx->cp_allocs[h]) hipFree(p);
  ctx->cp_allocs[h].clear();
}

// dinv = 1 / (diag(Adiag) + g * sum_k w_k R_ik^2): the diagonal of Adiag + g R diag(w) R^T
// (w = ALFD_INVW).  The general form takes the weight w, starts from ctx->dA instead of diag(A) when A is
// null, and with invert = false leaves the sum itself in dinv (which may be ctx->dA): chained calls add
// several such terms in a fixed order.
// ctx->dA = diag(A) on the rows of A (the caller zeroes what lies beyond them where it matters)
static void extract_diag(alfd_ctx *ctx, const DevCsr &A) {
  const int grid = grid_for_rows(A.nrows, A.L);
  with_lanes(A.L, [&](auto l) {
    hipLaunchKernelGGL((extract_diag_kernel<decltype(l)::value>), dim3(grid), dim3(kBlock), 0, ctx->stream, A.nrows, A.rp,
                       A.col, A.val, ctx->dA);
  });
}
static int diag_plus_m(alfd_ctx *ctx, const DevCsr *A, DevCsr &R, const double *w, double g, int64_t n, double *dinv,
                       bool invert);
static int diag_plus_m(alfd_ctx *ctx, const DevCsr &A, DevCsr &R, double g, int64_t n, double *dinv) {
  return diag_plus_m(ctx, &A, R, ctx->diag[ALFD_INVW], g, n, dinv, true);
}
static int diag_plus(alfd_ctx *ctx, int slot_diag, int slot_rows, double g, int64_t n, double *dinv) {
  return diag_plus_m(ctx, ctx->mat[slot_diag], ctx->mat[slot_rows], g, n, dinv);
}
static int diag_plus_m(alfd_ctx *ctx, const DevCsr *A, DevCsr &R, const double *w, double g, int64_t n, double *dinv,
                       bool invert) {
  if (A && pad_chunk(n) > ctx->diag_cap) {
    // a replicated multigrid level may be longer than this rank's largest block (many ranks): grow the two scratch vectors
    RC(ws_alloc_zero(ctx, &ctx->dA, pad_chunk(n)));
    RC(ws_alloc_zero(ctx, &ctx->s_aug, pad_chunk(n)));
    ctx->diag_cap = pad_chunk(n);
  }
  if (A) HIPC(hipMemsetAsync(ctx->dA, 0, pad_chunk(n) * sizeof(double), ctx->stream));
  HIPC(hipMemsetAsync(ctx->s_aug, 0, pad_chunk(n) * sizeof(double), ctx->stream));
  if (A) extract_diag(ctx, *A);
  // a rank with no rows of R of its own may still own W entries its peers need
  if (ctx->nranks > 1 && (ctx->local || ctx->host_alltoallv || R.n_halo > 0 || R.send_off.back() > 0))
    RC(halo_exchange(ctx, R, w));
  if (R.n_list > 0)
    hipLaunchKernelGGL(aug_diag_rows_kernel, dim3((unsigned)((R.n_list + 255) / 256)), dim3(256), 0,
                       ctx->stream, R.n_list, R.rp, R.col, R.val, R.sparse ? R.rows : nullptr,
                       w, R.halo, R.n_local_cols, ctx->s_aug);
  hipLaunchKernelGGL(aug_diag_finish_kernel, dim3((unsigned)std::max<int64_t>(1, (n + 255) / 256)), dim3(256), 0, ctx->stream, n,
                     g, ctx->dA, ctx->s_aug, dinv, invert ? 1 : 0);
  HIPC(hipGetLastError());
  return ALFD_OK;
}

// *lambda = |D^-1 Op v| after cheb_power_its normalised steps from the start vector in v; apply(x, y): y = Op x.
// v and wv (the second work vector) change roles every step and hold no result afterwards.
template <class Apply>
static int power_lambda(alfd_ctx *ctx, int64_t npad, const double *dinv, double *v, double *wv, Apply apply, double *lambda) {
  *lambda = 0;
  ctx->setup_counts[ALFD_SC_POWER_ITERATIONS]++;
  for (int it = 0; it < ctx->cfg.cheb_power_its; ++it) {
    RC(dot_async(ctx, npad, v, v, S_TMP));
    RC(read_scalars(ctx, S_TMP, 1));
    const double nv = std::sqrt(ctx->sc_host[S_TMP]);
    VEC_LAUNCH(scale_kernel, npad, 16, (const double *)nullptr, 0, 0, 1.0 / nv, v);
    RC(apply(v, wv));
    VEC_LAUNCH(pmul_scale_kernel, npad, 24, 1.0, dinv, wv, wv);
    RC(dot_async(ctx, npad, wv, wv, S_TMP));
    RC(read_scalars(ctx, S_TMP, 1));
    *lambda = std::sqrt(ctx->sc_host[S_TMP]);
    std::swap(v, wv);
  }
  return ALFD_OK;
}

// Reductions over replicated vectors for the lifetime of the guard: the flag is cleared on every way out
struct ReplicatedDots {
  alfd_ctx *ctx;
  explicit ReplicatedDots(alfd_ctx *c) : ctx(c) { ctx->dots_replicated = true; }
  ~ReplicatedDots() { ctx->dots_replicated = false; }
  ReplicatedDots(const ReplicatedDots &) = delete;
  ReplicatedDots &operator=(const ReplicatedDots &) = delete;
};

// lambda_max(D^-1 Op) by power iteration from the integer-hash start vector
static int power_iteration(alfd_ctx *ctx, int op) {
  const alfd_config &c = ctx->cfg;
  const int64_t npad = op_npad(ctx, op);
  double *v = ctx->w_p, *wv = ctx->w_Ap;
  HIPC(hipMemsetAsync(v, 0, npad * sizeof(double), ctx->stream));
  HIPC(hipMemsetAsync(wv, 0, npad * sizeof(double), ctx->stream));
  auto fill = [&](int blk, double *dst) {
    const int64_t goff = ctx->nranks > 1 ? ctx->part[blk][ctx->rank] : 0;
    hipLaunchKernelGGL(hash_vector_kernel, dim3((unsigned)std::max<int64_t>(1, (ctx->n[blk] + 255) / 256)), dim3(256), 0,
                       ctx->stream, ctx->n[blk], goff, dst);
  };
  if (op == OP_AUG2) {
    fill(0, v);
    fill(1, v + ctx->off[1]);
  } else {
    fill((op == OP_AUG || op == OP_K) ? 0 : 1, v);
  }
  double lam = 0;
  RC(power_lambda(ctx, npad, op_dinv(ctx, op), v, wv, [&](const double *x, double *y) { return op_apply(ctx, op, x, y); }, &lam));
  ctx->lam_max[op] = lam * c.cheb_safety;
  HIPC(hipMemsetAsync(ctx->w_p, 0, ctx->wmax * sizeof(double), ctx->stream));
  HIPC(hipMemsetAsync(ctx->w_Ap, 0, ctx->wmax * sizeof(double), ctx->stream));
  return ALFD_OK;
}

// ======================================================================
// Aggregation multigrid for the augmented block (ALFD_PREC_MULTILEVEL).
// Level l+1 = Galerkin coarsening of level l through the caller's aggregates:
//   A_{l+1} = P^T A_l P,  C_{l+1} = C_l P,  Aug_{l+1} = A_{l+1} + gamma C_{l+1}^T invW C_{l+1}
// (kept factored on every level, like the fine operator).  The cycle is a
// symmetric V-cycle: Chebyshev pre-smoothing from zero, coarse correction,
// Chebyshev post-smoothing of the residual; the coarsest level is "solved" by a
// high-degree Chebyshev sweep.  Every piece is a fixed polynomial in SPD
// operators, so the preconditioner is a fixed SPD operator and plain CG applies.
// What of hierarchy h follows the coupling and the penalty: the coarsest inverse, the row masks, the tail table and (h = 0)
// the interface patch, with the workspace they live in; with `operators` also C_l / Ct_l of the levels l >= 1.
static void free_coupling(alfd_ctx *ctx, int h, bool operators) {
  alfd_ctx::Hierarchy &H = ctx->hier[h];
  for (MlLevel &L : H.ml) {
    if (operators)
      for (LevelStore *S : {&L.loc, &L.rep})
        for (DevCsr *m : {&S->C, &S->Ct}) csr_free(*m);
    L.tail_mask = nullptr;
  }
  H.tail_tab = nullptr;
  csr_free(H.inv);
  if (h == 0) {
    for (DevCsr *m : {&ctx->patch.Ass, &ctx->patch.As, &ctx->patch.Ats, &ctx->patch.Cs, &ctx->patch.Cts, &ctx->patch.Cts_loc,
                      &ctx->patch.Ctg})
      csr_free(*m);
    ctx->patch = alfd_ctx::Patch();
  }
  cp_release(ctx, h);
}

static void free_levels(alfd_ctx *ctx) {
  for (int h = 0; h < 2; ++h) {
    alfd_ctx::Hierarchy &H = ctx->hier[h];
    free_coupling(ctx, h, true);
    for (MlLevel &L : H.ml)
      for (LevelStore *S : {&L.loc, &L.rep})
        for (DevCsr *m : {&S->A, &S->P, &S->R}) csr_free(*m);
    H.ml.clear();
    H.coarse_A = H.coarse_C = H.coarse_Ct = HostCsr();
  }
  ctx->ml_rep_level = -1;
}

static int download_csr(alfd_ctx *ctx, const DevCsr &m, HostCsr &h) {
  h.nrows = m.nrows;
  h.ncols = m.ncols;
  h.col.resize(m.nnz);
  h.val.resize(m.nnz);
  HIPC(hipMemcpyAsync(h.col.data(), m.col, m.nnz * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipMemcpyAsync(h.val.data(), m.val, m.nnz * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  h.rp.assign(m.nrows + 1, 0);
  if (m.sparse) {
    std::vector<int32_t> rows(m.n_list);
    std::vector<int64_t> crp(m.n_list + 1);
    HIPC(hipMemcpyAsync(rows.data(), m.rows, m.n_list * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipMemcpyAsync(crp.data(), m.rp, (m.n_list + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < m.n_list; ++i) h.rp[rows[i] + 1] = crp[i + 1] - crp[i];
    for (int64_t r = 0; r < m.nrows; ++r) h.rp[r + 1] += h.rp[r];
  } else {
    HIPC(hipMemcpyAsync(h.rp.data(), m.rp, (m.nrows + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
  }
  return ALFD_OK;
}

// The deferred window plan of a matrix held in the batch-major form (upload_matrix), built from its device copy.
static int ensure_window_plan(alfd_ctx *ctx, DevCsr &m) {
  if (!m.present || !m.win_deferred) return ALFD_OK;
  HostCsr h;
  RC(download_csr(ctx, m, h));
  m.win_deferred = false;
  const int tag = m.tag;
  RC(build_window(ctx, m, h.rp.data(), h.col.data(), h.val.data(), m.win_user, true));
  m.tag = tag;
  return ALFD_OK;
}
static int ensure_window_plans(alfd_ctx *ctx) {
  for (DevCsr &m : ctx->mat) RC(ensure_window_plan(ctx, m));
  for (alfd_ctx::Hierarchy &H : ctx->hier)
    for (MlLevel &L : H.ml)
      for (LevelStore *S : {&L.loc, &L.rep}) RC(ensure_window_plan(ctx, S->A));
  return ALFD_OK;
}

// GLOBAL ids of the local column space [owned | halo] of an uploaded matrix; c0 = global id of its first owned column
static std::vector<int32_t> global_cols(const DevCsr &m, int64_t c0) {
  std::vector<int32_t> ids((size_t)m.n_local_cols + m.halo_globals.size());
  for (int32_t j = 0; j < m.n_local_cols; ++j) ids[j] = (int32_t)(c0 + j);
  std::copy(m.halo_globals.begin(), m.halo_globals.end(), ids.begin() + m.n_local_cols);
  return ids;
}

// the rows of b below those of a
static void append_rows(HostCsr &a, const HostCsr &b) {
  a.nrows += b.nrows;
  for (int64_t i = 0; i < b.nrows; ++i) a.rp.push_back(a.rp.back() + (b.rp[i + 1] - b.rp[i]));
  a.col.insert(a.col.end(), b.col.begin(), b.col.end());
  a.val.insert(a.val.end(), b.val.begin(), b.val.end());
}

static void transpose_host(const HostCsr &a, HostCsr &t) {
  t.nrows = a.ncols;
  t.ncols = a.nrows;
  const int64_t nnz = a.nnz();
  t.rp.assign(t.nrows + 1, 0);
  t.col.resize(nnz);
  t.val.resize(nnz);
  for (int64_t k = 0; k < nnz; ++k) t.rp[a.col[k] + 1]++;
  for (int64_t r = 0; r < t.nrows; ++r) t.rp[r + 1] += t.rp[r];
  std::vector<int64_t> cur(t.rp.begin(), t.rp.end() - 1);
  for (int64_t r = 0; r < a.nrows; ++r)
    for (int64_t k = a.rp[r]; k < a.rp[r + 1]; ++k) {
      const int64_t p = cur[a.col[k]]++;
      t.col[p] = (int32_t)r;
      t.val[p] = a.val[k];
    }
}

// out = R A Q for aggregation-type transfers.  Row I of out collects the fine rows i with
// agg_row[i] == I (agg_row == nullptr: I == i); column J collects agg_col[j] == J.
// Canonical accumulation order (the oracle follows it too): fine rows ascending, entries
// in CSR order, each added to its coarse entry as it is met; the finished row is sorted
// by column.
static void galerkin(const HostCsr &A, const int32_t *agg_row, const double *w_row, int64_t n_rows_c,
                     const int32_t *agg_col, const double *w_col, int64_t n_cols_c, HostCsr &out) {
  std::vector<int64_t> mem_ptr;
  std::vector<int32_t> mem;
  if (agg_row) {
    mem_ptr.assign(n_rows_c + 1, 0);
    for (int64_t i = 0; i < A.nrows; ++i)
      if (agg_row[i] >= 0) mem_ptr[agg_row[i] + 1]++;
    for (int64_t I = 0; I < n_rows_c; ++I) mem_ptr[I + 1] += mem_ptr[I];
    mem.resize(mem_ptr[n_rows_c]);
    std::vector<int64_t> cur(mem_ptr.begin(), mem_ptr.end() - 1);
    for (int64_t i = 0; i < A.nrows; ++i)
      if (agg_row[i] >= 0) mem[cur[agg_row[i]]++] = (int32_t)i;
  }
  const int T = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::vector<int64_t>> t_cnt(T);
  std::vector<std::vector<int32_t>> t_col(T);
  std::vector<std::vector<double>> t_val(T);
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t]() {
      const int64_t I0 = n_rows_c * t / T, I1 = n_rows_c * (t + 1) / T;
      std::vector<int64_t> marker(n_cols_c, -1);
      std::vector<std::pair<int32_t, double>> row;
      for (int64_t I = I0; I < I1; ++I) {
        row.clear();
        const int64_t m0 = agg_row ? mem_ptr[I] : I, m1 = agg_row ? mem_ptr[I + 1] : I + 1;
        for (int64_t mi = m0; mi < m1; ++mi) {
          const int64_t i = agg_row ? mem[mi] : mi;
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
        t_cnt[t].push_back((int64_t)row.size());
        for (auto &e : row) {
          t_col[t].push_back(e.first);
          t_val[t].push_back(e.second);
        }
      }
    });
  for (auto &x : th) x.join();
  out.nrows = n_rows_c;
  out.ncols = n_cols_c;
  out.rp.assign(1, 0);
  out.col.clear();
  out.val.clear();
  for (int t = 0; t < T; ++t) {
    for (int64_t c : t_cnt[t]) out.rp.push_back(out.rp.back() + c);
    out.col.insert(out.col.end(), t_col[t].begin(), t_col[t].end());
    out.val.insert(out.val.end(), t_val[t].begin(), t_val[t].end());
  }
}

static int upload_matrix(alfd_ctx *ctx, int slot, int64_t nrows, int64_t ncols, const int64_t *rp,
                         const int32_t *col, const double *val);
static int upload_level(alfd_ctx *ctx, DevCsr &dst, const HostCsr &h) {
  static const int32_t no_col = 0;
  static const double no_val = 0;
  RC(upload_matrix(ctx, kScratchSlot, h.nrows, h.ncols, h.rp.data(), h.col.empty() ? &no_col : h.col.data(),
                   h.val.empty() ? &no_val : h.val.data()));
  csr_free(dst);
  dst = std::move(ctx->mat[kScratchSlot]);
  ctx->mat[kScratchSlot] = DevCsr();
  dst.tag = 1;
  return ALFD_OK;
}

// ---- the factored operators of the hierarchy: Aug = A + gamma Ct invW C of a level (rank-local or replicated) and of
// the interface patch.  level_view() / patch_aug() are the only places that know which of these an AugOp names.
struct AugOp {   // the operands of one factored operator and the sweep vectors that go with it
  DevCsr *A = nullptr, *C = nullptr, *Ct = nullptr;
  int clsA = ALFD_T_SPMV_OTHER;
  const double *w = nullptr;   // invW over the multipliers that C addresses
  double gamma = 0;            // the penalty weight: gamma, or gamma2 on the immersed hierarchy
  double *tlam = nullptr;      // invW .* (C x)
  const uint8_t *mask = nullptr;
  int64_t npad = 0;
  const double *dinv = nullptr;
  double *cd = nullptr, *cres = nullptr, *ctmp = nullptr;
  double *cd2 = nullptr, *z2 = nullptr;   // levels whose tails may run inside the A launch: the ping-pong partners of cd and of the sweep's iterate
  double lmax = 0;
};

// One level as the V-cycle sees it: its operator, its vectors, and the transfer pair to the next coarser level with
// that level's r / z (null on the coarsest level)
struct LevelView {
  AugOp op;
  double *r = nullptr, *z = nullptr, *t = nullptr;
  DevCsr *R = nullptr, *P = nullptr;
  double *rc = nullptr, *zc = nullptr;
};

// Hierarchy h = 1 (the immersed block) reads (A2, M, M, gamma2) where hierarchy 0 reads (A, C, Ct, gamma); it is never
// partitioned.  Levels of hierarchy 0 from ml_rep_level on are replicated.  The level above the first replicated one
// keeps the rank-local pair: ml_cycle gathers the restricted residual there.
static LevelView level_view(alfd_ctx *ctx, int h, int l) {
  MlLevel &L = ctx->hier[h].ml[l];
  const bool rep = h == 0 && ctx->ml_rep_level >= 0 && l >= ctx->ml_rep_level;   // never level 0
  LevelStore &S = rep ? L.rep : L.loc;
  LevelView V;
  AugOp &F = V.op;
  F.A = l > 0 ? &S.A : &ctx->mat[h == 0 ? ALFD_A : ALFD_A2];
  F.C = l > 0 ? &S.C : &ctx->mat[h == 0 ? ALFD_C : ALFD_M];
  F.Ct = l > 0 ? &S.Ct : &ctx->mat[h == 0 ? ALFD_CT : ALFD_M];
  F.clsA = l == 0 && h == 0 ? ALFD_T_SPMV_A : ALFD_T_SPMV_OTHER;
  F.w = rep ? ctx->g_w : ctx->diag[ALFD_INVW];
  F.gamma = h == 0 ? ctx->cfg.gamma : ctx->cfg.gamma2;
  F.tlam = rep ? ctx->g_tlam : ctx->t_lam;
  F.mask = L.tail_mask;
  F.npad = S.npad;
  F.dinv = S.dinv;
  F.cd = S.cd, F.cres = S.cres, F.ctmp = S.ctmp;
  F.cd2 = rep ? nullptr : L.tail_d2, F.z2 = rep ? nullptr : L.tail_z2;
  F.lmax = L.lmax;
  V.r = S.r, V.z = S.z, V.t = S.t;
  if (l + 1 < (int)ctx->hier[h].ml.size()) {
    MlLevel &M = ctx->hier[h].ml[l + 1];
    LevelStore &N = rep ? M.rep : M.loc;
    V.R = &N.R, V.P = &N.P;
    V.rc = N.r, V.zc = N.z;
  }
  return V;
}

static AugOp patch_aug(alfd_ctx *ctx) {
  alfd_ctx::Patch &Q = ctx->patch;
  AugOp F;
  F.A = &Q.Ass, F.C = &Q.Cs, F.Ct = &Q.Cts;
  F.w = Q.rep ? ctx->g_w : ctx->diag[ALFD_INVW];       // replicated patch: the whole multiplier space
  F.tlam = Q.rep ? ctx->g_tlam : ctx->t_lam;
  F.gamma = ctx->cfg.gamma;
  F.mask = Q.tail_mask;
  F.npad = Q.mpad;
  F.dinv = Q.dinv;
  F.cd = Q.cd, F.cres = Q.cres, F.ctmp = Q.ctmp;
  F.lmax = Q.lmax;
  return F;
}

// y = A x and tlam = invW .* (C x): the first two launches of aug_apply, or their pair launch
static int fused_AC(alfd_ctx *ctx, const AugOp &F, const double *x, double *y) {
  return spmv_AC(ctx, *F.A, F.clsA, *F.C, F.w, x, y, F.tlam);
}

// y = Aug x.  On level 0 these are the launches of op_apply(OP_AUG) with the diagonal weight: setup() refuses the
// multilevel preconditioner together with the nested grad-div term.
static int aug_apply(alfd_ctx *ctx, const AugOp &F, const double *x, double *y) {
  if (ctx->cfg.aug_assembled) return spmv_m(ctx, *F.A, F.clsA, x, y, 0);   // operator form: A already holds the AL term
  RC(fused_AC(ctx, F, x, y));
  return spmv_m(ctx, *F.Ct, ALFD_T_SPMV_OTHER, F.tlam, y, 1, F.gamma);
}

// *lmax = cheb_safety * lambda_max(D^-1 Aug) of the factored operator F (its dinv, its npad) by power iteration from the
// integer-hash vector: entry i < n from global index goff + i.  v and wv, npad zeros on entry, are zero again on return.
static int aug_lambda_max(alfd_ctx *ctx, const AugOp &F, int64_t n, int64_t goff, double *v, double *wv, double *lmax) {
  if (n > 0)
    hipLaunchKernelGGL(hash_vector_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, goff, v);
  double lam = 0;
  RC(power_lambda(ctx, F.npad, F.dinv, v, wv, [&](const double *x, double *y) { return aug_apply(ctx, F, x, y); }, &lam));
  *lmax = lam * ctx->cfg.cheb_safety;
  HIPC(hipMemsetAsync(v, 0, F.npad * sizeof(double), ctx->stream));
  HIPC(hipMemsetAsync(wv, 0, F.npad * sizeof(double), ctx->stream));
  return ALFD_OK;
}

// ---- fused smoother steps ("ml_fuse").  One application of a factored operator inside a Chebyshev
// sweep or a residual is three dependent launches plus the element-wise kernel that consumes it.  Here the last two
// become one (aug_tail); the arithmetic of every element is the same, so are the bits.

// does spmv_launch_local run m on spmv_kernel<L, *, *> (no batch-major, window or stream form)?
static bool plain_form(const alfd_ctx *ctx, const DevCsr &m) {
  return m.present && !m.vs.on && !m.win && !(m.L == 64 && !m.sparse && ctx->spmv_stream_R > 0);
}

// Everything else keeps the separate launches: Ct in another storage form, partitioned contexts (halo exchanges),
// the nested grad-div term, the exact W^-1, a level without mask.
static bool fused_ok(const alfd_ctx *ctx, const AugOp &F) {
  return ctx->ml_fuse && ctx->nranks == 1 && !ctx->cfg.aug_assembled && !gd_nested(ctx) &&
         ctx->cfg.w_inverse == ALFD_W_DIAGONAL && F.mask && F.A->present && F.C->present && plain_form(ctx, *F.Ct);
}

// ---- the tails inside the A launch ("ml_tail_in_spmv").  For a row that Ct does not list the tail is
// an element-wise expression of the A x value its workgroup has just formed: the batch-major kernel applies it at its
// block end (TM instantiations of spmv_vs_kernel), the tail launch shrinks to its rows party.

// the LDS per workgroup that keeps eight of them resident on a CU (160 KB), DESIGN section 5
constexpr size_t kVsTailLdsLimit = 20 * 1024;

// Does A run the instantiations that have the epilogue, within the LDS bound, with fewer than half of its rows in Ct?
static bool tail_in_form(alfd_ctx *ctx, const DevCsr &A, const DevCsr &Ct, int64_t npad) {
  if (!A.present || A.sparse || A.n_list == 0 || A.nrows > npad || A.nrows > INT32_MAX) return false;
  if (!(A.vs.on && ctx->vs_enable && !ctx->vi_off) || A.vs.L != 64 || A.vs.NW != 4 || A.vs.nb <= 0) return false;
  if ((size_t)(A.vs.wide ? VsFmt<1>::kWinOff : VsFmt<0>::kWinOff) + (size_t)A.vs.tail_lds > kVsTailLdsLimit) return false;
  // side rows have no block end: their tails run in a launch of their own behind it ("ml_tail_side_rows", one rank)
  if (A.vs.side_n > 0 && !(ctx->ml_tail_side_rows && ctx->nranks == 1)) return false;
  if (!Ct.present || 2 * Ct.n_list >= A.nrows) return false;   // e.g. the patch operator: every row is Ct's, nothing to gain
  return vs_lds_base_ok(ctx);
}

static bool tail_in_ok(alfd_ctx *ctx, const AugOp &F) {
  return ctx->ml_tail_in_spmv && fused_ok(ctx, F) && F.cd2 && F.z2 && !a32_active(ctx, *F.A) &&
         tail_in_form(ctx, *F.A, *F.Ct, F.npad);
}

// the vectors mode stores (beside y, which the rows of Ct get)
static int tail_outputs(int mode, const AugTailArgs &p, const double *out[3]) {
  int n = 0;
  if (mode == TAIL_STEP || mode == TAIL_RES || (mode == TAIL_RES_INIT && p.store_res)) out[n++] = p.res;
  if (mode == TAIL_STEP) out[n++] = p.d;
  if (mode == TAIL_STEP || mode == TAIL_LAST || mode == TAIL_RES_INIT) out[n++] = p.z;
  if (mode == TAIL_LAST_ADD || mode == TAIL_RES_INIT_ADD) out[n++] = p.zout;
  return n;
}
static bool tail_writes(int mode, const AugTailArgs &p, const double *y, const double *x) {
  const double *out[3];
  const int n = tail_outputs(mode, p, out);
  bool hit = y == x;
  for (int i = 0; i < n; ++i) hit = hit || out[i] == x;
  return hit;
}

// y = A x with the tail of `mode` on the rows Ct does not list, tlam = w .* (C x) beside it (the second party of the
// launch where the pair launch applies, a launch of its own where it does not).  Inside the launch other workgroups
// still stage x while the first ones store: an output that is x would be a race, and is refused here.
// Side rows ("ml_tail_side_rows"): a second launch behind the first, spmv_side_rows_tail_kernel, forms their sums and
// applies their tails; the same refusal covers it.
// vec_bytes: per element, of the element-wise kernel(s) the tail stands for (they read y back: 8 of them are not moved,
// nor are the 8 of the y store).
static int launch_vs_tail(alfd_ctx *ctx, const AugOp &F, const double *x, double *y, int mode, AugTailArgs p, double vec_bytes) {
  const DevCsr &A = *F.A;
  if (mode < TAIL_STEP || mode > TAIL_RES_INIT) return ctx->err = "tail mode without a block-end epilogue", ALFD_E_INVALID;
  if (!tail_in_form(ctx, A, *F.Ct, F.npad) || !F.mask) return ctx->err = "operator without the block-end epilogue", ALFD_E_UNSUPPORTED;
  if (!p.zin) p.zin = p.z;
  if (tail_writes(mode, p, y, x))
    return ctx->err = "block-end epilogue: an output vector is the vector the product reads", ALFD_E_INVALID;
  const DevCsr::Vs &v = A.vs;
  const bool pair = F.C && !v.wide && pair_ok(ctx, A, *F.C) == 1;
  const bool vi = !ctx->vi_off, vs = ctx->vs_enable != 0 && !ctx->vi_off;
  const double ew = (vec_bytes - 16.0) * (double)A.nrows;
  VsTail ta;
  ta.p = p;
  ta.mask = F.mask;
  {
    Timer tm(ctx, F.clsA, A.algorithmic_bytes() + (pair ? F.C->algorithmic_bytes() : 0.0) + ew,
             A.streamed_bytes(vi, vs) + (pair ? F.C->streamed_bytes(vi, vs) : 0.0) + ew);
    const PairC pc = pair ? pair_c(*F.C, F.w, F.tlam, (uint32_t)v.nb, 256) : PairC{};   // 4 waves (tail_in_form)
    const unsigned grid = (unsigned)v.nb + (pair ? pc.nC : 0u);
    with_flag(A.tag, [&](auto tg) {
      with_const_or_last<TAIL_STEP, TAIL_LAST, TAIL_LAST_ADD, TAIL_RES, TAIL_RES_INIT>(mode, [&](auto tm_) {
        constexpr int TAG = decltype(tg)::value, TM = decltype(tm_)::value;
        if (v.wide) launch_vs_kernel<0, TAG, 4, 1, false, TM>(ctx, A, x, y, 0.0, nullptr, nullptr, grid, 0, NoPair(), ta);
        else if (pair) launch_vs_kernel<0, TAG, 4, 0, true, TM>(ctx, A, x, y, 0.0, nullptr, nullptr, grid, 0, pc, ta);
        else launch_vs_kernel<0, TAG, 4, 0, false, TM>(ctx, A, x, y, 0.0, nullptr, nullptr, grid, 0, NoPair(), ta);
      });
    });
    if (v.side_n > 0)   // kSideAll: one rank (tail_in_form).  The batch-major launch before it has finished with x.
      with_const_or_last<TAIL_STEP, TAIL_LAST, TAIL_LAST_ADD, TAIL_RES, TAIL_RES_INIT>(mode, [&](auto tm_) {
        hipLaunchKernelGGL((spmv_side_rows_tail_kernel<decltype(tm_)::value>), dim3((unsigned)side_grid(v.side_n)), dim3(kBlock), 0,
                           ctx->stream, v.side_n, v.side_rows, v.side_rp, v.side_col, v.side_val, x, y, F.mask, p);
      });
    HIPC(hipGetLastError());
    ++ctx->fused_tail_launches;
    if (pair || !F.C) return ALFD_OK;
  }
  return spmv_m(ctx, *F.C, ALFD_T_SPMV_OTHER, x, F.tlam, 2, 0.0, F.w);
}

// p.y += gamma Ct tlam, then the element-wise operation of the mode; vec_bytes: per element, of the kernel(s) replaced.
// rows_only: the rows of Ct alone -- every other row had its tail at the block end of the A launch (launch_vs_tail)
static int aug_tail(alfd_ctx *ctx, const AugOp &F, int mode, AugTailArgs p, double vec_bytes, bool rows_only = false) {
  const DevCsr &m = *F.Ct;
  if (!p.zin) p.zin = p.z;
  if (rows_only) vec_bytes = 0.0;
  const int nb_rows = m.n_list > 0 ? grid_for_rows(m.n_list, m.L) : 0;
  const unsigned grid = (unsigned)nb_rows + (rows_only ? 0u : (unsigned)(F.npad / kChunk));
  if (grid == 0) return ALFD_OK;
  Timer tm(ctx, ALFD_T_SPMV_OTHER, m.algorithmic_bytes() + vec_bytes * (double)F.npad,
           m.streamed_bytes(false) + vec_bytes * (double)F.npad);
  with_lanes(m.L, [&](auto l) {   // as spmv_launch_local
    with_const_or_last<TAIL_STEP, TAIL_LAST, TAIL_LAST_ADD, TAIL_RES, TAIL_RES_INIT, TAIL_RES_INIT_ADD>(mode, [&](auto md) {
      hipLaunchKernelGGL((aug_tail_kernel<decltype(l)::value, decltype(md)::value>), dim3(grid), dim3(kBlock), 0, ctx->stream,
                         m.n_list, m.rp, m.col, m.val, m.sparse ? m.rows : (const int32_t *)nullptr, F.tlam, nb_rows, F.mask,
                         p);
    });
  });
  HIPC(hipGetLastError());
  return ALFD_OK;
}

// One application of F inside a sweep or a residual: y = A x, tlam = w .* (C x), then the tail of `mode` with p.y = y.
// x null: y and tlam hold the products already.  Where the level qualifies (tail_in_ok) and no output of the tail is x,
// the tail of the rows outside Ct runs inside the A launch; a step that must deliver into the vector its own product
// reads keeps the two launches (no copy pass is added for it).
static int aug_op_tail(alfd_ctx *ctx, const AugOp &F, const double *x, double *y, int mode, AugTailArgs p, double vec_bytes) {
  p.y = y;
  if (!p.zin) p.zin = p.z;
  if (x && mode <= TAIL_RES_INIT && tail_in_ok(ctx, F) && !tail_writes(mode, p, y, x)) {
    RC(launch_vs_tail(ctx, F, x, y, mode, p, vec_bytes));
    return aug_tail(ctx, F, mode, p, vec_bytes, true);
  }
  if (x) RC(fused_AC(ctx, F, x, y));
  return aug_tail(ctx, F, mode, p, vec_bytes);
}

// The Chebyshev sweep of cheb_sweep on the operands of F.  have_init: z already holds the first
// direction inv_theta * (dinv .* r) (fused_correct wrote it).  zout: the result is added to zout, z is scratch.
// The first step reads its direction from z and its residual from r, the last stores neither: after a sweep
// cd / cres are only ever read by the next step of the same sweep.
static int cheb_fused(alfd_ctx *ctx, const AugOp &F, int degree, double ratio, const double *r, double *z, double *zout,
                      bool have_init) {
  ChebCoef k(F.lmax, ratio);
  if (!have_init) VEC_LAUNCH(cheb_init_z_kernel, F.npad, 24, 1.0 / k.theta, F.dinv, r, z);
  // Where the tails run inside the A launch no step may store into the vector its product reads: the direction
  // alternates between cd and cd2, and the first step, which multiplies the iterate itself, leaves the new iterate in
  // z2; later steps read it from there and store it where the caller wants it.  Same expressions, other addresses.
  const bool pingpong = tail_in_ok(ctx, F);
  const double *zc = z, *dc = z;   // where the iterate and the direction are (the first direction is the iterate)
  for (int j = 1; j < degree; ++j) {
    AugTailArgs p;
    k.step(p.c1, p.c2);
    p.gamma = F.gamma;
    const bool last = j == degree - 1;
    p.dinv = F.dinv, p.rin = j == 1 ? r : F.cres, p.din = dc, p.zin = zc;
    p.res = F.cres, p.zout = zout;
    p.d = pingpong && dc == F.cd ? F.cd2 : F.cd;
    p.z = pingpong && !last && dc == z ? F.z2 : z;
    RC(aug_op_tail(ctx, F, dc, F.ctmp, !last ? TAIL_STEP : zout ? TAIL_LAST_ADD : TAIL_LAST, p, last && zout ? 88.0 : 64.0));
    dc = p.d, zc = p.z;
  }
  HIPC(hipGetLastError());
  return ALFD_OK;
}

// z = p_k(D^-1 Aug) D^-1 r, k = degree (Chebyshev, zero start)
static int aug_cheb(alfd_ctx *ctx, const AugOp &F, int degree, double ratio, const double *r, double *z) {
  if (fused_ok(ctx, F)) return cheb_fused(ctx, F, degree, ratio, r, z, nullptr, false);
  return cheb_sweep(ctx, F.npad, F.dinv, F.lmax, ratio, degree, F.cd, F.cres, F.ctmp, r, z,
                    [&](const double *x, double *y) { return aug_apply(ctx, F, x, y); });
}

// t = r - Aug x (x null: t holds A x and tlam holds invW .* (C x))
static int fused_residual(alfd_ctx *ctx, const AugOp &F, const double *x, const double *r, double *t) {
  AugTailArgs p;
  p.gamma = F.gamma, p.rin = r, p.res = t;
  return aug_op_tail(ctx, F, x, t, TAIL_RES, p, 24.0);
}

// The residual t = r - Aug x as above and the sweep on it: zc = q(t), or zout += q(t) with zc as scratch
static int fused_correct(alfd_ctx *ctx, const AugOp &F, int degree, double ratio, const double *x, const double *r, double *t,
                         double *zc, double *zout) {
  AugTailArgs p;
  p.gamma = F.gamma, p.c1 = 1.0 / ChebCoef(F.lmax, ratio).theta;
  p.dinv = F.dinv, p.rin = r, p.res = t, p.z = zc, p.zout = zout;
  p.store_res = degree > 1;
  if (degree <= 1 && zout) return aug_op_tail(ctx, F, x, t, TAIL_RES_INIT_ADD, p, 24.0 + 32.0 + 24.0);
  RC(aug_op_tail(ctx, F, x, t, TAIL_RES_INIT, p, 24.0 + (degree > 1 ? 40.0 : 32.0)));
  return cheb_fused(ctx, F, degree, ratio, t, zc, zout, true);
}

// the ping-pong vectors of level l of hierarchy h, where its operator can run the tails inside the A launch (coupling
// workspace, as the mask the answer depends on)
static int build_tail_vectors(alfd_ctx *ctx, int h, int l) {
  MlLevel &L = ctx->hier[h].ml[l];
  L.tail_z2 = L.tail_d2 = nullptr;
  const AugOp F = level_view(ctx, h, l).op;
  const bool form = L.tail_mask && ctx->nranks == 1 && tail_in_form(ctx, *F.A, *F.Ct, F.npad);
  if (ctx->cfg.log_level > 0 || std::getenv("ALFD_LOG_UPLOAD"))
    std::fprintf(stderr, "[alfd] hierarchy %d level %d (%lld rows, %lld in Ct): tails inside the A launch %s\n", h, l,
                 (long long)F.A->nrows, (long long)F.Ct->n_list, form ? "possible" : "not possible");
  if (!form) return ALFD_OK;
  RC(cp_alloc_zero(ctx, h, &L.tail_z2, F.npad));
  return cp_alloc_zero(ctx, h, &L.tail_d2, F.npad);
}

// the mask of aug_tail_kernel for the operator of hierarchy h whose Ct is m (coupling workspace: released with it)
static int build_tail_mask(alfd_ctx *ctx, int h, const DevCsr &m, int64_t npad, uint8_t **mask) {
  *mask = nullptr;
  if (ctx->nranks > 1 || !m.present || npad == 0 || m.nrows > npad) return ALFD_OK;
  double *q = nullptr;
  RC(cp_alloc_zero(ctx, h, &q, npad / 8));
  *mask = reinterpret_cast<uint8_t *>(q);
  if (m.n_list > 0)
    hipLaunchKernelGGL(mark_rows_kernel, dim3((unsigned)((m.n_list + 255) / 256)), dim3(256), 0, ctx->stream, m.n_list,
                       m.sparse ? m.rows : (const int32_t *)nullptr, *mask);
  HIPC(hipGetLastError());
  return ALFD_OK;
}

// ---- the coarse tail of hierarchy 1 in one launch ("ml_tail_rows", ml_tail_kernel)
static_assert(kTailMaxLevels == ALFD_MAX_LEVELS + 1, "TailTable holds every level of a hierarchy");

static TailCsr tail_csr(const DevCsr &m) {
  TailCsr t;
  t.rp = m.rp, t.col = m.col, t.val = m.val, t.rows = m.sparse ? m.rows : nullptr;
  t.n_list = m.n_list, t.nrows = m.nrows;
  t.L = m.L, t.sparse = m.sparse ? 1 : 0;
  return t;
}

// The level descriptors: operands as level_view() names them, Chebyshev coefficients as cheb_sweep() steps them
static int build_tail_table(alfd_ctx *ctx) {
  const alfd_config &c = ctx->cfg;
  alfd_ctx::Hierarchy &H = ctx->hier[1];
  const int last = (int)H.ml.size() - 1;
  std::vector<TailTable> tab(1);
  TailTable &T = tab[0];
  std::memset(&T, 0, sizeof(T));
  T.nlev = last + 1;
  T.has_inv = H.inv.present ? 1 : 0;
  if (H.inv.present) T.inv = tail_csr(H.inv);
  for (int l = 1; l <= last; ++l) {
    const LevelView V = level_view(ctx, 1, l);
    TailLevel &F = T.lev[l];
    F.A = tail_csr(*V.op.A), F.C = tail_csr(*V.op.C), F.Ct = tail_csr(*V.op.Ct);
    if (l < last) F.R = tail_csr(*V.R), F.P = tail_csr(*V.P);
    F.dinv = V.op.dinv, F.w = V.op.w, F.tlam = V.op.tlam;
    F.r = V.r, F.z = V.z, F.t = V.t, F.cd = V.op.cd, F.cres = V.op.cres, F.ctmp = V.op.ctmp;
    F.gamma = V.op.gamma, F.npad = V.op.npad;
    F.degree = l == last ? c.ml_coarse_degree : c.ml_smooth_degree_coarse > 0 ? c.ml_smooth_degree_coarse : c.ml_smooth_degree;
    ChebCoef k(V.op.lmax, l == last ? c.ml_coarse_ratio : c.ml_smooth_ratio);
    F.inv_theta = 1.0 / k.theta;
    for (int j = 1; j < F.degree && j <= kTailMaxDegree; ++j) k.step(F.c1[j - 1], F.c2[j - 1]);
  }
  double *q = nullptr;
  RC(cp_alloc_zero(ctx, 1, &q, (int64_t)((sizeof(TailTable) + 7) / 8)));
  H.tail_tab = reinterpret_cast<TailTable *>(q);
  HIPC(hipMemcpyAsync(H.tail_tab, &T, sizeof(TailTable), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));   // T leaves scope
  return ALFD_OK;
}

// May ml_tail_kernel take levels l .. last of hierarchy 1, called with (r, z)?  Every operator there in CSR form, the
// factored diagonal-weight operator on one rank (as fused_ok), coefficients within the descriptor.
static bool tail_ok(alfd_ctx *ctx, int l, const double *r, const double *z) {
  const alfd_config &c = ctx->cfg;
  alfd_ctx::Hierarchy &H = ctx->hier[1];
  const int last = (int)H.ml.size() - 1;
  if (!H.tail_tab || l < 1 || H.ml[l].loc.n > ctx->ml_tail_rows || r != H.ml[l].loc.r || z != H.ml[l].loc.z) return false;
  if (ctx->nranks != 1 || c.aug_assembled || c.w_inverse != ALFD_W_DIAGONAL) return false;
  const int sdeg = c.ml_smooth_degree_coarse > 0 ? c.ml_smooth_degree_coarse : c.ml_smooth_degree;
  if (sdeg - 1 > kTailMaxDegree || (!H.inv.present && c.ml_coarse_degree - 1 > kTailMaxDegree)) return false;
  if (H.inv.present && !tail_form(H.inv)) return false;
  for (int j = l; j <= last; ++j) {
    const LevelStore &L = H.ml[j].loc;
    if (!tail_form(L.A) || !tail_form(L.C) || !tail_form(L.Ct)) return false;
    if (j > l && (!tail_form(L.R) || !tail_form(L.P))) return false;
  }
  return true;
}

// device vector pieces (offs[p+1] - offs[p] doubles on rank p) -> the whole vector on every rank
static int allgather_pieces(alfd_ctx *ctx, const double *mine, const std::vector<int64_t> &offs, int64_t piece, double *send,
                            double *stage, double *whole) {
  const int64_t n_me = offs[ctx->rank + 1] - offs[ctx->rank];
  if (n_me > 0) HIPC(hipMemcpyAsync(send, mine, n_me * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  RC(comm_allgather(ctx, send, stage, (size_t)piece * sizeof(double)));
  for (int p = 0; p < ctx->nranks; ++p) {
    const int64_t np = offs[p + 1] - offs[p];
    if (np > 0)
      HIPC(hipMemcpyAsync(whole + offs[p], stage + (int64_t)p * piece, np * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  }
  return ALFD_OK;
}

// z = V-cycle(r) on level l of hierarchy h
static int ml_cycle(alfd_ctx *ctx, int h, int l, const double *r, double *z) {
  const alfd_config &c = ctx->cfg;
  alfd_ctx::Hierarchy &H = ctx->hier[h];
  const int last = (int)H.ml.size() - 1;
  if (h == 1 && ctx->ml_tail_rows > 0 && tail_ok(ctx, l, r, z)) {
    Timer tm(ctx, ALFD_T_SPMV_OTHER, 0.0);
    hipLaunchKernelGGL(ml_tail_kernel, dim3(1), dim3(kTailBlock), 0, ctx->stream, H.tail_tab, l);
    HIPC(hipGetLastError());
    return ALFD_OK;
  }
  const LevelView L = level_view(ctx, h, l);
  const AugOp &F = L.op;
  // level 0 of hierarchy 0: smoother steps and both residuals take slot A through its single-precision copy (the
  // levels below never name slot A)
  const A32Scope a32(ctx, h == 0 && l == 0 && ctx->a32_used);
  if (l == last) {
    if (H.inv.present) return spmv_m(ctx, H.inv, ALFD_T_SPMV_OTHER, r, z, 0);   // z = Aug_c^-1 r
    return aug_cheb(ctx, F, c.ml_coarse_degree, c.ml_coarse_ratio, r, z);
  }
  const int sdeg = l > 0 && c.ml_smooth_degree_coarse > 0 ? c.ml_smooth_degree_coarse : c.ml_smooth_degree;
  const bool fuse = fused_ok(ctx, F);
  RC(aug_cheb(ctx, F, sdeg, c.ml_smooth_ratio, r, z));                       // pre-smoothing from zero
  if (fuse) {
    RC(fused_residual(ctx, F, z, r, L.t));
  } else {
    RC(aug_apply(ctx, F, z, L.t));
    VEC_LAUNCH(sub_from_kernel, F.npad, 24, r, L.t);                         // t = r - Aug z
  }
  RC(spmv_m(ctx, *L.R, ALFD_T_SPMV_OTHER, L.t, L.rc, 0));                    // r_c = P^T t
  if (h == 0 && l + 1 == ctx->ml_rep_level) {
    // the restricted residual is gathered once; everything below runs replicated, without exchanges
    MlLevel &N = H.ml[l + 1];
    RC(allgather_pieces(ctx, N.loc.r, N.offs, N.maxpiece, N.send, N.stage, N.rep.r));
    RC(ml_cycle(ctx, h, l + 1, N.rep.r, N.rep.z));
    // z += P e_c: aggregates -> my slice of e_c; CSR prolongators address the replicated vector by global ids
    RC(spmv_m(ctx, N.loc.P, ALFD_T_SPMV_OTHER, N.P_global_cols ? N.rep.z : N.rep.z + N.offs[ctx->rank], z, 1, 1.0));
  } else {
    RC(ml_cycle(ctx, h, l + 1, L.rc, L.zc));
    RC(spmv_m(ctx, *L.P, ALFD_T_SPMV_OTHER, L.zc, z, 1, 1.0));               // z += P e_c
  }
  if (fuse) {
    RC(fused_correct(ctx, F, sdeg, c.ml_smooth_ratio, z, r, L.t, L.r, z));   // z += post-smoothing of r - Aug z
    return ALFD_OK;
  }
  RC(aug_apply(ctx, F, z, L.t));
  VEC_LAUNCH(sub_from_kernel, F.npad, 24, r, L.t);
  RC(aug_cheb(ctx, F, sdeg, c.ml_smooth_ratio, L.t, L.r));                   // post-smoothing correction
  VEC_LAUNCH(axpy_kernel, F.npad, 24, (const double *)nullptr, 0, 1.0, L.r, z);
  HIPC(hipGetLastError());
  return ALFD_OK;
}

// The multilevel inner preconditioner: the V-cycle, wrapped (ml_patch_degree > 0) into two corrections on the
// interface patch:  z1 = E q E^T r;  z2 = z1 + V(r - Aug z1);  z = z2 + E q E^T (r - Aug z2)  -- symmetric.
// ml_apply on a partitioned context: same arithmetic, the patch polynomial runs redundantly on every rank
static int ml_apply_rep(alfd_ctx *ctx, const double *r, double *z) {
  alfd_ctx::Patch &Q = ctx->patch;
  const int64_t n0p = pad_chunk(ctx->n[0]);
  const unsigned gm = (unsigned)std::max<int64_t>(1, (Q.m_loc + 255) / 256);
  const bool pen = !ctx->cfg.aug_assembled;
  const int last = ctx->nblocks - 1;
  const int64_t s0 = Q.soff[ctx->rank];
  const AugOp F = patch_aug(ctx);
  const int pdeg = ctx->cfg.ml_patch_degree;
  const double pratio = ctx->cfg.ml_patch_ratio;
  if (Q.m_loc > 0) hipLaunchKernelGGL(gather_kernel, dim3(gm), dim3(256), 0, ctx->stream, Q.m_loc, Q.S, r, Q.loc);
  RC(allgather_pieces(ctx, Q.loc, Q.soff, Q.piece, Q.send, Q.stage, Q.rS));
  RC(aug_cheb(ctx, F, pdeg, pratio, Q.rS, Q.zS));
  VEC_LAUNCH(scale_copy_kernel, n0p, 16, 1.0, r, Q.rr);
  RC(spmv_m(ctx, Q.Ats, ALFD_T_SPMV_OTHER, Q.zS, Q.rr, 1, -1.0));
  if (pen) {
    RC(spmv_m(ctx, Q.Cs, ALFD_T_SPMV_OTHER, Q.zS, ctx->g_tlam, 2, 0.0, ctx->g_w));
    RC(spmv_m(ctx, Q.Ctg, ALFD_T_SPMV_OTHER, ctx->g_tlam, Q.rr, 1, -ctx->cfg.gamma));
  }
  RC(ml_cycle(ctx, 0, 0, Q.rr, z));
  if (Q.m_loc > 0) hipLaunchKernelGGL(scatter_add_kernel, dim3(gm), dim3(256), 0, ctx->stream, Q.m_loc, Q.S, Q.zS + s0, z);
  RC(spmv_m(ctx, Q.As, ALFD_T_SPMV_OTHER, z, Q.loc, 0));                          // my rows of (A z) on S
  if (pen) {
    RC(spmv(ctx, ALFD_C, z, ctx->t_lam, 2, 0.0, ctx->diag[ALFD_INVW]));          // my multipliers of W^-1 C z
    RC(allgather_pieces(ctx, ctx->t_lam, ctx->part[last], Q.lam_piece, Q.lam_send, Q.lam_stage, ctx->g_tlam));
    RC(spmv_m(ctx, Q.Cts_loc, ALFD_T_SPMV_OTHER, ctx->g_tlam, Q.loc, 1, ctx->cfg.gamma));
  }
  RC(allgather_pieces(ctx, Q.loc, Q.soff, Q.piece, Q.send, Q.stage, Q.uS));
  VEC_LAUNCH(sub_from_kernel, Q.mpad, 24, Q.rS, Q.uS);
  RC(aug_cheb(ctx, F, pdeg, pratio, Q.uS, Q.eS));
  if (Q.m_loc > 0) hipLaunchKernelGGL(scatter_add_kernel, dim3(gm), dim3(256), 0, ctx->stream, Q.m_loc, Q.S, Q.eS + s0, z);
  HIPC(hipGetLastError());
  return ALFD_OK;
}

static int ml_apply(alfd_ctx *ctx, const double *r, double *z) {
  alfd_ctx::Patch &Q = ctx->patch;
  if (!Q.on) return ml_cycle(ctx, 0, 0, r, z);
  if (Q.rep) return ml_apply_rep(ctx, r, z);
  const int64_t n0p = pad_chunk(ctx->n[0]);
  const unsigned gm = (unsigned)((Q.m + 255) / 256);
  const bool pen = !ctx->cfg.aug_assembled;
  const double *w = ctx->diag[ALFD_INVW];
  const AugOp F = patch_aug(ctx);
  const int pdeg = ctx->cfg.ml_patch_degree;
  const double pratio = ctx->cfg.ml_patch_ratio;
  hipLaunchKernelGGL(gather_kernel, dim3(gm), dim3(256), 0, ctx->stream, Q.m, Q.S, r, Q.rS);
  RC(aug_cheb(ctx, F, pdeg, pratio, Q.rS, Q.zS));
  VEC_LAUNCH(scale_copy_kernel, n0p, 16, 1.0, r, Q.rr);                           // rr = r (a blit copy costs 10x this kernel)
  RC(spmv_m(ctx, Q.Ats, ALFD_T_SPMV_OTHER, Q.zS, Q.rr, 1, -1.0));                 // rr -= A[:,S] zS
  if (pen) {
    RC(spmv_m(ctx, Q.Cs, ALFD_T_SPMV_OTHER, Q.zS, ctx->t_lam, 2, 0.0, w));
    RC(spmv(ctx, ALFD_CT, ctx->t_lam, Q.rr, 1, -ctx->cfg.gamma));                 // rr -= gamma Ct W^-1 C[:,S] zS
  }
  RC(ml_cycle(ctx, 0, 0, Q.rr, z));
  hipLaunchKernelGGL(scatter_add_kernel, dim3(gm), dim3(256), 0, ctx->stream, Q.m, Q.S, Q.zS, z);
  if (pen) RC(spmv_AC(ctx, Q.As, ALFD_T_SPMV_OTHER, ctx->mat[ALFD_C], w, z, Q.uS, ctx->t_lam));   // (Aug z) on S
  else RC(spmv_m(ctx, Q.As, ALFD_T_SPMV_OTHER, z, Q.uS, 0));
  if (fused_ok(ctx, F)) {
    RC(fused_correct(ctx, F, pdeg, pratio, nullptr, Q.rS, Q.uS, Q.eS, nullptr));
  } else {
    if (pen) RC(spmv_m(ctx, Q.Cts, ALFD_T_SPMV_OTHER, ctx->t_lam, Q.uS, 1, ctx->cfg.gamma));
    VEC_LAUNCH(sub_from_kernel, Q.mpad, 24, Q.rS, Q.uS);                          // uS = r_S - (Aug z)_S
    RC(aug_cheb(ctx, F, pdeg, pratio, Q.uS, Q.eS));
  }
  hipLaunchKernelGGL(scatter_add_kernel, dim3(gm), dim3(256), 0, ctx->stream, Q.m, Q.S, Q.eS, z);
  HIPC(hipGetLastError());
  return ALFD_OK;
}

// out = A * Pm on the host, multi-threaded over row ranges.  Every output entry (i, J) is ONE sequential fma
// chain: entries k of row i of A in CSR order, entries of row col_k of Pm in CSR order,
// acc_J = fma(a_ik, p_kJ, acc_J) from 0; the finished row is sorted by column (the oracle repeats this).
static void spgemm_host(const HostCsr &A, const HostCsr &Pm, HostCsr &out) {
  const int64_t nrows = A.nrows, nc = Pm.ncols;
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(16u, std::max(1u, std::thread::hardware_concurrency())),
                                                           (nrows + 4095) / 4096));
  std::vector<std::vector<int32_t>> t_cnt(T), t_col(T);
  std::vector<std::vector<double>> t_val(T);
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t]() {
      const int64_t i0 = nrows * t / T, i1 = nrows * (t + 1) / T;
      std::vector<int64_t> stamp(nc, -1);
      std::vector<double> acc(nc, 0.0);
      std::vector<int32_t> touched;
      t_cnt[t].reserve(i1 - i0);
      for (int64_t i = i0; i < i1; ++i) {
        touched.clear();
        for (int64_t k = A.rp[i]; k < A.rp[i + 1]; ++k) {
          const double a = A.val[k];
          const int64_t j = A.col[k];
          for (int64_t e = Pm.rp[j]; e < Pm.rp[j + 1]; ++e) {
            const int32_t J = Pm.col[e];
            if (stamp[J] != i) {
              stamp[J] = i;
              acc[J] = std::fma(a, Pm.val[e], 0.0);
              touched.push_back(J);
            } else {
              acc[J] = std::fma(a, Pm.val[e], acc[J]);
            }
          }
        }
        std::sort(touched.begin(), touched.end());
        t_cnt[t].push_back((int32_t)touched.size());
        for (int32_t J : touched) {
          t_col[t].push_back(J);
          t_val[t].push_back(acc[J]);
        }
      }
    });
  for (auto &x : th) x.join();
  out.nrows = nrows;
  out.ncols = nc;
  out.rp.assign(1, 0);
  out.rp.reserve(nrows + 1);
  int64_t total = 0;
  for (int t = 0; t < T; ++t) total += (int64_t)t_col[t].size();
  out.col.clear();
  out.val.clear();
  out.col.reserve(total);
  out.val.reserve(total);
  for (int t = 0; t < T; ++t) {
    for (int32_t c : t_cnt[t]) out.rp.push_back(out.rp.back() + c);
    out.col.insert(out.col.end(), t_col[t].begin(), t_col[t].end());
    out.val.insert(out.val.end(), t_val[t].begin(), t_val[t].end());
    std::vector<int32_t>().swap(t_col[t]);
    std::vector<double>().swap(t_val[t]);
  }
}

// rows `rows` of A with compact row numbering (full_rows = 0) or as rows of an nrows_out-row matrix whose other
// rows are empty (full_rows = 1); columns kept where colmap[col] >= 0 (renumbered) or all (colmap == nullptr)
static void extract_host(const HostCsr &A, const std::vector<int32_t> &rows, const int32_t *colmap, int64_t ncols,
                         bool full_rows, HostCsr &out) {
  out.nrows = full_rows ? A.nrows : (int64_t)rows.size();
  out.ncols = ncols;
  out.rp.assign(out.nrows + 1, 0);
  out.col.clear();
  out.val.clear();
  int64_t next = 0;   // next output row to close
  for (size_t q = 0; q < rows.size(); ++q) {
    const int64_t i = rows[q], orow = full_rows ? i : (int64_t)q;
    for (; next <= orow; ++next) out.rp[next] = (int64_t)out.col.size();
    for (int64_t k = A.rp[i]; k < A.rp[i + 1]; ++k) {
      const int32_t c = colmap ? colmap[A.col[k]] : A.col[k];
      if (c < 0) continue;
      out.col.push_back(c);
      out.val.push_back(A.val[k]);
    }
  }
  for (; next <= out.nrows; ++next) out.rp[next] = (int64_t)out.col.size();
}

static int upload_level_part(alfd_ctx *ctx, DevCsr &dst, const HostCsr &h, const int64_t *col_offsets, bool local_only);

// A CSR matrix in plain device arrays (intermediate products of the Galerkin setup)
struct DevRawCsr {
  int64_t nrows = 0, ncols = 0, nnz = 0;
  int64_t *rp = nullptr;
  int32_t *col = nullptr;
  double *val = nullptr;
  void release() {
    if (rp) hipFree(rp);
    if (col) hipFree(col);
    if (val) hipFree(val);
    rp = nullptr, col = nullptr, val = nullptr;
  }
};

// out = A * P on the device (spgemm_rows_kernel: the canonical fma chains of spgemm_host, bit for bit).
// *fits = false when a row has more distinct columns than the kernel's hash set holds (nothing is returned then).
static int dev_spgemm(alfd_ctx *ctx, int64_t nrows, const int64_t *arp, const int32_t *acol, const double *aval,
                      const int64_t *prp, const int32_t *pcol, const double *pval, int64_t ncols_out, DevRawCsr &out,
                      bool *fits) {
  *fits = false;
  out = DevRawCsr();
  out.nrows = nrows;
  out.ncols = ncols_out;
  int32_t *counts = nullptr, *ovf = nullptr;
  HIPC(hipMalloc((void **)&counts, std::max<int64_t>(nrows, 1) * sizeof(int32_t)));
  HIPC(hipMalloc((void **)&ovf, sizeof(int32_t)));
  HIPC(hipMemsetAsync(ovf, 0, sizeof(int32_t), ctx->stream));
  HIPC(hipMalloc((void **)&out.rp, (nrows + 1) * sizeof(int64_t)));
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(nrows, 256 * 64));
  hipLaunchKernelGGL(spgemm_rows_kernel, dim3(grid), dim3(64), 0, ctx->stream, nrows, arp, acol, aval, prp, pcol, pval, 0,
                     counts, (const int64_t *)nullptr, (int32_t *)nullptr, (double *)nullptr, ovf);
  std::vector<int32_t> hc(nrows);
  int32_t hovf = 0;
  if (nrows) HIPC(hipMemcpyAsync(hc.data(), counts, nrows * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipMemcpyAsync(&hovf, ovf, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  if (hovf) {
    hipFree(counts);
    hipFree(ovf);
    out.release();
    return ALFD_OK;
  }
  std::vector<int64_t> rp(nrows + 1, 0);
  for (int64_t i = 0; i < nrows; ++i) rp[i + 1] = rp[i] + hc[i];
  out.nnz = rp[nrows];
  HIPC(hipMemcpyAsync(out.rp, rp.data(), (nrows + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMalloc((void **)&out.col, std::max<int64_t>(out.nnz, 1) * sizeof(int32_t)));
  HIPC(hipMalloc((void **)&out.val, std::max<int64_t>(out.nnz, 1) * sizeof(double)));
  hipLaunchKernelGGL(spgemm_rows_kernel, dim3(grid), dim3(64), 0, ctx->stream, nrows, arp, acol, aval, prp, pcol, pval, 1,
                     counts, (const int64_t *)out.rp, out.col, out.val, ovf);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(ctx->stream));
  hipFree(counts);
  hipFree(ovf);
  *fits = true;
  return ALFD_OK;
}

static int download_raw(alfd_ctx *ctx, const DevRawCsr &d, HostCsr &h) {
  h.nrows = d.nrows;
  h.ncols = d.ncols;
  h.rp.resize(d.nrows + 1);
  h.col.resize(d.nnz);
  h.val.resize(d.nnz);
  HIPC(hipMemcpyAsync(h.rp.data(), d.rp, (d.nrows + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  if (d.nnz) {
    HIPC(hipMemcpyAsync(h.col.data(), d.col, d.nnz * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipMemcpyAsync(h.val.data(), d.val, d.nnz * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  return ALFD_OK;
}

// Host CSR with the shape of the device matrix A but only the rows that reach the interface patch filled in (the rows
// with a column in S, which contain S itself): found and gathered on the device, so that the patch setup does not need
// a host copy of A (21 GB at N = 74).  pos[j] >= 0 marks the columns of S.
static int fetch_patch_rows(alfd_ctx *ctx, const DevCsr &A, const std::vector<int32_t> &pos, HostCsr &out,
                            std::vector<int32_t> &Trows) {
  const int64_t n = A.nrows;
  int32_t *d_pos = nullptr, *d_rows = nullptr, *d_col = nullptr;
  uint8_t *d_flag = nullptr;
  int64_t *d_orp = nullptr;
  double *d_val = nullptr;
  HIPC(hipMalloc((void **)&d_pos, std::max<int64_t>(A.ncols, 1) * sizeof(int32_t)));
  HIPC(hipMalloc((void **)&d_flag, std::max<int64_t>(n, 1)));
  HIPC(hipMemcpyAsync(d_pos, pos.data(), pos.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(rows_touching_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->stream, n, A.rp, A.col, d_pos, d_flag);
  std::vector<uint8_t> flag(n);
  std::vector<int64_t> rp(n + 1);
  HIPC(hipMemcpyAsync(flag.data(), d_flag, n, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipMemcpyAsync(rp.data(), A.rp, (n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  Trows.clear();
  for (int64_t i = 0; i < n; ++i)
    if (flag[i]) Trows.push_back((int32_t)i);
  const int64_t nt = (int64_t)Trows.size();
  std::vector<int64_t> orp(nt + 1, 0);
  for (int64_t q = 0; q < nt; ++q) orp[q + 1] = orp[q] + (rp[Trows[q] + 1] - rp[Trows[q]]);
  const int64_t nnz = orp[nt];
  HIPC(hipMalloc((void **)&d_rows, std::max<int64_t>(nt, 1) * sizeof(int32_t)));
  HIPC(hipMalloc((void **)&d_orp, (nt + 1) * sizeof(int64_t)));
  HIPC(hipMalloc((void **)&d_col, std::max<int64_t>(nnz, 1) * sizeof(int32_t)));
  HIPC(hipMalloc((void **)&d_val, std::max<int64_t>(nnz, 1) * sizeof(double)));
  HIPC(hipMemcpyAsync(d_rows, Trows.data(), nt * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(d_orp, orp.data(), (nt + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  if (nt > 0)
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((nt + 3) / 4)), dim3(256), 0, ctx->stream, nt, d_rows, A.rp, A.col,
                       A.val, d_orp, d_col, d_val);
  out.nrows = n;
  out.ncols = A.ncols;
  out.col.resize(nnz);
  out.val.resize(nnz);
  HIPC(hipMemcpyAsync(out.col.data(), d_col, nnz * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipMemcpyAsync(out.val.data(), d_val, nnz * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  out.rp.assign(n + 1, 0);
  for (int64_t q = 0; q < nt; ++q) out.rp[Trows[q] + 1] = orp[q + 1] - orp[q];
  for (int64_t i = 0; i < n; ++i) out.rp[i + 1] += out.rp[i];
  for (void *q : {(void *)d_pos, (void *)d_flag, (void *)d_rows, (void *)d_orp, (void *)d_col, (void *)d_val}) hipFree(q);
  return ALFD_OK;
}

// S, the patch operators and lambda_max(D^-1 Aug_SS); A / C / Ct are the host copies of the level-0 operators
static int patch_setup(alfd_ctx *ctx, const HostCsr *A_full, const HostCsr &C, const HostCsr &Ct) {
  alfd_ctx::Patch &Q = ctx->patch;
  const alfd_config &c = ctx->cfg;
  const int64_t n = ctx->n[0];
  std::vector<int32_t> S, Trows, pos(n, -1);
  for (int64_t i = 0; i < n; ++i)
    if (Ct.rp[i + 1] > Ct.rp[i]) {
      pos[i] = (int32_t)S.size();
      S.push_back((int32_t)i);
    }
  const int64_t m = (int64_t)S.size();
  if (m == 0) return ALFD_OK;
  HostCsr A_patch;      // without a host copy of A: only the rows that reach the patch, gathered on the device
  if (!A_full) RC(fetch_patch_rows(ctx, ctx->mat[ALFD_A], pos, A_patch, Trows));
  const HostCsr &A = A_full ? *A_full : A_patch;
  if (A_full) {
    // rows of A with a column in S (the rows E^T-corrections reach): scanned in parallel, kept in order
    const int T = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::vector<int32_t>> part(T);
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
      th.emplace_back([&, t]() {
        for (int64_t i = n * t / T; i < n * (t + 1) / T; ++i) {
          bool hit = false;
          for (int64_t k = A.rp[i]; k < A.rp[i + 1] && !hit; ++k) hit = pos[A.col[k]] >= 0;
          if (hit) part[t].push_back((int32_t)i);
        }
      });
    for (auto &x : th) x.join();
    for (auto &v : part) Trows.insert(Trows.end(), v.begin(), v.end());
  }
  std::vector<int32_t> lam_rows(C.nrows);
  for (int64_t k = 0; k < C.nrows; ++k) lam_rows[k] = (int32_t)k;
  HostCsr h;
  extract_host(A, S, pos.data(), m, false, h);
  RC(upload_level(ctx, Q.Ass, h));
  extract_host(A, S, nullptr, n, false, h);
  RC(upload_level(ctx, Q.As, h));
  extract_host(A, Trows, pos.data(), m, true, h);
  RC(upload_level(ctx, Q.Ats, h));
  extract_host(C, lam_rows, pos.data(), m, false, h);
  RC(upload_level(ctx, Q.Cs, h));
  extract_host(Ct, S, nullptr, Ct.ncols, false, h);
  RC(upload_level(ctx, Q.Cts, h));
  Q.m = m;
  Q.mpad = pad_chunk(m);
  void *q = nullptr;
  HIPC(hipMalloc(&q, m * sizeof(int32_t)));
  ctx->cp_allocs[0].push_back(q);
  Q.S = static_cast<int32_t *>(q);
  HIPC(hipMemcpyAsync(Q.S, S.data(), m * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  for (double **v : {&Q.dinv, &Q.rS, &Q.zS, &Q.uS, &Q.eS, &Q.cd, &Q.cres, &Q.ctmp}) RC(cp_alloc_zero(ctx, 0, v, Q.mpad));
  RC(cp_alloc_zero(ctx, 0, &Q.rr, pad_chunk(n)));
  const unsigned gm = (unsigned)((m + 255) / 256);
  hipLaunchKernelGGL(gather_kernel, dim3(gm), dim3(256), 0, ctx->stream, m, Q.S, ctx->dinv_aug, Q.dinv);
  // lambda_max(D^-1 Aug_SS): power iteration from the integer-hash vector (patch-compact index)
  RC(aug_lambda_max(ctx, patch_aug(ctx), m, 0, Q.rS, Q.zS, &Q.lmax));
  RC(build_tail_mask(ctx, 0, Q.Cts, Q.mpad, &Q.tail_mask));
  HIPC(hipStreamSynchronize(ctx->stream));
  Q.on = true;
  ctx->setup_counts[ALFD_SC_PATCH_BUILDS]++;
  if (c.log_level > 0 && ctx->rank == 0)
    std::fprintf(stderr, "[alfd] interface patch: %lld rows, A[S,S] %lld nnz, %lld rows of A touch it, lambda_max %.3f\n",
                 (long long)m, (long long)Q.Ass.nnz, (long long)Trows.size(), Q.lmax);
  return ALFD_OK;
}

// ------------------------------------------------- sanity checks of the drivers
// cond(C Ct) by unpreconditioned CG (immersed_laplace.cc:987-1010, stokes_immersed_boundary.cc:1157-1180,
// elliptic_interface.cc:986-1009) and the constraint residual (elliptic_interface.cc:973-984).

// A CSR matrix in the plain row-per-lane-group form with a given lane count (no sparse-row list, no window formats)
static int upload_plain(alfd_ctx *ctx, DevCsr &m, const HostCsr &h, int L) {
  csr_free(m);
  m.nrows = m.n_list = h.nrows;
  m.ncols = h.ncols;
  m.n_local_cols = (int32_t)h.ncols;
  m.nnz = h.nnz();
  m.L = L;
  m.longest = 0;
  for (int64_t r = 0; r < h.nrows; ++r) m.longest = std::max(m.longest, h.rp[r + 1] - h.rp[r]);
  m.tag = 1;
  RC(csr_alloc(ctx, m, &m.rp, h.nrows + 1));
  RC(csr_alloc(ctx, m, &m.col, m.nnz));
  RC(csr_alloc(ctx, m, &m.val, m.nnz));
  HIPC(hipMemcpyAsync(m.rp, h.rp.data(), (h.nrows + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  if (m.nnz) {
    HIPC(hipMemcpyAsync(m.col, h.col.data(), m.nnz * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipMemcpyAsync(m.val, h.val.data(), m.nnz * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  }
  HIPC(hipStreamSynchronize(ctx->stream));   // h may go away
  m.present = true;
  return ALFD_OK;
}

static int spectrum_alloc(alfd_ctx *ctx, double **p, int64_t count) {
  void *q = nullptr;
  HIPC(hipMalloc(&q, std::max<int64_t>(count, 1) * sizeof(double)));
  ctx->spec.owned.push_back(q);
  *p = static_cast<double *>(q);
  HIPC(hipMemsetAsync(q, 0, std::max<int64_t>(count, 1) * sizeof(double), ctx->stream));
  return ALFD_OK;
}

// Ct[S,:] and C[:,S]: rows keep their entry order and the lane count of the slot they come from, so C[:,S] (Ct[S,:] x)
// has the bits of the product through the full slots (an empty row of Ct contributes fma(c, 0, acc) there).
static int spectrum_prepare(alfd_ctx *ctx) {
  alfd_ctx::Spectrum &Q = ctx->spec;
  if (Q.Cs) return ALFD_OK;
  const DevCsr &dC = ctx->mat[ALFD_C], &dCt = ctx->mat[ALFD_CT];
  alfd_ctx::Patch &P = ctx->patch;
  const int64_t nl = ctx->n[ctx->nblocks - 1];
  if (P.on && !P.rep && !P.Cs.sparse && !P.Cts.sparse && P.Cs.L == dC.L && P.Cts.L == dCt.L && P.Cs.nnz == dC.nnz &&
      P.Cts.nnz == dCt.nnz) {
    Q.Cs = &P.Cs;
    Q.Cts = &P.Cts;
    Q.m = P.m;
  } else {
    HostCsr C, Ct, h;
    RC(download_csr(ctx, dC, C));
    RC(download_csr(ctx, dCt, Ct));
    std::vector<int32_t> S, pos(Ct.nrows, -1), lam_rows(C.nrows);
    for (int64_t i = 0; i < Ct.nrows; ++i)
      if (Ct.rp[i + 1] > Ct.rp[i]) {
        pos[i] = (int32_t)S.size();
        S.push_back((int32_t)i);
      }
    for (int64_t k = 0; k < C.nrows; ++k) lam_rows[k] = (int32_t)k;
    Q.m = (int64_t)S.size();
    extract_host(C, lam_rows, pos.data(), Q.m, false, h);
    RC(upload_plain(ctx, Q.own_Cs, h, dC.L));
    extract_host(Ct, S, nullptr, Ct.ncols, false, h);
    RC(upload_plain(ctx, Q.own_Cts, h, dCt.L));
    Q.Cs = &Q.own_Cs;
    Q.Cts = &Q.own_Cts;
  }
  const int64_t nlp = pad_chunk(nl);
  RC(spectrum_alloc(ctx, &Q.t, pad_chunk(std::max<int64_t>(Q.m, 1))));
  RC(spectrum_alloc(ctx, &Q.x, nlp));
  RC(spectrum_alloc(ctx, &Q.ones, nlp));
  std::vector<double> one(nl, 1.0);
  if (nl) HIPC(hipMemcpyAsync(Q.ones, one.data(), nl * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  return ALFD_OK;
}

// The device-stepped CG on C Ct (kernels.hpp: spc_*): pcg_mp_device with the identity preconditioner, two gated
// products per iteration and the recording finish.  6 launches per iteration and one mirror launch per group,
// whatever n_u is.  Works on the n_* set (the caller holds it); coef = [alpha_1 .. | beta_1 ..], max_steps each.
static int pcg_cct_device(alfd_ctx *ctx, const alfd_control &ctrl, int *its_out, State *st_out, double *res_out) {
  alfd_ctx::Spectrum &Q = ctx->spec;
  const DevCsr &Cs = *Q.Cs, &Cts = *Q.Cts;
  const int64_t n = ctx->n[ctx->nblocks - 1], npad = pad_chunk(n), nb = npad / kChunk;
  double *r = ctx->n_r, *p = ctx->n_p, *Ap = ctx->n_Ap, *sc = ctx->n_sc, *x = Q.x, *t = Q.t;
  double *part_rr = ctx->n_partial, *part_pap = ctx->n_partial + 2 * ctx->pstride;
  const unsigned grid = (unsigned)nb;
  auto update = [&](int first) {
    Timer tm(ctx, ALFD_T_VEC, first ? 24.0 * npad : 48.0 * npad);
    hipLaunchKernelGGL(spc_update_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, sc, first, part_pap, nb, n, p, Ap, x,
                       r, part_rr);
  };
  auto finish = [&](int step) {
    Timer tm(ctx, ALFD_T_DOT, 16.0 * nb);
    hipLaunchKernelGGL(spc_finish_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, part_rr, part_pap, nb, sc, Q.coef, step,
                       ctrl.kind, ctrl.max_steps, ctrl.tol, ctrl.reduce);
  };
  auto product = [&](const DevCsr &m, const double *in, double *out) {
    Timer tm(ctx, ALFD_T_SPMV_OTHER, m.algorithmic_bytes());
    const int sgrid = grid_for_rows(m.nrows, m.L);
    with_lanes(m.L, [&](auto l) {
      hipLaunchKernelGGL((nmp_spmv_kernel<decltype(l)::value>), dim3(sgrid), dim3(kBlock), 0, ctx->stream, sc, m.nrows, m.rp,
                         m.col, m.val, in, out);
    });
  };
  update(1);
  finish(0);
  HIPC(hipGetLastError());
  int enq = 0;   // iterations enqueued so far
  for (;;) {
    const int group = std::max(1, ctx->spec_group);
    for (int g = 0; g < group && enq < ctrl.max_steps; ++g) {
      const int it = ++enq;
      {
        Timer tm(ctx, ALFD_T_VEC, it == 1 ? 16.0 * npad : 24.0 * npad);
        hipLaunchKernelGGL(nmp_p_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, sc, it == 1 ? 1 : 0, r, p);
      }
      product(Cts, p, t);
      product(Cs, t, Ap);
      {
        Timer tm(ctx, ALFD_T_DOT, 16.0 * npad);
        hipLaunchKernelGGL(nmp_dot_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, sc, p, Ap, part_pap);
      }
      update(0);
      finish(it);
    }
    HIPC(hipGetLastError());
    {
      Timer tm(ctx, ALFD_T_DOT, 8.0 * (S_NRTOL + 1));
      hipLaunchKernelGGL(mirror_scalars_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, sc, ctx->n_sc_host, (int)(S_NRTOL + 1));
    }
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(ctx->stream));
    const double *h = ctx->n_sc_host;
    if (h[S_NSTATE] != 0.0) {
      *its_out = (int)h[S_NSTEP];
      *st_out = h[S_NSTATE] == 1.0 ? SUCCESS : FAILURE;
      *res_out = std::sqrt(h[S_RR]);
      return ALFD_OK;
    }
    if (enq >= ctrl.max_steps) return ctx->err = "CG on C Ct: the device stop rule did not end the solve", ALFD_E_INVALID;
  }
}

// Extreme eigenvalues of the CG-Lanczos matrix T_k (alfd.h) by Sturm-count bisection down to neighbouring doubles.
static int host_tridiagonal_extremes(int32_t k, const double *alpha, const double *beta, double *lmin, double *lmax) {
  if (k < 1 || !alpha || !lmin || !lmax || (k > 1 && !beta)) return ALFD_E_INVALID;
  for (int32_t j = 0; j < k; ++j)
    if (!std::isfinite(alpha[j]) || !(alpha[j] > 0.0)) return ALFD_E_INVALID;
  for (int32_t j = 0; j + 1 < k; ++j)
    if (!std::isfinite(beta[j]) || beta[j] < 0.0) return ALFD_E_INVALID;
  if (k == 1) {
    *lmin = *lmax = 1.0 / alpha[0];
    return ALFD_OK;
  }
  std::vector<double> d(k), e2(k, 0.0);   // diagonal; e2[j] = eta_{j+1}^2 couples rows j and j + 1
  double glo = 0, ghi = 0, emax = 0;
  for (int32_t j = 0; j < k; ++j) d[j] = 1.0 / alpha[j] + (j > 0 ? beta[j - 1] / alpha[j - 1] : 0.0);
  std::vector<double> e(k, 0.0);
  for (int32_t j = 0; j + 1 < k; ++j) {
    e[j] = std::sqrt(beta[j]) / alpha[j];
    e2[j] = e[j] * e[j];
    emax = std::max(emax, e2[j]);
  }
  for (int32_t j = 0; j < k; ++j) {
    const double rad = (j > 0 ? e[j - 1] : 0.0) + e[j];
    if (!std::isfinite(d[j]) || !std::isfinite(rad) || !std::isfinite(e2[j])) return ALFD_E_INVALID;
    glo = j == 0 ? d[j] - rad : std::min(glo, d[j] - rad);
    ghi = j == 0 ? d[j] + rad : std::max(ghi, d[j] + rad);
  }
  const double pivmin = std::numeric_limits<double>::min() * std::max(1.0, emax);
  auto count_below = [&](double x) {   // number of eigenvalues of T_k below x
    int32_t c = 0;
    double q = d[0] - x;
    for (int32_t j = 0;; ++j) {
      if (std::fabs(q) < pivmin) q = -pivmin;
      if (q < 0.0) ++c;
      if (j + 1 == k) return c;
      q = d[j + 1] - x - e2[j] / q;
    }
  };
  const double norm = std::max(std::fabs(glo), std::fabs(ghi));
  const double wlo = glo - 1e-12 * norm - pivmin, whi = ghi + 1e-12 * norm + pivmin;   // count(wlo) = 0, count(whi) = k
  auto bisect = [&](int32_t want) {   // the largest x with count_below(x) < want, between neighbouring doubles
    double lo = wlo, hi = whi;
    for (;;) {
      const double mid = lo + 0.5 * (hi - lo);
      if (!(mid > lo) || !(mid < hi)) return lo;
      if (count_below(mid) >= want) hi = mid;
      else lo = mid;
    }
  };
  *lmin = bisect(1);
  *lmax = bisect(k);
  return ALFD_OK;
}

static int estimate_spectrum(alfd_ctx *ctx, const alfd_control &ctrl, alfd_spectrum *out) {
  alfd_ctx::Spectrum &Q = ctx->spec;
  RC(spectrum_prepare(ctx));
  Q.have = false;
  Q.alpha.clear();
  Q.beta.clear();
  int its = 0;
  State st = FAILURE;
  // r_0 = 1 on n_lambda rows: its canonical sum of squares is the integer n_lambda, exactly, in any order
  const double res0 = std::sqrt((double)ctx->n[ctx->nblocks - 1]);
  double res = 0;
  RC(nested_claim(ctx, NESTED_CCT));
  int rc;
  if (!ctx->spec_host_stepped) {
    rc = ALFD_OK;
    if (Q.coef_cap < 2 * (int64_t)ctrl.max_steps) {
      rc = spectrum_alloc(ctx, &Q.coef, 2 * (int64_t)ctrl.max_steps);
      if (rc == ALFD_OK) Q.coef_cap = 2 * (int64_t)ctrl.max_steps;
    }
    if (rc == ALFD_OK) rc = pcg_cct_device(ctx, ctrl, &its, &st, &res);
    if (rc == ALFD_OK && its > 0) {
      Q.alpha.resize(its);
      Q.beta.resize(its - 1);
      hipError_t e = hipMemcpyAsync(Q.alpha.data(), Q.coef, its * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess && its > 1)
        e = hipMemcpyAsync(Q.beta.data(), Q.coef + ctrl.max_steps, (its - 1) * sizeof(double), hipMemcpyDeviceToHost,
                           ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
      if (e != hipSuccess) ctx->err = std::string("coefficient readback: ") + hipGetErrorString(e), rc = ALFD_E_HIP;
    }
  } else {
    CgRecord rec;
    nested_swap_ws(ctx);
    rc = pcg(ctx, OP_CCT, ALFD_PREC_IDENTITY, ctrl, Q.ones, Q.x, &its, &st, &res, &rec);
    nested_swap_ws(ctx);
    Q.alpha = std::move(rec.alpha);
    Q.beta = std::move(rec.beta);
  }
  ctx->n_owner = NESTED_FREE;
  flush_timers(ctx);
  if (rc != ALFD_OK) return rc;
  Q.have = true;
  std::memset(out, 0, sizeof(*out));
  out->converged = st == SUCCESS ? 1 : 0;
  out->steps = its;
  out->initial_residual = res0;
  out->last_residual = its == 0 ? res0 : res;
  out->lambda_min = out->lambda_max = out->condition = std::nan("");
  if (its == 0) {
    if (st == SUCCESS) return ALFD_OK;   // the start already met the stop rule: nothing to estimate from
    return ctx->err = "CG on C Ct broke down in its first step (p.Ap <= 0): no estimate", ALFD_E_BREAKDOWN;
  }
  if (host_tridiagonal_extremes(its, Q.alpha.data(), Q.beta.data(), &out->lambda_min, &out->lambda_max) != ALFD_OK)
    return ctx->err = "CG on C Ct: non-finite coefficients, no estimate", ALFD_E_BREAKDOWN;
  out->condition = out->lambda_max / out->lambda_min;
  if (ctx->cfg.log_level >= 1 && ctx->rank == 0) {
    std::printf("Condition number estimate: %g\n", out->condition);
    std::fflush(stdout);
    if (!out->converged) std::fprintf(stderr, "***CCt solve not successfull (see condition number above)***\n");
  }
  return ALFD_OK;
}

static int to_device(alfd_ctx *ctx, const double *const *blocks, double *dev);
// || (last block row of AA) x - g ||_inf: the last block of system_apply (same launches), then the two-stage max
static int constraint_residual(alfd_ctx *ctx, const double *const *x_blocks, const double *g, double *linf) {
  alfd_ctx::Spectrum &Q = ctx->spec;
  const int last = ctx->nblocks - 1;
  const int64_t n = ctx->n[last], nb = pad_chunk(n) / kChunk;
  if (!Q.linf) RC(spectrum_alloc(ctx, &Q.linf, nb + 1 + pad_chunk(n)));
  double *part = Q.linf + 1, *dg = Q.linf + 1 + nb;
  RC(to_device(ctx, x_blocks, ctx->st_in));
  HIPC(hipMemsetAsync(ctx->st_out, 0, ctx->ntot() * sizeof(double), ctx->stream));
  const double *x = ctx->st_in;
  double *y = ctx->st_out + ctx->off[last];
  RC(spmv(ctx, ALFD_C, x + ctx->off[0], y, 0));
  if (is_elliptic(ctx->cfg.variant)) RC(spmv(ctx, ALFD_M, x + ctx->off[1], y, 1, -1.0));   // y2 = C x0 - M x1
  if (g && n) HIPC(hipMemcpyAsync(dg, g, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (nb > 0) {
    Timer tm(ctx, ALFD_T_VEC, (g ? 16.0 : 8.0) * n);
    hipLaunchKernelGGL(linf_diff_partial_kernel, dim3((unsigned)nb), dim3(kBlock), 0, ctx->stream, n, y,
                       g ? dg : (const double *)nullptr, part);
  }
  hipLaunchKernelGGL(linf_final_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, part, nb, Q.linf);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(linf, Q.linf, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  return ALFD_OK;
}

// Explicit inverse of the coarsest Aug_c = A_c + gamma Ct_c W^-1 C_c: dense Cholesky on the host, every entry a
// sequential fma chain (the oracle repeats the loops), uploaded as a dense CSR so that z = Aug_c^-1 r runs in
// the canonical SpMV order.  ML solves its coarsest level directly as well (KLU, utilities.h:304-317).
static int coarse_inverse(alfd_ctx *ctx, const HostCsr &A, const HostCsr &C, const HostCsr &Ct, const std::vector<double> &w,
                          double gamma, DevCsr &inv) {
  const int64_t n = A.nrows;
  std::vector<double> D((size_t)n * n, 0.0);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t k = A.rp[i]; k < A.rp[i + 1]; ++k) D[i * n + A.col[k]] = A.val[k];
  if (!ctx->cfg.aug_assembled)
    for (int64_t i = 0; i < n; ++i)
      for (int64_t k = Ct.rp[i]; k < Ct.rp[i + 1]; ++k) {
        const int64_t lam = Ct.col[k];
        const double sfac = (gamma * w[lam]) * Ct.val[k];
        for (int64_t e = C.rp[lam]; e < C.rp[lam + 1]; ++e)
          D[i * n + C.col[e]] = std::fma(sfac, C.val[e], D[i * n + C.col[e]]);
      }
  const int T = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  auto par_for = [&](int64_t lo, int64_t hi, const std::function<void(int64_t)> &body) {
    if (hi - lo < 256) {
      for (int64_t i = lo; i < hi; ++i) body(i);
      return;
    }
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
      th.emplace_back([&, t]() {
        for (int64_t i = lo + (hi - lo) * t / T; i < lo + (hi - lo) * (t + 1) / T; ++i) body(i);
      });
    for (auto &x : th) x.join();
  };
  for (int64_t j = 0; j < n; ++j) {
    double d = D[j * n + j];
    for (int64_t k = 0; k < j; ++k) d = std::fma(-D[j * n + k], D[j * n + k], d);
    if (!(d > 0.0)) return ctx->err = "coarsest multigrid operator is not positive definite", ALFD_E_BREAKDOWN;
    const double ljj = std::sqrt(d);
    D[j * n + j] = ljj;
    par_for(j + 1, n, [&](int64_t i) {
      double sacc = D[i * n + j];
      for (int64_t k = 0; k < j; ++k) sacc = std::fma(-D[i * n + k], D[j * n + k], sacc);
      D[i * n + j] = sacc / ljj;
    });
  }
  HostCsr X;
  X.nrows = X.ncols = n;
  X.rp.resize(n + 1);
  X.col.resize((size_t)n * n);
  X.val.assign((size_t)n * n, 0.0);
  for (int64_t i = 0; i <= n; ++i) X.rp[i] = i * n;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < n; ++j) X.col[i * n + j] = (int32_t)j;
  {
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
      th.emplace_back([&, t]() {
        std::vector<double> y(n), x(n);
        for (int64_t c = n * t / T; c < n * (t + 1) / T; ++c) {
          std::fill(y.begin(), y.end(), 0.0);
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
          for (int64_t i = 0; i < n; ++i) X.val[i * n + c] = x[i];
        }
      });
    for (auto &x : th) x.join();
  }
  RC(upload_level_part(ctx, inv, X, nullptr, true));   // never partitioned: every rank that has it has it whole
  return ALFD_OK;
}

// Aggregate ids over the LOCAL index space [owned | halo] of a matrix' column space:
// the owned part is given, the halo part is fetched from the owners through the
// matrix' own halo plan (ids travel as exactly representable doubles).
static int exchange_ids(alfd_ctx *ctx, DevCsr &m, const std::vector<int32_t> &owned, std::vector<int32_t> &all) {
  all.assign(owned.begin(), owned.end());
  if (ctx->nranks == 1) return ALFD_OK;
  std::vector<double> v(owned.begin(), owned.end());
  double *d = nullptr;
  HIPC(hipMalloc((void **)&d, std::max<size_t>(v.size(), 1) * sizeof(double)));
  HIPC(hipMemcpyAsync(d, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  int rc = ALFD_OK;
  if (ctx->local || ctx->host_alltoallv || m.n_halo > 0 || m.send_off.back() > 0) rc = halo_exchange(ctx, m, d);
  if (rc == ALFD_OK && m.n_halo > 0) {
    std::vector<double> h(m.n_halo);
    hipMemcpyAsync(h.data(), m.halo, m.n_halo * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    hipStreamSynchronize(ctx->stream);
    for (double x : h) all.push_back((int32_t)x);
  }
  hipStreamSynchronize(ctx->stream);
  hipFree(d);
  return rc;
}

static int upload_level_part(alfd_ctx *ctx, DevCsr &dst, const HostCsr &h, const int64_t *col_offsets,
                             bool local_only) {
  ctx->up_col_offsets = col_offsets;
  ctx->up_local_only = local_only;
  const int rc = upload_level(ctx, dst, h);
  ctx->up_col_offsets = nullptr;
  ctx->up_local_only = false;
  return rc;
}

// All ranks contribute `bytes` bytes (sizes may differ); out = the contributions in rank order.
static int allgather_bytes(alfd_ctx *ctx, const void *data, size_t bytes, std::vector<char> &out,
                           std::vector<size_t> &sizes) {
  const int P = ctx->nranks;
  int64_t mine = (int64_t)bytes;
  std::vector<int64_t> all(P);
  int64_t *d_m = nullptr, *d_a = nullptr;
  HIPC(hipMalloc((void **)&d_m, sizeof(int64_t)));
  HIPC(hipMalloc((void **)&d_a, sizeof(int64_t) * P));
  HIPC(hipMemcpyAsync(d_m, &mine, sizeof(mine), hipMemcpyHostToDevice, ctx->stream));
  int rc = comm_allgather(ctx, d_m, d_a, sizeof(int64_t));
  if (rc == ALFD_OK) {
    hipMemcpyAsync(all.data(), d_a, sizeof(int64_t) * P, hipMemcpyDeviceToHost, ctx->stream);
    hipStreamSynchronize(ctx->stream);
  }
  hipFree(d_m);
  hipFree(d_a);
  if (rc != ALFD_OK) return rc;
  size_t maxb = 8;
  sizes.assign(P, 0);
  for (int p = 0; p < P; ++p) {
    sizes[p] = (size_t)all[p];
    maxb = std::max(maxb, (sizes[p] + 7) / 8 * 8);
  }
  char *d_s = nullptr, *d_r = nullptr;
  HIPC(hipMalloc((void **)&d_s, maxb));
  HIPC(hipMalloc((void **)&d_r, maxb * P));
  HIPC(hipMemsetAsync(d_s, 0, maxb, ctx->stream));
  if (bytes) HIPC(hipMemcpyAsync(d_s, data, bytes, hipMemcpyHostToDevice, ctx->stream));
  rc = comm_allgather(ctx, d_s, d_r, maxb);
  std::vector<char> stage(maxb * P);
  if (rc == ALFD_OK) {
    hipMemcpyAsync(stage.data(), d_r, stage.size(), hipMemcpyDeviceToHost, ctx->stream);
    hipStreamSynchronize(ctx->stream);
  }
  hipFree(d_s);
  hipFree(d_r);
  if (rc != ALFD_OK) return rc;
  out.clear();
  for (int p = 0; p < P; ++p) out.insert(out.end(), stage.begin() + p * maxb, stage.begin() + p * maxb + sizes[p]);
  return ALFD_OK;
}

// Global CSR (rows of all ranks in rank order) from every rank's local rows.  shift: per-rank
// amount added to the column ids of that rank's piece (rank-local ids -> global), or nullptr.
static int gather_csr(alfd_ctx *ctx, const HostCsr &loc, const int64_t *shift, int64_t ncols_global, HostCsr &g) {
  std::vector<int32_t> len(loc.nrows);
  for (int64_t r = 0; r < loc.nrows; ++r) len[r] = (int32_t)(loc.rp[r + 1] - loc.rp[r]);
  std::vector<char> blen, bcol, bval;
  std::vector<size_t> slen, scol, sval;
  RC(allgather_bytes(ctx, len.data(), len.size() * 4, blen, slen));
  RC(allgather_bytes(ctx, loc.col.data(), (size_t)loc.nnz() * 4, bcol, scol));
  RC(allgather_bytes(ctx, loc.val.data(), (size_t)loc.nnz() * 8, bval, sval));
  const int64_t nrows = (int64_t)(blen.size() / 4), nnz = (int64_t)(bcol.size() / 4);
  g.nrows = nrows;
  g.ncols = ncols_global;
  g.rp.assign(nrows + 1, 0);
  const int32_t *gl = reinterpret_cast<const int32_t *>(blen.data());
  for (int64_t r = 0; r < nrows; ++r) g.rp[r + 1] = g.rp[r] + gl[r];
  g.col.resize(nnz);
  g.val.resize(nnz);
  std::memcpy(g.col.data(), bcol.data(), (size_t)nnz * 4);
  std::memcpy(g.val.data(), bval.data(), (size_t)nnz * 8);
  if (g.rp[nrows] != nnz) return ctx->err = "gather_csr: inconsistent pieces", ALFD_E_COMM;
  if (shift) {
    int64_t k = 0;
    for (int p = 0; p < ctx->nranks; ++p) {
      const int64_t np = (int64_t)(scol[p] / 4);
      for (int64_t q = 0; q < np; ++q) g.col[k + q] = (int32_t)(g.col[k + q] + shift[p]);
      k += np;
    }
  }
  return ALFD_OK;
}

// device vector pieces (n_local each, rank order) -> global device vector on every rank
static int gather_vec(alfd_ctx *ctx, const double *d_local, int64_t n_local, double *d_global) {
  std::vector<double> h(n_local);
  HIPC(hipMemcpyAsync(h.data(), d_local, n_local * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  std::vector<char> out;
  std::vector<size_t> sizes;
  RC(allgather_bytes(ctx, h.data(), h.size() * 8, out, sizes));
  HIPC(hipMemcpyAsync(d_global, out.data(), out.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  return ALFD_OK;
}

// ---------------------------------------------------------------------------
// Algebraic aggregation (alfd_build_aggregates): the counterpart of ML's uncoupled aggregation
// (utilities.h:304-317: aggregation_threshold, constant modes per component) for operators that
// come without grid information -- a matrix replayed from an .alfd file, a locally refined mesh
// with hanging-node rows.  Unknowns are taken node-major with `bs` components per node.  Per
// level: node graph with w_IJ = max |a_ij| over the bs x bs block, strong if
// w_IJ >= theta sqrt(d_I d_J) (d = max |a_ii| of the node); rows that hold only their diagonal
// (Dirichlet / constrained rows) stay out (-1).  Greedy passes in natural order (deterministic):
// (1) a free node whose strong neighbours are all free founds an aggregate with its strongest
// free neighbours (at most max_size nodes); (2) leftovers join the founded aggregate they are most
// strongly tied to; (3) what is still free founds aggregates of its own.  The next level's graph
// is that of the Galerkin product with the piecewise-constant prolongator.
// The node graph of one level, in two steps so that a row-partitioned context can form the rows of its own nodes
// (sa_node_diag_kernel / sa_node_graph_kernel compute the same bits on the device; max and fabs are exact):
//   node_diag_host:  d_I = max |a_ii| and the fixed flag of the nodes of A's rows.  A holds the rows [row0, row0 +
//                    A.nrows) of the level's operator with GLOBAL column ids; d / fixed are indexed by local node.
//   node_graph_host: per local node the strong neighbours J ascending with w_IJ = max |a_ij|; d / fixed of ALL nodes
//                    (nn of them), neighbours as global node ids.
static void node_diag_host(const HostCsr &A, int64_t row0, int bs, std::vector<double> &d, std::vector<int32_t> &fixed) {
  const int64_t nl = A.nrows / bs;
  d.assign(nl, 0.0);
  fixed.assign(nl, 1);
  for (int64_t i = 0; i < nl * bs; ++i) {
    const int64_t I = i / bs;
    for (int64_t k = A.rp[i]; k < A.rp[i + 1]; ++k) {
      if (A.col[k] == row0 + i) d[I] = std::max(d[I], std::fabs(A.val[k]));
      else if (A.val[k] != 0.0) fixed[I] = 0;
    }
  }
}

static void node_graph_host(const HostCsr &A, int64_t row0, int bs, double theta, int64_t nn, const double *d,
                            const int32_t *fixed, std::vector<int64_t> &gp, std::vector<int32_t> &gc,
                            std::vector<double> &gw) {
  const int64_t nl = A.nrows / bs, node0 = row0 / bs;
  gp.assign(nl + 1, 0);
  gc.clear();
  gw.clear();
  std::vector<double> w(nn, 0.0);
  std::vector<int32_t> touched;
  for (int64_t Il = 0; Il < nl; ++Il) {
    const int64_t I = node0 + Il;
    touched.clear();
    if (!fixed[I])
      for (int64_t i = Il * bs; i < (Il + 1) * bs; ++i)
        for (int64_t k = A.rp[i]; k < A.rp[i + 1]; ++k) {
          const int64_t J = A.col[k] / bs;
          if (J == I || J >= nn || fixed[J]) continue;
          const double v = std::fabs(A.val[k]);
          if (v == 0.0) continue;
          if (w[J] == 0.0) touched.push_back((int32_t)J);
          w[J] = std::max(w[J], v);
        }
    std::sort(touched.begin(), touched.end());
    for (int32_t J : touched) {
      if (w[J] >= theta * std::sqrt(d[I] * d[J])) {
        gc.push_back(J);
        gw.push_back(w[J]);
      }
      w[J] = 0.0;
    }
    gp[Il + 1] = (int64_t)gc.size();
  }
}

// The three greedy passes over a node graph (nn nodes, strong edges gp / gc / gw, the fixed flags); agg gets n entries.
static void aggregate_graph(int64_t n, int64_t nn, int bs, int max_size, const int32_t *fixed, const int64_t *gp,
                            const int32_t *gc, const double *gw, std::vector<int32_t> &agg, int64_t &n_coarse) {
  std::vector<int32_t> na(nn, -1);  // node -> aggregate
  int32_t nagg = 0;
  std::vector<std::pair<double, int32_t>> cand;
  // pass 1
  for (int64_t I = 0; I < nn; ++I) {
    if (fixed[I] || na[I] >= 0) continue;
    bool all_free = true;
    for (int64_t k = gp[I]; k < gp[I + 1] && all_free; ++k) all_free = na[gc[k]] < 0;
    if (!all_free) continue;
    cand.clear();
    for (int64_t k = gp[I]; k < gp[I + 1]; ++k) cand.emplace_back(-gw[k], gc[k]);
    std::sort(cand.begin(), cand.end());   // strongest first, ties by node id
    na[I] = nagg;
    for (size_t q = 0; q < cand.size() && (int)q + 1 < max_size; ++q) na[cand[q].second] = nagg;
    ++nagg;
  }
  // pass 2: join the most strongly tied aggregate of pass 1
  const int32_t nagg1 = nagg;
  std::vector<int32_t> join(nn, -1);
  for (int64_t I = 0; I < nn; ++I) {
    if (fixed[I] || na[I] >= 0) continue;
    double best = 0.0;
    for (int64_t k = gp[I]; k < gp[I + 1]; ++k) {
      const int32_t a = na[gc[k]];
      if (a >= 0 && a < nagg1 && gw[k] > best) best = gw[k], join[I] = a;
    }
  }
  for (int64_t I = 0; I < nn; ++I)
    if (join[I] >= 0) na[I] = join[I];
  // pass 3: the rest founds its own aggregates (with whatever free strong neighbours are left)
  for (int64_t I = 0; I < nn; ++I) {
    if (fixed[I] || na[I] >= 0) continue;
    na[I] = nagg;
    int taken = 1;
    for (int64_t k = gp[I]; k < gp[I + 1] && taken < max_size; ++k)
      if (na[gc[k]] < 0) na[gc[k]] = nagg, ++taken;
    ++nagg;
  }
  agg.assign(n, -1);
  for (int64_t i = 0; i < nn * bs; ++i)
    if (na[i / bs] >= 0) agg[i] = (int32_t)(na[i / bs] * bs + i % bs);
  n_coarse = (int64_t)nagg * bs;
}

static void aggregate_level(const HostCsr &A, int bs, double theta, int max_size, std::vector<int32_t> &agg,
                            int64_t &n_coarse) {
  const int64_t nn = A.nrows / bs;
  std::vector<double> d, gw;
  std::vector<int32_t> fixed, gc;
  std::vector<int64_t> gp;
  node_diag_host(A, 0, bs, d, fixed);
  node_graph_host(A, 0, bs, theta, nn, d.data(), fixed.data(), gp, gc, gw);
  aggregate_graph(A.nrows, nn, bs, max_size, fixed.data(), gp.data(), gc.data(), gw.data(), agg, n_coarse);
}

// Every rank contributes the status of its local phase; all return the first non-zero one (rank order), so that no rank
// runs into the next collective while a peer has left (*any_flag: some rank raised `flag`).
static int joint_status(alfd_ctx *ctx, int local, int flag, int *any_flag) {
  if (any_flag) *any_flag = flag;
  if (ctx->nranks == 1) return local;
  const int64_t mine[2] = {local, flag};
  std::vector<char> all;
  std::vector<size_t> sz;
  const std::string keep = ctx->err;
  const int rc = allgather_bytes(ctx, mine, sizeof(mine), all, sz);
  if (rc != ALFD_OK) return rc;
  int first = ALFD_OK, who = -1;
  for (int p = 0; p < ctx->nranks; ++p) {
    int64_t v[2];
    std::memcpy(v, all.data() + (size_t)p * sizeof(mine), sizeof(mine));
    if (first == ALFD_OK && v[0] != ALFD_OK) first = (int)v[0], who = p;
    if (any_flag && v[1]) *any_flag = 1;
  }
  if (first != ALFD_OK && who != ctx->rank) ctx->err = "rank " + std::to_string(who) + " failed in a collective build step";
  else ctx->err = keep;
  return first;
}

// The node graph of slot A's resident rows on the device (sa_node_diag_kernel, sa_node_graph_kernel); collective on a
// partitioned context: d and the fixed flags of all nodes are all-gathered (one double and one int per node), nothing
// else moves and A is not downloaded.  A node with more than kNgMaxOut neighbour nodes on ANY rank sends all ranks to
// node_graph_host on their downloaded rows (same bits).
static int strength_graph_dev(alfd_ctx *ctx, int bs, double theta) {
  alfd_ctx::StrengthGraph &G = ctx->sg;
  G = alfd_ctx::StrengthGraph();
  const DevCsr &A = ctx->mat[ALFD_A];
  const int P = ctx->nranks, rk = ctx->rank;
  const int64_t row0 = P > 1 ? ctx->part[0][rk] : 0, N = P > 1 ? ctx->part[0].back() : A.nrows;
  const int64_t nl = A.nrows / bs, nn = N / bs, node0 = row0 / bs;
  const int32_t nlc = P > 1 ? A.n_local_cols : (int32_t)A.ncols;
  int32_t *d_halo = nullptr, *d_fl = nullptr, *d_fg = nullptr, *d_cnt = nullptr, *d_ovf = nullptr, *d_gc = nullptr;
  double *d_dl = nullptr, *d_dg = nullptr, *d_gw = nullptr;
  int64_t *d_gp = nullptr;
  auto release = [&]() {
    for (void *p : {(void *)d_halo, (void *)d_fl, (void *)d_fg, (void *)d_cnt, (void *)d_ovf, (void *)d_gc, (void *)d_dl,
                    (void *)d_dg, (void *)d_gw, (void *)d_gp})
      if (p) hipFree(p);
  };
  auto hip = [&](hipError_t e) -> int {
    if (e == hipSuccess) return ALFD_OK;
    ctx->err = std::string("HIP error in the strength graph: ") + hipGetErrorString(e);
    return (int)ALFD_E_HIP;
  };
#define SG(call)                     \
  do {                               \
    const int rc__ = hip(call);      \
    if (rc__ != ALFD_OK) return rc__; \
  } while (0)
  std::vector<double> dl(nl);
  std::vector<int32_t> fl(nl);
  // ---- phase 1 (local): d and the fixed flags of the own nodes
  auto phase1 = [&]() -> int {
    if (!A.halo_globals.empty()) {
      SG(hipMalloc((void **)&d_halo, A.halo_globals.size() * sizeof(int32_t)));
      SG(hipMemcpyAsync(d_halo, A.halo_globals.data(), A.halo_globals.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                        ctx->stream));
    }
    SG(hipMalloc((void **)&d_dl, std::max<int64_t>(nl, 1) * sizeof(double)));
    SG(hipMalloc((void **)&d_fl, std::max<int64_t>(nl, 1) * sizeof(int32_t)));
    if (nl > 0) {
      hipLaunchKernelGGL(sa_node_diag_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, ctx->stream, nl, bs, node0,
                         A.rp, A.col, A.val, nlc, row0, d_halo, d_dl, d_fl);
      SG(hipGetLastError());
      SG(hipMemcpyAsync(dl.data(), d_dl, nl * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      SG(hipMemcpyAsync(fl.data(), d_fl, nl * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    SG(hipStreamSynchronize(ctx->stream));
    return ALFD_OK;
  };
  int rc = joint_status(ctx, phase1(), 0, nullptr);
  if (rc != ALFD_OK) return release(), rc;
  // ---- d / fixed of all nodes
  std::vector<double> dg;
  std::vector<int32_t> fg;
  if (P == 1) {
    dg = dl;
    fg = fl;
  } else {
    std::vector<char> bd, bf;
    std::vector<size_t> sz;
    rc = allgather_bytes(ctx, dl.data(), dl.size() * sizeof(double), bd, sz);
    if (rc == ALFD_OK) rc = allgather_bytes(ctx, fl.data(), fl.size() * sizeof(int32_t), bf, sz);
    if (rc != ALFD_OK) return release(), rc;      // a failed transport fails on every rank
    if ((int64_t)(bd.size() / sizeof(double)) != nn || (int64_t)(bf.size() / sizeof(int32_t)) != nn)
      return release(), ctx->err = "alfd_build_strength_graph: the ranks' rows of A do not add up to the partition", ALFD_E_COMM;
    dg.resize(nn);
    fg.resize(nn);
    std::memcpy(dg.data(), bd.data(), bd.size());
    std::memcpy(fg.data(), bf.data(), bf.size());
  }
  // ---- phase 2 (local): count the strong neighbours of every own node
  std::vector<int32_t> hc(nl);
  int32_t hovf = 0;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(nl, 256 * 64));
  auto launch = [&](int pass) {
    hipLaunchKernelGGL(sa_node_graph_kernel, dim3(grid), dim3(64), 0, ctx->stream, nl, node0, nn, bs, theta, A.rp, A.col,
                       A.val, nlc, row0, d_halo, d_dg, d_fg, pass, d_cnt, d_gp, d_gc, d_gw, d_ovf);
  };
  auto phase2 = [&]() -> int {
    SG(hipMalloc((void **)&d_dg, std::max<int64_t>(nn, 1) * sizeof(double)));
    SG(hipMalloc((void **)&d_fg, std::max<int64_t>(nn, 1) * sizeof(int32_t)));
    SG(hipMalloc((void **)&d_cnt, std::max<int64_t>(nl, 1) * sizeof(int32_t)));
    SG(hipMalloc((void **)&d_ovf, sizeof(int32_t)));
    SG(hipMalloc((void **)&d_gp, (nl + 1) * sizeof(int64_t)));
    SG(hipMemcpyAsync(d_dg, dg.data(), nn * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    SG(hipMemcpyAsync(d_fg, fg.data(), nn * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    SG(hipMemsetAsync(d_ovf, 0, sizeof(int32_t), ctx->stream));
    if (nl > 0) {
      launch(0);
      SG(hipGetLastError());
      SG(hipMemcpyAsync(hc.data(), d_cnt, nl * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    SG(hipMemcpyAsync(&hovf, d_ovf, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SG(hipStreamSynchronize(ctx->stream));
    return ALFD_OK;
  };
  int any_ovf = 0;
  {
    const int loc = phase2();
    rc = joint_status(ctx, loc, hovf, &any_ovf);
  }
  if (rc != ALFD_OK) return release(), rc;
  // ---- phase 3 (local): fill, or all ranks on the host
  auto phase3 = [&]() -> int {
    if (any_ovf) {
      HostCsr h;
      RC(download_csr(ctx, A, h));
      for (size_t k = 0; k < h.col.size(); ++k)
        h.col[k] = (int32_t)(h.col[k] < nlc ? row0 + h.col[k] : A.halo_globals[h.col[k] - nlc]);
      node_graph_host(h, row0, bs, theta, nn, dg.data(), fg.data(), G.gp, G.gc, G.gw);
      return ALFD_OK;
    }
    G.gp.assign(nl + 1, 0);
    for (int64_t I = 0; I < nl; ++I) G.gp[I + 1] = G.gp[I] + hc[I];
    const int64_t nnz = G.gp[nl];
    G.gc.resize(nnz);
    G.gw.resize(nnz);
    SG(hipMalloc((void **)&d_gc, std::max<int64_t>(nnz, 1) * sizeof(int32_t)));
    SG(hipMalloc((void **)&d_gw, std::max<int64_t>(nnz, 1) * sizeof(double)));
    SG(hipMemcpyAsync(d_gp, G.gp.data(), (nl + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    if (nl > 0) {
      launch(1);
      SG(hipGetLastError());
    }
    if (nnz > 0) {
      SG(hipMemcpyAsync(G.gc.data(), d_gc, nnz * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
      SG(hipMemcpyAsync(G.gw.data(), d_gw, nnz * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    SG(hipStreamSynchronize(ctx->stream));
    return ALFD_OK;
  };
  rc = joint_status(ctx, phase3(), 0, nullptr);
#undef SG
  release();
  if (rc != ALFD_OK) return G = alfd_ctx::StrengthGraph(), rc;
  G.have = true;
  G.on_device = !any_ovf;
  G.n_nodes = nl;
  G.node0 = node0;
  G.d = dl;
  G.fixed = fl;
  return ALFD_OK;
}

// Rows of a row-partitioned CSR matrix (this rank holds the global rows [row_off[rank], row_off[rank + 1]) as `loc`,
// any column space) for an arbitrary list of GLOBAL row ids: out gets one row per entry of `want`, in that order.
// Collective (setup only): requests and answers travel through all-gathers, so every rank sees all of them.
static int fetch_rows(alfd_ctx *ctx, const HostCsr &loc, const int64_t *row_off, const std::vector<int64_t> &want,
                      HostCsr &out) {
  const int P = ctx->nranks, me = ctx->rank;
  std::vector<char> breq, bans;
  std::vector<size_t> sreq, sans;
  RC(allgather_bytes(ctx, want.data(), want.size() * sizeof(int64_t), breq, sreq));
  std::vector<std::vector<int64_t>> req(P);
  {
    size_t pos = 0;
    for (int p = 0; p < P; ++p) {
      req[p].resize(sreq[p] / sizeof(int64_t));
      std::memcpy(req[p].data(), breq.data() + pos, sreq[p]);
      pos += sreq[p];
    }
  }
  // my answers: for every requester, the rows I own in its request order: int64 len, int32 cols (padded to 8), double vals
  std::vector<char> ans;
  auto put = [&](const void *q, size_t n) { ans.insert(ans.end(), (const char *)q, (const char *)q + n); };
  for (int p = 0; p < P; ++p)
    for (int64_t g : req[p]) {
      if (g < row_off[me] || g >= row_off[me + 1]) continue;
      const int64_t i = g - row_off[me], k0 = loc.rp[i], len = loc.rp[i + 1] - k0;
      put(&len, 8);
      put(loc.col.data() + k0, (size_t)len * 4);
      if (len & 1) {
        const int32_t z = 0;
        put(&z, 4);
      }
      put(loc.val.data() + k0, (size_t)len * 8);
    }
  RC(allgather_bytes(ctx, ans.data(), ans.size(), bans, sans));
  out.nrows = (int64_t)want.size();
  out.ncols = loc.ncols;
  out.rp.assign(1, 0);
  out.col.clear();
  out.val.clear();
  std::vector<size_t> base(P + 1, 0);
  for (int o = 0; o < P; ++o) base[o + 1] = base[o] + sans[o];
  // walk every owner's blob in the order it was written; keep what was meant for me, placed by request position
  std::vector<std::pair<const char *, int64_t>> mine(want.size(), {nullptr, 0});
  for (int o = 0; o < P; ++o) {
    const char *q = bans.data() + base[o];
    for (int p = 0; p < P; ++p)
      for (size_t t = 0; t < req[p].size(); ++t) {
        const int64_t g = req[p][t];
        if (g < row_off[o] || g >= row_off[o + 1]) continue;
        int64_t len;
        std::memcpy(&len, q, 8);
        if (p == me) mine[t] = {q + 8, len};
        q += 8 + (size_t)((len + 1) / 2 * 2) * 4 + (size_t)len * 8;
      }
  }
  for (size_t t = 0; t < want.size(); ++t) {
    if (!mine[t].first) return ctx->err = "fetch_rows: a requested row has no owner", ALFD_E_COMM;
    const int64_t len = mine[t].second;
    const int32_t *c = (const int32_t *)mine[t].first;
    const double *v = (const double *)(mine[t].first + (size_t)((len + 1) / 2 * 2) * 4);
    out.col.insert(out.col.end(), c, c + len);
    out.val.insert(out.val.end(), v, v + len);
    out.rp.push_back((int64_t)out.col.size());
  }
  return ALFD_OK;
}

static int upload_raw(alfd_ctx *ctx, const HostCsr &h, DevRawCsr &d) {
  d = DevRawCsr();
  d.nrows = h.nrows;
  d.ncols = h.ncols;
  d.nnz = h.nnz();
  HIPC(hipMalloc((void **)&d.rp, (h.nrows + 1) * sizeof(int64_t)));
  HIPC(hipMalloc((void **)&d.col, std::max<int64_t>(d.nnz, 1) * sizeof(int32_t)));
  HIPC(hipMalloc((void **)&d.val, std::max<int64_t>(d.nnz, 1) * sizeof(double)));
  HIPC(hipMemcpyAsync(d.rp, h.rp.data(), (h.nrows + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  if (d.nnz) {
    HIPC(hipMemcpyAsync(d.col, h.col.data(), d.nnz * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipMemcpyAsync(d.val, h.val.data(), d.nnz * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  return ALFD_OK;
}

// out = A * Pm with the device kernel whatever the size; on the host when a row does not fit (*on_device = false).
// Both in the canonical order (alfd_sparse_product, and product() above its size gate).
static int product_dev(alfd_ctx *ctx, const HostCsr &A, const HostCsr &Pm, HostCsr &out, bool *on_device) {
  *on_device = false;
  DevRawCsr dA, dP, dC;
  RC(upload_raw(ctx, A, dA));
  RC(upload_raw(ctx, Pm, dP));
  bool fits = false;
  const int rc = dev_spgemm(ctx, A.nrows, dA.rp, dA.col, dA.val, dP.rp, dP.col, dP.val, Pm.ncols, dC, &fits);
  dA.release();
  dP.release();
  if (rc != ALFD_OK) return rc;
  if (fits) {
    const int rc2 = download_raw(ctx, dC, out);
    dC.release();
    *on_device = rc2 == ALFD_OK;
    return rc2;
  }
  spgemm_host(A, Pm, out);
  return ALFD_OK;
}

// out = A * Pm with the device kernel when the product is large enough to pay for the transfers and it fits, else on
// the host (both in the canonical order)
static int product(alfd_ctx *ctx, const HostCsr &A, const HostCsr &Pm, HostCsr &out) {
  if (ctx->ml_gpu_galerkin && A.nnz() > 200000) {
    bool on_device = false;
    return product_dev(ctx, A, Pm, out, &on_device);
  }
  spgemm_host(A, Pm, out);
  return ALFD_OK;
}

// ======================================================================
// Smoothed aggregation (alfd_build_smoothed_aggregation, alfd_host_smoothed_prolongator): per level
//   P = P_tent - omega D^-1 Aug P_tent,  Aug = A + gamma Ct diag(w) C,  C = Ct^T,  D = diag(Aug),
// P_tent the piecewise-constant prolongator of aggregate_level.  The operator the level's cycle smooths with is the one
// that is smoothed here (ML receives the augmented block in the reference).  Canonical order:
//   d_i  = fma(gamma, s_i, a_ii), s_i a sequential fma over row i of Ct of (w_k c_ik) c_ik   (diag_plus)
//   pen  = Ct Tw, Tw_kJ = (gamma w_k) T_kJ, T = C P_tent                                   (spgemm canonical order)
//   P_iJ = fma(-omega / d_i, s, [J == agg_i]),  s = (sum of a_ik over row i in CSR order with agg_k == J) + pen_iJ
// The pattern is the structural union; nothing is dropped by value.  The host rows below and sa_prolongator_kernel
// compute the same bits.
struct SaPenalty {
  const HostCsr *Ct = nullptr, *C = nullptr;   // Ct: n x m, C = Ct^T
  const double *w = nullptr;                   // W^-1 diagonal (m)
  double gamma = 0.0;
  bool on() const { return Ct != nullptr; }
};

static void sa_diag(const HostCsr &A, const SaPenalty &pen, std::vector<double> &d) {
  d.assign(A.nrows, 0.0);
  for (int64_t i = 0; i < A.nrows; ++i)
    for (int64_t k = A.rp[i]; k < A.rp[i + 1]; ++k)
      if (A.col[k] == i) d[i] = A.val[k];
  if (!pen.on()) return;
  const HostCsr &Ct = *pen.Ct;
  for (int64_t i = 0; i < A.nrows; ++i) {
    double s = 0.0;
    for (int64_t k = Ct.rp[i]; k < Ct.rp[i + 1]; ++k) s = std::fma(pen.w[Ct.col[k]] * Ct.val[k], Ct.val[k], s);
    d[i] = std::fma(pen.gamma, s, d[i]);
  }
}

// y = M x row by row (each row one sequential fma chain), row ranges on up to 16 threads
static void sa_spmv_host(const HostCsr &M, const double *x, double *y) {
  const int64_t n = M.nrows;
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(16u, std::max(1u, std::thread::hardware_concurrency())),
                                                           (n + 16383) / 16384));
  auto work = [&](int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i) {
      double s = 0.0;
      for (int64_t k = M.rp[i]; k < M.rp[i + 1]; ++k) s = std::fma(M.val[k], x[M.col[k]], s);
      y[i] = s;
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < T; ++t) th.emplace_back(work, n * t / T, n * (t + 1) / T);
  work(0, n / T);
  for (auto &x_ : th) x_.join();
}

// lambda_max(D^-1 Aug) by power iteration from the integer-hash start vector of hash_vector_kernel, `its` steps, no
// safety factor; every reduction is one sequential sum (deterministic)
static double sa_lambda(const HostCsr &A, const SaPenalty &pen, const std::vector<double> &d, int its) {
  const int64_t n = A.nrows;
  std::vector<double> v(n), y(n), t(pen.on() ? pen.C->nrows : 0), u(pen.on() ? n : 0);
  for (int64_t i = 0; i < n; ++i) v[i] = 1.0 + (double)(((uint64_t)i * 2654435761ull) & 1023ull) * (1.0 / 1024.0);
  double lam = 0.0;
  for (int it = 0; it < its; ++it) {
    double nv = 0.0;
    for (int64_t i = 0; i < n; ++i) nv = std::fma(v[i], v[i], nv);
    const double sc = 1.0 / std::sqrt(nv);
    for (int64_t i = 0; i < n; ++i) v[i] = v[i] * sc;
    sa_spmv_host(A, v.data(), y.data());
    if (pen.on()) {
      sa_spmv_host(*pen.C, v.data(), t.data());
      for (size_t k = 0; k < t.size(); ++k) t[k] = pen.w[k] * t[k];
      sa_spmv_host(*pen.Ct, t.data(), u.data());
      for (int64_t i = 0; i < n; ++i) y[i] = std::fma(pen.gamma, u[i], y[i]);
    }
    double ny = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      y[i] = y[i] / d[i];
      ny = std::fma(y[i], y[i], ny);
    }
    lam = std::sqrt(ny);
    std::swap(v, y);
  }
  return lam;
}

// the tentative prolongator as a CSR matrix (only for the small product C P_tent)
static void sa_tentative(const std::vector<int32_t> &agg, int64_t nc, HostCsr &Pt) {
  const int64_t n = (int64_t)agg.size();
  Pt.nrows = n;
  Pt.ncols = nc;
  Pt.rp.assign(n + 1, 0);
  Pt.col.clear();
  Pt.val.clear();
  for (int64_t i = 0; i < n; ++i) {
    if (agg[i] >= 0) {
      Pt.col.push_back(agg[i]);
      Pt.val.push_back(1.0);
    }
    Pt.rp[i + 1] = (int64_t)Pt.col.size();
  }
}

// Tw = diag(gamma w) (C P_tent) in place
static void sa_scale_rows(HostCsr &T, const double *w, double gamma) {
  for (int64_t k = 0; k < T.nrows; ++k) {
    const double s = gamma * w[k];
    for (int64_t e = T.rp[k]; e < T.rp[k + 1]; ++e) T.val[e] = s * T.val[e];
  }
}

// the rows of P on the host (overflow fallback of sa_prolongator_kernel and alfd_host_smoothed_prolongator);
// Q = pen (n x nc, sorted rows) or nullptr
static void sa_rows_host(const HostCsr &A, const std::vector<int32_t> &agg, int64_t nc, const std::vector<double> &f,
                         const HostCsr *Q, HostCsr &P) {
  const int64_t n = A.nrows;
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(16u, std::max(1u, std::thread::hardware_concurrency())),
                                                           (n + 4095) / 4096));
  std::vector<std::vector<int32_t>> t_cnt(T), t_col(T);
  std::vector<std::vector<double>> t_val(T);
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t]() {
      const int64_t i0 = n * t / T, i1 = n * (t + 1) / T;
      std::vector<int64_t> stamp(nc, -1);
      std::vector<double> acc(nc, 0.0);
      std::vector<int32_t> touched;
      auto add = [&](int64_t i, int32_t J, double v) {
        if (stamp[J] != i) {
          stamp[J] = i;
          acc[J] = 0.0;
          touched.push_back(J);
        }
        acc[J] = acc[J] + v;
      };
      for (int64_t i = i0; i < i1; ++i) {
        touched.clear();
        const int32_t gi = agg[i];
        if (gi >= 0) {
          for (int64_t k = A.rp[i]; k < A.rp[i + 1]; ++k) {
            const int32_t J = agg[A.col[k]];
            if (J >= 0) add(i, J, A.val[k]);
          }
          if (Q)
            for (int64_t q = Q->rp[i]; q < Q->rp[i + 1]; ++q) add(i, Q->col[q], Q->val[q]);
          if (stamp[gi] != i) add(i, gi, 0.0);
        }
        std::sort(touched.begin(), touched.end());
        t_cnt[t].push_back((int32_t)touched.size());
        for (int32_t J : touched) {
          t_col[t].push_back(J);
          t_val[t].push_back(std::fma(f[i], acc[J], J == gi ? 1.0 : 0.0));
        }
      }
    });
  for (auto &x : th) x.join();
  P.nrows = n;
  P.ncols = nc;
  P.rp.assign(1, 0);
  P.col.clear();
  P.val.clear();
  for (int t = 0; t < T; ++t) {
    for (int32_t c : t_cnt[t]) P.rp.push_back(P.rp.back() + c);
    P.col.insert(P.col.end(), t_col[t].begin(), t_col[t].end());
    P.val.insert(P.val.end(), t_val[t].begin(), t_val[t].end());
  }
}

// The truncation rule of the smoothed prolongator on the host (alfd_host_truncate_prolongator and the overflow fallback
// of sa_truncated_prolongator_kernel, same bits; canonical order: DESIGN.md section 4).  P has sorted rows, every row
// with agg[i] >= 0 holds column agg[i]; rows with agg[i] < 0 come out empty.
static void sa_truncate_host(const HostCsr &P, const std::vector<int32_t> &agg, int bs, double tau, int cap, HostCsr &T) {
  const int64_t n = P.nrows;
  T.nrows = n;
  T.ncols = P.ncols;
  T.rp.assign(n + 1, 0);
  T.col.clear();
  T.val.clear();
  std::vector<char> keep;
  std::vector<double> v;
  std::vector<int64_t> order;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t gi = agg[i];
    const int64_t e0 = P.rp[i], len = P.rp[i + 1] - e0;
    if (gi >= 0 && len > 0) {
      const int32_t *J = P.col.data() + e0;
      v.assign(P.val.begin() + e0, P.val.begin() + e0 + len);
      double m = 0.0;
      for (int64_t t = 0; t < len; ++t)
        if (std::fabs(v[t]) > m) m = std::fabs(v[t]);
      const double thr = tau * m;
      keep.assign(len, 0);
      int64_t nk = 0;
      for (int64_t t = 0; t < len; ++t) nk += keep[t] = (!(std::fabs(v[t]) < thr) || J[t] == gi) ? 1 : 0;
      if (cap > 0 && nk > cap) {
        order.clear();
        for (int64_t t = 0; t < len; ++t)
          if (keep[t] && J[t] != gi) order.push_back(t);
        std::stable_sort(order.begin(), order.end(),
                         [&](int64_t a, int64_t b) { return std::fabs(v[a]) > std::fabs(v[b]); });
        for (size_t q = (size_t)(cap - 1); q < order.size(); ++q) keep[order[q]] = 0;
        nk = cap;
      }
      if (nk < len)
        for (int c = 0; c < bs; ++c) {
          double t = 0.0, best = -1.0;
          int64_t at = -1, nd = 0;
          for (int64_t u = 0; u < len; ++u) {
            if (J[u] % bs != c) continue;
            if (keep[u]) {
              if (std::fabs(P.val[e0 + u]) > best) best = std::fabs(P.val[e0 + u]), at = u;
            } else {
              t = t + P.val[e0 + u];
              ++nd;
            }
          }
          if (nd > 0 && at >= 0) v[at] = v[at] + t;
        }
      for (int64_t t = 0; t < len; ++t)
        if (keep[t]) {
          T.col.push_back(J[t]);
          T.val.push_back(v[t]);
        }
    }
    T.rp[i + 1] = (int64_t)T.col.size();
  }
}

// f_i = -omega / d_i (rows without an aggregate: 0, never read)
static void sa_factors(const std::vector<int32_t> &agg, const std::vector<double> &d, double omega, std::vector<double> &f) {
  f.assign(agg.size(), 0.0);
  for (size_t i = 0; i < agg.size(); ++i)
    if (agg[i] >= 0) f[i] = -omega / d[i];
}

// the penalty rows gamma Ct diag(w) C P_tent (an empty matrix without penalty)
static int sa_penalty_rows(alfd_ctx *ctx, const SaPenalty &pen, const std::vector<int32_t> &agg, int64_t nc, HostCsr &Q) {
  Q = HostCsr();
  if (!pen.on()) return ALFD_OK;
  HostCsr Pt, Tm;
  sa_tentative(agg, nc, Pt);
  if (ctx) RC(product(ctx, *pen.C, Pt, Tm));
  else spgemm_host(*pen.C, Pt, Tm);
  sa_scale_rows(Tm, pen.w, pen.gamma);
  if (ctx) RC(product(ctx, *pen.Ct, Tm, Q));
  else spgemm_host(*pen.Ct, Tm, Q);
  return ALFD_OK;
}

// P on the device; *fits = false when a row has more distinct coarse ids than the kernel holds.  tau == 0 and cap == 0:
// sa_prolongator_kernel; otherwise sa_truncated_prolongator_kernel, whose counts, row pointer and arrays hold the kept
// entries only (the untruncated P exists nowhere).
// (the rows of A are device arrays: an uploaded copy, or the global-column view of a partitioned context's resident rows
// with agg = [agg of the own rows | agg of all unknowns], see sa_global_cols_kernel)
static int sa_prolongator_dev_raw(alfd_ctx *ctx, int64_t n, const int64_t *arp, const int32_t *acol, const double *aval,
                                  const std::vector<int32_t> &agg, int64_t nc, const std::vector<double> &f,
                                  const HostCsr &Q, int bs, double tau, int cap, HostCsr &P, bool *fits) {
  *fits = false;
  const bool trunc = tau != 0.0 || cap != 0;
  struct {
    const int64_t *rp;
    const int32_t *col;
    const double *val;
    void release() {}
  } dA{arp, acol, aval};
  DevRawCsr dQ, dP;
  const int64_t n_agg = (int64_t)agg.size();
  const bool pen = !Q.rp.empty();
  if (pen) RC(upload_raw(ctx, Q, dQ));
  int32_t *d_agg = nullptr, *counts = nullptr, *ovf = nullptr;
  double *d_f = nullptr;
  auto release = [&]() {
    dA.release();
    dQ.release();
    dP.release();
    for (void *p : {(void *)d_agg, (void *)counts, (void *)ovf, (void *)d_f})
      if (p) hipFree(p);
  };
  auto fail = [&](hipError_t e) {
    release();
    ctx->err = std::string("HIP error in the smoothed-aggregation prolongator: ") + hipGetErrorString(e);
    return ALFD_E_HIP;
  };
  hipError_t e;
  if ((e = hipMalloc((void **)&d_agg, std::max<int64_t>(n_agg, 1) * sizeof(int32_t))) != hipSuccess) return fail(e);
  if ((e = hipMalloc((void **)&d_f, std::max<int64_t>(n, 1) * sizeof(double))) != hipSuccess) return fail(e);
  if ((e = hipMalloc((void **)&counts, std::max<int64_t>(n, 1) * sizeof(int32_t))) != hipSuccess) return fail(e);
  if ((e = hipMalloc((void **)&ovf, sizeof(int32_t))) != hipSuccess) return fail(e);
  if ((e = hipMalloc((void **)&dP.rp, (n + 1) * sizeof(int64_t))) != hipSuccess) return fail(e);
  if (n_agg && (e = hipMemcpyAsync(d_agg, agg.data(), n_agg * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream)) != hipSuccess)
    return fail(e);
  if (n && (e = hipMemcpyAsync(d_f, f.data(), n * sizeof(double), hipMemcpyHostToDevice, ctx->stream)) != hipSuccess)
    return fail(e);
  if ((e = hipMemsetAsync(ovf, 0, sizeof(int32_t), ctx->stream)) != hipSuccess) return fail(e);
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(n, 256 * 64));
  const int64_t *qrp = pen ? dQ.rp : nullptr;
  auto launch = [&](int pass, const int64_t *prp, int32_t *pcol, double *pval) {
    if (trunc)
      hipLaunchKernelGGL(sa_truncated_prolongator_kernel, dim3(grid), dim3(64), 0, ctx->stream, n, dA.rp, dA.col, dA.val,
                         d_agg, d_f, qrp, dQ.col, dQ.val, bs, tau, cap, pass, counts, prp, pcol, pval, ovf);
    else
      hipLaunchKernelGGL(sa_prolongator_kernel, dim3(grid), dim3(64), 0, ctx->stream, n, dA.rp, dA.col, dA.val, d_agg, d_f,
                         qrp, dQ.col, dQ.val, pass, counts, prp, pcol, pval, ovf);
  };
  launch(0, nullptr, nullptr, nullptr);
  if ((e = hipGetLastError()) != hipSuccess) return fail(e);
  std::vector<int32_t> hc(n);
  int32_t hovf = 0;
  if (n && (e = hipMemcpyAsync(hc.data(), counts, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess)
    return fail(e);
  if ((e = hipMemcpyAsync(&hovf, ovf, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) return fail(e);
  if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return fail(e);
  if (hovf) {
    release();
    return ALFD_OK;
  }
  P.nrows = n;
  P.ncols = nc;
  P.rp.assign(n + 1, 0);
  for (int64_t i = 0; i < n; ++i) P.rp[i + 1] = P.rp[i] + hc[i];
  const int64_t nnz = P.rp[n];
  dP.nrows = n;
  dP.ncols = nc;
  dP.nnz = nnz;
  if ((e = hipMemcpyAsync(dP.rp, P.rp.data(), (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream)) != hipSuccess)
    return fail(e);
  if ((e = hipMalloc((void **)&dP.col, std::max<int64_t>(nnz, 1) * sizeof(int32_t))) != hipSuccess) return fail(e);
  if ((e = hipMalloc((void **)&dP.val, std::max<int64_t>(nnz, 1) * sizeof(double))) != hipSuccess) return fail(e);
  launch(1, dP.rp, dP.col, dP.val);
  if ((e = hipGetLastError()) != hipSuccess) return fail(e);
  P.col.resize(nnz);
  P.val.resize(nnz);
  if (nnz && (e = hipMemcpyAsync(P.col.data(), dP.col, nnz * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess)
    return fail(e);
  if (nnz && (e = hipMemcpyAsync(P.val.data(), dP.val, nnz * sizeof(double), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess)
    return fail(e);
  if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return fail(e);
  release();
  *fits = true;
  return ALFD_OK;
}

static int sa_prolongator_dev(alfd_ctx *ctx, const HostCsr &A, const std::vector<int32_t> &agg, int64_t nc,
                              const std::vector<double> &f, const HostCsr &Q, int bs, double tau, int cap, HostCsr &P,
                              bool *fits) {
  *fits = false;
  DevRawCsr dA;
  RC(upload_raw(ctx, A, dA));
  const int rc = sa_prolongator_dev_raw(ctx, A.nrows, dA.rp, dA.col, dA.val, agg, nc, f, Q, bs, tau, cap, P, fits);
  dA.release();
  return rc;
}

// The interface patch of a partitioned context: S is split by row ownership, the patch operators are gathered whole on
// every rank (they are small), the polynomial runs redundantly; see ml_apply_rep.
static int patch_setup_rep(alfd_ctx *ctx) {
  alfd_ctx::Patch &Q = ctx->patch;
  const int P = ctx->nranks, rk = ctx->rank, last = ctx->nblocks - 1;
  const std::vector<int64_t> &off0 = ctx->part[0], &offl = ctx->part[last];
  DevCsr &dA = ctx->mat[ALFD_A], &dC = ctx->mat[ALFD_C], &dCt = ctx->mat[ALFD_CT];
  const int64_t n_loc = ctx->n[0];
  HostCsr Ct, C;
  RC(download_csr(ctx, dCt, Ct));
  RC(download_csr(ctx, dC, C));
  std::vector<int32_t> S;
  for (int64_t i = 0; i < n_loc; ++i)
    if (Ct.rp[i + 1] > Ct.rp[i]) S.push_back((int32_t)i);
  // global S: every rank's list of global row ids, in rank order
  std::vector<int64_t> Sg(S.size());
  for (size_t q = 0; q < S.size(); ++q) Sg[q] = off0[rk] + S[q];
  std::vector<char> ball;
  std::vector<size_t> sz;
  RC(allgather_bytes(ctx, Sg.data(), Sg.size() * sizeof(int64_t), ball, sz));
  Q.soff.assign(P + 1, 0);
  for (int p = 0; p < P; ++p) Q.soff[p + 1] = Q.soff[p] + (int64_t)(sz[p] / sizeof(int64_t));
  const int64_t m = Q.soff[P];
  if (m == 0) return ALFD_OK;
  std::vector<int64_t> Sall(m);
  std::memcpy(Sall.data(), ball.data(), (size_t)m * sizeof(int64_t));     // ascending: rank order = global order
  auto patch_id = [&](int64_t g) -> int32_t {
    auto it = std::lower_bound(Sall.begin(), Sall.end(), g);
    return it != Sall.end() && *it == g ? (int32_t)(it - Sall.begin()) : -1;
  };
  // patch ids over the LOCAL column spaces [owned | halo] of A and of C
  auto make_pos = [&](const DevCsr &mtx, std::vector<int32_t> &pos) {
    pos.assign((size_t)mtx.n_local_cols + mtx.halo_globals.size(), -1);
    for (size_t q = 0; q < S.size(); ++q) pos[S[q]] = (int32_t)(Q.soff[rk] + (int64_t)q);
    for (size_t h = 0; h < mtx.halo_globals.size(); ++h) pos[mtx.n_local_cols + h] = patch_id(mtx.halo_globals[h]);
  };
  std::vector<int32_t> posA, posC, Trows;
  make_pos(dA, posA);
  make_pos(dC, posC);
  HostCsr A_patch, h, g;
  RC(fetch_patch_rows(ctx, dA, posA, A_patch, Trows));
  // replicated operators: my rows, then gathered in rank order
  extract_host(A_patch, S, posA.data(), m, false, h);
  RC(gather_csr(ctx, h, nullptr, m, g));
  RC(upload_level_part(ctx, Q.Ass, g, nullptr, true));
  std::vector<int32_t> lam_rows(C.nrows);
  for (int64_t k = 0; k < C.nrows; ++k) lam_rows[k] = (int32_t)k;
  extract_host(C, lam_rows, posC.data(), m, false, h);
  RC(gather_csr(ctx, h, nullptr, m, g));
  RC(upload_level_part(ctx, Q.Cs, g, nullptr, true));
  // Ct rows over GLOBAL multiplier ids
  const std::vector<int32_t> lamg = global_cols(dCt, offl[rk]);
  HostCsr Ctg = Ct;
  Ctg.ncols = offl.back();
  for (int64_t i = 0; i < Ctg.nrows; ++i) {   // rows re-sorted by the global id (the local order puts halo ids last)
    std::vector<std::pair<int32_t, double>> row;
    for (int64_t k = Ct.rp[i]; k < Ct.rp[i + 1]; ++k) row.emplace_back(lamg[Ct.col[k]], Ct.val[k]);
    std::sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    for (size_t k = 0; k < row.size(); ++k) Ctg.col[Ct.rp[i] + k] = row[k].first, Ctg.val[Ct.rp[i] + k] = row[k].second;
  }
  extract_host(Ctg, S, nullptr, Ctg.ncols, false, h);
  RC(upload_level_part(ctx, Q.Cts_loc, h, nullptr, true));
  RC(gather_csr(ctx, h, nullptr, Ctg.ncols, g));
  RC(upload_level_part(ctx, Q.Cts, g, nullptr, true));
  RC(upload_level_part(ctx, Q.Ctg, Ctg, nullptr, true));
  Q.Ass.rep = Q.Cs.rep = Q.Cts.rep = true;
  // my rows of A[:, S] (patch ids, local-only) and of A[S, :] (global fine ids, halo on the fine vector)
  extract_host(A_patch, Trows, posA.data(), m, true, h);
  RC(upload_level_part(ctx, Q.Ats, h, nullptr, true));
  extract_host(A_patch, S, nullptr, A_patch.ncols, false, h);
  const std::vector<int32_t> fineg = global_cols(dA, off0[rk]);
  for (int32_t &col : h.col) col = fineg[col];
  h.ncols = off0.back();
  RC(upload_level_part(ctx, Q.As, h, off0.data(), false));
  Q.m = m;
  Q.mpad = pad_chunk(m);
  Q.m_loc = (int64_t)S.size();
  for (int p = 0; p < P; ++p) {
    Q.piece = std::max(Q.piece, Q.soff[p + 1] - Q.soff[p]);
    Q.lam_piece = std::max(Q.lam_piece, offl[p + 1] - offl[p]);
  }
  void *q = nullptr;
  HIPC(hipMalloc(&q, std::max<int64_t>(Q.m_loc, 1) * sizeof(int32_t)));
  ctx->ws_allocs.push_back(q);
  Q.S = static_cast<int32_t *>(q);
  if (Q.m_loc) HIPC(hipMemcpyAsync(Q.S, S.data(), Q.m_loc * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  for (double **v : {&Q.dinv, &Q.rS, &Q.zS, &Q.uS, &Q.eS, &Q.cd, &Q.cres, &Q.ctmp}) RC(ws_alloc_zero(ctx, v, Q.mpad));
  RC(ws_alloc_zero(ctx, &Q.rr, pad_chunk(n_loc)));
  RC(ws_alloc_zero(ctx, &Q.loc, pad_chunk(std::max<int64_t>(Q.m_loc, 1))));
  RC(ws_alloc_zero(ctx, &Q.send, Q.piece));
  RC(ws_alloc_zero(ctx, &Q.stage, Q.piece * P));
  RC(ws_alloc_zero(ctx, &Q.lam_send, Q.lam_piece));
  RC(ws_alloc_zero(ctx, &Q.lam_stage, Q.lam_piece * P));
  Q.rep = true;
  // 1 / diag(Aug) on S: my entries, gathered
  const unsigned gm = (unsigned)std::max<int64_t>(1, (Q.m_loc + 255) / 256);
  if (Q.m_loc) hipLaunchKernelGGL(gather_kernel, dim3(gm), dim3(256), 0, ctx->stream, Q.m_loc, Q.S, ctx->dinv_aug, Q.loc);
  RC(allgather_pieces(ctx, Q.loc, Q.soff, Q.piece, Q.send, Q.stage, Q.dinv));
  // lambda_max(D^-1 Aug_SS) on the replicated patch: plain reductions, the same on every rank
  {
    ReplicatedDots rd(ctx);
    RC(aug_lambda_max(ctx, patch_aug(ctx), m, 0, Q.rS, Q.zS, &Q.lmax));
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  Q.on = true;
  return ALFD_OK;
}

// The level-0 products of a partitioned hierarchy, replicated: A_1 = P_0^T (A P_0) and C_1 = C P_0 (C1 may be null) whole
// on every rank, with the bits of the single-rank products; Rg = this rank's rows of P_0^T over GLOBAL fine ids.  P0 =
// this rank's rows of P_0 (global coarse ids), coff = the ranks' ranges of the coarse ids (the rank that forms a coarse
// row).  Remote rows of P_0 and A P_0 come from their owners (fetch_rows).  built = false (caller-supplied
// prolongators): the rows of A's halo, so a coarse unknown's fine support must lie in its rank's rows + halo of A.
// built = true (alfd_build_smoothed_aggregation on a partitioned context, whose global aggregates do not respect the
// slabs and whose smoothed columns reach one hop further): also every fine row in the support of an owned coarse
// unknown that this rank does not own -- known from an all-gather of (forming rank, fine row) pairs, one per remote
// rank a row of P_0 touches -- so any contiguous split of the coarse ids is valid and the result does not depend on it.
// Shared by alfd_setup and the builder (which needs A_1 and C_1 for the aggregation of level 1).
static int rep_level0_products(alfd_ctx *ctx, const HostCsr &P0, const std::vector<int64_t> &coff, bool built, HostCsr &A1,
                               HostCsr *C1, HostCsr &Rg) {
  const int P = ctx->nranks, rk = ctx->rank;
  const std::vector<int64_t> &off0 = ctx->part[0];
  const int64_t n1 = P0.ncols;
  DevCsr &dA = ctx->mat[ALFD_A], &dC = ctx->mat[ALFD_C];
  std::vector<int64_t> extra;   // fine rows beyond A's halo whose prolongator rows reach an owned coarse unknown
  if (built) {
    std::vector<int64_t> pairs;   // (forming rank, global fine row), one per remote rank a row touches
    std::vector<char> hit(P);
    for (int64_t q = 0; q < P0.nrows; ++q) {
      std::fill(hit.begin(), hit.end(), 0);
      for (int64_t k = P0.rp[q]; k < P0.rp[q + 1]; ++k) {
        const int p = (int)(std::upper_bound(coff.begin(), coff.end(), (int64_t)P0.col[k]) - coff.begin()) - 1;
        if (p != rk && p >= 0 && p < P && !hit[p]) {
          hit[p] = 1;
          pairs.push_back(p);
          pairs.push_back(off0[rk] + q);
        }
      }
    }
    std::vector<char> ball;
    std::vector<size_t> sz;
    RC(allgather_bytes(ctx, pairs.data(), pairs.size() * sizeof(int64_t), ball, sz));
    const int64_t *all = reinterpret_cast<const int64_t *>(ball.data());
    const size_t npairs = ball.size() / (2 * sizeof(int64_t));
    std::vector<int64_t> halo(dA.halo_globals.begin(), dA.halo_globals.end());   // sorted
    for (size_t t = 0; t < npairs; ++t)
      if (all[2 * t] == rk && !std::binary_search(halo.begin(), halo.end(), all[2 * t + 1])) extra.push_back(all[2 * t + 1]);
    std::sort(extra.begin(), extra.end());
  }
  // A's rows in its LOCAL column space [owned | halo]: the prolongator rows in that order
  auto perm_rows = [&](const DevCsr &m, const std::vector<int64_t> &more, HostCsr &Pperm, std::vector<int64_t> &colg) -> int {
    std::vector<int64_t> want(m.halo_globals.begin(), m.halo_globals.end());
    want.insert(want.end(), more.begin(), more.end());
    HostCsr halo;
    RC(fetch_rows(ctx, P0, off0.data(), want, halo));
    Pperm = P0;
    append_rows(Pperm, halo);
    colg.resize(Pperm.nrows);
    for (int64_t q = 0; q < P0.nrows; ++q) colg[q] = off0[rk] + q;
    for (size_t q = 0; q < want.size(); ++q) colg[P0.nrows + q] = want[q];
    return ALFD_OK;
  };
  HostCsr PpA, PpC, AP_loc, AP_halo, CP_loc;
  std::vector<int64_t> colgA, colgC;
  RC(perm_rows(dA, extra, PpA, colgA));
  {   // A_r * P on the device, fetched (its rows are served to the neighbours below)
    DevRawCsr dP, dAP;
    RC(upload_raw(ctx, PpA, dP));
    bool fits = false;
    RC(dev_spgemm(ctx, dA.nrows, dA.rp, dA.col, dA.val, dP.rp, dP.col, dP.val, n1, dAP, &fits));
    dP.release();
    if (fits) {
      RC(download_raw(ctx, dAP, AP_loc));
      dAP.release();
    } else {
      // a row with more than kSgMaxOut columns: this rank forms its rows on the host (same bits).  The product of a
      // rank's rows is rank-local, so the peers may stay on the device; every rank goes on to the fetch_rows below.
      HostCsr Al;
      RC(download_csr(ctx, dA, Al));   // columns in the local space [owned | halo], the row order of PpA
      Al.ncols = PpA.nrows;
      spgemm_host(Al, PpA, AP_loc);
    }
  }
  {
    std::vector<int64_t> want(dA.halo_globals.begin(), dA.halo_globals.end());
    want.insert(want.end(), extra.begin(), extra.end());
    RC(fetch_rows(ctx, AP_loc, off0.data(), want, AP_halo));
  }
  // R_owned: one row per owned coarse unknown, entries over the local fine space [owned | halo] in GLOBAL fine order
  const int64_t c0 = coff[rk], nc_loc = coff[rk + 1] - c0;
  HostCsr Rl, APp;
  {
    std::vector<int64_t> cnt(nc_loc + 1, 0);
    for (int64_t q = 0; q < PpA.nrows; ++q)
      for (int64_t k = PpA.rp[q]; k < PpA.rp[q + 1]; ++k) {
        const int64_t I = PpA.col[k];
        if (I >= c0 && I < c0 + nc_loc) cnt[I - c0 + 1]++;
      }
    for (int64_t I = 0; I < nc_loc; ++I) cnt[I + 1] += cnt[I];
    std::vector<std::pair<int64_t, std::pair<int32_t, double>>> ent(cnt[nc_loc]);   // (global fine id, (local index, value))
    std::vector<int64_t> cur(cnt.begin(), cnt.end() - 1);
    for (int64_t q = 0; q < PpA.nrows; ++q)
      for (int64_t k = PpA.rp[q]; k < PpA.rp[q + 1]; ++k) {
        const int64_t I = PpA.col[k];
        if (I >= c0 && I < c0 + nc_loc) ent[cur[I - c0]++] = {colgA[q], {(int32_t)q, PpA.val[k]}};
      }
    Rl.nrows = nc_loc;
    Rl.ncols = PpA.nrows;
    Rl.rp = cnt;
    Rl.col.resize(ent.size());
    Rl.val.resize(ent.size());
    for (int64_t I = 0; I < nc_loc; ++I) {
      std::sort(ent.begin() + cnt[I], ent.begin() + cnt[I + 1], [](const auto &a, const auto &b) { return a.first < b.first; });
      for (int64_t k = cnt[I]; k < cnt[I + 1]; ++k) Rl.col[k] = ent[k].second.first, Rl.val[k] = ent[k].second.second;
    }
    APp = AP_loc;
    append_rows(APp, AP_halo);
  }
  {
    // every prolongator entry must have been seen by the rank that forms its coarse row: the fine rows in the support
    // of an owned coarse unknown have to lie in this rank's rows or in A's halo (coarse partition aligned with the fine one)
    int64_t cnt2[2] = {(int64_t)Rl.col.size(), P0.nnz()};
    std::vector<char> ball;
    std::vector<size_t> sz;
    RC(allgather_bytes(ctx, cnt2, sizeof(cnt2), ball, sz));
    int64_t seen = 0, total = 0;
    for (int p = 0; p < P; ++p) {
      int64_t v[2];
      std::memcpy(v, ball.data() + (size_t)p * sizeof(cnt2), sizeof(cnt2));
      seen += v[0];
      total += v[1];
    }
    if (seen != total)
      return ctx->err = "partitioned CSR prolongator: a coarse unknown's fine support leaves its rank's rows + halo of A "
                        "(alfd_set_aggregate_partition must follow the fine partition)", ALFD_E_INVALID;
  }
  HostCsr A1_loc;
  RC(product(ctx, Rl, APp, A1_loc));
  RC(gather_csr(ctx, A1_loc, nullptr, n1, A1));
  // C_1 = C P: rows of the owned multipliers, then gathered
  if (C1) {
    RC(perm_rows(dC, {}, PpC, colgC));
    {
      HostCsr Cl;
      RC(download_csr(ctx, dC, Cl));
      Cl.ncols = PpC.nrows;
      RC(product(ctx, Cl, PpC, CP_loc));
    }
    RC(gather_csr(ctx, CP_loc, nullptr, n1, *C1));
  }
  Rg = Rl;
  Rg.ncols = off0.back();
  for (size_t k = 0; k < Rg.col.size(); ++k) Rg.col[k] = (int32_t)colgA[Rl.col[k]];
  return ALFD_OK;
}

// The zeroed work vectors of a record, npad entries each (the caller has set n and npad): r and z, which the transfers
// read and write; with `sweep` also those of a Chebyshev sweep and a residual on the level.  dinv is the caller's.
static int store_vectors(alfd_ctx *ctx, LevelStore &S, bool sweep) {
  for (double **v : {&S.r, &S.z}) RC(ws_alloc_zero(ctx, v, S.npad));
  if (sweep)
    for (double **v : {&S.t, &S.cd, &S.cres, &S.ctmp}) RC(ws_alloc_zero(ctx, v, S.npad));
  return ALFD_OK;
}

// Level l of hierarchy 0 becomes a REPLICATED level: A, C, Ct (whole) on every rank and the vectors of the record, dinv
// zero.  offs = the ranks' ranges of the level's unknowns; `first`: the level the restricted residual is gathered into,
// which holds the buffers of that all-gather.  The caller fills dinv and uploads the transfer pair rep.P / rep.R.
static int replicate_level(alfd_ctx *ctx, int l, const HostCsr &A, const HostCsr &C, const HostCsr &Ct,
                           const std::vector<int64_t> &offs, bool first) {
  MlLevel &L = ctx->hier[0].ml[l];
  LevelStore &S = L.rep;
  L.offs = offs;
  S.n = A.nrows;
  S.npad = pad_chunk(S.n);
  RC(upload_level_part(ctx, S.A, A, nullptr, true));
  RC(upload_level_part(ctx, S.C, C, nullptr, true));
  RC(upload_level_part(ctx, S.Ct, Ct, nullptr, true));
  S.A.rep = S.C.rep = S.Ct.rep = true;
  RC(ws_alloc_zero(ctx, &S.dinv, S.npad));
  RC(store_vectors(ctx, S, true));
  if (first) {
    for (int p = 0; p < ctx->nranks; ++p) L.maxpiece = std::max(L.maxpiece, offs[p + 1] - offs[p]);
    L.maxpiece = std::max<int64_t>(L.maxpiece, 1);
    RC(ws_alloc_zero(ctx, &L.send, L.maxpiece));
    RC(ws_alloc_zero(ctx, &L.stage, L.maxpiece * ctx->nranks));
  }
  return ALFD_OK;
}

// ALFD_PREC_MULTILEVEL through CSR prolongators on a ROW-PARTITIONED context (round 3): the fine level stays
// partitioned, every level below it -- and the interface patch -- is REPLICATED on all ranks.  Level 0: this rank holds
// the prolongator rows of its own fine unknowns (global coarse ids) and alfd_set_aggregate_partition(0, ...) names the
// rank that forms each coarse row; levels >= 1: the whole prolongator on every rank.  The hierarchy is the single-rank
// one bit for bit: a coarse row's Galerkin chain and restriction sum run over its fine rows in GLOBAL order, remote
// prolongator / A P rows are fetched from their owners (fetch_rows), finished rows are all-gathered.  Only the level-0
// reductions differ from a single-rank run (rank-ordered sums, as on every partitioned path).
static int ml_setup_rep_prolongators(alfd_ctx *ctx, int nlev) {
  const alfd_config &c = ctx->cfg;
  const int P = ctx->nranks, rk = ctx->rank, last = ctx->nblocks - 1;
  for (int l = 0; l < nlev; ++l)
    if (ctx->hier[0].P[l].rp.empty())
      return ctx->err = "partitioned context: CSR prolongators and aggregates cannot be mixed", ALFD_E_UNSUPPORTED;
  const std::vector<int64_t> &off0 = ctx->part[0], &coff = ctx->ml_coff[0];
  const HostCsr &P0 = ctx->hier[0].P[0];
  const int64_t n_loc = ctx->n[0], n1 = P0.ncols;
  if ((int)coff.size() != P + 1 || coff.back() != n1 || P0.nrows != n_loc)
    return ctx->err = "partitioned CSR prolongator: level 0 needs this rank's rows and alfd_set_aggregate_partition(0, coarse offsets)",
           ALFD_E_INVALID;
  for (int l = 1; l < nlev; ++l)
    if (ctx->hier[0].P[l].nrows != ctx->hier[0].P[l - 1].ncols)
      return ctx->err = "partitioned CSR prolongator: levels >= 1 must be given whole on every rank", ALFD_E_INVALID;
  free_levels(ctx);
  ctx->hier[0].ml.assign(nlev + 1, MlLevel());
  // ---- level 0 (partitioned): vectors only, operators are the slots
  {
    MlLevel &L = ctx->hier[0].ml[0];
    L.loc.n = n_loc;
    L.loc.npad = pad_chunk(n_loc);
    RC(store_vectors(ctx, L.loc, true));
    L.loc.dinv = ctx->dinv_aug;
    L.lmax = ctx->lam_max[OP_AUG];
  }
  HostCsr A1, C1, Ct1;
  {
    PhaseClock pc(ctx, ALFD_SETUP_ML_GALERKIN);
    HostCsr Rg;
    RC(rep_level0_products(ctx, P0, coff, ctx->hier[0].built_partitioned, A1, &C1, Rg));
    transpose_host(C1, Ct1);
    // the partitioned transfer pair of level 0 <-> 1: R rows of the owned coarse unknowns (global fine columns, halo on
    // the fine vector), P rows of the owned fine unknowns addressing the replicated coarse vector
    MlLevel &N = ctx->hier[0].ml[1];
    PhaseClock pu(ctx, ALFD_SETUP_ML_UPLOAD);
    RC(upload_level_part(ctx, N.loc.R, Rg, off0.data(), false));
    RC(upload_level_part(ctx, N.loc.P, P0, nullptr, true));
    N.P_global_cols = true;
  }
  // ---- replicated levels 1 .. nlev
  const int64_t lam_global = ctx->part[last].back(), lam_pad = pad_chunk(lam_global);
  RC(ws_alloc_zero(ctx, &ctx->g_w, lam_pad));
  RC(ws_alloc_zero(ctx, &ctx->g_tlam, lam_pad));
  RC(gather_vec(ctx, ctx->diag[ALFD_INVW], ctx->n[last], ctx->g_w));
  ctx->ml_rep_level = 1;
  HostCsr A = std::move(A1), C = std::move(C1), Ct = std::move(Ct1), An, Cn, Ctn, R;
  for (int l = 1; l <= nlev; ++l) {
    MlLevel &L = ctx->hier[0].ml[l];
    std::vector<int64_t> offs(P + 1, 0);
    if (l == 1) offs = coff;
    else for (int p = 0; p <= P; ++p) offs[p] = A.nrows * p / P;      // no partitioned piece below level 1
    L.loc.n = l == 1 ? coff[rk + 1] - coff[rk] : 0;
    L.loc.npad = pad_chunk(std::max<int64_t>(L.loc.n, 1));
    RC(store_vectors(ctx, L.loc, false));
    {
      PhaseClock pu(ctx, ALFD_SETUP_ML_UPLOAD);
      RC(replicate_level(ctx, l, A, C, Ct, offs, l == 1));
    }
    {
      // diagonal and lambda_max on the replicated operator: plain (single-rank) reductions, the same on every rank
      PhaseClock pl(ctx, ALFD_SETUP_ML_LAMBDA);
      ReplicatedDots rd(ctx);
      double *w_save = ctx->diag[ALFD_INVW];
      ctx->diag[ALFD_INVW] = ctx->g_w;        // diag_plus_m reads the weight through the slot
      const int rc = diag_plus_m(ctx, L.rep.A, L.rep.Ct, c.aug_assembled ? 0.0 : c.gamma, L.rep.n, L.rep.dinv);
      ctx->diag[ALFD_INVW] = w_save;
      if (rc != ALFD_OK) return rc;
      RC(aug_lambda_max(ctx, level_view(ctx, 0, l).op, L.rep.n, 0, L.rep.t, L.rep.r, &L.lmax));
    }
    if (l == nlev) break;
    const HostCsr &Pm = ctx->hier[0].P[l];
    {
      PhaseClock pg(ctx, ALFD_SETUP_ML_GALERKIN);
      HostCsr AP;
      transpose_host(Pm, R);
      RC(product(ctx, A, Pm, AP));
      RC(product(ctx, R, AP, An));
      RC(product(ctx, C, Pm, Cn));
      transpose_host(Cn, Ctn);
    }
    MlLevel &N = ctx->hier[0].ml[l + 1];
    PhaseClock pu(ctx, ALFD_SETUP_ML_UPLOAD);
    RC(upload_level_part(ctx, N.rep.P, Pm, nullptr, true));
    RC(upload_level_part(ctx, N.rep.R, R, nullptr, true));
    N.rep.P.rep = N.rep.R.rep = true;
    A = std::move(An);
    C = std::move(Cn);
    Ct = std::move(Ctn);
  }
  if (c.ml_coarse_direct > 0 && ctx->hier[0].ml[nlev].rep.n > 0 && ctx->hier[0].ml[nlev].rep.n <= c.ml_coarse_direct) {
    PhaseClock pc(ctx, ALFD_SETUP_ML_COARSE);
    std::vector<double> w(lam_global);
    HIPC(hipMemcpyAsync(w.data(), ctx->g_w, w.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    RC(coarse_inverse(ctx, A, C, Ct, w, c.gamma, ctx->hier[0].inv));
    ctx->hier[0].inv.rep = true;
  }
  if (c.ml_patch_degree > 0) {
    PhaseClock pc(ctx, ALFD_SETUP_ML_PATCH);
    RC(patch_setup_rep(ctx));
  }
  return ALFD_OK;
}

// Vectors of level l of hierarchy h (n unknowns, the first of them the global index goff).  Level 0 takes 1 / diag and
// lambda_max from its inner operator; a level below gets 1 / diag(Aug_l) and lambda_max(D^-1 Aug_l) by power iteration
// from the integer-hash vector (global index) -- its operators are in place by then.
// The two halves: level_vectors allocates (sizes follow A and P alone), level_penalty fills what follows C, invW and the
// penalty weight.  alfd_setup runs both, alfd_setup_coupling the second on the vectors it finds.
static int level_vectors(alfd_ctx *ctx, int h, int l, int64_t n) {
  LevelStore &S = ctx->hier[h].ml[l].loc;
  S.n = n;
  S.npad = pad_chunk(n);
  RC(store_vectors(ctx, S, true));
  if (l > 0) RC(ws_alloc_zero(ctx, &S.dinv, S.npad));
  return ALFD_OK;
}
static int level_penalty(alfd_ctx *ctx, int h, int l, int64_t goff) {
  const alfd_config &c = ctx->cfg;
  MlLevel &L = ctx->hier[h].ml[l];
  LevelStore &S = L.loc;
  if (l == 0) {
    S.dinv = h == 0 ? ctx->dinv_aug : ctx->dinv_a22;
    L.lmax = ctx->lam_max[h == 0 ? OP_AUG : OP_A22];
    return ALFD_OK;
  }
  PhaseClock pc(ctx, ALFD_SETUP_ML_LAMBDA);
  const AugOp F = level_view(ctx, h, l).op;
  RC(diag_plus_m(ctx, S.A, S.Ct, c.aug_assembled ? 0.0 : F.gamma, S.n, S.dinv));
  // the work vectors of the power iteration: zero after alfd_setup's allocation, whatever a solve left there otherwise
  HIPC(hipMemsetAsync(S.t, 0, S.npad * sizeof(double), ctx->stream));
  HIPC(hipMemsetAsync(S.r, 0, S.npad * sizeof(double), ctx->stream));
  return aug_lambda_max(ctx, F, S.n, goff, S.t, S.r, &L.lmax);
}

// The next level Nx through a general CSR prolongator Pm (single rank): A_c = P^T (A P), C_c = C P, Ct_c = C_c^T from the
// device operators dA, dC.  The three products run on the device (spgemm_rows_kernel; results fetched for the format
// planner) when gpu_products allows and they fit, else on the host from hA / hC (null: fetched from the device here).
// An, Cn, Ctn return the host copies of the new level.
//
// Two halves, each with its own fallback (the device and the host product have the same bits, so which of them ran
// never shows): csr_level_A uploads P, R = P^T and A_c and depends on A and P alone; csr_level_C forms C_c and Ct_c
// with the P that csr_level_A uploaded.  alfd_setup runs both, alfd_setup_coupling only the second.
static int csr_level_A(alfd_ctx *ctx, const HostCsr &Pm, DevCsr &dA, bool gpu_products, const HostCsr *hA, LevelStore &Nx,
                       HostCsr &An) {
  HostCsr R;
  {
    PhaseClock pc(ctx, ALFD_SETUP_ML_UPLOAD);
    transpose_host(Pm, R);
    RC(upload_level_part(ctx, Nx.P, Pm, nullptr, true));
    RC(upload_level_part(ctx, Nx.R, R, nullptr, true));
    ctx->setup_counts[ALFD_SC_TRANSFER_UPLOADS] += 2;
  }
  bool done = false;
  if (gpu_products && !dA.sparse && !Nx.P.sparse && !Nx.R.sparse && dA.nnz > 0) {
    PhaseClock pc(ctx, ALFD_SETUP_ML_GALERKIN);
    DevRawCsr AP, RAP;
    bool f1 = false, f2 = false;
    RC(dev_spgemm(ctx, dA.nrows, dA.rp, dA.col, dA.val, Nx.P.rp, Nx.P.col, Nx.P.val, Pm.ncols, AP, &f1));
    if (f1) RC(dev_spgemm(ctx, Nx.R.nrows, Nx.R.rp, Nx.R.col, Nx.R.val, AP.rp, AP.col, AP.val, Pm.ncols, RAP, &f2));
    AP.release();
    if (f2) {
      RC(download_raw(ctx, RAP, An));
      done = true;
    }
    RAP.release();
  }
  if (!done) {
    HostCsr fA;
    if (!hA) {
      PhaseClock pc(ctx, ALFD_SETUP_ML_FETCH);
      RC(download_csr(ctx, dA, fA));
    }
    PhaseClock pc(ctx, ALFD_SETUP_ML_GALERKIN);
    HostCsr AP;
    spgemm_host(hA ? *hA : fA, Pm, AP);
    spgemm_host(R, AP, An);
  }
  ctx->setup_counts[ALFD_SC_PRODUCTS_A] += 2;
  PhaseClock pc(ctx, ALFD_SETUP_ML_UPLOAD);
  RC(upload_level_part(ctx, Nx.A, An, nullptr, false));
  ctx->setup_counts[ALFD_SC_LEVEL_A_UPLOADS]++;
  return ALFD_OK;
}

static int csr_level_C(alfd_ctx *ctx, const HostCsr &Pm, DevCsr &dC, bool gpu_products, const HostCsr *hC, LevelStore &Nx,
                       HostCsr &Cn, HostCsr &Ctn) {
  bool done = false;
  if (gpu_products && !dC.sparse && !Nx.P.sparse) {
    PhaseClock pc(ctx, ALFD_SETUP_ML_GALERKIN);
    DevRawCsr CP;
    bool f3 = false;
    RC(dev_spgemm(ctx, dC.nrows, dC.rp, dC.col, dC.val, Nx.P.rp, Nx.P.col, Nx.P.val, Pm.ncols, CP, &f3));
    if (f3) {
      RC(download_raw(ctx, CP, Cn));
      done = true;
    }
    CP.release();
  }
  if (!done) {
    HostCsr fC;
    if (!hC) {
      PhaseClock pc(ctx, ALFD_SETUP_ML_FETCH);
      RC(download_csr(ctx, dC, fC));
    }
    PhaseClock pc(ctx, ALFD_SETUP_ML_GALERKIN);
    spgemm_host(hC ? *hC : fC, Pm, Cn);
  }
  {
    PhaseClock pc(ctx, ALFD_SETUP_ML_GALERKIN);
    transpose_host(Cn, Ctn);
  }
  ctx->setup_counts[ALFD_SC_PRODUCTS_C]++;
  PhaseClock pc(ctx, ALFD_SETUP_ML_UPLOAD);
  RC(upload_level_part(ctx, Nx.C, Cn, nullptr, false));
  RC(upload_level_part(ctx, Nx.Ct, Ctn, nullptr, false));
  return ALFD_OK;
}

// full: alfd_setup, everything.  Otherwise alfd_setup_coupling on the hierarchy a full setup left (one rank, CSR
// prolongators throughout; checked by the caller): A_l, P_l, R_l and the level vectors stay, the patch, the penalty
// parts of every level and the coarsest inverse are redone, and with c_changed (CT or C uploaded) C_l and Ct_l as well.
static int ml_setup(alfd_ctx *ctx, bool full, bool c_changed) {
  const alfd_config &c = ctx->cfg;
  ctx->dots_replicated = false;   // the Krylov dots reduce across ranks, whatever an earlier setup left behind
  if (c.ml_smooth_degree < 1 || c.ml_coarse_degree < 1 || !(c.ml_smooth_ratio > 1.0) || !(c.ml_coarse_ratio > 1.0))
    return ctx->err = "bad multilevel parameters", ALFD_E_INVALID;
  // before the dispatch to the replicated setup: a ratio <= 1 (or NaN) makes delta <= 0 and the patch polynomial NaN
  if (c.ml_patch_degree < 0) return ctx->err = "negative ml_patch_degree", ALFD_E_INVALID;
  if (c.ml_patch_degree > 0 && !(c.ml_patch_ratio > 1.0)) return ctx->err = "bad ml_patch_ratio", ALFD_E_INVALID;
  int nlev = 0;
  bool any_P = false;
  while (nlev < ALFD_MAX_LEVELS && (!ctx->hier[0].agg[nlev].empty() || !ctx->hier[0].P[nlev].rp.empty())) {
    any_P = any_P || !ctx->hier[0].P[nlev].rp.empty();
    ++nlev;
  }
  if (nlev == 0)
    return ctx->err = "alfd_set_aggregates / alfd_set_prolongator must precede alfd_setup for ALFD_PREC_MULTILEVEL", ALFD_E_NOT_SETUP;
  if (ctx->nranks > 1 && any_P) return ml_setup_rep_prolongators(ctx, nlev);
  if (ctx->nranks > 1 && (c.ml_patch_degree > 0 || c.ml_coarse_direct > 0))
    return ctx->err = "partitioned context: the interface patch and the direct coarsest solve need CSR prolongators", ALFD_E_UNSUPPORTED;
  const int rk = ctx->rank, last = ctx->nblocks - 1;
  // rank offsets of every level's unknowns: level 0 = block 0, level l+1 = ml_coff[l]
  std::vector<std::vector<int64_t>> off(nlev + 1);
  if (ctx->nranks > 1) {
    off[0] = ctx->part[0];
    for (int l = 0; l < nlev; ++l) {
      if ((int)ctx->ml_coff[l].size() != ctx->nranks + 1 || ctx->ml_coff[l].back() != ctx->hier[0].ncoarse[l])
        return ctx->err = "alfd_set_aggregate_partition missing or inconsistent for level " + std::to_string(l),
               ALFD_E_INVALID;
      off[l + 1] = ctx->ml_coff[l];
    }
  } else {
    off[0] = {0, ctx->n[0]};
    for (int l = 0; l < nlev; ++l) off[l + 1] = {0, ctx->hier[0].ncoarse[l]};
  }
  for (int l = 0; l < nlev; ++l) {
    const bool isP = !ctx->hier[0].P[l].rp.empty();
    if ((isP ? ctx->hier[0].P[l].nrows : (int64_t)ctx->hier[0].agg[l].size()) != off[l][rk + 1] - off[l][rk])
      return ctx->err = "aggregates / prolongator of level " + std::to_string(l) + " do not match this rank's unknowns", ALFD_E_INVALID;
  }
  if (full) {
    free_levels(ctx);
    ctx->hier[0].ml.assign(nlev + 1, MlLevel());
  } else {
    free_coupling(ctx, 0, c_changed);
  }
  // multi-rank: levels with few unknowns are replicated on every rank after the partitioned build
  // (their kernels take microseconds, their halo exchanges would dominate)
  int rep_from = -1;
  if (ctx->nranks > 1 && ctx->ml_rep_threshold > 0)
    for (int l = 1; l <= nlev; ++l)
      if (off[l].back() <= ctx->ml_rep_threshold) {
        rep_from = l;
        break;
      }
  struct Stash {
    HostCsr A, C, Ct, P, R;
  };
  std::vector<Stash> stash(nlev + 1);
  HostCsr A, C, Ct, An, Cn, Ctn, P, R;
  // Host copies: C and Ct are small and always fetched.  A (21 GB at N = 74) only when a level needs it on the host:
  // the aggregation levels' product, or a CSR-prolongator level whose product does not fit the device kernel.  The
  // device products (ALFD_ML_GPU_GALERKIN=0 switches them off) and the device-side patch-row gather need no host A.
  bool have_host_A = false;
  auto fetch_A = [&](const DevCsr &dA) -> int {
    if (have_host_A) return ALFD_OK;
    PhaseClock pc(ctx, ALFD_SETUP_ML_FETCH);
    RC(download_csr(ctx, dA, A));
    have_host_A = true;
    return ALFD_OK;
  };
  {
    PhaseClock pc(ctx, ALFD_SETUP_ML_FETCH);
    RC(download_csr(ctx, ctx->mat[ALFD_C], C));
    RC(download_csr(ctx, ctx->mat[ALFD_CT], Ct));
  }
  const bool gpu_products = ctx->ml_gpu_galerkin && ctx->nranks == 1;
  if (full && (!gpu_products || ctx->hier[0].P[0].rp.empty())) RC(fetch_A(ctx->mat[ALFD_A]));
  const int64_t lam0 = ctx->nranks > 1 ? ctx->part[last][rk] : 0;
  const int64_t lam_global = ctx->nranks > 1 ? ctx->part[last].back() : ctx->n[last];
  if (c.ml_patch_degree > 0) {
    PhaseClock pc(ctx, ALFD_SETUP_ML_PATCH);
    RC(patch_setup(ctx, have_host_A ? &A : nullptr, C, Ct));
  }
  for (int l = 0; l <= nlev; ++l) {
    LevelStore &L = ctx->hier[0].ml[l].loc;
    const int64_t n = off[l][rk + 1] - off[l][rk];
    if (full) RC(level_vectors(ctx, 0, l, n));
    RC(level_penalty(ctx, 0, l, off[l][rk]));
    if (l == nlev) break;
    if (!ctx->hier[0].P[l].rp.empty()) {
      // ---- next level through a general CSR prolongator (single rank)
      LevelStore &Nx = ctx->hier[0].ml[l + 1].loc;
      if (full)
        RC(csr_level_A(ctx, ctx->hier[0].P[l], l == 0 ? ctx->mat[ALFD_A] : L.A, gpu_products, have_host_A ? &A : nullptr, Nx, An));
      if (full || c_changed)
        RC(csr_level_C(ctx, ctx->hier[0].P[l], l == 0 ? ctx->mat[ALFD_C] : L.C, gpu_products, &C, Nx, Cn, Ctn));
      if (l + 1 < nlev) {
        // host copies of the new level: the next level's fallback product, aggregation levels
        if (full) A = std::move(An), have_host_A = true;
        if (full || c_changed) C = std::move(Cn), Ct = std::move(Ctn);
      }
      continue;
    }
    // ---- next level: Galerkin products of this rank's rows
    if (l == 0) RC(fetch_A(ctx->mat[ALFD_A]));
    const std::vector<int32_t> &aggG = ctx->hier[0].agg[l];  // owned fine dof -> GLOBAL coarse id (or -1)
    const double *w = ctx->hier[0].wgt[l].empty() ? nullptr : ctx->hier[0].wgt[l].data();
    if (w && ctx->nranks > 1) return ctx->err = "weighted aggregates are single-rank for now", ALFD_E_UNSUPPORTED;
    const int64_t c0 = off[l + 1][rk], nc_loc = off[l + 1][rk + 1] - c0, nc_glob = off[l + 1].back();
    std::vector<int32_t> agg_rows(n);  // owned fine dof -> LOCAL coarse row
    for (int64_t i = 0; i < n; ++i) {
      if (aggG[i] >= 0 && (aggG[i] < c0 || aggG[i] >= c0 + nc_loc))
        return ctx->err = "an aggregate spans two ranks", ALFD_E_INVALID;
      agg_rows[i] = aggG[i] < 0 ? -1 : (int32_t)(aggG[i] - c0);
    }
    DevCsr &dA = l == 0 ? ctx->mat[ALFD_A] : L.A;
    DevCsr &dC = l == 0 ? ctx->mat[ALFD_C] : L.C;
    DevCsr &dCt = l == 0 ? ctx->mat[ALFD_CT] : L.Ct;
    std::vector<int32_t> aggA, aggC;
    RC(exchange_ids(ctx, dA, aggG, aggA));   // columns of A_l: [owned | halo of A_l]
    RC(exchange_ids(ctx, dC, aggG, aggC));   // columns of C_l: [owned | halo of C_l]
    auto tg0 = std::chrono::steady_clock::now();
    galerkin(A, agg_rows.data(), w, nc_loc, aggA.data(), w, nc_glob, An);
    galerkin(C, nullptr, nullptr, C.nrows, aggC.data(), w, nc_glob, Cn);
    // Ct_{l+1} = P^T Ct_l: rows grouped by aggregate, multiplier columns back to GLOBAL ids
    const std::vector<int32_t> lam_ids = global_cols(dCt, lam0);
    galerkin(Ct, agg_rows.data(), w, nc_loc, lam_ids.data(), nullptr, lam_global, Ctn);
    // transfers are rank-local: P (n x nc_loc, one entry per represented row), R = P^T
    P.nrows = n;
    P.ncols = nc_loc;
    P.rp.assign(n + 1, 0);
    P.col.clear();
    P.val.clear();
    for (int64_t i = 0; i < n; ++i) {
      if (agg_rows[i] >= 0) {
        P.col.push_back(agg_rows[i]);
        P.val.push_back(w ? w[i] : 1.0);
      }
      P.rp[i + 1] = (int64_t)P.col.size();
    }
    transpose_host(P, R);
    ctx->setup_s[ALFD_SETUP_ML_GALERKIN] += std::chrono::duration<double>(std::chrono::steady_clock::now() - tg0).count();
    LevelStore &Nx = ctx->hier[0].ml[l + 1].loc;
    PhaseClock pc(ctx, ALFD_SETUP_ML_UPLOAD);
    RC(upload_level_part(ctx, Nx.A, An, off[l + 1].data(), false));
    RC(upload_level_part(ctx, Nx.C, Cn, off[l + 1].data(), false));
    RC(upload_level_part(ctx, Nx.Ct, Ctn, ctx->nranks > 1 ? ctx->part[last].data() : nullptr, false));
    RC(upload_level_part(ctx, Nx.P, P, nullptr, true));
    RC(upload_level_part(ctx, Nx.R, R, nullptr, true));
    // counted as the CSR-prolongator path counts: P^T (A P), formed by galerkin() in one pass, is two products with an
    // A_l operand; C P is one with a C_l operand, and Ct_{l+1} = P^T Ct_l stands where that path transposes C_{l+1}
    ctx->setup_counts[ALFD_SC_PRODUCTS_A] += 2;
    ctx->setup_counts[ALFD_SC_PRODUCTS_C]++;
    ctx->setup_counts[ALFD_SC_LEVEL_A_UPLOADS]++;
    ctx->setup_counts[ALFD_SC_TRANSFER_UPLOADS] += 2;
    if (rep_from > 0 && l + 1 >= rep_from) {
      stash[l + 1].A = An;  // global column ids
      stash[l + 1].C = Cn;
      stash[l + 1].Ct = Ctn;
      stash[l + 1].P = P;   // rank-local ids
      stash[l + 1].R = R;
    }
    // host copies of the new level in its LOCAL column space, for the next Galerkin step
    if (l + 1 < nlev) {
      RC(download_csr(ctx, Nx.A, A));
      RC(download_csr(ctx, Nx.C, C));
      RC(download_csr(ctx, Nx.Ct, Ct));
    }
  }
  if (c.ml_coarse_direct > 0 && ctx->hier[0].ml[nlev].loc.n > 0 && ctx->hier[0].ml[nlev].loc.n <= c.ml_coarse_direct) {
    // An / Cn / Ctn still hold the coarsest level (global = local column ids on one rank): kept for alfd_setup_coupling
    alfd_ctx::Hierarchy &H = ctx->hier[0];
    if (full) H.coarse_A = std::move(An);
    if (full || c_changed) H.coarse_C = std::move(Cn), H.coarse_Ct = std::move(Ctn);
    std::vector<double> w(ctx->n[last]);
    HIPC(hipMemcpyAsync(w.data(), ctx->diag[ALFD_INVW], w.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    PhaseClock pc(ctx, ALFD_SETUP_ML_COARSE);
    RC(coarse_inverse(ctx, H.coarse_A, H.coarse_C, H.coarse_Ct, w, c.gamma, H.inv));
  }
  if (rep_from > 0) {
    // ---- replicate levels rep_from .. nlev: gather operators, diagonals and W on every rank
    const int64_t lam_pad = pad_chunk(lam_global);
    RC(ws_alloc_zero(ctx, &ctx->g_w, lam_pad));
    RC(ws_alloc_zero(ctx, &ctx->g_tlam, lam_pad));
    RC(gather_vec(ctx, ctx->diag[ALFD_INVW], ctx->n[last], ctx->g_w));
    for (int l = rep_from; l <= nlev; ++l) {
      MlLevel &L = ctx->hier[0].ml[l];
      const int64_t n_all = off[l].back();
      HostCsr wholeA, wholeC, wholeCt, g;
      RC(gather_csr(ctx, stash[l].A, nullptr, n_all, wholeA));
      RC(gather_csr(ctx, stash[l].C, nullptr, n_all, wholeC));
      RC(gather_csr(ctx, stash[l].Ct, nullptr, lam_global, wholeCt));
      RC(replicate_level(ctx, l, wholeA, wholeC, wholeCt, off[l], l == rep_from));
      if (l > rep_from) {
        RC(gather_csr(ctx, stash[l].P, off[l].data(), n_all, g));        // n_{l-1} x n_l
        RC(upload_level_part(ctx, L.rep.P, g, nullptr, true));
        RC(gather_csr(ctx, stash[l].R, off[l - 1].data(), off[l - 1].back(), g));  // n_l x n_{l-1}
        RC(upload_level_part(ctx, L.rep.R, g, nullptr, true));
        L.rep.P.rep = L.rep.R.rep = true;
      }
      RC(gather_vec(ctx, L.loc.dinv, L.loc.n, L.rep.dinv));
    }
    ctx->ml_rep_level = rep_from;
  }
  for (int l = 0; l <= nlev; ++l)
  {
    RC(build_tail_mask(ctx, 0, l == 0 ? ctx->mat[ALFD_CT] : ctx->hier[0].ml[l].loc.Ct, ctx->hier[0].ml[l].loc.npad, &ctx->hier[0].ml[l].tail_mask));
    RC(build_tail_vectors(ctx, 0, l));
  }
  return ALFD_OK;
}

// The second hierarchy (ALFD_PREC_MULTILEVEL on an elliptic variant): the V-cycle for A22 = A2 + gamma2 M invW M, built
// from (A2, M, M, invW, gamma2) by the steps hierarchy 0 takes on (A, C, Ct, invW, gamma) -- level_vectors / level_penalty,
// csr_level_A / csr_level_C, the
// explicit coarsest inverse, the masks of the fused smoother.  CSR prolongators, one rank, no interface patch (M touches
// every row).  Without prolongators of block 1 there is no such hierarchy and A22 keeps the Chebyshev sweep.
// full / c_changed as in ml_setup, c_changed standing for an upload of M.
static int ml_setup_immersed(alfd_ctx *ctx, bool full, bool c_changed) {
  const alfd_config &c = ctx->cfg;
  alfd_ctx::Hierarchy &H = ctx->hier[1];
  int nlev = 0;
  H.tail_tab = nullptr;
  while (nlev < ALFD_MAX_LEVELS && !H.P[nlev].rp.empty()) ++nlev;
  if (nlev == 0) return ALFD_OK;
  if (!is_elliptic(c.variant))
    return ctx->err = "a block-1 hierarchy needs the immersed operators A2 and M of the elliptic-interface variants", ALFD_E_INVALID;
  if (ctx->nranks > 1) return ctx->err = "the block-1 hierarchy is single-rank", ALFD_E_UNSUPPORTED;
  for (int l = 0; l < nlev; ++l)
    if (H.P[l].nrows != (l == 0 ? ctx->n[1] : H.P[l - 1].ncols))
      return ctx->err = "block-1 prolongator of level " + std::to_string(l) + " does not match the unknowns of that level",
             ALFD_E_INVALID;
  if (full)
    H.ml.assign(nlev + 1, MlLevel());
  else
    free_coupling(ctx, 1, c_changed);
  const bool gpu_products = ctx->ml_gpu_galerkin != 0;
  HostCsr An, Cn, Ctn, A, C;
  for (int l = 0; l <= nlev; ++l) {
    LevelStore &L = H.ml[l].loc;
    if (full) RC(level_vectors(ctx, 1, l, l == 0 ? ctx->n[1] : H.ncoarse[l - 1]));
    RC(level_penalty(ctx, 1, l, 0));
    if (l == nlev) break;
    LevelStore &Nx = H.ml[l + 1].loc;
    if (full) RC(csr_level_A(ctx, H.P[l], l == 0 ? ctx->mat[ALFD_A2] : L.A, gpu_products, l == 0 ? nullptr : &A, Nx, An));
    if (full || c_changed)
      RC(csr_level_C(ctx, H.P[l], l == 0 ? ctx->mat[ALFD_M] : L.C, gpu_products, l == 0 ? nullptr : &C, Nx, Cn, Ctn));
    if (l + 1 < nlev) {
      if (full) A = std::move(An);
      if (full || c_changed) C = std::move(Cn);
    }
  }
  if (c.ml_coarse_direct > 0 && H.ml[nlev].loc.n <= c.ml_coarse_direct) {
    if (full) H.coarse_A = std::move(An);
    if (full || c_changed) H.coarse_C = std::move(Cn), H.coarse_Ct = std::move(Ctn);
    std::vector<double> w(ctx->n[2]);
    HIPC(hipMemcpyAsync(w.data(), ctx->diag[ALFD_INVW], w.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    PhaseClock pc(ctx, ALFD_SETUP_ML_COARSE);
    RC(coarse_inverse(ctx, H.coarse_A, H.coarse_C, H.coarse_Ct, w, c.gamma2, H.inv));
  }
  for (int l = 0; l <= nlev; ++l)
  {
    RC(build_tail_mask(ctx, 1, l == 0 ? ctx->mat[ALFD_M] : H.ml[l].loc.Ct, H.ml[l].loc.npad, &H.ml[l].tail_mask));
    RC(build_tail_vectors(ctx, 1, l));
  }
  return build_tail_table(ctx);
}

// 1 / diag(M) of the exact W^-1 into dinv_m (allocated, padding zero), from the host copy of slot M
static int mass_diagonal(alfd_ctx *ctx) {
  const HostCsr &M = ctx->h_M;
  const int last = ctx->nblocks - 1;
  if (!ctx->mat[ALFD_M].present || M.rp.empty() || M.nrows != ctx->n[last])
    return ctx->err = "slot M (immersed mass matrix) must be set for the exact W^-1", ALFD_E_NOT_SETUP;
  const int64_t nlp = pad_chunk(ctx->n[last]);
  const int64_t row0 = ctx->nranks > 1 ? ctx->part[last][ctx->rank] : 0;
  std::vector<double> dm(nlp, 0.0);
  for (int64_t i = 0; i < M.nrows; ++i) {
    double dii = 0.0;
    for (int64_t k = M.rp[i]; k < M.rp[i + 1]; ++k)
      if (M.col[k] == row0 + i) dii = M.val[k];
    if (!(dii > 0.0)) return ctx->err = "mass matrix needs a positive diagonal", ALFD_E_INVALID;
    dm[i] = 1.0 / dii;
  }
  HIPC(hipMemcpyAsync(ctx->dinv_m, dm.data(), nlp * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  return ALFD_OK;
}

// 1 / diag and lambda_max of the inner operators into the vectors setup() allocated: everything here follows the
// coupling, invW or a penalty weight
static int diag_lambda(alfd_ctx *ctx) {
  const alfd_config &c = ctx->cfg;
  const bool ell = is_elliptic(c.variant);
  const bool gd_off = !c.grad_div_in_A && (c.variant == ALFD_AL_STOKES || c.variant == ALFD_AL_STOKES_DIAG);
  const bool cheb = c.inner_prec == ALFD_PREC_CHEBYSHEV || c.inner_prec == ALFD_PREC_MULTILEVEL;
  const int64_t n0p = pad_chunk(ctx->n[0]);
  for (int k = 0; k < 7; ++k) ctx->lam_max[k] = 0;
  // diag(Aug) = diag(A) + gamma sum_k w_k Ct_ik^2 (no product matrix is formed)
  PhaseClock diag_clock(ctx, ALFD_SETUP_DIAG_LAMBDA);
  if (gd_off) {
    // d_i = fma(gamma_gd, sum_k l_k b_ki^2, fma(gamma, sum_k w_k c_ki^2, a_ii)), then 1 / d_i: the diagonal of the
    // surrogate Aug the inner preconditioner sees (op_apply, exact_w = false); DESIGN section 4
    RC(diag_plus_m(ctx, &ctx->mat[ALFD_A], ctx->mat[ALFD_CT], ctx->diag[ALFD_INVW], c.gamma, ctx->n[0], ctx->dA, false));
    RC(diag_plus_m(ctx, nullptr, ctx->mat[ALFD_BT], ctx->diag[ALFD_MP_LUMPED_INV], c.gamma_grad_div, ctx->n[0],
                   ctx->dinv_aug, true));
  } else {
    RC(diag_plus(ctx, ALFD_A, ALFD_CT, c.aug_assembled ? 0.0 : c.gamma, ctx->n[0], ctx->dinv_aug));
  }
  if (ell) {
    // diag(A22_aug) = diag(A2) + gamma2 sum_k w_k M_ik^2
    RC(diag_plus(ctx, ALFD_A2, ALFD_M, c.gamma2, ctx->n[1], ctx->dinv_a22));
    if (c.variant == ALFD_AL_ELL_IDEAL) {
      HIPC(hipMemcpyAsync(ctx->dinv_aug2, ctx->dinv_aug, n0p * sizeof(double), hipMemcpyDeviceToDevice,
                          ctx->stream));
      HIPC(hipMemcpyAsync(ctx->dinv_aug2 + ctx->off[1], ctx->dinv_a22, pad_chunk(ctx->n[1]) * sizeof(double),
                          hipMemcpyDeviceToDevice, ctx->stream));
      if (cheb) RC(power_iteration(ctx, OP_AUG2));
    }
    // the modified variant's two inner CGs; the ideal one's block-diagonal multilevel preconditioner smooths with them too
    if (cheb && (c.variant == ALFD_AL_ELL_MODIFIED || c.inner_prec == ALFD_PREC_MULTILEVEL)) {
      RC(power_iteration(ctx, OP_AUG));
      RC(power_iteration(ctx, OP_A22));
    }
  } else if (cheb) {
    RC(power_iteration(ctx, OP_AUG));
  }
  ctx->lambda_max = ctx->lam_max[c.variant == ALFD_AL_ELL_IDEAL ? OP_AUG2 : OP_AUG];
  return ALFD_OK;
}

// The checks of gamma and gamma2 -- the two fields alfd_setup_coupling takes anew -- that both kinds of setup make:
// parameter sanity the reference asserts (elliptic_interface.cc:874-884, 912-920).  Reads the context only.
static int check_penalty_weights(alfd_ctx *ctx) {
  const alfd_config &c = ctx->cfg;
  if (c.variant == ALFD_AL_ELL_MODIFIED && c.gamma2 > 20.0)
    return ctx->err = "gamma_AL_immersed is too large for modified AL preconditioner", ALFD_E_INVALID;
  if (c.variant == ALFD_AL_ELL_MODIFIED && std::fabs(c.gamma2 - c.gamma) <= 1e-1)
    return ctx->err = "modified AL preconditioner: gamma_1 and gamma_2 should not be too close", ALFD_E_INVALID;
  if (c.variant == ALFD_AL_ELL_IDEAL && std::fabs(c.gamma - c.gamma2) >= 1e-12)
    return ctx->err = "ideal AL preconditioner: gamma must be identical", ALFD_E_INVALID;
  return ALFD_OK;
}

static void setup_begin(alfd_ctx *ctx) {
  for (int ph = ALFD_SETUP_DIAG_LAMBDA; ph < ALFD_SETUP_NPHASES; ++ph) ctx->setup_s[ph] = 0.0;
  for (int64_t &k : ctx->setup_counts) k = 0;
  ctx->upload_since_setup = false;
  ctx->is_setup = false;
  ctx->coupling_ready = false;   // until this setup succeeds
  ctx->a32_used = false;         // the setup itself runs on the 8-byte values of A
}
// a setup of either kind succeeded: what alfd_setup_coupling compares the next call against
static void setup_done(alfd_ctx *ctx, bool coupling_ready) {
  std::copy(ctx->gen, ctx->gen + ALFD_NSLOTS + 1, ctx->gen_setup);
  std::copy(ctx->dgen, ctx->dgen + ALFD_NDIAGS, ctx->dgen_setup);
  ctx->cfg_setup = ctx->cfg;
  ctx->needs_full = nullptr;
  ctx->coupling_ready = coupling_ready;
  ctx->is_setup = true;
  a32_decide_used(ctx);
}

static int setup(alfd_ctx *ctx) {
  if (!ctx->configured) return ctx->err = "alfd_configure not called", ALFD_E_NOT_SETUP;
  setup_begin(ctx);
  const alfd_config &c = ctx->cfg;
  const bool rat = c.variant == ALFD_RATIONAL;
  if (rat && ctx->nranks > 1) return ctx->err = "rational variant is single-rank", ALFD_E_UNSUPPORTED;
  if (c.outer_solver == ALFD_OUTER_MINRES && c.restart < 4)
    return ctx->err = "MinRes needs restart >= 4 (vector arena)", ALFD_E_INVALID;
  if (c.restart < 1 || c.restart > kMaxBasis - 1) return ctx->err = "restart out of range", ALFD_E_INVALID;
  if (c.fgmres_flavour != ALFD_FGMRES_DEALII_96 && c.fgmres_flavour != ALFD_FGMRES_DEALII_95)
    return ctx->err = "unknown alfd_config::fgmres_flavour", ALFD_E_INVALID;
  if (c.fgmres_flavour == ALFD_FGMRES_DEALII_95 && c.restart < 2)
    return ctx->err = "the deal.II <= 9.5 FGMRES loop needs restart >= 2", ALFD_E_INVALID;
  const bool ell = is_elliptic(c.variant);
  const bool gd_off = !c.grad_div_in_A && (c.variant == ALFD_AL_STOKES || c.variant == ALFD_AL_STOKES_DIAG);
  if (gd_off && c.inner_prec == ALFD_PREC_MULTILEVEL)
    return ctx->err = "grad_div_in_A = 0: no multilevel inner preconditioner (the reference throws ExcNotImplemented for "
                      "AMG without grad-div); use identity, Jacobi or Chebyshev",
           ALFD_E_UNSUPPORTED;
  if (gd_off && c.aug_assembled)
    return ctx->err = "grad_div_in_A = 0 needs the factored Aug (aug_assembled = 0)", ALFD_E_UNSUPPORTED;
  if ((c.inner_prec == ALFD_PREC_CHEBYSHEV || c.inner_prec == ALFD_PREC_MULTILEVEL) &&
      (c.cheb_degree < 1 || c.cheb_power_its < 1 || !(c.cheb_eig_ratio > 1.0)))
    return ctx->err = "bad Chebyshev parameters", ALFD_E_INVALID;
  RC(check_penalty_weights(ctx));
  ctx->nblocks = nblocks_of(c.variant);
  const int last = ctx->nblocks - 1;
  if (!ctx->mat[ALFD_A].present || !ctx->mat[ALFD_CT].present || !ctx->mat[ALFD_C].present ||
      (!ctx->diag[ALFD_INVW] && !rat))
    return ctx->err = "A, CT (and C) and INVW must be set", ALFD_E_NOT_SETUP;
  ctx->n[0] = ctx->mat[ALFD_A].nrows;
  ctx->n[last] = ctx->mat[ALFD_C].nrows;
  if (ctx->num.on() && ctx->num.n() != ctx->n[0])
    return ctx->err = "the numbering (alfd_set_numbering) does not have the size of block 0", ALFD_E_INVALID;
  if (rat) {
    const HostCsr &K = ctx->h_K, &M = ctx->h_M;
    if (K.rp.empty() || M.rp.empty()) return ctx->err = "KIMM and M must be set for the rational variant", ALFD_E_NOT_SETUP;
    if (K.nrows != ctx->n[1] || M.nrows != ctx->n[1] || K.col != M.col || K.rp != M.rp)
      return ctx->err = "KIMM and M must share one sparsity pattern (matrix.add)", ALFD_E_INVALID;
    if (!(c.rho_bound > 0)) return ctx->err = "rho_bound must be positive", ALFD_E_INVALID;
  }
  if (ell) {
    if (!ctx->mat[ALFD_A2].present || !ctx->mat[ALFD_M].present)
      return ctx->err = "A2 and M must be set for the elliptic-interface variants", ALFD_E_NOT_SETUP;
    ctx->n[1] = ctx->mat[ALFD_A2].nrows;
    if (ctx->n[1] != ctx->n[2] || ctx->mat[ALFD_M].nrows != ctx->n[1])
      return ctx->err = "elliptic interface: blocks 1 and 2 must have the same size", ALFD_E_INVALID;
  } else if (ctx->nblocks == 3) {
    if (!ctx->mat[ALFD_BT].present || !ctx->mat[ALFD_B].present || !ctx->mat[ALFD_MP].present ||
        !ctx->diag[ALFD_MP_LUMPED_INV])
      return ctx->err = "BT, B, MP and MP_LUMPED_INV must be set for the Stokes variants", ALFD_E_NOT_SETUP;
    ctx->n[1] = ctx->mat[ALFD_B].nrows;
  }
  if (ctx->mat[ALFD_CT].nrows != ctx->n[0] || (!rat && ctx->diag_n[ALFD_INVW] != ctx->n[last]))
    return ctx->err = "inconsistent block sizes", ALFD_E_INVALID;
  ctx->nmax = 0;
  for (int b = 0; b < ctx->nblocks; ++b) {
    ctx->off[b + 1] = ctx->off[b] + pad_chunk(ctx->n[b]);
    ctx->nmax = std::max(ctx->nmax, pad_chunk(ctx->n[b]));
  }
  // release the workspace of a previous setup()
  HIPC(hipStreamSynchronize(ctx->stream));
  for (void *p : ctx->ws_allocs) hipFree(p);
  ctx->ws_allocs.clear();
  spectrum_release(ctx);   // may point into the patch of the previous setup
  if (ctx->sc_host) hipHostFree(ctx->sc_host), ctx->sc_host = nullptr;
  const int64_t N = ctx->ntot(), n0p = pad_chunk(ctx->n[0]);
  ctx->wmax = c.variant == ALFD_AL_ELL_IDEAL ? ctx->off[2] : ctx->nmax;
  const int64_t wm = ctx->wmax;
  ctx->pstride = N / kChunk + 1;
  RC(ws_alloc_zero(ctx, &ctx->sc, kNumScalars));
  HIPC(hipHostMalloc((void **)&ctx->sc_host, kNumScalars * sizeof(double), hipHostMallocMapped));
  RC(ws_alloc_zero(ctx, &ctx->partial, (int64_t)(kMaxBasis + 2) * ctx->pstride));
  RC(ws_alloc_zero(ctx, &ctx->gather, (int64_t)ctx->nranks * (kMaxBasis + 2)));
  RC(ws_alloc_zero(ctx, &ctx->dinv_aug, n0p));
  RC(ws_alloc_zero(ctx, &ctx->dA, ctx->nmax));
  RC(ws_alloc_zero(ctx, &ctx->s_aug, ctx->nmax));
  ctx->diag_cap = ctx->nmax;
  RC(ws_alloc_zero(ctx, &ctx->w_r, wm));
  RC(ws_alloc_zero(ctx, &ctx->w_z, wm));
  RC(ws_alloc_zero(ctx, &ctx->w_p, wm));
  RC(ws_alloc_zero(ctx, &ctx->w_Ap, wm));
  RC(ws_alloc_zero(ctx, &ctx->c_d, wm));
  RC(ws_alloc_zero(ctx, &ctx->c_res, wm));
  RC(ws_alloc_zero(ctx, &ctx->c_tmp, wm));
  RC(ws_alloc_zero(ctx, &ctx->t_lam, pad_chunk(ctx->n[last])));
  RC(ws_alloc_zero(ctx, &ctx->q_tmp, ctx->nmax));
  RC(ws_alloc_zero(ctx, &ctx->rhs_tmp, std::max(n0p, wm)));
  RC(ws_alloc_zero(ctx, &ctx->V, (int64_t)(c.restart + 1) * N));
  RC(ws_alloc_zero(ctx, &ctx->Z, (int64_t)c.restart * N));
  RC(ws_alloc_zero(ctx, &ctx->xb, N));
  RC(ws_alloc_zero(ctx, &ctx->bb, N));
  RC(ws_alloc_zero(ctx, &ctx->io, N));
  RC(ws_alloc_zero(ctx, &ctx->st_in, N));
  RC(ws_alloc_zero(ctx, &ctx->st_out, N));
  for (int k = 0; k < 7; ++k) ctx->lam_max[k] = 0;
  if (ctx->n_sc_host) hipHostFree(ctx->n_sc_host), ctx->n_sc_host = nullptr;
  ctx->n_owner = NESTED_FREE;
  // the n_* set of the nested solves (mass_solve, nested_mp_solve): as long as the longer of the two blocks
  // (and the CG of alfd_estimate_spectrum on the multiplier block, which is there for every variant)
  const int64_t n_nested = std::max<int64_t>(pad_chunk(ctx->n[last]), gd_off ? pad_chunk(ctx->n[1]) : 0);
  {
    RC(ws_alloc_zero(ctx, &ctx->n_r, n_nested));
    RC(ws_alloc_zero(ctx, &ctx->n_z, n_nested));
    RC(ws_alloc_zero(ctx, &ctx->n_p, n_nested));
    RC(ws_alloc_zero(ctx, &ctx->n_Ap, n_nested));
    RC(ws_alloc_zero(ctx, &ctx->n_sc, kNumScalars));
    HIPC(hipHostMalloc((void **)&ctx->n_sc_host, kNumScalars * sizeof(double), hipHostMallocMapped));
    RC(ws_alloc_zero(ctx, &ctx->n_partial, (int64_t)(kMaxBasis + 2) * ctx->pstride));
    RC(ws_alloc_zero(ctx, &ctx->n_gather, (int64_t)ctx->nranks * (kMaxBasis + 2)));
  }
  if (gd_off) {
    RC(ws_alloc_zero(ctx, &ctx->gd_bx, pad_chunk(ctx->n[1])));
    RC(ws_alloc_zero(ctx, &ctx->gd_q, pad_chunk(ctx->n[1])));
  }
  if (c.w_inverse != ALFD_W_DIAGONAL) {
    // exact W^-1 = (M^-1)^2 or M^-1: nested Jacobi CG on the immersed mass matrix
    if (c.w_inverse != ALFD_W_MASS_INV_SQUARED && c.w_inverse != ALFD_W_MASS_INV)
      return ctx->err = "unknown alfd_config::w_inverse", ALFD_E_INVALID;
    if (rat) return ctx->err = "the rational variant has no W^-1", ALFD_E_UNSUPPORTED;
    const int64_t nlp = pad_chunk(ctx->n[last]);
    RC(ws_alloc_zero(ctx, &ctx->dinv_m, nlp));
    RC(ws_alloc_zero(ctx, &ctx->m_tmp, nlp));
    RC(ws_alloc_zero(ctx, &ctx->m_tmp2, nlp));
    RC(mass_diagonal(ctx));
  }
  const bool cheb = c.inner_prec == ALFD_PREC_CHEBYSHEV || c.inner_prec == ALFD_PREC_MULTILEVEL;
  if (rat) {
    // K_inv: Jacobi / Chebyshev-Jacobi CG on K itself
    RC(ws_alloc_zero(ctx, &ctx->dinv_k, n0p));
    extract_diag(ctx, ctx->mat[ALFD_A]);
    hipLaunchKernelGGL(inv_diag_kernel, dim3((unsigned)std::max<int64_t>(1, (ctx->n[0] + 255) / 256)), dim3(256), 0, ctx->stream,
                       ctx->n[0], ctx->dA, ctx->dinv_k);
    if (cheb) RC(power_iteration(ctx, OP_K));
    // block-diagonal matrix of the 21 immersed systems, segment s at rows/cols s*npl
    const HostCsr &K = ctx->h_K, &M = ctx->h_M;
    const int64_t n1 = ctx->n[1], npl = pad_chunk(n1), nnz1 = K.rp[n1];
    std::vector<int64_t> rp((size_t)npl * kRatSystems + 1, 0);
    std::vector<int32_t> col((size_t)nnz1 * kRatSystems);
    std::vector<double> val((size_t)nnz1 * kRatSystems);
    for (int sidx = 0; sidx < kRatSystems; ++sidx) {
      const double sh = sidx < 20 ? -(c.rho_bound * kRatPoles[sidx]) : 0.0;  // matrix.add(-rho p_i, M)
      for (int64_t r = 0; r < npl; ++r) {
        const int64_t gr = (int64_t)sidx * npl + r;
        rp[gr + 1] = rp[gr] + (r < n1 ? K.rp[r + 1] - K.rp[r] : 0);
      }
      for (int64_t k = 0; k < nnz1; ++k) {
        col[(size_t)sidx * nnz1 + k] = (int32_t)(K.col[k] + sidx * npl);
        val[(size_t)sidx * nnz1 + k] = sidx < 20 ? std::fma(sh, M.val[k], K.val[k]) : M.val[k];
      }
    }
    {
      // upload through the generic path into a scratch slot object
      RC(upload_matrix(ctx, kScratchSlot, npl * kRatSystems, npl * kRatSystems, rp.data(), col.data(),
                       val.data()));
      csr_free(ctx->rat_mat);
      ctx->rat_mat = std::move(ctx->mat[kScratchSlot]);
      ctx->mat[kScratchSlot] = DevCsr();
    }
    const int64_t nt = npl * kRatSystems;
    RC(ws_alloc_zero(ctx, &ctx->rt_r, nt));
    RC(ws_alloc_zero(ctx, &ctx->rt_z, nt));
    RC(ws_alloc_zero(ctx, &ctx->rt_p, nt));
    RC(ws_alloc_zero(ctx, &ctx->rt_Ap, nt));
    RC(ws_alloc_zero(ctx, &ctx->rt_x, nt));
    RC(ws_alloc_zero(ctx, &ctx->rt_dinv, nt));
    RC(ws_alloc_zero(ctx, &ctx->rt_partial, nt / kChunk + 1));
    RC(ws_alloc_zero(ctx, &ctx->rt_scb, kRatSystems * kBS));
    RC(ws_alloc_zero(ctx, &ctx->rt_coef, kRatSystems));
    if (ctx->rt_scb_host) hipHostFree(ctx->rt_scb_host), ctx->rt_scb_host = nullptr;
    HIPC(hipHostMalloc((void **)&ctx->rt_scb_host, kRatSystems * kBS * sizeof(double)));
    {
      // 1/diag of the shifted systems (same fma as the values above), 1 for the
      // unpreconditioned mass solve, 0 in the padding
      std::vector<double> dinv((size_t)nt, 0.0);
      for (int sidx = 0; sidx < kRatSystems; ++sidx) {
        const double sh = sidx < 20 ? -(c.rho_bound * kRatPoles[sidx]) : 0.0;
        for (int64_t r = 0; r < n1; ++r) {
          double d = 1.0;
          if (sidx < 20)
            for (int64_t k = K.rp[r]; k < K.rp[r + 1]; ++k)
              if (K.col[k] == r) d = 1.0 / std::fma(sh, M.val[k], K.val[k]);
          dinv[(size_t)sidx * npl + r] = d;
        }
      }
      HIPC(hipMemcpyAsync(ctx->rt_dinv, dinv.data(), nt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
      HIPC(hipStreamSynchronize(ctx->stream));
    }
    double coef[kRatSystems];
    for (int sidx = 0; sidx < 20; ++sidx) coef[sidx] = c.rho_bound * kRatRes[sidx + 1];
    coef[20] = kRatRes[0];
    HIPC(hipMemcpyAsync(ctx->rt_coef, coef, sizeof(coef), hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    ctx->lambda_max = ctx->lam_max[OP_K];
    setup_done(ctx, false);
    return ALFD_OK;
  }
  if (c.aug_assembled && is_elliptic(c.variant))
    return ctx->err = "aug_assembled (operator form) is implemented for the AL2 / Stokes variants", ALFD_E_UNSUPPORTED;
  if (ell) {
    RC(ws_alloc_zero(ctx, &ctx->dinv_a22, pad_chunk(ctx->n[1])));
    if (c.variant == ALFD_AL_ELL_IDEAL) RC(ws_alloc_zero(ctx, &ctx->dinv_aug2, ctx->off[2]));
  }
  RC(diag_lambda(ctx));
  free_levels(ctx);
  if (c.inner_prec == ALFD_PREC_MULTILEVEL) {
    if (c.variant == ALFD_AL_ELL_IDEAL &&
        (ctx->hier[1].P[0].rp.empty() || (ctx->hier[0].P[0].rp.empty() && ctx->hier[0].agg[0].empty())))
      return ctx->err = "multilevel inner preconditioner: the 2x2 block CG of the ideal variant needs a hierarchy on both "
                        "blocks (alfd_set_prolongator_block)", ALFD_E_UNSUPPORTED;
    RC(ml_setup(ctx, true, true));
    RC(ml_setup_immersed(ctx, true, true));
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  setup_done(ctx, true);
  return ALFD_OK;
}

// Do two configs differ in more than gamma, gamma2 and the stop rules of alfd_set_controls?
// alfd_config has no padding (the sum of its members, checked below), so comparing the bytes compares the fields
static_assert(sizeof(alfd_config) == 18 * sizeof(int32_t) + 9 * sizeof(double) + 5 * sizeof(alfd_control) &&
                  sizeof(alfd_control) == 2 * sizeof(int32_t) + 2 * sizeof(double),
              "alfd_config gained padding or a member: config_needs_setup compares its bytes");
static bool config_needs_setup(const alfd_config &now, const alfd_config &then) {
  alfd_config a = now;
  a.gamma = then.gamma, a.gamma2 = then.gamma2;
  a.outer = then.outer, a.inner = then.inner, a.mp_inner = then.mp_inner;
  return std::memcmp(&a, &then, sizeof(alfd_config)) != 0;
}

// alfd_setup_coupling: the coupling halves of setup() on the context a setup left.  Everything up to setup_begin only
// reads the context.
static int setup_coupling(alfd_ctx *ctx) {
  const alfd_config &c = ctx->cfg;
  const std::string fn = "alfd_setup_coupling: ";
  // the same answer on every rank, before any exchange
  if (ctx->nranks > 1) return ctx->err = fn + "partitioned contexts keep using alfd_setup", ALFD_E_UNSUPPORTED;
  if (ctx->configured && c.variant == ALFD_RATIONAL)
    return ctx->err = fn + "the rational variant keeps using alfd_setup", ALFD_E_UNSUPPORTED;
  if (!ctx->configured || !ctx->coupling_ready)
    return ctx->err = fn + "the context was never set up (alfd_setup first)", ALFD_E_NOT_SETUP;
  const bool ml = c.inner_prec == ALFD_PREC_MULTILEVEL;
  if (ctx->needs_full) return ctx->err = fn + ctx->needs_full + " since the last setup: needs alfd_setup", ALFD_E_INVALID;
  if (config_needs_setup(c, ctx->cfg_setup))
    return ctx->err = fn + "the configuration differs in more than gamma, gamma2 and the controls: needs alfd_setup",
           ALFD_E_INVALID;
  if (c.aug_assembled)
    return ctx->err = fn + "aug_assembled = 1 keeps the coupling inside A: needs alfd_setup", ALFD_E_INVALID;
  RC(check_penalty_weights(ctx));   // a gamma / gamma2 that alfd_setup refuses is refused here, with its message
  for (int s = 0; s < ALFD_NSLOTS; ++s)
    if (s != ALFD_CT && s != ALFD_C && s != ALFD_M && ctx->gen[s] != ctx->gen_setup[s])
      return ctx->err = fn + "matrix slot " + std::to_string(s) + " was uploaded since the last setup: needs alfd_setup",
             ALFD_E_INVALID;
  for (int s = 0; s < ALFD_NDIAGS; ++s)
    if (s != ALFD_INVW && ctx->dgen[s] != ctx->dgen_setup[s])
      return ctx->err = fn + "diagonal " + std::to_string(s) + " was uploaded since the last setup: needs alfd_setup",
             ALFD_E_INVALID;
  const int last = ctx->nblocks - 1;
  const DevCsr &Ct = ctx->mat[ALFD_CT], &C = ctx->mat[ALFD_C], &M = ctx->mat[ALFD_M];
  const bool uses_M = is_elliptic(c.variant) || c.w_inverse != ALFD_W_DIAGONAL;
  if (Ct.nrows != ctx->n[0] || Ct.ncols != ctx->n[last] || C.nrows != ctx->n[last] || C.ncols != ctx->n[0] ||
      ctx->diag_n[ALFD_INVW] != ctx->n[last] ||
      (uses_M && (!M.present || M.nrows != ctx->n[last] || M.ncols != ctx->n[last] || ctx->h_M.nrows != ctx->n[last])))
    return ctx->err = fn + "a block size changed: needs alfd_setup", ALFD_E_INVALID;
  if (ml) {
    int nlev = 0;
    while (nlev < ALFD_MAX_LEVELS && (!ctx->hier[0].agg[nlev].empty() || !ctx->hier[0].P[nlev].rp.empty())) {
      if (ctx->hier[0].P[nlev].rp.empty())
        return ctx->err = fn + "a hierarchy given as aggregates keeps using alfd_setup", ALFD_E_UNSUPPORTED;
      ++nlev;
    }
    if ((int)ctx->hier[0].ml.size() != nlev + 1)
      return ctx->err = fn + "the hierarchy is not the one of the last setup: needs alfd_setup", ALFD_E_INVALID;
  }
  const bool c_changed = ctx->gen[ALFD_CT] != ctx->gen_setup[ALFD_CT] || ctx->gen[ALFD_C] != ctx->gen_setup[ALFD_C];
  const bool m_changed = ctx->gen[ALFD_M] != ctx->gen_setup[ALFD_M];
  // hierarchy 1 reads (A2, M, M, invW, gamma2): untouched when none of the last three changed
  const bool h1_changed = m_changed || ctx->dgen[ALFD_INVW] != ctx->dgen_setup[ALFD_INVW] || c.gamma2 != ctx->cfg_setup.gamma2;
  // ---- from here on the context changes; a failure leaves it to alfd_setup
  setup_begin(ctx);
  HIPC(hipStreamSynchronize(ctx->stream));
  spectrum_release(ctx);   // may point into the patch
  ctx->n_owner = NESTED_FREE;
  if (c.w_inverse != ALFD_W_DIAGONAL) RC(mass_diagonal(ctx));
  RC(diag_lambda(ctx));
  if (ml) {
    RC(ml_setup(ctx, false, c_changed));
    if (h1_changed && !ctx->hier[1].ml.empty()) RC(ml_setup_immersed(ctx, false, m_changed));
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  setup_done(ctx, true);
  return ALFD_OK;
}

// at most 2048 workgroups, every one with the same number of chunks (up to one): 2527 chunks -> 1264 x 2
static unsigned block_grid(int64_t nchunks) {
  const int64_t per = (nchunks + 2047) / 2048;
  return (unsigned)((nchunks + per - 1) / per);
}

// alfd_set_numbering: every block-vector call checks that the numbering still fits block 0
static int numbering_fits(alfd_ctx *ctx) {
  if (ctx->num.on() && ctx->num.n() != ctx->n[0])
    return ctx->err = "the numbering (alfd_set_numbering) has " + std::to_string((long long)ctx->num.n()) +
                      " entries, block 0 has " + std::to_string((long long)ctx->n[0]), ALFD_E_INVALID;
  return ALFD_OK;
}
// the table of block 0 alone, its caller side the device stage (host-pointer calls under a numbering)
static BlockTable stage_table(alfd_ctx *ctx) {
  BlockTable t;
  std::memset(&t, 0, sizeof(t));
  t.nblocks = 1;
  t.p[0] = ctx->num.stage;
  t.n[0] = ctx->n[0];
  for (int b = 1; b <= kMaxBlocks; ++b) t.off[b] = ctx->off[1];
  return t;
}
static void launch_unpack_perm(alfd_ctx *ctx, const BlockTable &t, const double *dev, int64_t nchunks) {
  if (ctx->num_unpack_scatter)
    hipLaunchKernelGGL(unpack_blocks_perm_scatter_kernel, dim3(block_grid(nchunks)), dim3(kBlock), 0, ctx->stream, t,
                       ctx->num.perm, dev, nchunks);
  else
    hipLaunchKernelGGL(unpack_blocks_perm_kernel, dim3(block_grid(nchunks)), dim3(kBlock), 0, ctx->stream, t,
                       ctx->num.inv, dev, nchunks);
}

// host blocks <-> padded device block vector.  Under a numbering block 0 stops at the device stage in the caller's
// order and moves between there and the internal vector in the permuting pack / unpack kernels.
static int to_device(alfd_ctx *ctx, const double *const *blocks, double *dev) {
  RC(numbering_fits(ctx));
  const bool perm = ctx->num.on() && ctx->n[0] > 0;
  HIPC(hipMemsetAsync(dev, 0, ctx->ntot() * sizeof(double), ctx->stream));
  for (int b = perm ? 1 : 0; b < ctx->nblocks; ++b)
    HIPC(hipMemcpyAsync(dev + ctx->off[b], blocks[b], ctx->n[b] * sizeof(double), hipMemcpyHostToDevice,
                        ctx->stream));
  if (perm) {
    HIPC(hipMemcpyAsync(ctx->num.stage, blocks[0], ctx->n[0] * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const int64_t nchunks = ctx->off[1] / kChunk;
    hipLaunchKernelGGL(pack_blocks_perm_kernel, dim3(block_grid(nchunks)), dim3(kBlock), 0, ctx->stream,
                       stage_table(ctx), ctx->num.perm, dev, nchunks);
    HIPC(hipGetLastError());
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  return ALFD_OK;
}
static int to_host(alfd_ctx *ctx, const double *dev, double *const *blocks) {
  RC(numbering_fits(ctx));
  const bool perm = ctx->num.on() && ctx->n[0] > 0;
  if (perm) {
    launch_unpack_perm(ctx, stage_table(ctx), dev, ctx->off[1] / kChunk);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(blocks[0], ctx->num.stage, ctx->n[0] * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  for (int b = perm ? 1 : 0; b < ctx->nblocks; ++b)
    HIPC(hipMemcpyAsync(blocks[b], dev + ctx->off[b], ctx->n[b] * sizeof(double), hipMemcpyDeviceToHost,
                        ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  return ALFD_OK;
}

// ---- caller DEVICE blocks <-> padded device block vector (the *_device entry points)
static_assert(kMaxBlocks == ALFD_MAX_BLOCKS, "BlockTable size");

// Every non-empty block must be device memory of the context's device; nothing has been launched when this refuses.
// hipPointerGetAttributes leaves a sticky error for an address the runtime does not know: it is cleared, so that the
// next HIPC(hipGetLastError()) of the context does not trip over it.
static int check_device_blocks(alfd_ctx *ctx, const double *const *blocks, const char *what) {
  for (int b = 0; b < ctx->nblocks; ++b) {
    if (ctx->n[b] == 0) continue;   // a null pointer is fine there
    const std::string name = std::string(what) + "[" + std::to_string(b) + "]";
    if (!blocks[b]) return ctx->err = name + " is a null pointer for a non-empty block", ALFD_E_INVALID;
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof(at));
    const hipError_t e = hipPointerGetAttributes(&at, blocks[b]);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return ctx->err = name + " is not device memory (" + hipGetErrorString(e) + ")", ALFD_E_INVALID;
    }
    if (at.type != hipMemoryTypeDevice)
      return ctx->err = name + " is not device memory (host, managed or unregistered address)", ALFD_E_INVALID;
    if (at.device != ctx->device)
      return ctx->err = name + " lives on device " + std::to_string(at.device) + ", the context on device " +
                        std::to_string(ctx->device), ALFD_E_INVALID;
    // the block must end inside its allocation (unpack writes n[b] doubles there); where the runtime cannot tell the
    // extent of an allocation the block is taken as given
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)blocks[b]) != hipSuccess) {
      (void)hipGetLastError();
      continue;
    }
    const char *end = static_cast<const char *>(base) + size;
    const char *p = reinterpret_cast<const char *>(blocks[b]);
    if (p < static_cast<const char *>(base) || (size_t)(end - p) < (size_t)ctx->n[b] * sizeof(double))
      return ctx->err = name + ": " + std::to_string(ctx->n[b]) + " doubles do not fit the allocation, which ends " +
                        std::to_string((long long)(end - p)) + " bytes after the pointer", ALFD_E_INVALID;
  }
  return ALFD_OK;
}

// The library's stream waits (on the device) for everything the caller has enqueued on `s` so far.
static int await_stream(alfd_ctx *ctx, void *s) {
  hipStream_t caller = static_cast<hipStream_t>(s);
  if (caller == ctx->stream) return ALFD_OK;
  if (!ctx->ev_in) HIPC(hipEventCreateWithFlags(&ctx->ev_in, hipEventDisableTiming));
  HIPC(hipEventRecord(ctx->ev_in, caller));
  HIPC(hipStreamWaitEvent(ctx->stream, ctx->ev_in, 0));
  return ALFD_OK;
}

static BlockTable block_table(alfd_ctx *ctx, const double *const *blocks) {
  BlockTable t;
  std::memset(&t, 0, sizeof(t));
  t.nblocks = ctx->nblocks;
  for (int b = 0; b < ctx->nblocks; ++b) {
    t.p[b] = const_cast<double *>(blocks[b]);
    t.n[b] = ctx->n[b];
    t.off[b] = ctx->off[b];
  }
  for (int b = ctx->nblocks; b <= kMaxBlocks; ++b) t.off[b] = ctx->ntot();
  return t;
}
// dev (ntot() doubles) <- blocks, padding zeroed; enqueued on ctx->stream, no synchronisation.  Under a numbering
// (alfd_set_numbering) block 0 is gathered through it in the same launch.
static int pack_device(alfd_ctx *ctx, const double *const *blocks, double *dev) {
  RC(numbering_fits(ctx));
  const int64_t nchunks = ctx->ntot() / kChunk;
  if (nchunks == 0) return ALFD_OK;
  if (ctx->num.on())
    hipLaunchKernelGGL(pack_blocks_perm_kernel, dim3(block_grid(nchunks)), dim3(kBlock), 0, ctx->stream,
                       block_table(ctx, blocks), ctx->num.perm, dev, nchunks);
  else
    hipLaunchKernelGGL(pack_blocks_kernel, dim3(block_grid(nchunks)), dim3(kBlock), 0, ctx->stream,
                       block_table(ctx, blocks), dev, nchunks);
  HIPC(hipGetLastError());
  return ALFD_OK;
}
// blocks <- dev, the first n[b] entries of every block; synchronises: on return the blocks are complete
static int unpack_device(alfd_ctx *ctx, const double *dev, double *const *blocks) {
  RC(numbering_fits(ctx));
  const int64_t nchunks = ctx->ntot() / kChunk;
  if (nchunks > 0) {
    if (ctx->num.on())
      launch_unpack_perm(ctx, block_table(ctx, blocks), dev, nchunks);
    else
      hipLaunchKernelGGL(unpack_blocks_kernel, dim3(block_grid(nchunks)), dim3(kBlock), 0, ctx->stream,
                         block_table(ctx, blocks), dev, nchunks);
    HIPC(hipGetLastError());
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  return ALFD_OK;
}

static void reset_stats(alfd_ctx *ctx) {
  ctx->inner_its = ctx->mp_its = 0;
  ctx->inner_its_op[0] = ctx->inner_its_op[1] = ctx->inner_its_op[2] = 0;
  ctx->inner_failures = ctx->precond_applications = 0;
  ctx->rational_its = 0;
  ctx->mass_its = 0;
}
static void fill_result(alfd_ctx *ctx, alfd_result *res, int status) {
  res->status = status;
  res->inner_iterations = ctx->inner_its;
  res->mp_iterations = ctx->mp_its;
  res->inner_failures = ctx->inner_failures;
  res->precond_applications = ctx->precond_applications;
  res->lambda_max = ctx->lambda_max;
  res->rational_iterations = ctx->rational_its;
  res->mass_iterations = ctx->mass_its;
}

}  // namespace alfd

// an input that only alfd_setup takes in was set: alfd_setup_coupling refuses until then
static void hierarchy_input_changed(alfd_ctx *ctx) {
  ctx->is_setup = false;
  ctx->needs_full = "a prolongator, aggregates or a row-block hint was set";
}

// =================================================================== C ABI
#define CHECK_CTX()                       \
  if (!ctx) return ALFD_E_INVALID;        \
  if (hipSetDevice(ctx->device) != hipSuccess) return ctx->err = "hipSetDevice failed", ALFD_E_HIP
#define CHECK_SETUP() \
  if (!ctx->is_setup) return ctx->err = "alfd_setup not called", ALFD_E_NOT_SETUP

extern "C" {

int alfd_abi_version(void) { return ALFD_ABI_VERSION; }

const char *alfd_strerror(int s) {
  switch (s) {
    case ALFD_OK: return "ok";
    case ALFD_E_INVALID: return "invalid argument";
    case ALFD_E_HIP: return "HIP runtime error";
    case ALFD_E_NO_CONVERGENCE_OUTER: return "FGMRES: no convergence (SolverControl::NoConvergence)";
    case ALFD_E_NO_CONVERGENCE_INNER: return "inner CG: no convergence (SolverControl::NoConvergence)";
    case ALFD_E_BREAKDOWN: return "breakdown (NaN residual)";
    case ALFD_E_NOT_SETUP: return "context not set up";
    case ALFD_E_COMM: return "RCCL error";
    case ALFD_E_UNSUPPORTED: return "not implemented";
    default: return "unknown status";
  }
}

const char *alfd_last_error(alfd_ctx_t ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int alfd_create(alfd_ctx_t *out, int device_id) {
  if (!out) return ALFD_E_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev)
    return ALFD_E_HIP;  // no GPU: fail loudly, there is no CPU path
  if (hipSetDevice(device_id) != hipSuccess) return ALFD_E_HIP;
  alfd_ctx *ctx = new alfd_ctx;
  ctx->device = device_id;
  if (hipStreamCreateWithFlags(&ctx->xstream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_x, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_halo, hipEventDisableTiming) != hipSuccess)
    ctx->xstream = nullptr;   // no overlap then
  if (const char *e = std::getenv("ALFD_SPMV_OVERLAP_HALO")) ctx->overlap_halo = std::atoi(e);
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return ALFD_E_HIP;
  }
  alfd_default_config(&ctx->cfg, ALFD_AL_STOKES);
  if (const char *e = std::getenv("ALFD_SPMV_STREAM_R")) ctx->spmv_stream_R = std::atoi(e);
  if (const char *e = std::getenv("ALFD_SPMV_STREAM_U")) ctx->spmv_stream_U = std::atoi(e);
  if (const char *e = std::getenv("ALFD_SPMV_PREC32_R")) ctx->a32_R = std::atoi(e);
  if (const char *e = std::getenv("ALFD_SPMV_PREC32_U")) ctx->a32_U = std::atoi(e);
  if (const char *e = std::getenv("ALFD_SPMV_NT")) ctx->spmv_nt = std::atoi(e);
  if (const char *e = std::getenv("ALFD_SPMV_GRID")) ctx->spmv_grid_mult = std::max(1, std::atoi(e));
  if (const char *e = std::getenv("ALFD_SPMV_WINDOW")) ctx->win_enable = std::atoi(e);
  if (const char *e = std::getenv("ALFD_SPMV_WINDOW_RB")) ctx->win_RB = std::max(4, std::atoi(e));
  if (const char *e = std::getenv("ALFD_SPMV_WINDOW_MIN_BLOCKS")) ctx->win_min_blocks = std::max(1, std::atoi(e));
  if (const char *e = std::getenv("ALFD_SPMV_WINDOW_SHORT_MIN_BLOCKS")) ctx->win_short_min_blocks = std::max(1, std::atoi(e));
  if (const char *e = std::getenv("ALFD_SPMV_WINDOW_MAXW")) ctx->win_maxW = std::min(16384, std::max(256, std::atoi(e)));
  if (const char *e = std::getenv("ALFD_ML_REPLICATE")) ctx->ml_rep_threshold = std::atoll(e);
  if (const char *e = std::getenv("ALFD_ML_GPU_GALERKIN")) ctx->ml_gpu_galerkin = std::atoi(e);
  if (const char *e = std::getenv("ALFD_ML_FUSE")) ctx->ml_fuse = std::max(0, std::min(3, std::atoi(e)));
  if (const char *e = std::getenv("ALFD_ML_TAIL_IN_SPMV")) ctx->ml_tail_in_spmv = std::atoi(e) != 0 ? 1 : 0;
  if (const char *e = std::getenv("ALFD_SPMV_VI_LEVELS")) ctx->vi_levels = std::atoi(e);
  if (const char *e = std::getenv("ALFD_SPMV_BATCH_MAJOR")) ctx->vs_enable = std::atoi(e);
  if (const char *e = std::getenv("ALFD_SPMV_BATCH_MAJOR_ROWS")) ctx->vs_RB = std::max(4, std::min(kVsMaxRows, std::atoi(e)));
  if (const char *e = std::getenv("ALFD_SPMV_SMALL_SHAPES")) ctx->vs_small = std::atoi(e) != 0;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) ctx->vs_cus = prop.multiProcessorCount;
  }
  if (const char *e = std::getenv("ALFD_SPMV_VI_XCD")) ctx->vi_xcd = std::atoi(e);
  if (const char *e = std::getenv("ALFD_SPMV_VI_BATCHED")) ctx->vi_batched = std::atoi(e);
  if (const char *e = std::getenv("ALFD_SPMV_WINDOW_RB_VI")) ctx->win_RB_vi = std::atoi(e);
  if (const char *e = std::getenv("ALFD_SPMV_VI_R")) ctx->vi_rows_R = std::atoi(e);
  if (const char *e = std::getenv("ALFD_SPMV_VI_J")) ctx->vi_rows_J = std::atoi(e);
  if (const char *e = std::getenv("ALFD_SPMV_VALUE_INDEX")) ctx->win_vi = std::atoi(e);
  if (const char *e = std::getenv("ALFD_SPMV_GROUP_R")) ctx->spmv_group_R = std::atoi(e);
  if (const char *e = std::getenv("ALFD_SPMV_GROUP_U")) ctx->spmv_group_U = std::atoi(e);
  if (const char *e = std::getenv("ALFD_SPMV_WINDOW_SHORT")) ctx->win_short_scale = std::max(0, std::atoi(e));
  if (const char *e = std::getenv("ALFD_SPMV_WINDOW_GAP")) ctx->win_gap = std::max(1, std::atoi(e));
  if (const char *e = std::getenv("ALFD_SPMV_WINDOW_XCD")) ctx->win_xcd = std::atoi(e);
  *out = ctx;
  return ALFD_OK;
}

int alfd_destroy(alfd_ctx_t ctx) {
  if (!ctx) return ALFD_E_INVALID;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  flush_timers(ctx);
  free_levels(ctx);
  spectrum_release(ctx);
  csr_free(ctx->rat_mat);
  for (DevCsr &m : ctx->mat) csr_free(m);
  for (void *p : ctx->ws_allocs) hipFree(p);
  for (void *p : ctx->allocs) hipFree(p);
  if (ctx->sc_host) hipHostFree(ctx->sc_host);
  if (ctx->n_sc_host) hipHostFree(ctx->n_sc_host);
  if (ctx->rt_scb_host) hipHostFree(ctx->rt_scb_host);
  if (ctx->nccl) ncclCommDestroy(ctx->nccl);
  if (ctx->xstream) hipStreamDestroy(ctx->xstream);
  if (ctx->ev_x) hipEventDestroy(ctx->ev_x);
  if (ctx->ev_halo) hipEventDestroy(ctx->ev_halo);
  if (ctx->ev_in) hipEventDestroy(ctx->ev_in);
  if (ctx->num.perm) hipFree(ctx->num.perm);
  if (ctx->num.inv) hipFree(ctx->num.inv);
  if (ctx->num.stage) hipFree(ctx->num.stage);
  hipStreamDestroy(ctx->stream);
  delete ctx;
  return ALFD_OK;
}

// renumbering across a row partition is not implemented: a context has a numbering or more than one rank
static int numbering_bars_partition(alfd_ctx *ctx) {
  if (ctx->num.on())
    return ctx->err = "a context with a numbering (alfd_set_numbering) cannot be partitioned", ALFD_E_UNSUPPORTED;
  return ALFD_OK;
}

int alfd_comm_unique_id(void *id_out, size_t bytes) {
  static_assert(sizeof(ncclUniqueId) <= ALFD_UNIQUE_ID_BYTES, "unique id size");
  if (!id_out || bytes < sizeof(ncclUniqueId)) return ALFD_E_INVALID;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return ALFD_E_COMM;
  std::memset(id_out, 0, bytes);
  std::memcpy(id_out, &id, sizeof(id));
  return ALFD_OK;
}

int alfd_comm_init(alfd_ctx_t ctx, int rank, int nranks, const void *id, size_t bytes) {
  CHECK_CTX();
  if (nranks < 1 || rank < 0 || rank >= nranks) return ALFD_E_INVALID;
  if (nranks > 1) RC(numbering_bars_partition(ctx));
  ctx->rank = rank;
  ctx->nranks = nranks;
  if (nranks == 1) return ALFD_OK;
  if (!id || bytes < sizeof(ncclUniqueId)) return ALFD_E_INVALID;
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  if (ncclCommInitRank(&ctx->nccl, nranks, uid, rank) != ncclSuccess)
    return ctx->err = "ncclCommInitRank failed", ALFD_E_COMM;
  if (rank == 0) {   // which RCCL this process resolved (the library links $(ROCM)/lib/librccl, torch bundles its own copy)
    int v = 0;
    if (ncclGetVersion(&v) == ncclSuccess) std::fprintf(stderr, "[alfd] RCCL version %d, %d ranks\n", v, nranks);
  }
  return ALFD_OK;
}

int alfd_local_group_create(int nranks, alfd_local_group **out) {
  if (!out || nranks < 1) return ALFD_E_INVALID;
  alfd_local_group *g = new alfd_local_group;
  g->n = nranks;
  g->buf.assign(nranks, nullptr);
  g->off.assign(nranks, nullptr);
  *out = g;
  return ALFD_OK;
}

int alfd_local_group_destroy(alfd_local_group *g) {
  if (!g) return ALFD_E_INVALID;
  delete g;
  return ALFD_OK;
}

int alfd_comm_init_local(alfd_ctx_t ctx, alfd_local_group *g, int rank) {
  CHECK_CTX();
  if (!g || rank < 0 || rank >= g->n) return ALFD_E_INVALID;
  if (g->n > 1) RC(numbering_bars_partition(ctx));
  ctx->rank = rank;
  ctx->nranks = g->n;
  ctx->local = g->n > 1 ? g : nullptr;
  return ALFD_OK;
}

int alfd_comm_init_host(alfd_ctx_t ctx, int rank, int nranks, alfd_host_allgather_fn allgather,
                        alfd_host_alltoallv_fn alltoallv, void *user) {
  CHECK_CTX();
  if (nranks < 1 || rank < 0 || rank >= nranks || !allgather || !alltoallv) return ALFD_E_INVALID;
  if (nranks > 1) RC(numbering_bars_partition(ctx));
  ctx->rank = rank;
  ctx->nranks = nranks;
  if (nranks == 1) return ALFD_OK;
  ctx->host_allgather = allgather;
  ctx->host_alltoallv = alltoallv;
  ctx->host_user = user;
  return ALFD_OK;
}

int alfd_set_partition(alfd_ctx_t ctx, int nblocks, const int64_t *const *offsets) {
  CHECK_CTX();
  if (nblocks < 2 || nblocks > ALFD_MAX_BLOCKS || !offsets) return ALFD_E_INVALID;
  if (ctx->nranks > 1) RC(numbering_bars_partition(ctx));
  ctx->part.assign(nblocks, {});
  for (int b = 0; b < nblocks; ++b) {
    ctx->part[b].assign(offsets[b], offsets[b] + ctx->nranks + 1);
    for (int r = 0; r < ctx->nranks; ++r)
      if (ctx->part[b][r + 1] < ctx->part[b][r]) return ctx->err = "partition not monotone", ALFD_E_INVALID;
  }
  ctx->nblocks = nblocks;
  return ALFD_OK;
}

int alfd_set_matrix(alfd_ctx_t ctx, int slot, int64_t nrows, int64_t ncols, const int64_t *row_ptr,
                    const int32_t *col, const double *val) {
  CHECK_CTX();
  if (slot < 0 || slot >= ALFD_NSLOTS || nrows < 0 || ncols < 0 || !row_ptr) return ALFD_E_INVALID;
  if (ncols > 2147483647LL) return ctx->err = "more than 2^31-1 columns", ALFD_E_INVALID;
  if (row_ptr[0] != 0) return ctx->err = "row_ptr[0] != 0", ALFD_E_INVALID;
  const int64_t nnz = row_ptr[nrows];
  if (nnz > 0 && (!col || !val)) return ALFD_E_INVALID;
  for (int64_t r = 0; r < nrows; ++r)
    if (row_ptr[r + 1] < row_ptr[r]) return ctx->err = "row_ptr not monotone", ALFD_E_INVALID;
  for (int64_t k = 0; k < nnz; ++k)
    if (col[k] < 0 || col[k] >= ncols) return ctx->err = "column index out of range", ALFD_E_INVALID;
  // alfd_set_numbering: the caller's operator becomes the internal one before anything below sees it -- rows of A, BT,
  // CT in the new order, columns of A, B, C renamed, a row's entries sorted by new column (alfd_host_permute_csr)
  std::vector<int64_t> prp;
  std::vector<int32_t> pcol;
  std::vector<double> pval;
  if (ctx->num.on()) {
    const bool by_row = slot == ALFD_A || slot == ALFD_BT || slot == ALFD_CT;
    const bool by_col = slot == ALFD_A || slot == ALFD_B || slot == ALFD_C;
    if ((by_row && nrows != ctx->num.n()) || (by_col && ncols != ctx->num.n()))
      return ctx->err = "alfd_set_matrix: the numbering (alfd_set_numbering) has " +
                        std::to_string((long long)ctx->num.n()) + " entries, the block-0 side of this operator " +
                        std::to_string((long long)(by_row ? nrows : ncols)), ALFD_E_INVALID;
    if (by_row || by_col) {
      prp.resize((size_t)nrows + 1);
      pcol.resize((size_t)nnz);
      pval.resize((size_t)nnz);
      if (alfd_host_permute_csr(nrows, row_ptr, col, val, by_row ? ctx->num.n2o.data() : nullptr,
                                by_col ? ctx->num.o2n.data() : nullptr, prp.data(), pcol.data(), pval.data()) != ALFD_OK)
        return ctx->err = "alfd_set_matrix: permuting the operator failed", ALFD_E_INVALID;
      row_ptr = prp.data(), col = pcol.data(), val = pval.data();
    }
  }
  ctx->is_setup = false;
  ctx->gen[slot]++;
  if (ctx->nranks > 1 && ctx->nblocks == 0)
    return ctx->err = "alfd_set_partition must precede alfd_set_matrix", ALFD_E_INVALID;
  if (!ctx->upload_since_setup) ctx->setup_s[ALFD_SETUP_UPLOAD] = 0.0, ctx->upload_since_setup = true;
  struct UploadClock {
    alfd_ctx *c;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~UploadClock() {
      hipStreamSynchronize(c->stream);
      c->setup_s[ALFD_SETUP_UPLOAD] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
  } upload_clock{ctx};
  RC(upload_matrix(ctx, slot, nrows, ncols, row_ptr, col, val));
  if (slot == ALFD_A) RC(a32_sync(ctx));   // the single-precision copy follows the new values (or goes with the old ones)
  if ((slot == ALFD_M || slot == ALFD_KIMM) && nnz <= (int64_t)1 << 26) {
    // the rational preconditioner builds its 21 shifted systems from these on the host
    HostCsr &h = slot == ALFD_M ? ctx->h_M : ctx->h_K;
    h.nrows = nrows;
    h.ncols = ncols;
    h.rp.assign(row_ptr, row_ptr + nrows + 1);
    h.col.assign(col, col + nnz);
    h.val.assign(val, val + nnz);
  }
  // single rank: the transposed operators are derived on upload, like
  // transpose_operator(Ct) (stokes...:927), and re-derived whenever CT / BT is uploaded
  // again (new values must not meet the transpose of the old ones); an explicit upload of
  // C / B overrides and is then left alone.
  if (slot == ALFD_C || slot == ALFD_B) ctx->mat[slot].derived = false;
  if (ctx->nranks == 1) {
    const int pairs[2][2] = {{ALFD_CT, ALFD_C}, {ALFD_BT, ALFD_B}};
    for (const auto &pr : pairs) {
      const DevCsr &t = ctx->mat[pr[1]];
      if (slot == pr[0] && (!t.present || t.derived)) {
        RC(upload_transpose(ctx, pr[1], nrows, ncols, row_ptr, col, val));
        ctx->mat[pr[1]].derived = true;
      }
    }
  }
  return ALFD_OK;
}

int alfd_set_diag(alfd_ctx_t ctx, int slot, int64_t n, const double *d) {
  CHECK_CTX();
  if (slot < 0 || slot >= ALFD_NDIAGS || n < 0 || (n > 0 && !d)) return ALFD_E_INVALID;
  ctx->is_setup = false;
  ctx->dgen[slot]++;
  if (ctx->diag[slot]) {
    ctx->allocs.erase(std::remove(ctx->allocs.begin(), ctx->allocs.end(), (void *)ctx->diag[slot]), ctx->allocs.end());
    hipFree(ctx->diag[slot]);
    ctx->diag[slot] = nullptr;
  }
  RC(dev_alloc_zero(ctx, &ctx->diag[slot], pad_chunk(n)));
  HIPC(hipMemcpyAsync(ctx->diag[slot], d, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  ctx->diag_n[slot] = n;
  return ALFD_OK;
}

void alfd_default_config(alfd_config *c, int variant) {
  std::memset(c, 0, sizeof(*c));
  c->variant = variant;
  c->restart = (variant == ALFD_AL_ELL_IDEAL || variant == ALFD_AL_ELL_MODIFIED) ? 50 : 30;
  c->orthogonalization = ALFD_ORTH_CGS2;
  c->grad_div_in_A = 1;
  c->gamma = 10.0;
  c->gamma_grad_div = 10.0;
  c->gamma2 = 1e-2;
  c->outer = {ALFD_CTRL_REDUCTION, 1000, 1e-8, 1e-12};
  c->inner = {ALFD_CTRL_ABS, 100, 1e-2, 0.0};
  c->mp_inner = {ALFD_CTRL_ABS, 100, 1e-6, 0.0};
  c->inner_prec = ALFD_PREC_CHEBYSHEV;
  c->cheb_degree = 4;
  c->cheb_power_its = 20;
  c->on_inner_failure = ALFD_INNER_THROW;
  c->cheb_eig_ratio = 30.0;
  c->cheb_safety = 1.2;
  c->log_level = 0;
  c->outer_solver = variant == ALFD_RATIONAL ? ALFD_OUTER_MINRES : ALFD_OUTER_FGMRES;
  c->rho_bound = 0.0;
  c->rational = {ALFD_CTRL_ABS, 2000, 1e-14, 0.0};
  c->ml_smooth_degree = 3;
  c->ml_coarse_degree = 40;
  c->ml_smooth_ratio = 4.0;
  c->ml_coarse_ratio = 400.0;
  c->w_inverse = ALFD_W_DIAGONAL;
  c->mass = {ALFD_CTRL_REDUCTION, 1000, 1e-30, 1e-14};
  c->ml_patch_degree = 0;
  c->ml_coarse_direct = 0;
  c->ml_patch_ratio = 30.0;
}

int alfd_set_aggregates(alfd_ctx_t ctx, int level, int64_t n_fine, const int32_t *agg, const double *weight,
                        int64_t n_coarse) {
  CHECK_CTX();
  if (level < 0 || level >= ALFD_MAX_LEVELS || n_fine < 1 || n_coarse < 1 || !agg) return ALFD_E_INVALID;
  for (int64_t i = 0; i < n_fine; ++i)
    if (agg[i] < -1 || agg[i] >= n_coarse) return ctx->err = "aggregate id out of range", ALFD_E_INVALID;
  if (level == 0 && ctx->num.on() && n_fine != ctx->num.n())
    return ctx->err = "alfd_set_aggregates: level 0 does not have the size of the numbering (alfd_set_numbering)", ALFD_E_INVALID;
  ctx->hier[0].agg[level].assign(agg, agg + n_fine);
  if (weight)
    ctx->hier[0].wgt[level].assign(weight, weight + n_fine);
  else
    ctx->hier[0].wgt[level].clear();
  if (level == 0 && ctx->num.on()) {   // the fine unknowns of level 0 are block 0: stored in the internal order
    for (int64_t k = 0; k < n_fine; ++k) ctx->hier[0].agg[0][k] = agg[ctx->num.n2o[k]];
    if (weight)
      for (int64_t k = 0; k < n_fine; ++k) ctx->hier[0].wgt[0][k] = weight[ctx->num.n2o[k]];
  }
  ctx->hier[0].ncoarse[level] = n_coarse;
  ctx->hier[0].P[level] = HostCsr();
  ctx->hier[0].built_partitioned = false;
  for (int l = level + 1; l < ALFD_MAX_LEVELS; ++l) ctx->hier[0].agg[l].clear(), ctx->hier[0].wgt[l].clear(), ctx->hier[0].P[l] = HostCsr();
  hierarchy_input_changed(ctx);
  return ALFD_OK;
}

// block 1 (the immersed hierarchy): CSR prolongators only, one rank
static int check_block(alfd_ctx_t ctx, int block) {
  if (block != 0 && block != 1) return ctx->err = "multigrid hierarchy: block must be 0 or 1", ALFD_E_INVALID;
  if (block == 1 && ctx->nranks > 1)
    return ctx->err = "the block-1 (immersed) hierarchy is single-rank", ALFD_E_UNSUPPORTED;
  return ALFD_OK;
}

int alfd_set_prolongator_block(alfd_ctx_t ctx, int block, int level, int64_t n_fine, int64_t n_coarse,
                               const int64_t *row_ptr, const int32_t *col, const double *val) {
  CHECK_CTX();
  RC(check_block(ctx, block));
  const std::string fn = block == 0 ? "alfd_set_prolongator" : "alfd_set_prolongator_block";   // block 0: the call behind alfd_set_prolongator
  if (level < 0 || level >= ALFD_MAX_LEVELS || n_fine < 0 || n_coarse <= 0 || n_coarse > INT32_MAX || !row_ptr ||
      row_ptr[0] != 0)
    return ctx->err = fn + ": bad arguments", ALFD_E_INVALID;
  for (int64_t i = 0; i < n_fine; ++i)
    if (row_ptr[i + 1] < row_ptr[i]) return ctx->err = fn + ": row_ptr must be monotone", ALFD_E_INVALID;
  const int64_t nnz = row_ptr[n_fine];
  if (nnz > 0 && (!col || !val)) return ctx->err = fn + ": col / val missing", ALFD_E_INVALID;
  for (int64_t i = 0; i < n_fine; ++i)
    for (int64_t k = row_ptr[i]; k < row_ptr[i + 1]; ++k)
      if (col[k] < 0 || col[k] >= n_coarse || (k > row_ptr[i] && col[k] <= col[k - 1]))
        return ctx->err = fn + ": columns must be ascending and inside [0, n_coarse)", ALFD_E_INVALID;
  alfd_ctx::Hierarchy &H = ctx->hier[block];
  HostCsr &P = H.P[level];
  if (block == 0 && level == 0 && ctx->num.on() && n_fine != ctx->num.n())
    return ctx->err = fn + ": level 0 does not have the size of the numbering (alfd_set_numbering)", ALFD_E_INVALID;
  P.nrows = n_fine;
  P.ncols = n_coarse;
  if (block == 0 && level == 0 && ctx->num.on()) {   // the rows of level 0 are block 0: stored in the internal order
    P.rp.resize((size_t)n_fine + 1);
    P.col.resize((size_t)nnz);
    P.val.resize((size_t)nnz);
    if (alfd_host_permute_csr(n_fine, row_ptr, col, val, ctx->num.n2o.data(), nullptr, P.rp.data(), P.col.data(),
                              P.val.data()) != ALFD_OK)
      return ctx->err = fn + ": permuting the rows failed", ALFD_E_INVALID;
  } else {
    P.rp.assign(row_ptr, row_ptr + n_fine + 1);
    P.col.assign(col, col + nnz);
    P.val.assign(val, val + nnz);
  }
  H.agg[level].clear();
  H.wgt[level].clear();
  H.ncoarse[level] = n_coarse;
  H.built_partitioned = false;   // a caller-supplied level: the halo condition of alfd_set_prolongator holds again
  for (int l = level + 1; l < ALFD_MAX_LEVELS; ++l) {   // levels below are redefined by later calls
    H.agg[l].clear();
    H.P[l] = HostCsr();
  }
  hierarchy_input_changed(ctx);
  return ALFD_OK;
}

int alfd_set_prolongator(alfd_ctx_t ctx, int level, int64_t n_fine, int64_t n_coarse, const int64_t *row_ptr,
                         const int32_t *col, const double *val) {
  return alfd_set_prolongator_block(ctx, 0, level, n_fine, n_coarse, row_ptr, col, val);
}

int alfd_clear_hierarchy(alfd_ctx_t ctx, int block) {
  CHECK_CTX();
  if (block != 0 && block != 1) return ctx->err = "multigrid hierarchy: block must be 0 or 1", ALFD_E_INVALID;
  ctx->hier[block].clear_input();
  hierarchy_input_changed(ctx);
  return ALFD_OK;
}

int alfd_get_inner_iterations(alfd_ctx_t ctx, int64_t counts[3]) {
  if (!ctx || !counts) return ALFD_E_INVALID;
  std::copy(ctx->inner_its_op, ctx->inner_its_op + 3, counts);
  return ALFD_OK;
}

int alfd_build_aggregates(alfd_ctx_t ctx, int32_t block_size, double threshold, int32_t max_aggregate_nodes,
                          int64_t min_coarse, int32_t max_levels, int32_t *levels_out) {
  CHECK_CTX();
  if (ctx->nranks > 1) return ctx->err = "alfd_build_aggregates is single-rank", ALFD_E_UNSUPPORTED;
  if (ctx->configured && gd_nested(ctx))
    return ctx->err = "alfd_build_aggregates: grad_div_in_A = 0 has no multilevel inner preconditioner", ALFD_E_UNSUPPORTED;
  if (!ctx->mat[ALFD_A].present) return ctx->err = "upload slot A first", ALFD_E_NOT_SETUP;
  if (block_size < 1 || !(threshold >= 0.0) || max_aggregate_nodes < 2 || min_coarse < 1) return ALFD_E_INVALID;
  if (ctx->mat[ALFD_A].nrows % block_size) return ctx->err = "rows of A are not a multiple of block_size", ALFD_E_INVALID;
  if (max_levels < 1 || max_levels > ALFD_MAX_LEVELS - 1) max_levels = ALFD_MAX_LEVELS - 1;
  HostCsr A, An;
  RC(download_csr(ctx, ctx->mat[ALFD_A], A));
  for (int l = 0; l < ALFD_MAX_LEVELS; ++l) ctx->hier[0].agg[l].clear(), ctx->hier[0].wgt[l].clear(), ctx->hier[0].P[l] = HostCsr();
  int nlev = 0;
  while (nlev < max_levels) {
    std::vector<int32_t> agg;
    int64_t nc = 0;
    aggregate_level(A, block_size, threshold, max_aggregate_nodes, agg, nc);
    if (nc < 1 || nc >= A.nrows) break;     // nothing left to coarsen
    ctx->hier[0].agg[nlev] = agg;
    ctx->hier[0].ncoarse[nlev] = nc;
    ++nlev;
    if (nc <= min_coarse) break;
    galerkin(A, agg.data(), nullptr, nc, agg.data(), nullptr, nc, An);
    std::swap(A, An);
  }
  if (nlev == 0) return ctx->err = "algebraic aggregation found nothing to coarsen", ALFD_E_INVALID;
  if (levels_out) *levels_out = nlev;
  hierarchy_input_changed(ctx);
  return ALFD_OK;
}

int alfd_host_aggregate_level(int64_t nrows, const int64_t *rp, const int32_t *col, const double *val,
                               int32_t block_size, double threshold, int32_t max_aggregate_nodes, int32_t *agg,
                               int64_t *n_coarse) {
  if (nrows < 1 || !rp || !col || !val || !agg || !n_coarse || block_size < 1 || nrows % block_size ||
      max_aggregate_nodes < 2 || !(threshold >= 0.0))
    return ALFD_E_INVALID;
  HostCsr A;
  A.nrows = A.ncols = nrows;
  A.rp.assign(rp, rp + nrows + 1);
  A.col.assign(col, col + rp[nrows]);
  A.val.assign(val, val + rp[nrows]);
  std::vector<int32_t> a;
  aggregate_level(A, block_size, threshold, max_aggregate_nodes, a, *n_coarse);
  std::copy(a.begin(), a.end(), agg);
  return ALFD_OK;
}

int alfd_host_strength_graph(int64_t nrows, const int64_t *rp, const int32_t *col, const double *val, int32_t block_size,
                             double threshold, double *d, int32_t *fixed, int64_t *node_ptr, int32_t *nbr, double *weight,
                             int64_t capacity, int64_t *nnz) {
  if (nrows < 1 || !rp || !col || !val || !nnz || block_size < 1 || nrows % block_size || !(threshold >= 0.0) ||
      rp[0] != 0)
    return ALFD_E_INVALID;
  for (int64_t i = 0; i < nrows; ++i)
    if (rp[i + 1] < rp[i]) return ALFD_E_INVALID;
  for (int64_t k = 0; k < rp[nrows]; ++k)
    if (col[k] < 0) return ALFD_E_INVALID;
  HostCsr A;
  A.nrows = A.ncols = nrows;
  A.rp.assign(rp, rp + nrows + 1);
  A.col.assign(col, col + rp[nrows]);
  A.val.assign(val, val + rp[nrows]);
  const int64_t nn = nrows / block_size;
  std::vector<double> dd, gw;
  std::vector<int32_t> fx, gc;
  std::vector<int64_t> gp;
  node_diag_host(A, 0, block_size, dd, fx);
  node_graph_host(A, 0, block_size, threshold, nn, dd.data(), fx.data(), gp, gc, gw);
  *nnz = gp[nn];
  if (d) std::copy(dd.begin(), dd.end(), d);
  if (fixed) std::copy(fx.begin(), fx.end(), fixed);
  if (node_ptr) std::copy(gp.begin(), gp.end(), node_ptr);
  if (nbr || weight) {
    if (capacity < gp[nn]) return ALFD_E_INVALID;
    if (nbr) std::copy(gc.begin(), gc.end(), nbr);
    if (weight) std::copy(gw.begin(), gw.end(), weight);
  }
  return ALFD_OK;
}

int alfd_host_aggregate_graph(int64_t n_nodes, const int32_t *fixed, const int64_t *node_ptr, const int32_t *nbr,
                              const double *weight, int32_t block_size, int32_t max_aggregate_nodes, int32_t *agg,
                              int64_t *n_coarse) {
  if (n_nodes < 1 || !fixed || !node_ptr || !agg || !n_coarse || block_size < 1 || max_aggregate_nodes < 2 ||
      node_ptr[0] != 0 || n_nodes > INT32_MAX / block_size)
    return ALFD_E_INVALID;
  for (int64_t I = 0; I < n_nodes; ++I)
    if (node_ptr[I + 1] < node_ptr[I]) return ALFD_E_INVALID;
  if (node_ptr[n_nodes] > 0 && (!nbr || !weight)) return ALFD_E_INVALID;
  for (int64_t k = 0; k < node_ptr[n_nodes]; ++k)
    if (nbr[k] < 0 || nbr[k] >= n_nodes) return ALFD_E_INVALID;
  std::vector<int32_t> a;
  aggregate_graph(n_nodes * block_size, n_nodes, block_size, max_aggregate_nodes, fixed, node_ptr, nbr, weight, a, *n_coarse);
  std::copy(a.begin(), a.end(), agg);
  return ALFD_OK;
}

int alfd_build_strength_graph(alfd_ctx_t ctx, int32_t block_size, double threshold, int64_t *n_nodes, int64_t *nnz) {
  CHECK_CTX();
  ctx->sg = alfd_ctx::StrengthGraph();
  // every check below reads what all ranks hold alike (arguments, the partition) or fails before any collective
  if (block_size < 1 || !(threshold >= 0.0) || !std::isfinite(threshold))
    return ctx->err = "alfd_build_strength_graph: bad arguments", ALFD_E_INVALID;
  if (ctx->nranks > 1) {
    if (ctx->part.empty()) return ctx->err = "alfd_set_partition must precede alfd_build_strength_graph", ALFD_E_INVALID;
    for (int64_t o : ctx->part[0])
      if (o % block_size)
        return ctx->err = "alfd_build_strength_graph: the partition offsets of block 0 must be multiples of block_size",
               ALFD_E_INVALID;
  }
  // rank-local preconditions: agreed on before the first exchange
  int loc = ALFD_OK;
  const DevCsr &A = ctx->mat[ALFD_A];
  const int64_t N = ctx->nranks > 1 ? ctx->part[0].back() : A.nrows;
  if (!A.present) ctx->err = "upload slot A first", loc = ALFD_E_NOT_SETUP;
  else if (A.sparse || A.ncols != N || A.nrows % block_size ||
           (ctx->nranks > 1 && A.nrows != ctx->part[0][ctx->rank + 1] - ctx->part[0][ctx->rank]))
    ctx->err = "alfd_build_strength_graph: slot A must hold this rank's rows of a square operator, a multiple of block_size",
    loc = ALFD_E_INVALID;
  RC(joint_status(ctx, loc, 0, nullptr));
  RC(strength_graph_dev(ctx, block_size, threshold));
  if (n_nodes) *n_nodes = ctx->sg.n_nodes;
  if (nnz) *nnz = ctx->sg.gp.back();
  return ALFD_OK;
}

int alfd_get_strength_graph(alfd_ctx_t ctx, double *d, int32_t *fixed, int64_t *node_ptr, int32_t *nbr, double *weight,
                            int64_t capacity, int32_t *on_device) {
  CHECK_CTX();
  const alfd_ctx::StrengthGraph &G = ctx->sg;
  if (!G.have) return ctx->err = "alfd_build_strength_graph first", ALFD_E_NOT_SETUP;
  if (d) std::copy(G.d.begin(), G.d.end(), d);
  if (fixed) std::copy(G.fixed.begin(), G.fixed.end(), fixed);
  if (node_ptr) std::copy(G.gp.begin(), G.gp.end(), node_ptr);
  if (nbr || weight) {
    if (capacity < G.gp.back()) return ALFD_E_INVALID;
    if (nbr) std::copy(G.gc.begin(), G.gc.end(), nbr);
    if (weight) std::copy(G.gw.begin(), G.gw.end(), weight);
  }
  if (on_device) *on_device = G.on_device ? 1 : 0;
  return ALFD_OK;
}

int alfd_get_aggregates(alfd_ctx_t ctx, int level, int32_t *agg, int64_t capacity, int64_t *n_fine, int64_t *n_coarse) {
  return alfd_get_aggregates_block(ctx, 0, level, agg, capacity, n_fine, n_coarse);
}

int alfd_get_aggregates_block(alfd_ctx_t ctx, int block, int level, int32_t *agg, int64_t capacity, int64_t *n_fine,
                              int64_t *n_coarse) {
  if (!ctx || (block != 0 && block != 1) || level < 0 || level >= ALFD_MAX_LEVELS || ctx->hier[block].agg[level].empty())
    return ALFD_E_INVALID;
  const std::vector<int32_t> &a = ctx->hier[block].agg[level];
  if (n_fine) *n_fine = (int64_t)a.size();
  if (n_coarse) *n_coarse = ctx->hier[block].ncoarse[level];
  if (agg) {
    if (capacity < (int64_t)a.size()) return ALFD_E_INVALID;
    if (block == 0 && level == 0 && ctx->num.on() && (int64_t)a.size() == ctx->num.n())   // back to the caller's order
      for (size_t i = 0; i < a.size(); ++i) agg[i] = a[(size_t)ctx->num.o2n[i]];
    else
      std::copy(a.begin(), a.end(), agg);
  }
  return ALFD_OK;
}

// One level's prolongator from its aggregates, d = diag(Aug) (sa_diag) and omega: the rows of sa_prolongator_dev, or
// the host rows and the host truncation when a row has more candidates than the kernels hold (*on_device = false; same
// bits).  sa_build_levels and alfd_smoothed_prolongator.
static int sa_level_prolongator(alfd_ctx *ctx, const HostCsr &A, const SaPenalty &pen, const std::vector<int32_t> &agg,
                                int64_t nc, const std::vector<double> &d, double omega, int bs, double tau, int cap,
                                HostCsr &P, bool *on_device) {
  std::vector<double> f;
  HostCsr Q;
  sa_factors(agg, d, omega, f);
  RC(sa_penalty_rows(ctx, pen, agg, nc, Q));
  bool fits = false;
  RC(sa_prolongator_dev(ctx, A, agg, nc, f, Q, bs, tau, cap, P, &fits));
  if (!fits) {
    sa_rows_host(A, agg, nc, f, pen.on() ? &Q : nullptr, P);
    if (tau != 0.0 || cap != 0) {
      HostCsr T;
      sa_truncate_host(P, agg, bs, tau, cap, T);
      std::swap(P, T);
    }
  }
  *on_device = fits;
  return ALFD_OK;
}

struct SaParams {
  int32_t block_size, max_aggregate_nodes, cap, max_levels, its;
  double threshold, damping, tau, gamma;
  int64_t min_coarse;
  bool use_pen;
};

// The levels nlev, nlev + 1, ... of a smoothed-aggregation hierarchy from the operators (A, C, Ct = C^T, w) of level
// nlev, whole on this rank: the single-rank build from level 0, the replicated levels >= 1 of a partitioned one.
static int sa_build_levels(alfd_ctx *ctx, alfd_ctx::Hierarchy &H, const SaParams &sp, HostCsr &A, HostCsr &C, HostCsr &Ct,
                           const std::vector<double> &w, int &nlev, double *omega_out) {
  const int32_t block_size = sp.block_size, max_aggregate_nodes = sp.max_aggregate_nodes, cap = sp.cap,
                max_levels = sp.max_levels;
  const int its = sp.its;
  const double threshold = sp.threshold, damping = sp.damping, tau = sp.tau, gamma = sp.gamma;
  const int64_t min_coarse = sp.min_coarse;
  const bool use_pen = sp.use_pen;
  HostCsr An, Cn, P, R, AP;
  std::vector<double> d;
  while (nlev < max_levels) {
    std::vector<int32_t> agg;
    int64_t nc = 0;
    aggregate_level(A, block_size, threshold, max_aggregate_nodes, agg, nc);
    if (nc < 1 || nc >= A.nrows) break;     // nothing left to coarsen
    SaPenalty pen;
    if (use_pen) pen.Ct = &Ct, pen.C = &C, pen.w = w.data(), pen.gamma = gamma;
    sa_diag(A, pen, d);
    const double lam = sa_lambda(A, pen, d, its);
    if (!(lam > 0.0) || !std::isfinite(lam)) {
      H.clear_input();
      return ctx->err = "alfd_build_smoothed_aggregation: lambda_max(D^-1 Aug) of level " + std::to_string(nlev) +
                        " is not positive and finite (zero diagonal?)", ALFD_E_INVALID;
    }
    const double omega = damping / lam;
    bool on_device = false;
    RC(sa_level_prolongator(ctx, A, pen, agg, nc, d, omega, block_size, tau, cap, P, &on_device));
    if (omega_out) omega_out[nlev] = omega;
    H.agg[nlev] = agg;
    H.P[nlev] = P;
    H.ncoarse[nlev] = nc;
    ++nlev;
    if (nc <= min_coarse || nlev >= max_levels) break;
    // next level: A_{l+1} = P^T (A P), C_{l+1} = C P (the Galerkin products of alfd_setup, same order)
    RC(product(ctx, A, P, AP));
    transpose_host(P, R);
    RC(product(ctx, R, AP, An));
    AP = HostCsr();
    std::swap(A, An);
    if (use_pen) {
      RC(product(ctx, C, P, Cn));
      std::swap(C, Cn);
      transpose_host(C, Ct);
    }
  }
  return ALFD_OK;
}

// alfd_build_smoothed_aggregation[_truncated] on a ROW-PARTITIONED context (block 0): the single-rank hierarchy bit for bit,
// whatever the partition.  Level 0 is built from the resident rows (A is not downloaded; the few rows of Ct and C are):
//   graph     sa_node_graph_kernel on the own nodes, d / fixed all-gathered; the graph rows are all-gathered and the three
//             greedy passes run redundantly on every rank (aggregates do not respect the slabs);
//   order     the resident rows already are in global CSR order, sa_global_cols_kernel renames their columns;
//   d, lambda sa_diag_rows_kernel, then its steps of sa_power_t_kernel / sa_power_rows_kernel on the replicated v with an
//             all-gather of y per step; both norms are the one sequential fma sum of sa_lambda over the whole vector, on
//             every rank's host;
//   penalty   gamma Ct W^-1 (C P_tent) by the generic product from the gathered C and the own rows of Ct;
//   P_0       sa_prolongator_kernel / sa_truncated_prolongator_kernel, unchanged, on the view (own rows of P_0).
// Levels >= 1: A_1, C_1 replicated by rep_level0_products, then sa_build_levels redundantly on every rank.  After every
// rank-local phase the ranks exchange a status word (joint_status): a failure is returned by all, and a row with more
// candidates than the kernel holds sends all ranks to the host routines together.
static int build_sa_partitioned(alfd_ctx *ctx, SaParams sp, int32_t *levels_out, double *omega_out, bool *touched) {
  alfd_ctx::Hierarchy &H = ctx->hier[0];
  const alfd_config &c = ctx->cfg;
  const int P = ctx->nranks, rk = ctx->rank, last = ctx->nblocks - 1, bs = sp.block_size;
  for (int64_t o : ctx->part[0])   // (the caller has checked that there is a partition)
    if (o % bs)
      return ctx->err = "alfd_build_smoothed_aggregation: the partition offsets of block 0 must be multiples of block_size",
             ALFD_E_INVALID;
  DevCsr &dA = ctx->mat[ALFD_A], &dCt = ctx->mat[ALFD_CT], &dC = ctx->mat[ALFD_C];
  const int64_t row0 = ctx->part[0][rk], n = ctx->part[0][rk + 1] - row0, N = ctx->part[0].back();
  const int64_t lam0 = ctx->part[last][rk], M = ctx->part[last].back();
  int loc = ALFD_OK;
  if (!dA.present) ctx->err = "upload slot A first", loc = ALFD_E_NOT_SETUP;
  else if (dA.sparse || dA.nrows != n || dA.ncols != N)
    ctx->err = "alfd_build_smoothed_aggregation: slot A must hold this rank's rows of the square operator", loc = ALFD_E_INVALID;
  RC(joint_status(ctx, loc, 0, nullptr));
  // the penalty term: the single-rank rule; the pieces must be there on every rank or on none
  const bool pen_cfg = ctx->configured && c.variant != ALFD_RATIONAL && c.w_inverse == ALFD_W_DIAGONAL && !c.aug_assembled &&
                       sp.gamma != 0.0;
  const bool have = pen_cfg && dCt.present && dC.present && ctx->diag[ALFD_INVW] != nullptr;
  loc = ALFD_OK;
  if (have && (dCt.nrows != n || dCt.ncols != M || dC.ncols != N || ctx->diag_n[ALFD_INVW] != dC.nrows))
    ctx->err = "alfd_build_smoothed_aggregation: Ct / C / W^-1 do not match A and the partition", loc = ALFD_E_INVALID;
  int any_have = 0, any_not = 0;
  RC(joint_status(ctx, loc, have ? 1 : 0, &any_have));
  RC(joint_status(ctx, ALFD_OK, have ? 0 : 1, &any_not));
  if (any_have && any_not)
    return ctx->err = "alfd_build_smoothed_aggregation: Ct, C and W^-1 must be uploaded on every rank or on none", ALFD_E_INVALID;
  sp.use_pen = have;
  H.clear_input();
  hierarchy_input_changed(ctx);
  *touched = true;
  // ---- aggregates: device graph rows, gathered; greedy passes on every rank
  RC(strength_graph_dev(ctx, bs, sp.threshold));
  const int64_t nn = N / bs;
  std::vector<int32_t> agg;
  int64_t nc = 0;
  {
    const alfd_ctx::StrengthGraph &G = ctx->sg;
    std::vector<int32_t> len(G.n_nodes);
    for (int64_t I = 0; I < G.n_nodes; ++I) len[I] = (int32_t)(G.gp[I + 1] - G.gp[I]);
    std::vector<char> bl, bc, bw, bf;
    std::vector<size_t> sz;
    RC(allgather_bytes(ctx, len.data(), len.size() * 4, bl, sz));
    RC(allgather_bytes(ctx, G.gc.data(), G.gc.size() * 4, bc, sz));
    RC(allgather_bytes(ctx, G.gw.data(), G.gw.size() * 8, bw, sz));
    RC(allgather_bytes(ctx, G.fixed.data(), G.fixed.size() * 4, bf, sz));
    if ((int64_t)(bl.size() / 4) != nn || (int64_t)(bf.size() / 4) != nn || bc.size() / 4 != bw.size() / 8)
      return ctx->err = "alfd_build_smoothed_aggregation: inconsistent graph pieces", ALFD_E_COMM;
    std::vector<int64_t> gp(nn + 1, 0);
    const int32_t *gl = reinterpret_cast<const int32_t *>(bl.data());
    for (int64_t I = 0; I < nn; ++I) gp[I + 1] = gp[I] + gl[I];
    if (gp[nn] != (int64_t)(bc.size() / 4)) return ctx->err = "alfd_build_smoothed_aggregation: inconsistent graph pieces", ALFD_E_COMM;
    aggregate_graph(N, nn, bs, sp.max_aggregate_nodes, reinterpret_cast<const int32_t *>(bf.data()), gp.data(),
                    reinterpret_cast<const int32_t *>(bc.data()), reinterpret_cast<const double *>(bw.data()), agg, nc);
  }
  if (nc < 1 || nc >= N) return ctx->err = "algebraic aggregation found nothing to coarsen", ALFD_E_INVALID;
  // ---- the build-time views: A's rows with columns n + global id (device), Ct / C rows with global ids (host)
  const int64_t shift = n;
  int32_t *d_haloA = nullptr, *d_vcol = nullptr;
  double *d_w = nullptr, *d_d = nullptr, *d_v = nullptr, *d_t = nullptr, *d_y = nullptr;
  DevRawCsr dCtl, dCg;
  auto release = [&]() {
    for (void *q : {(void *)d_haloA, (void *)d_vcol, (void *)d_w, (void *)d_d, (void *)d_v, (void *)d_t, (void *)d_y})
      if (q) hipFree(q);
    dCtl.release();
    dCg.release();
  };
  auto hip = [&](hipError_t e) -> int {
    if (e == hipSuccess) return ALFD_OK;
    ctx->err = std::string("HIP error in the partitioned smoothed-aggregation build: ") + hipGetErrorString(e);
    return (int)ALFD_E_HIP;
  };
#define SB(call)                      \
  do {                                \
    const int rc__ = hip(call);       \
    if (rc__ != ALFD_OK) return rc__; \
  } while (0)
  HostCsr Ctl, Cl, Cg;
  std::vector<double> w_loc, w_g;
  auto to_global = [](HostCsr &h, const DevCsr &m, int64_t c0, int64_t ncols_global) {
    const std::vector<int32_t> ids = global_cols(m, c0);
    for (int32_t &col : h.col) col = ids[col];
    h.ncols = ncols_global;
  };
  auto views = [&]() -> int {
    if (!dA.halo_globals.empty()) {
      SB(hipMalloc((void **)&d_haloA, dA.halo_globals.size() * sizeof(int32_t)));
      SB(hipMemcpyAsync(d_haloA, dA.halo_globals.data(), dA.halo_globals.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                        ctx->stream));
    }
    SB(hipMalloc((void **)&d_vcol, std::max<int64_t>(dA.nnz, 1) * sizeof(int32_t)));
    if (dA.nnz > 0) {
      hipLaunchKernelGGL(sa_global_cols_kernel, dim3((unsigned)((dA.nnz + 255) / 256)), dim3(256), 0, ctx->stream, dA.nnz,
                         dA.col, dA.n_local_cols, row0, d_haloA, shift, d_vcol);
      SB(hipGetLastError());
    }
    if (sp.use_pen) {
      RC(download_csr(ctx, dCt, Ctl));
      to_global(Ctl, dCt, lam0, M);
      RC(download_csr(ctx, dC, Cl));
      to_global(Cl, dC, row0, N);
      w_loc.resize(ctx->diag_n[ALFD_INVW]);
      if (!w_loc.empty())
        SB(hipMemcpyAsync(w_loc.data(), ctx->diag[ALFD_INVW], w_loc.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    SB(hipStreamSynchronize(ctx->stream));
    return ALFD_OK;
  };
  int rc = joint_status(ctx, views(), 0, nullptr);
  if (rc != ALFD_OK) return release(), rc;
  if (sp.use_pen) {
    rc = gather_csr(ctx, Cl, nullptr, N, Cg);
    std::vector<char> bw;
    std::vector<size_t> sz;
    if (rc == ALFD_OK) rc = allgather_bytes(ctx, w_loc.data(), w_loc.size() * 8, bw, sz);
    if (rc == ALFD_OK && ((int64_t)(bw.size() / 8) != M || Cg.nrows != M))
      ctx->err = "alfd_build_smoothed_aggregation: the ranks' rows of C / W^-1 do not add up to the partition", rc = ALFD_E_COMM;
    if (rc != ALFD_OK) return release(), rc;
    w_g.resize(M);
    std::memcpy(w_g.data(), bw.data(), bw.size());
  }
  // ---- d and lambda_max(D^-1 Aug)
  std::vector<double> d_loc(n), y_loc(n), v(N), y(N);
  const unsigned gn = (unsigned)std::max<int64_t>(1, (n + 255) / 256), gm = (unsigned)std::max<int64_t>(1, (M + 255) / 256);
  auto diag = [&]() -> int {
    if (sp.use_pen) {
      RC(upload_raw(ctx, Ctl, dCtl));
      RC(upload_raw(ctx, Cg, dCg));
      SB(hipMalloc((void **)&d_w, std::max<int64_t>(M, 1) * sizeof(double)));
      SB(hipMalloc((void **)&d_t, std::max<int64_t>(M, 1) * sizeof(double)));
      if (M > 0) SB(hipMemcpyAsync(d_w, w_g.data(), M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    SB(hipMalloc((void **)&d_d, std::max<int64_t>(n, 1) * sizeof(double)));
    SB(hipMalloc((void **)&d_y, std::max<int64_t>(n, 1) * sizeof(double)));
    SB(hipMalloc((void **)&d_v, std::max<int64_t>(N, 1) * sizeof(double)));
    if (n > 0) {
      hipLaunchKernelGGL(sa_diag_rows_kernel, dim3(gn), dim3(256), 0, ctx->stream, n, row0, shift, dA.rp, d_vcol, dA.val,
                         sp.use_pen ? dCtl.rp : nullptr, dCtl.col, dCtl.val, d_w, sp.gamma, d_d);
      SB(hipGetLastError());
      SB(hipMemcpyAsync(d_loc.data(), d_d, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    SB(hipStreamSynchronize(ctx->stream));
    return ALFD_OK;
  };
  rc = joint_status(ctx, diag(), 0, nullptr);
  if (rc != ALFD_OK) return release(), rc;
  for (int64_t i = 0; i < N; ++i) v[i] = 1.0 + (double)(((uint64_t)i * 2654435761ull) & 1023ull) * (1.0 / 1024.0);
  double lam = 0.0;
  int bad = ALFD_OK;   // a rank-local failure inside the loop: the rank keeps taking part, the status goes round afterwards
  auto step = [&]() -> int {
    SB(hipMemcpyAsync(d_v, v.data(), N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (sp.use_pen && M > 0)
      hipLaunchKernelGGL(sa_power_t_kernel, dim3(gm), dim3(256), 0, ctx->stream, M, dCg.rp, dCg.col, dCg.val, d_w, d_v, d_t);
    if (n > 0) {
      hipLaunchKernelGGL(sa_power_rows_kernel, dim3(gn), dim3(256), 0, ctx->stream, n, shift, dA.rp, d_vcol, dA.val,
                         sp.use_pen ? dCtl.rp : nullptr, dCtl.col, dCtl.val, d_t, sp.gamma, d_v, d_d, d_y);
      SB(hipGetLastError());
      SB(hipMemcpyAsync(y_loc.data(), d_y, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    SB(hipStreamSynchronize(ctx->stream));
    return ALFD_OK;
  };
  for (int it = 0; it < sp.its; ++it) {
    double nv = 0.0;
    for (int64_t i = 0; i < N; ++i) nv = std::fma(v[i], v[i], nv);
    const double sc = 1.0 / std::sqrt(nv);
    for (int64_t i = 0; i < N; ++i) v[i] = v[i] * sc;
    if (bad == ALFD_OK) bad = step();
    std::vector<char> by;
    std::vector<size_t> sz;
    rc = allgather_bytes(ctx, y_loc.data(), y_loc.size() * 8, by, sz);
    if (rc == ALFD_OK && (int64_t)(by.size() / 8) != N) ctx->err = "alfd_build_smoothed_aggregation: inconsistent vector pieces", rc = ALFD_E_COMM;
    if (rc != ALFD_OK) return release(), rc;
    std::memcpy(y.data(), by.data(), by.size());
    double ny = 0.0;
    for (int64_t i = 0; i < N; ++i) ny = std::fma(y[i], y[i], ny);
    lam = std::sqrt(ny);
    std::swap(v, y);
  }
  rc = joint_status(ctx, bad, 0, nullptr);
  if (rc != ALFD_OK) return release(), rc;
  if (!(lam > 0.0) || !std::isfinite(lam))
    return release(), ctx->err = "alfd_build_smoothed_aggregation: lambda_max(D^-1 Aug) of level 0 is not positive and finite "
                                 "(zero diagonal?)", ALFD_E_INVALID;
  const double omega = sp.damping / lam;
  // ---- the own rows of P_0
  std::vector<int32_t> agg_ext(agg.begin() + row0, agg.begin() + row0 + n);   // [agg of the own rows | agg of all unknowns]
  agg_ext.insert(agg_ext.end(), agg.begin(), agg.end());
  std::vector<double> f(n, 0.0);
  for (int64_t i = 0; i < n; ++i)
    if (agg_ext[i] >= 0) f[i] = -omega / d_loc[i];
  HostCsr Q, Pl;
  bool fits = false;
  auto rows = [&]() -> int {
    if (sp.use_pen) {
      HostCsr Pt, Tm;
      sa_tentative(agg, nc, Pt);
      RC(product(ctx, Cg, Pt, Tm));
      sa_scale_rows(Tm, w_g.data(), sp.gamma);
      RC(product(ctx, Ctl, Tm, Q));
    }
    return sa_prolongator_dev_raw(ctx, n, dA.rp, d_vcol, dA.val, agg_ext, nc, f, Q, bs, sp.tau, sp.cap, Pl, &fits);
  };
  int any_nofit = 0;
  {
    const int l = rows();
    rc = joint_status(ctx, l, fits ? 0 : 1, &any_nofit);
  }
  if (rc != ALFD_OK) return release(), rc;
  if (any_nofit) {   // a row beyond the kernel's candidate set on some rank: every rank takes the host routines (same bits)
    auto host_rows = [&]() -> int {
      HostCsr h;
      RC(download_csr(ctx, dA, h));
      const std::vector<int32_t> ids = global_cols(dA, row0);
      for (int32_t &col : h.col) col = (int32_t)(shift + ids[col]);
      sa_rows_host(h, agg_ext, nc, f, sp.use_pen ? &Q : nullptr, Pl);
      if (sp.tau != 0.0 || sp.cap != 0) {
        HostCsr T;
        sa_truncate_host(Pl, agg_ext, bs, sp.tau, sp.cap, T);
        std::swap(Pl, T);
      }
      return ALFD_OK;
    };
    rc = joint_status(ctx, host_rows(), 0, nullptr);
    if (rc != ALFD_OK) return release(), rc;
  }
  release();
#undef SB
  H.agg[0].assign(agg_ext.begin(), agg_ext.begin() + n);
  H.P[0] = Pl;
  H.ncoarse[0] = nc;
  H.built_partitioned = true;
  std::vector<int64_t> &coff = ctx->ml_coff[0];   // any contiguous split is valid: whole nodes, evenly
  coff.assign(P + 1, 0);
  for (int p = 0; p <= P; ++p) coff[p] = (nc / bs) * p / P * bs;
  if (omega_out) omega_out[0] = omega;
  int nlev = 1;
  if (!(nc <= sp.min_coarse || nlev >= sp.max_levels)) {
    // ---- levels >= 1: the replicated Galerkin products of alfd_setup, then the single-rank loop on every rank
    HostCsr A1, C1, Ct1, Rg;
    RC(rep_level0_products(ctx, Pl, coff, true, A1, sp.use_pen ? &C1 : nullptr, Rg));
    if (sp.use_pen) transpose_host(C1, Ct1);
    const int l = sa_build_levels(ctx, H, sp, A1, C1, Ct1, w_g, nlev, omega_out);
    RC(joint_status(ctx, l, 0, nullptr));
  }
  if (levels_out) *levels_out = nlev;
  return ALFD_OK;
}

// alfd_build_smoothed_aggregation (tau = 0, cap = 0: nothing is truncated) and alfd_build_smoothed_aggregation_truncated
// on (A, Ct, invW, gamma) for block 0, on (A2, M, invW, gamma2) for block 1 (alfd_build_smoothed_aggregation_block)
static int build_smoothed_aggregation(alfd_ctx_t ctx, int block, int32_t block_size, double threshold,
                                      int32_t max_aggregate_nodes, double damping, double tau, int32_t cap, int64_t min_coarse,
                                      int32_t max_levels, int32_t *levels_out, double *omega_out) {
  CHECK_CTX();
  RC(check_block(ctx, block));
  const bool part = ctx->nranks > 1;   // block 0 on a partitioned context: collective, the rank-local checks are joint
  // a rank group that has no row partition yet has nothing the collective build could work on, and the single-rank
  // build is not defined on it: the answer such a context always got (the same on every rank, before any exchange)
  if (part && ctx->part.empty())
    return ctx->err = "alfd_build_smoothed_aggregation on a rank group needs alfd_set_partition (the single-rank build "
                      "does not run there)", ALFD_E_UNSUPPORTED;
  alfd_ctx::Hierarchy &H = ctx->hier[block];
  const int slotA = block == 0 ? ALFD_A : ALFD_A2, slotCt = block == 0 ? ALFD_CT : ALFD_M;
  if (block == 1 && !ctx->mat[slotA].present)
    return ctx->err = "a block-1 hierarchy needs slot A2 (the elliptic-interface variants)", ALFD_E_INVALID;
  if (ctx->configured && gd_nested(ctx))
    return ctx->err = "alfd_build_smoothed_aggregation: grad_div_in_A = 0 has no multilevel inner preconditioner", ALFD_E_UNSUPPORTED;
  if (!part && !ctx->mat[slotA].present) return ctx->err = "upload slot A first", ALFD_E_NOT_SETUP;
  if (block_size < 1 || !(threshold >= 0.0) || !std::isfinite(threshold) || max_aggregate_nodes < 2 || min_coarse < 1 ||
      !(damping > 0.0) || !std::isfinite(damping))
    return ctx->err = "alfd_build_smoothed_aggregation: bad arguments", ALFD_E_INVALID;
  if (!(tau >= 0.0) || !(tau < 1.0) || cap < 0) {
    H.clear_input();
    hierarchy_input_changed(ctx);
    return ctx->err = "alfd_build_smoothed_aggregation_truncated: drop_tolerance must be in [0, 1), max_row_entries >= 0",
           ALFD_E_INVALID;
  }
  if (!part && ctx->mat[slotA].nrows % block_size) return ctx->err = "rows of A are not a multiple of block_size", ALFD_E_INVALID;
  if (!part && ctx->mat[slotA].nrows != ctx->mat[slotA].ncols) return ctx->err = "A is not square", ALFD_E_INVALID;
  if (max_levels < 1 || max_levels > ALFD_MAX_LEVELS - 1) max_levels = ALFD_MAX_LEVELS - 1;
  const int its = ctx->configured ? ctx->cfg.cheb_power_its : 20;
  if (its < 1) return ctx->err = "cheb_power_its must be >= 1", ALFD_E_INVALID;
  if (part) {
    const SaParams sp{block_size, max_aggregate_nodes, cap, max_levels, its, threshold, damping, tau, ctx->cfg.gamma,
                      min_coarse, false};
    bool touched = false;   // a failure after the old hierarchy went leaves none behind
    const int rc = build_sa_partitioned(ctx, sp, levels_out, omega_out, &touched);
    if (rc != ALFD_OK && touched) H.clear_input();
    return rc;
  }
  // the penalty term: an AL variant with a diagonal W^-1, a non-zero gamma, A not already augmented, Ct and W^-1 present
  const alfd_config &c = ctx->cfg;
  const double gamma = block == 0 ? c.gamma : c.gamma2;
  const bool use_pen = ctx->configured && c.variant != ALFD_RATIONAL && c.w_inverse == ALFD_W_DIAGONAL &&
                       !c.aug_assembled && gamma != 0.0 && ctx->mat[slotCt].present && ctx->diag[ALFD_INVW] &&
                       (block == 0 || is_elliptic(c.variant));
  HostCsr A, C, Ct;
  std::vector<double> w;
  RC(download_csr(ctx, ctx->mat[slotA], A));
  if (use_pen) {
    RC(download_csr(ctx, ctx->mat[slotCt], Ct));
    if (Ct.nrows != A.nrows || ctx->diag_n[ALFD_INVW] != Ct.ncols)
      return ctx->err = "alfd_build_smoothed_aggregation: Ct / W^-1 do not match A", ALFD_E_INVALID;
    w.resize(Ct.ncols);
    if (!w.empty())
      HIPC(hipMemcpyAsync(w.data(), ctx->diag[ALFD_INVW], w.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    transpose_host(Ct, C);
  }
  H.clear_input();
  hierarchy_input_changed(ctx);
  int nlev = 0;
  const SaParams sp{block_size, max_aggregate_nodes, cap, max_levels, its, threshold, damping, tau, gamma, min_coarse, use_pen};
  RC(sa_build_levels(ctx, H, sp, A, C, Ct, w, nlev, omega_out));
  if (nlev == 0) return ctx->err = "algebraic aggregation found nothing to coarsen", ALFD_E_INVALID;
  if (levels_out) *levels_out = nlev;
  return ALFD_OK;
}

int alfd_build_smoothed_aggregation(alfd_ctx_t ctx, int32_t block_size, double threshold, int32_t max_aggregate_nodes,
                                    double damping, int64_t min_coarse, int32_t max_levels, int32_t *levels_out,
                                    double *omega_out) {
  return build_smoothed_aggregation(ctx, 0, block_size, threshold, max_aggregate_nodes, damping, 0.0, 0, min_coarse,
                                    max_levels, levels_out, omega_out);
}

int alfd_build_smoothed_aggregation_truncated(alfd_ctx_t ctx, int32_t block_size, double threshold,
                                              int32_t max_aggregate_nodes, double damping, double drop_tolerance,
                                              int32_t max_row_entries, int64_t min_coarse, int32_t max_levels,
                                              int32_t *levels_out, double *omega_out) {
  return build_smoothed_aggregation(ctx, 0, block_size, threshold, max_aggregate_nodes, damping, drop_tolerance,
                                    max_row_entries, min_coarse, max_levels, levels_out, omega_out);
}

int alfd_build_smoothed_aggregation_block(alfd_ctx_t ctx, int block, int32_t block_size, double threshold,
                                          int32_t max_aggregate_nodes, double damping, double drop_tolerance,
                                          int32_t max_row_entries, int64_t min_coarse, int32_t max_levels,
                                          int32_t *levels_out, double *omega_out) {
  return build_smoothed_aggregation(ctx, block, block_size, threshold, max_aggregate_nodes, damping, drop_tolerance,
                                    max_row_entries, min_coarse, max_levels, levels_out, omega_out);
}

int alfd_get_prolongator(alfd_ctx_t ctx, int level, int64_t *row_ptr, int32_t *col, double *val, int64_t capacity,
                         int64_t *n_fine, int64_t *n_coarse, int64_t *nnz) {
  return alfd_get_prolongator_block(ctx, 0, level, row_ptr, col, val, capacity, n_fine, n_coarse, nnz);
}

int alfd_get_prolongator_block(alfd_ctx_t ctx, int block, int level, int64_t *row_ptr, int32_t *col, double *val,
                               int64_t capacity, int64_t *n_fine, int64_t *n_coarse, int64_t *nnz) {
  if (!ctx || (block != 0 && block != 1) || level < 0 || level >= ALFD_MAX_LEVELS || ctx->hier[block].P[level].rp.empty())
    return ALFD_E_INVALID;
  const HostCsr &P = ctx->hier[block].P[level];
  if (n_fine) *n_fine = P.nrows;
  if (n_coarse) *n_coarse = P.ncols;
  if (nnz) *nnz = P.nnz();
  if (block == 0 && level == 0 && ctx->num.on() && P.nrows == ctx->num.n()) {   // rows back in the caller's order
    const std::vector<int64_t> &o2n = ctx->num.o2n;
    if ((col || val) && capacity < P.nnz()) return ALFD_E_INVALID;
    int64_t o = 0;
    for (int64_t i = 0; i < P.nrows; ++i) {
      const int64_t k0 = P.rp[o2n[i]], len = P.rp[o2n[i] + 1] - k0;
      if (row_ptr) row_ptr[i] = o;
      if (col) std::copy(P.col.begin() + k0, P.col.begin() + k0 + len, col + o);
      if (val) std::copy(P.val.begin() + k0, P.val.begin() + k0 + len, val + o);
      o += len;
    }
    if (row_ptr) row_ptr[P.nrows] = o;
    return ALFD_OK;
  }
  if (row_ptr) std::copy(P.rp.begin(), P.rp.end(), row_ptr);
  if (col || val) {
    if (capacity < P.nnz()) return ALFD_E_INVALID;
    if (col) std::copy(P.col.begin(), P.col.end(), col);
    if (val) std::copy(P.val.begin(), P.val.end(), val);
  }
  return ALFD_OK;
}

// ---- geometric hierarchies from support points (point_hierarchy.hpp; the rule: alfd.h)
// the two-call protocol of the CSR results on a point_hierarchy::Csr
static int point_csr_result(const point_hierarchy::Csr &P, int64_t *row_ptr, int32_t *col, double *val, int64_t capacity,
                            int64_t *nnz) {
  *nnz = P.rp.back();
  if (row_ptr) std::copy(P.rp.begin(), P.rp.end(), row_ptr);
  if (col || val) {
    if (capacity < P.rp.back()) return ALFD_E_INVALID;
    if (col) std::copy(P.col.begin(), P.col.end(), col);
    if (val) std::copy(P.val.begin(), P.val.end(), val);
  }
  return ALFD_OK;
}

int alfd_host_point_lattice(int64_t n, int32_t dim, const double *points, int32_t *cells, double *lo, double *delta,
                            int32_t *index, int32_t *complete) {
  point_hierarchy::Lattice L;
  if (!point_hierarchy::lattice(n, dim, points, L)) return ALFD_E_INVALID;
  for (int d = 0; d < dim; ++d) {
    if (cells) cells[d] = (int32_t)L.m[d];
    if (lo) lo[d] = L.lo[d];
    if (delta) delta[d] = L.delta[d];
  }
  if (index) std::copy(L.idx.begin(), L.idx.end(), index);
  if (complete) *complete = L.complete ? 1 : 0;
  return ALFD_OK;
}

int alfd_host_point_prolongator(int64_t n, int32_t dim, const double *points, int32_t ncomp, const int32_t *component,
                                const uint8_t *constrained, const int32_t *base, int32_t boundary_unknowns,
                                int64_t *p_row_ptr, int32_t *p_col, double *p_val, int64_t capacity, int64_t *nnz,
                                int64_t *n_coarse) {
  if (!nnz || ncomp < 1) return ALFD_E_INVALID;
  point_hierarchy::Lattice L;
  point_hierarchy::Csr P;
  int64_t cells[3];
  if (!point_hierarchy::lattice(n, dim, points, L) ||
      !point_hierarchy::point_prolongator(n, L, ncomp, component, constrained, base, boundary_unknowns != 0, P, cells))
    return ALFD_E_INVALID;
  if (n_coarse) *n_coarse = P.ncols;
  return point_csr_result(P, p_row_ptr, p_col, p_val, capacity, nnz);
}

int alfd_host_grid_prolongator(int32_t dim, int32_t ncomp, const int32_t *fine_cells, const int32_t *coarse_cells,
                               int32_t boundary_unknowns, int64_t *p_row_ptr, int32_t *p_col, double *p_val,
                               int64_t capacity, int64_t *n_fine, int64_t *n_coarse, int64_t *nnz) {
  if (!nnz || dim < 1 || dim > 3 || !fine_cells || !coarse_cells) return ALFD_E_INVALID;
  const int64_t fine[3] = {fine_cells[0], dim > 1 ? fine_cells[1] : 1, dim > 2 ? fine_cells[2] : 1};
  const int64_t coarse[3] = {coarse_cells[0], dim > 1 ? coarse_cells[1] : 1, dim > 2 ? coarse_cells[2] : 1};
  point_hierarchy::Csr P;
  if (!point_hierarchy::grid_prolongator(dim, ncomp, fine, coarse, boundary_unknowns != 0, P)) return ALFD_E_INVALID;
  if (n_fine) *n_fine = P.nrows;
  if (n_coarse) *n_coarse = P.ncols;
  return point_csr_result(P, p_row_ptr, p_col, p_val, capacity, nnz);
}

int alfd_host_point_hierarchy_cells(int32_t dim, int32_t ncomp, const int32_t *lattice_cells, const int32_t *base,
                                    int32_t boundary_unknowns, int64_t min_coarse, int32_t max_levels, int32_t *levels_out,
                                    int32_t *cells_out) {
  if (dim < 1 || dim > 3 || ncomp < 1 || ncomp > 64 || !lattice_cells || min_coarse < 1 || !levels_out) return ALFD_E_INVALID;
  if (max_levels < 1 || max_levels > ALFD_MAX_LEVELS - 1) max_levels = ALFD_MAX_LEVELS - 1;
  int64_t m[3] = {0, 0, 0};
  for (int d = 0; d < dim; ++d) {
    if (lattice_cells[d] < 0) return ALFD_E_INVALID;
    m[d] = lattice_cells[d];
  }
  std::vector<int64_t> cells;
  if (!point_hierarchy::level_cells(dim, ncomp, m, base, boundary_unknowns != 0, min_coarse, max_levels, cells))
    return ALFD_E_INVALID;
  *levels_out = (int32_t)(cells.size() / dim);
  if (cells_out)
    for (size_t k = 0; k < cells.size(); ++k) cells_out[k] = (int32_t)cells[k];
  return ALFD_OK;
}

int alfd_build_geometric_from_points(alfd_ctx_t ctx, int block, int64_t n, int32_t dim, const double *points,
                                     const int32_t *component, const uint8_t *constrained, const int32_t *base,
                                     int64_t min_coarse, int32_t max_levels, int32_t *levels_out, int32_t *cells_out) {
  CHECK_CTX();
  const std::string fn = "alfd_build_geometric_from_points: ";
  if (ctx->nranks > 1) return ctx->err = fn + "not available on a partitioned context", ALFD_E_UNSUPPORTED;
  RC(check_block(ctx, block));
  const DevCsr &A = ctx->mat[block == 0 ? ALFD_A : ALFD_A2];
  if (!A.present) return ctx->err = fn + (block == 0 ? "upload slot A first" : "upload slot A2 first"), ALFD_E_NOT_SETUP;
  if (n != A.nrows) return ctx->err = fn + "n is not the row count of the block's operator", ALFD_E_INVALID;
  if (dim < 1 || dim > 3 || !points || min_coarse < 1) return ctx->err = fn + "bad arguments", ALFD_E_INVALID;
  if (block == 1 && constrained) return ctx->err = fn + "block 1 has no constrained unknowns", ALFD_E_INVALID;
  if (max_levels < 1 || max_levels > ALFD_MAX_LEVELS - 1) max_levels = ALFD_MAX_LEVELS - 1;
  const bool renum = block == 0 && ctx->num.on();
  if (renum && n != ctx->num.n()) return ctx->err = fn + "n is not the size of the numbering (alfd_set_numbering)", ALFD_E_INVALID;
  point_hierarchy::Lattice L;
  if (!point_hierarchy::lattice(n, dim, points, L))
    return ctx->err = fn + "the points are not finite or no lattice", ALFD_E_INVALID;
  std::vector<uint8_t> lone;
  if (block == 0 && !constrained) {   // the rows of the resident A that hold nothing but their diagonal, in the caller's numbering
    std::vector<int32_t> fixed((size_t)n);
    int32_t *d_fixed = nullptr;
    double *d_diag = nullptr;
    auto release = [&]() {
      if (d_fixed) hipFree(d_fixed);
      if (d_diag) hipFree(d_diag);
    };
    auto flags = [&]() -> int {
      HIPC(hipMalloc((void **)&d_fixed, n * sizeof(int32_t)));
      HIPC(hipMalloc((void **)&d_diag, n * sizeof(double)));
      hipLaunchKernelGGL(sa_node_diag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, 1, (int64_t)0,
                         A.rp, A.col, A.val, (int32_t)A.ncols, (int64_t)0, (const int32_t *)nullptr, d_diag, d_fixed);
      HIPC(hipGetLastError());
      HIPC(hipMemcpyAsync(fixed.data(), d_fixed, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
      HIPC(hipStreamSynchronize(ctx->stream));
      return ALFD_OK;
    };
    if (A.sparse) {   // rows kept as a list (more than half of them empty): the host routine on a copy
      HostCsr h;
      std::vector<double> d;
      RC(download_csr(ctx, A, h));
      node_diag_host(h, 0, 1, d, fixed);
    } else {
      const int rc = flags();
      release();
      RC(rc);
    }
    lone.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) lone[(size_t)i] = fixed[(size_t)(renum ? ctx->num.o2n[i] : i)] != 0;
    constrained = lone.data();
  }
  std::vector<point_hierarchy::Csr> levels;
  std::vector<int64_t> cells;
  if (!point_hierarchy::hierarchy(n, L, 0, component, constrained, base, block == 1, min_coarse, max_levels, levels, cells))
    return ctx->err = fn + "the unknowns per node, the components or the base grid do not fit the lattice (an incomplete "
                           "lattice needs base)", ALFD_E_INVALID;
  // the inputs the block had are kept aside until every level is in: a refusal below hands them back untouched
  alfd_ctx::Hierarchy &H = ctx->hier[block];
  struct Kept {
    std::vector<int32_t> agg[ALFD_MAX_LEVELS];
    std::vector<double> wgt[ALFD_MAX_LEVELS];
    HostCsr P[ALFD_MAX_LEVELS];
    int64_t ncoarse[ALFD_MAX_LEVELS];
    bool built_partitioned, is_setup;
    const char *needs_full;
  } kept;
  auto exchange = [&]() {
    for (int l = 0; l < ALFD_MAX_LEVELS; ++l)
      kept.agg[l].swap(H.agg[l]), kept.wgt[l].swap(H.wgt[l]), std::swap(kept.P[l], H.P[l]), std::swap(kept.ncoarse[l], H.ncoarse[l]);
  };
  for (int l = 0; l < ALFD_MAX_LEVELS; ++l) kept.ncoarse[l] = 0;
  kept.built_partitioned = H.built_partitioned, kept.is_setup = ctx->is_setup, kept.needs_full = ctx->needs_full;
  exchange();   // H is now empty, as after clear_input()
  H.built_partitioned = false;
  for (size_t l = 0; l < levels.size(); ++l) {
    const point_hierarchy::Csr &P = levels[l];
    const int rc = alfd_set_prolongator_block(ctx, block, (int)l, P.nrows, P.ncols, P.rp.data(), P.col.data(), P.val.data());
    if (rc != ALFD_OK) {
      exchange();
      H.built_partitioned = kept.built_partitioned, ctx->is_setup = kept.is_setup, ctx->needs_full = kept.needs_full;
      return rc;
    }
  }
  hierarchy_input_changed(ctx);
  if (levels_out) *levels_out = (int32_t)levels.size();
  if (cells_out)
    for (size_t k = 0; k < cells.size(); ++k) cells_out[k] = (int32_t)cells[k];
  return ALFD_OK;
}

// The operands of one level's prolongator from the caller's arrays (alfd_host_smoothed_prolongator,
// alfd_smoothed_prolongator): A, Ct / C and the penalty view, the aggregates, d = diag(Aug) and its check.
struct SaLevelInput {
  HostCsr A, Ct, C;
  SaPenalty pen;
  std::vector<int32_t> agg;
  std::vector<double> d;
};

static int sa_level_input(int64_t nrows, const int64_t *row_ptr, const int32_t *col, const double *val, int64_t n_mult,
                          const int64_t *ct_row_ptr, const int32_t *ct_col, const double *ct_val, const double *w_inv,
                          double gamma, const int32_t *agg, int64_t n_coarse, double omega, const int64_t *nnz,
                          SaLevelInput &in) {
  if (nrows < 1 || !row_ptr || !col || !val || !agg || n_coarse < 1 || n_coarse > INT32_MAX || !nnz ||
      !std::isfinite(omega) || !std::isfinite(gamma) || row_ptr[0] != 0)
    return ALFD_E_INVALID;
  for (int64_t i = 0; i < nrows; ++i)
    if (row_ptr[i + 1] < row_ptr[i] || agg[i] < -1 || agg[i] >= n_coarse) return ALFD_E_INVALID;
  for (int64_t k = 0; k < row_ptr[nrows]; ++k)
    if (col[k] < 0 || col[k] >= nrows) return ALFD_E_INVALID;
  HostCsr &A = in.A, &Ct = in.Ct;
  A.nrows = A.ncols = nrows;
  A.rp.assign(row_ptr, row_ptr + nrows + 1);
  A.col.assign(col, col + A.rp[nrows]);
  A.val.assign(val, val + A.rp[nrows]);
  if (ct_row_ptr) {
    if (n_mult < 0 || !ct_col || !ct_val || !w_inv || ct_row_ptr[0] != 0) return ALFD_E_INVALID;
    for (int64_t i = 0; i < nrows; ++i)
      if (ct_row_ptr[i + 1] < ct_row_ptr[i]) return ALFD_E_INVALID;
    for (int64_t k = 0; k < ct_row_ptr[nrows]; ++k)
      if (ct_col[k] < 0 || ct_col[k] >= n_mult) return ALFD_E_INVALID;
    Ct.nrows = nrows;
    Ct.ncols = n_mult;
    Ct.rp.assign(ct_row_ptr, ct_row_ptr + nrows + 1);
    Ct.col.assign(ct_col, ct_col + Ct.rp[nrows]);
    Ct.val.assign(ct_val, ct_val + Ct.rp[nrows]);
    transpose_host(Ct, in.C);
    in.pen.Ct = &in.Ct, in.pen.C = &in.C, in.pen.w = w_inv, in.pen.gamma = gamma;
  }
  in.agg.assign(agg, agg + nrows);
  sa_diag(A, in.pen, in.d);
  for (int64_t i = 0; i < nrows; ++i)
    if (in.agg[i] >= 0 && !(in.d[i] != 0.0)) return ALFD_E_INVALID;
  return ALFD_OK;
}

// the two-call protocol of the CSR results: sizes and the row pointer first, then the arrays with capacity
static int csr_result(const HostCsr &M, int64_t *row_ptr, int32_t *col, double *val, int64_t capacity, int64_t *nnz) {
  *nnz = M.nnz();
  if (row_ptr) std::copy(M.rp.begin(), M.rp.end(), row_ptr);
  if (col || val) {
    if (capacity < M.nnz()) return ALFD_E_INVALID;
    if (col) std::copy(M.col.begin(), M.col.end(), col);
    if (val) std::copy(M.val.begin(), M.val.end(), val);
  }
  return ALFD_OK;
}

int alfd_host_smoothed_prolongator(int64_t nrows, const int64_t *row_ptr, const int32_t *col, const double *val,
                                   int64_t n_mult, const int64_t *ct_row_ptr, const int32_t *ct_col, const double *ct_val,
                                   const double *w_inv, double gamma, const int32_t *agg, int64_t n_coarse, double omega,
                                   int64_t *p_row_ptr, int32_t *p_col, double *p_val, int64_t capacity, int64_t *nnz) {
  SaLevelInput in;
  RC(sa_level_input(nrows, row_ptr, col, val, n_mult, ct_row_ptr, ct_col, ct_val, w_inv, gamma, agg, n_coarse, omega, nnz, in));
  HostCsr Q, P;
  std::vector<double> f;
  sa_factors(in.agg, in.d, omega, f);
  RC(sa_penalty_rows(nullptr, in.pen, in.agg, n_coarse, Q));
  sa_rows_host(in.A, in.agg, n_coarse, f, in.pen.on() ? &Q : nullptr, P);
  return csr_result(P, p_row_ptr, p_col, p_val, capacity, nnz);
}

int alfd_smoothed_prolongator(alfd_ctx_t ctx, int64_t nrows, const int64_t *row_ptr, const int32_t *col, const double *val,
                              int64_t n_mult, const int64_t *ct_row_ptr, const int32_t *ct_col, const double *ct_val,
                              const double *w_inv, double gamma, const int32_t *agg, int64_t n_coarse, double omega,
                              int32_t block_size, double drop_tolerance, int32_t max_row_entries, int64_t *p_row_ptr,
                              int32_t *p_col, double *p_val, int64_t capacity, int64_t *nnz, int32_t *on_device) {
  CHECK_CTX();
  if (block_size < 1 || !(drop_tolerance >= 0.0) || !(drop_tolerance < 1.0) || max_row_entries < 0)
    return ctx->err = "alfd_smoothed_prolongator: bad block_size, drop_tolerance or max_row_entries", ALFD_E_INVALID;
  SaLevelInput in;
  if (sa_level_input(nrows, row_ptr, col, val, n_mult, ct_row_ptr, ct_col, ct_val, w_inv, gamma, agg, n_coarse, omega, nnz,
                     in) != ALFD_OK)
    return ctx->err = "alfd_smoothed_prolongator: bad arguments (shapes, column or aggregate ranges, a zero diagonal)",
           ALFD_E_INVALID;
  HostCsr P;
  bool dev = false;
  RC(sa_level_prolongator(ctx, in.A, in.pen, in.agg, n_coarse, in.d, omega, block_size, drop_tolerance, max_row_entries,
                          P, &dev));
  if (on_device) *on_device = dev ? 1 : 0;
  return csr_result(P, p_row_ptr, p_col, p_val, capacity, nnz);
}

// a caller's CSR arrays as a HostCsr; false for a bad shape, row pointer or column
static bool csr_input(int64_t nrows, int64_t ncols, const int64_t *row_ptr, const int32_t *col, const double *val,
                      HostCsr &M) {
  if (nrows < 0 || ncols < 0 || ncols > INT32_MAX || !row_ptr || row_ptr[0] != 0) return false;
  for (int64_t i = 0; i < nrows; ++i)
    if (row_ptr[i + 1] < row_ptr[i]) return false;
  const int64_t nnz = row_ptr[nrows];
  if (nnz > 0 && (!col || !val)) return false;
  for (int64_t k = 0; k < nnz; ++k)
    if (col[k] < 0 || col[k] >= ncols) return false;
  M.nrows = nrows;
  M.ncols = ncols;
  M.rp.assign(row_ptr, row_ptr + nrows + 1);
  M.col.assign(col, col + nnz);
  M.val.assign(val, val + nnz);
  return true;
}

int alfd_host_sparse_product(int64_t a_nrows, int64_t a_ncols, const int64_t *a_row_ptr, const int32_t *a_col,
                             const double *a_val, int64_t p_ncols, const int64_t *p_row_ptr, const int32_t *p_col,
                             const double *p_val, int64_t *out_row_ptr, int32_t *out_col, double *out_val,
                             int64_t capacity, int64_t *nnz) {
  HostCsr A, Pm, out;
  if (!nnz || !csr_input(a_nrows, a_ncols, a_row_ptr, a_col, a_val, A) ||
      !csr_input(a_ncols, p_ncols, p_row_ptr, p_col, p_val, Pm))
    return ALFD_E_INVALID;
  spgemm_host(A, Pm, out);
  return csr_result(out, out_row_ptr, out_col, out_val, capacity, nnz);
}

int alfd_sparse_product(alfd_ctx_t ctx, int64_t a_nrows, int64_t a_ncols, const int64_t *a_row_ptr, const int32_t *a_col,
                        const double *a_val, int64_t p_ncols, const int64_t *p_row_ptr, const int32_t *p_col,
                        const double *p_val, int64_t *out_row_ptr, int32_t *out_col, double *out_val, int64_t capacity,
                        int64_t *nnz, int32_t *on_device) {
  CHECK_CTX();
  HostCsr A, Pm, out;
  if (!nnz || !csr_input(a_nrows, a_ncols, a_row_ptr, a_col, a_val, A) ||
      !csr_input(a_ncols, p_ncols, p_row_ptr, p_col, p_val, Pm))
    return ctx->err = "alfd_sparse_product: bad arguments (shapes, row pointers or column ranges)", ALFD_E_INVALID;
  bool dev = false;
  RC(product_dev(ctx, A, Pm, out, &dev));
  if (on_device) *on_device = dev ? 1 : 0;
  return csr_result(out, out_row_ptr, out_col, out_val, capacity, nnz);
}

int alfd_host_truncate_prolongator(int64_t nrows, int64_t n_coarse, const int64_t *p_row_ptr, const int32_t *p_col,
                                   const double *p_val, const int32_t *agg, int32_t block_size, double drop_tolerance,
                                   int32_t max_row_entries, int64_t *out_row_ptr, int32_t *out_col, double *out_val,
                                   int64_t capacity, int64_t *nnz) {
  if (nrows < 1 || n_coarse < 1 || n_coarse > INT32_MAX || !p_row_ptr || !p_col || !p_val || !agg || !nnz ||
      block_size < 1 || !(drop_tolerance >= 0.0) || !(drop_tolerance < 1.0) || max_row_entries < 0 || p_row_ptr[0] != 0)
    return ALFD_E_INVALID;
  for (int64_t i = 0; i < nrows; ++i) {
    if (p_row_ptr[i + 1] < p_row_ptr[i] || agg[i] < -1 || agg[i] >= n_coarse) return ALFD_E_INVALID;
    bool has = agg[i] < 0;
    for (int64_t e = p_row_ptr[i]; e < p_row_ptr[i + 1]; ++e) {
      if (p_col[e] < 0 || p_col[e] >= n_coarse || (e > p_row_ptr[i] && p_col[e] <= p_col[e - 1])) return ALFD_E_INVALID;
      has = has || p_col[e] == agg[i];
    }
    if (!has) return ALFD_E_INVALID;
  }
  HostCsr P, T;
  P.nrows = nrows;
  P.ncols = n_coarse;
  P.rp.assign(p_row_ptr, p_row_ptr + nrows + 1);
  P.col.assign(p_col, p_col + P.rp[nrows]);
  P.val.assign(p_val, p_val + P.rp[nrows]);
  sa_truncate_host(P, std::vector<int32_t>(agg, agg + nrows), block_size, drop_tolerance, max_row_entries, T);
  *nnz = T.nnz();
  if (out_row_ptr) std::copy(T.rp.begin(), T.rp.end(), out_row_ptr);
  if (out_col || out_val) {
    if (capacity < T.nnz()) return ALFD_E_INVALID;
    if (out_col) std::copy(T.col.begin(), T.col.end(), out_col);
    if (out_val) std::copy(T.val.begin(), T.val.end(), out_val);
  }
  return ALFD_OK;
}

int alfd_set_aggregate_partition(alfd_ctx_t ctx, int level, const int64_t *coarse_offsets) {
  CHECK_CTX();
  if (level < 0 || level >= ALFD_MAX_LEVELS || !coarse_offsets) return ALFD_E_INVALID;
  ctx->ml_coff[level].assign(coarse_offsets, coarse_offsets + ctx->nranks + 1);
  hierarchy_input_changed(ctx);
  return ALFD_OK;
}

int alfd_configure(alfd_ctx_t ctx, const alfd_config *cfg) {
  CHECK_CTX();
  if (!cfg) return ALFD_E_INVALID;
  if (cfg->variant < ALFD_AL2 || cfg->variant > ALFD_RATIONAL) return ALFD_E_INVALID;
  ctx->cfg = *cfg;
  ctx->configured = true;
  ctx->is_setup = false;
  return ALFD_OK;
}

int alfd_set_controls(alfd_ctx_t ctx, const alfd_control *outer, const alfd_control *inner, const alfd_control *mp_inner) {
  CHECK_CTX();
  if (!ctx->configured) return ctx->err = "alfd_configure not called", ALFD_E_NOT_SETUP;
  for (const alfd_control *c : {outer, inner, mp_inner})
    if (c && (c->kind < ALFD_CTRL_ABS || c->kind > ALFD_CTRL_FIXED_ITERS || c->max_steps < 0))
      return ctx->err = "alfd_set_controls: bad control", ALFD_E_INVALID;
  if (outer) ctx->cfg.outer = *outer;
  if (inner) ctx->cfg.inner = *inner;
  if (mp_inner) ctx->cfg.mp_inner = *mp_inner;
  return ALFD_OK;
}

int alfd_setup(alfd_ctx_t ctx) {
  CHECK_CTX();
  return setup(ctx);
}

int alfd_setup_coupling(alfd_ctx_t ctx) {
  CHECK_CTX();
  return setup_coupling(ctx);
}

int alfd_get_setup_counts(alfd_ctx_t ctx, int64_t *counts) {
  if (!ctx || !counts) return ALFD_E_INVALID;
  std::copy(ctx->setup_counts, ctx->setup_counts + ALFD_SC_NCOUNTS, counts);
  return ALFD_OK;
}

int alfd_precond_apply(alfd_ctx_t ctx, const double *const *src, double *const *dst, alfd_result *res) {
  CHECK_CTX();
  CHECK_SETUP();
  if (!src || !dst) return ALFD_E_INVALID;
  reset_stats(ctx);
  RC(to_device(ctx, src, ctx->st_in));
  HIPC(hipMemsetAsync(ctx->st_out, 0, ctx->ntot() * sizeof(double), ctx->stream));
  const int rc = precond_apply(ctx, ctx->st_in, ctx->st_out);
  RC(to_host(ctx, ctx->st_out, dst));
  if (res) {
    std::memset(res, 0, sizeof(*res));
    fill_result(ctx, res, rc);
  }
  return rc;
}

int alfd_system_apply(alfd_ctx_t ctx, const double *const *src, double *const *dst) {
  CHECK_CTX();
  CHECK_SETUP();
  if (!src || !dst) return ALFD_E_INVALID;
  RC(to_device(ctx, src, ctx->st_in));
  HIPC(hipMemsetAsync(ctx->st_out, 0, ctx->ntot() * sizeof(double), ctx->stream));
  RC(system_apply(ctx, ctx->st_in, ctx->st_out));
  return to_host(ctx, ctx->st_out, dst);
}

int alfd_augment_rhs(alfd_ctx_t ctx, double *const *rhs) {
  CHECK_CTX();
  CHECK_SETUP();
  if (!rhs) return ALFD_E_INVALID;
  if (!ctx->diag[ALFD_INVW] || ctx->cfg.variant == ALFD_RATIONAL)
    return ctx->err = "rhs augmentation applies to the AL variants only", ALFD_E_UNSUPPORTED;
  const int last = ctx->nblocks - 1;
  RC(to_device(ctx, rhs, ctx->st_in));
  RC(winv_scale(ctx, 1.0, ctx->st_in + ctx->off[last], ctx->t_lam));
  RC(spmv(ctx, ALFD_CT, ctx->t_lam, ctx->st_in + ctx->off[0], 1, ctx->cfg.gamma));
  return to_host(ctx, ctx->st_in, rhs);
}

int alfd_upload_rhs(alfd_ctx_t ctx, const double *const *rhs, const double *const *x0) {
  CHECK_CTX();
  CHECK_SETUP();
  if (!rhs) return ALFD_E_INVALID;
  RC(to_device(ctx, rhs, ctx->bb));
  if (x0)
    RC(to_device(ctx, x0, ctx->io));
  else
    HIPC(hipMemsetAsync(ctx->io, 0, ctx->ntot() * sizeof(double), ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  return ALFD_OK;
}

int alfd_solve_resident(alfd_ctx_t ctx, alfd_result *res) {
  CHECK_CTX();
  CHECK_SETUP();
  if (!res) return ALFD_E_INVALID;
  std::memset(res, 0, sizeof(*res));
  reset_stats(ctx);
  // x <- initial guess kept in io (so the solve can be repeated)
  HIPC(hipMemcpyAsync(ctx->xb, ctx->io, ctx->ntot() * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = ctx->cfg.outer_solver == ALFD_OUTER_MINRES               ? minres(ctx, res)
                 : ctx->cfg.fgmres_flavour == ALFD_FGMRES_DEALII_95 ? fgmres_dealii95(ctx, res)
                                                                    : fgmres(ctx, res);
  hipStreamSynchronize(ctx->stream);
  res->solve_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  flush_timers(ctx);
  fill_result(ctx, res, rc);
  return rc;
}

int alfd_download_solution(alfd_ctx_t ctx, double *const *x) {
  CHECK_CTX();
  CHECK_SETUP();
  if (!x) return ALFD_E_INVALID;
  return to_host(ctx, ctx->xb, x);
}

int alfd_solve(alfd_ctx_t ctx, const double *const *rhs, double *const *x, alfd_result *res) {
  CHECK_CTX();
  CHECK_SETUP();
  if (!rhs || !x || !res) return ALFD_E_INVALID;
  RC(alfd_upload_rhs(ctx, rhs, x));
  const int rc = alfd_solve_resident(ctx, res);
  const int rc2 = alfd_download_solution(ctx, x);
  return rc != ALFD_OK ? rc : rc2;
}

// ---- the same calls on caller DEVICE blocks: validate, await the caller's stream, pack (all inputs before any
// output is written, so outputs may alias inputs), run the code of the host-pointer call, unpack, synchronise.
int alfd_upload_rhs_device(alfd_ctx_t ctx, const double *const *rhs, const double *const *x0, void *stream) {
  CHECK_CTX();
  CHECK_SETUP();
  if (!rhs) return ALFD_E_INVALID;
  RC(check_device_blocks(ctx, rhs, "rhs_blocks"));
  if (x0) RC(check_device_blocks(ctx, x0, "x0_blocks"));
  RC(await_stream(ctx, stream));
  RC(pack_device(ctx, rhs, ctx->bb));
  if (x0)
    RC(pack_device(ctx, x0, ctx->io));
  else
    HIPC(hipMemsetAsync(ctx->io, 0, ctx->ntot() * sizeof(double), ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  return ALFD_OK;
}

int alfd_download_solution_device(alfd_ctx_t ctx, double *const *x, void *stream) {
  CHECK_CTX();
  CHECK_SETUP();
  if (!x) return ALFD_E_INVALID;
  RC(check_device_blocks(ctx, x, "x_blocks"));
  RC(await_stream(ctx, stream));   // work the caller has queued on x (readers included) ends before x is written
  return unpack_device(ctx, ctx->xb, x);
}

int alfd_solve_device(alfd_ctx_t ctx, const double *const *rhs, double *const *x, alfd_result *res, void *stream) {
  CHECK_CTX();
  CHECK_SETUP();
  if (!rhs || !x || !res) return ALFD_E_INVALID;
  RC(check_device_blocks(ctx, rhs, "rhs_blocks"));
  RC(check_device_blocks(ctx, x, "x_blocks"));
  RC(await_stream(ctx, stream));
  RC(pack_device(ctx, rhs, ctx->bb));
  RC(pack_device(ctx, x, ctx->io));
  const int rc = alfd_solve_resident(ctx, res);
  const int rc2 = unpack_device(ctx, ctx->xb, x);
  return rc != ALFD_OK ? rc : rc2;
}

int alfd_precond_apply_device(alfd_ctx_t ctx, const double *const *src, double *const *dst, alfd_result *res,
                              void *stream) {
  CHECK_CTX();
  CHECK_SETUP();
  if (!src || !dst) return ALFD_E_INVALID;
  RC(check_device_blocks(ctx, src, "src_blocks"));
  RC(check_device_blocks(ctx, dst, "dst_blocks"));
  RC(await_stream(ctx, stream));
  reset_stats(ctx);
  RC(pack_device(ctx, src, ctx->st_in));
  HIPC(hipMemsetAsync(ctx->st_out, 0, ctx->ntot() * sizeof(double), ctx->stream));
  const int rc = precond_apply(ctx, ctx->st_in, ctx->st_out);
  RC(unpack_device(ctx, ctx->st_out, dst));
  if (res) {
    std::memset(res, 0, sizeof(*res));
    fill_result(ctx, res, rc);
  }
  return rc;
}

int alfd_system_apply_device(alfd_ctx_t ctx, const double *const *src, double *const *dst, void *stream) {
  CHECK_CTX();
  CHECK_SETUP();
  if (!src || !dst) return ALFD_E_INVALID;
  RC(check_device_blocks(ctx, src, "src_blocks"));
  RC(check_device_blocks(ctx, dst, "dst_blocks"));
  RC(await_stream(ctx, stream));
  RC(pack_device(ctx, src, ctx->st_in));
  HIPC(hipMemsetAsync(ctx->st_out, 0, ctx->ntot() * sizeof(double), ctx->stream));
  RC(system_apply(ctx, ctx->st_in, ctx->st_out));
  return unpack_device(ctx, ctx->st_out, dst);
}

int alfd_augment_rhs_device(alfd_ctx_t ctx, double *const *rhs, void *stream) {
  CHECK_CTX();
  CHECK_SETUP();
  if (!rhs) return ALFD_E_INVALID;
  if (!ctx->diag[ALFD_INVW] || ctx->cfg.variant == ALFD_RATIONAL)
    return ctx->err = "rhs augmentation applies to the AL variants only", ALFD_E_UNSUPPORTED;
  RC(check_device_blocks(ctx, rhs, "rhs_blocks"));
  RC(await_stream(ctx, stream));
  const int last = ctx->nblocks - 1;
  RC(pack_device(ctx, rhs, ctx->st_in));
  RC(winv_scale(ctx, 1.0, ctx->st_in + ctx->off[last], ctx->t_lam));
  RC(spmv(ctx, ALFD_CT, ctx->t_lam, ctx->st_in + ctx->off[0], 1, ctx->cfg.gamma));
  return unpack_device(ctx, ctx->st_in, rhs);
}

int alfd_get_history(alfd_ctx_t ctx, double *out, int32_t capacity, int32_t *count) {
  if (!ctx) return ALFD_E_INVALID;
  if (count) *count = (int32_t)ctx->history.size();
  if (out)
    for (int32_t i = 0; i < capacity && i < (int32_t)ctx->history.size(); ++i) out[i] = ctx->history[i];
  return ALFD_OK;
}

int alfd_spmv(alfd_ctx_t ctx, int slot, const double *x, double *y, int mode, double alpha) {
  CHECK_CTX();
  if (slot < 0 || slot >= ALFD_NSLOTS || !ctx->mat[slot].present) return ALFD_E_INVALID;
  if (!x || !y || (mode != 0 && mode != 1)) return ALFD_E_INVALID;
  const DevCsr &m = ctx->mat[slot];
  // partitioned context: collective over the ranks; x = this rank's owned columns, y = its rows
  const int64_t nx = ctx->nranks > 1 ? (int64_t)m.n_local_cols : m.ncols;
  double *dx = nullptr, *dy = nullptr;
  HIPC(hipMalloc((void **)&dx, std::max<int64_t>(nx, 1) * sizeof(double)));
  HIPC(hipMalloc((void **)&dy, std::max<int64_t>(m.nrows, 1) * sizeof(double)));
  HIPC(hipMemcpyAsync(dx, x, nx * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(dy, y, m.nrows * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const int rc = spmv(ctx, slot, dx, dy, mode, alpha);
  if (rc == ALFD_OK) {
    HIPC(hipMemcpyAsync(y, dy, m.nrows * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
  }
  hipFree(dx);
  hipFree(dy);
  return rc;
}

int alfd_spmv_scaled(alfd_ctx_t ctx, int slot, const double *x, const double *d, double *y, double *y2) {
  CHECK_CTX();
  if (slot < 0 || slot >= ALFD_NSLOTS || !ctx->mat[slot].present) return ALFD_E_INVALID;
  if (!x || !d || !y || y2 == y) return ALFD_E_INVALID;   // the kernels take y and y2 as __restrict__
  const DevCsr &m = ctx->mat[slot];
  const int64_t nx = ctx->nranks > 1 ? (int64_t)m.n_local_cols : m.ncols;
  const size_t rows = std::max<int64_t>(m.nrows, 1) * sizeof(double), nb = m.nrows * sizeof(double);
  double *dx = nullptr, *dd = nullptr, *dy = nullptr, *dy2 = nullptr;
  HIPC(hipMalloc((void **)&dx, std::max<int64_t>(nx, 1) * sizeof(double)));
  HIPC(hipMalloc((void **)&dd, rows));
  HIPC(hipMalloc((void **)&dy, rows));
  if (y2) HIPC(hipMalloc((void **)&dy2, rows));
  HIPC(hipMemcpyAsync(dx, x, nx * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(dd, d, nb, hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(dy, y, nb, hipMemcpyHostToDevice, ctx->stream));
  if (y2) HIPC(hipMemcpyAsync(dy2, y2, nb, hipMemcpyHostToDevice, ctx->stream));
  // the solver's own call: epilogue 2 (t = W^-1 .* (C x)) or 3 (y_lambda = C x and t beside it)
  const int rc = spmv(ctx, slot, dx, dy, y2 ? 3 : 2, 0.0, dd, dy2);
  if (rc == ALFD_OK) {
    HIPC(hipMemcpyAsync(y, dy, nb, hipMemcpyDeviceToHost, ctx->stream));
    if (y2) HIPC(hipMemcpyAsync(y2, dy2, nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
  }
  hipFree(dx);
  hipFree(dd);
  hipFree(dy);
  hipFree(dy2);
  return rc;
}

int alfd_spmv_pair(alfd_ctx_t ctx, int slot_a, int slot_c, const double *x, const double *d, double *y, double *t) {
  CHECK_CTX();
  for (int slot : {slot_a, slot_c})
    if (slot < 0 || slot >= ALFD_NSLOTS || !ctx->mat[slot].present) return ALFD_E_INVALID;
  if (!x || !d || !y || !t || t == y) return ALFD_E_INVALID;
  const DevCsr &A = ctx->mat[slot_a], &Cm = ctx->mat[slot_c];
  const int form = pair_forms(ctx, A, Cm);
  if (!form) return ctx->err = "alfd_spmv_pair: the two slots do not qualify for the pair launch", ALFD_E_UNSUPPORTED;
  double *dx = nullptr, *dd = nullptr, *dy = nullptr, *dt = nullptr;
  HIPC(hipMalloc((void **)&dx, A.ncols * sizeof(double)));
  HIPC(hipMalloc((void **)&dd, Cm.nrows * sizeof(double)));
  HIPC(hipMalloc((void **)&dy, A.nrows * sizeof(double)));
  HIPC(hipMalloc((void **)&dt, Cm.nrows * sizeof(double)));
  HIPC(hipMemcpyAsync(dx, x, A.ncols * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(dd, d, Cm.nrows * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(dy, y, A.nrows * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(dt, t, Cm.nrows * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const int rc = launch_pair(ctx, form, A, slot_a == ALFD_A ? ALFD_T_SPMV_A : ALFD_T_SPMV_OTHER, Cm, dd, dx, dy, dt);
  if (rc == ALFD_OK) {
    HIPC(hipMemcpyAsync(y, dy, A.nrows * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipMemcpyAsync(t, dt, Cm.nrows * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
  }
  hipFree(dx);
  hipFree(dd);
  hipFree(dy);
  hipFree(dt);
  return rc;
}

int alfd_get_fused_tail_launches(alfd_ctx_t ctx, int64_t *count) {
  CHECK_CTX();
  if (!count) return ALFD_E_INVALID;
  *count = ctx->fused_tail_launches;
  return ALFD_OK;
}

int alfd_spmv_tail_step(alfd_ctx_t ctx, int slot_a, int form, const alfd_tail_step *s) {
  CHECK_CTX();
  if (!s || (form != 0 && form != 1) || slot_a < 0 || slot_a >= ALFD_NSLOTS || !ctx->mat[slot_a].present) return ALFD_E_INVALID;
  if (s->slot_c >= ALFD_NSLOTS || (s->slot_c >= 0 && (!ctx->mat[s->slot_c].present || !s->w))) return ALFD_E_INVALID;
  if (s->mode < TAIL_STEP || s->mode > TAIL_RES_INIT_ADD || !s->x || !s->y || !s->t || !s->rin || !s->ct_rp) return ALFD_E_INVALID;
  DevCsr &A = ctx->mat[slot_a];
  DevCsr *Cm = s->slot_c >= 0 ? &ctx->mat[s->slot_c] : nullptr;
  const int64_t n = A.nrows, nt = s->ct_ncols;
  if (s->ct_nrows != n || nt < 1 || (Cm && (Cm->nrows != nt || Cm->ncols != A.ncols))) return ALFD_E_INVALID;
  const int mode = s->mode;
  const bool step = mode <= TAIL_LAST_ADD, add = mode == TAIL_LAST_ADD || mode == TAIL_RES_INIT_ADD;
  const double *outs[3];
  AugTailArgs hp;   // the caller's (host) vectors in the fields the mode uses
  hp.dinv = s->dinv, hp.rin = s->rin, hp.din = s->din, hp.zin = s->zin;
  hp.res = s->res, hp.d = s->d, hp.z = s->z, hp.zout = s->zout, hp.store_res = s->store_res;
  const int nout = tail_outputs(mode, hp, outs);
  for (int i = 0; i < nout; ++i)
    if (!outs[i]) return ALFD_E_INVALID;
  if ((mode != TAIL_RES && !s->dinv) || (step && (!s->din || !s->zin))) return ALFD_E_INVALID;
  if (ctx->nranks != 1 || ctx->cfg.w_inverse != ALFD_W_DIAGONAL || ctx->cfg.aug_assembled || gd_nested(ctx))
    return ctx->err = "alfd_spmv_tail_step: one rank, the diagonal W^-1 and the factored operator", ALFD_E_UNSUPPORTED;
  static const int32_t no_col = 0;
  static const double no_val = 0;
  const bool empty = s->ct_rp[n] == 0;
  RC(upload_matrix(ctx, kScratchSlot, n, nt, s->ct_rp, empty ? &no_col : s->ct_col, empty ? &no_val : s->ct_val));
  DevCsr Ct = std::move(ctx->mat[kScratchSlot]);
  ctx->mat[kScratchSlot] = DevCsr();
  // the device images: npad entries for the vectors over the rows of A (the sweep of aug_tail_kernel covers the padding),
  // one image per distinct host address, so that an output passed at x's address IS x on the device
  const int64_t npad = pad_chunk(n);
  struct Img { const double *h; double *d; int64_t len; bool out; };
  std::vector<Img> img;
  int rc = ALFD_OK;
  auto dev = [&](const double *h, int64_t len, bool out) -> double * {
    if (!h) return nullptr;
    for (Img &g : img)
      if (g.h == h) return g.out = g.out || out, g.d;
    const int64_t cap = std::max<int64_t>(std::max(len, npad), 1);
    double *d = nullptr;
    if (hipMalloc((void **)&d, cap * sizeof(double)) != hipSuccess) return rc = ALFD_E_HIP, nullptr;
    hipMemsetAsync(d, 0, cap * sizeof(double), ctx->stream);
    hipMemcpyAsync(d, h, len * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    img.push_back(Img{h, d, len, out});
    return d;
  };
  AugOp F;
  F.A = &A, F.C = Cm, F.Ct = &Ct;
  F.clsA = slot_a == ALFD_A ? ALFD_T_SPMV_A : ALFD_T_SPMV_OTHER;
  F.gamma = s->gamma, F.npad = npad;
  const double *dx = dev(s->x, A.ncols, false);
  double *dy = dev(s->y, n, true);
  F.tlam = dev(s->t, nt, Cm != nullptr);
  F.w = Cm ? dev(s->w, nt, false) : nullptr;
  AugTailArgs p;
  p.gamma = s->gamma, p.c1 = s->c1, p.c2 = s->c2, p.store_res = s->store_res;
  p.rin = dev(s->rin, n, false);
  if (mode != TAIL_RES) p.dinv = dev(s->dinv, n, false);
  if (step) p.din = dev(s->din, n, false), p.zin = dev(s->zin, n, false);
  // every output vector the caller names is staged and written back, stored by the mode or not: a store that should
  // not be there shows
  p.res = dev(s->res, n, true), p.d = dev(s->d, n, true), p.z = dev(s->z, n, true), p.zout = dev(s->zout, n, true);
  p.y = dy;
  uint8_t *mask = nullptr;
  if (rc == ALFD_OK && hipMalloc((void **)&mask, (size_t)npad) != hipSuccess) rc = ALFD_E_HIP;
  if (rc == ALFD_OK) {
    hipMemsetAsync(mask, 0, (size_t)npad, ctx->stream);
    if (Ct.n_list > 0)
      hipLaunchKernelGGL(mark_rows_kernel, dim3((unsigned)((Ct.n_list + 255) / 256)), dim3(256), 0, ctx->stream, Ct.n_list,
                         Ct.sparse ? Ct.rows : (const int32_t *)nullptr, mask);
    F.mask = mask;
    if (!plain_form(ctx, Ct))
      rc = (ctx->err = "alfd_spmv_tail_step: Ct is not resident as plain CSR rows", ALFD_E_UNSUPPORTED);
  }
  if (rc == ALFD_OK) {
    if (form == 0) {   // (a): the A launch with the block-end epilogue, then the rows party of the tail
      rc = launch_vs_tail(ctx, F, dx, dy, mode, p, 0.0);
      if (rc == ALFD_OK) rc = aug_tail(ctx, F, mode, p, 0.0, true);
    } else {           // (b): y = A x (with C: the solver's pair launch or its two launches), then the whole tail
      rc = Cm ? spmv_AC(ctx, A, F.clsA, *Cm, F.w, dx, dy, F.tlam) : spmv_m(ctx, A, F.clsA, dx, dy, 0);
      if (rc == ALFD_OK) rc = aug_tail(ctx, F, mode, p, 0.0);
    }
  }
  if (rc == ALFD_OK) {
    for (const Img &g : img)
      if (g.out) hipMemcpyAsync(const_cast<double *>(g.h), g.d, g.len * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) rc = ALFD_E_HIP;
  } else {
    hipStreamSynchronize(ctx->stream);
  }
  for (const Img &g : img) hipFree(g.d);
  hipFree(mask);
  csr_free(Ct);
  return rc;
}

int alfd_inner_prec_apply(alfd_ctx_t ctx, int op, const double *r, double *z) {
  CHECK_CTX();
  CHECK_SETUP();
  if (!r || !z) return ALFD_E_INVALID;
  const int v = ctx->cfg.variant;
  int kind = -1;
  if (op == ALFD_INNER_OP_AUG &&
      (v == ALFD_AL2 || v == ALFD_AL_STOKES || v == ALFD_AL_STOKES_DIAG || v == ALFD_AL_ELL_MODIFIED))
    kind = OP_AUG;
  else if (op == ALFD_INNER_OP_A22 && v == ALFD_AL_ELL_MODIFIED)
    kind = OP_A22;
  else if (op == ALFD_INNER_OP_AUG2 && v == ALFD_AL_ELL_IDEAL)
    kind = OP_AUG2;
  if (kind < 0)
    return ctx->err = "alfd_inner_prec_apply: the configured variant has no such inner operator", ALFD_E_INVALID;
  // the blocks the operator spans, at their places in the staging vectors of the depth-1 calls
  const int b0 = kind == OP_A22 ? 1 : 0, b1 = kind == OP_AUG2 ? 1 : b0;
  const int64_t npad = op_npad(ctx, kind);
  double *dr = ctx->st_in + ctx->off[b0], *dz = ctx->st_out + ctx->off[b0];
  HIPC(hipMemsetAsync(ctx->st_in, 0, ctx->ntot() * sizeof(double), ctx->stream));
  HIPC(hipMemsetAsync(ctx->st_out, 0, ctx->ntot() * sizeof(double), ctx->stream));
  int64_t at = 0;
  for (int b = b0; b <= b1; ++b) {
    HIPC(hipMemcpyAsync(ctx->st_in + ctx->off[b], r + at, ctx->n[b] * sizeof(double), hipMemcpyHostToDevice,
                        ctx->stream));
    at += ctx->n[b];
  }
  // the dispatch of pcg(): what the inner CG of this operator calls once per iteration
  const int prec = ctx->cfg.inner_prec;
  if (prec == ALFD_PREC_IDENTITY) {
    HIPC(hipMemcpyAsync(dz, dr, npad * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  } else if (prec == ALFD_PREC_JACOBI) {
    VEC_LAUNCH(jacobi_dot_kernel, npad, 24, op_dinv(ctx, kind), dr, dz, ctx->partial);
    HIPC(hipGetLastError());
  } else if (prec == ALFD_PREC_MULTILEVEL && ml_covers(ctx, kind)) {
    RC(ml_prec(ctx, kind, dr, dz));
  } else {
    RC(cheb_apply(ctx, kind, dr, dz, npad));
  }
  at = 0;
  for (int b = b0; b <= b1; ++b) {
    HIPC(hipMemcpyAsync(z + at, ctx->st_out + ctx->off[b], ctx->n[b] * sizeof(double), hipMemcpyDeviceToHost,
                        ctx->stream));
    at += ctx->n[b];
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  return ALFD_OK;
}

int alfd_dot(alfd_ctx_t ctx, int64_t n, const double *x, const double *y, double *result) {
  CHECK_CTX();
  if (n < 0 || !x || !y || !result) return ALFD_E_INVALID;
  const int64_t npad = pad_chunk(std::max<int64_t>(n, 1));
  double *dx = nullptr, *dy = nullptr, *part = nullptr, *sc = nullptr;
  HIPC(hipMalloc((void **)&dx, npad * sizeof(double)));
  HIPC(hipMalloc((void **)&dy, npad * sizeof(double)));
  HIPC(hipMalloc((void **)&part, (npad / kChunk) * sizeof(double)));
  HIPC(hipMalloc((void **)&sc, kNumScalars * sizeof(double)));
  HIPC(hipMemsetAsync(dx, 0, npad * sizeof(double), ctx->stream));
  HIPC(hipMemsetAsync(dy, 0, npad * sizeof(double), ctx->stream));
  HIPC(hipMemcpyAsync(dx, x, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(dy, y, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(dot_partial_kernel, dim3((unsigned)(npad / kChunk)), dim3(kBlock), 0, ctx->stream, dx,
                     dy, part);
  hipLaunchKernelGGL(dot_final_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, part, npad / kChunk,
                     (int64_t)0, sc, (int)S_TMP, (int)FIN_STORE);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(result, sc + S_TMP, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  hipFree(dx);
  hipFree(dy);
  hipFree(part);
  hipFree(sc);
  return ALFD_OK;
}

int alfd_host_halo_plan(int64_t nnz, const int32_t *col, const int64_t *col_offsets, int nranks, int rank,
                        int32_t *col_local, int32_t *halo_globals, int64_t halo_capacity, int64_t *n_halo,
                        int64_t *recv_off) {
  if (nnz < 0 || nranks < 1 || rank < 0 || rank >= nranks || !col_offsets || !col_local || !n_halo || !recv_off ||
      (nnz > 0 && !col))
    return ALFD_E_INVALID;
  std::vector<int32_t> hal;
  host_halo_plan(nnz, col, col_offsets, nranks, rank, col_local, hal, recv_off);
  *n_halo = (int64_t)hal.size();
  if (halo_globals) {
    if ((int64_t)hal.size() > halo_capacity) return ALFD_E_INVALID;
    std::copy(hal.begin(), hal.end(), halo_globals);
  }
  return ALFD_OK;
}

int alfd_matrix_lanes(alfd_ctx_t ctx, int slot, int32_t *lanes) {
  if (!ctx || slot < 0 || slot >= ALFD_NSLOTS || !lanes || !ctx->mat[slot].present) return ALFD_E_INVALID;
  *lanes = ctx->mat[slot].L;
  return ALFD_OK;
}

int alfd_bench_spmv(alfd_ctx_t ctx, int slot, int32_t reps, double *ms_per_launch, double *bytes) {
  CHECK_CTX();
  if (slot < 0 || slot >= ALFD_NSLOTS || !ctx->mat[slot].present || reps < 1) return ALFD_E_INVALID;
  if (ctx->nranks > 1) return ALFD_E_UNSUPPORTED;
  const DevCsr &m = ctx->mat[slot];
  double *dx = nullptr, *dy = nullptr;
  HIPC(hipMalloc((void **)&dx, std::max<int64_t>(m.ncols, 1) * sizeof(double)));
  HIPC(hipMalloc((void **)&dy, std::max<int64_t>(m.nrows, 1) * sizeof(double)));
  hipLaunchKernelGGL(hash_vector_kernel, dim3((unsigned)std::max<int64_t>(1, (m.ncols + 255) / 256)), dim3(256), 0, ctx->stream,
                     m.ncols, (int64_t)0, dx);
  const int was = ctx->timing;
  ctx->timing = 0;
  for (int i = 0; i < 2; ++i) RC(spmv(ctx, slot, dx, dy, 0));
  hipEvent_t a, b;
  HIPC(hipEventCreate(&a));
  HIPC(hipEventCreate(&b));
  HIPC(hipEventRecord(a, ctx->stream));
  for (int i = 0; i < reps; ++i) RC(spmv(ctx, slot, dx, dy, 0));
  HIPC(hipEventRecord(b, ctx->stream));
  HIPC(hipEventSynchronize(b));
  float ms = 0;
  HIPC(hipEventElapsedTime(&ms, a, b));
  ctx->timing = was;
  hipEventDestroy(a);
  hipEventDestroy(b);
  hipFree(dx);
  hipFree(dy);
  if (ms_per_launch) *ms_per_launch = (double)ms / reps;
  if (bytes) *bytes = m.algorithmic_bytes();
  return ALFD_OK;
}

int alfd_bench_spmv_format(alfd_ctx_t ctx, int slot, int32_t reps, int use_value_index, double *ms_per_launch,
                           double *streamed_bytes) {
  CHECK_CTX();
  if (slot < 0 || slot >= ALFD_NSLOTS || !ctx->mat[slot].present) return ALFD_E_INVALID;
  const bool was_off = ctx->vi_off;
  if (!use_value_index) RC(ensure_window_plan(ctx, ctx->mat[slot]));
  ctx->vi_off = !use_value_index;
  const int rc = alfd_bench_spmv(ctx, slot, reps, ms_per_launch, nullptr);
  ctx->vi_off = was_off;
  if (streamed_bytes) *streamed_bytes = ctx->mat[slot].streamed_bytes(use_value_index != 0, ctx->vs_enable != 0);
  return rc;
}

int alfd_set_preconditioner_values(alfd_ctx_t ctx, int kind) {
  CHECK_CTX();
  if (kind != ALFD_PREC_VALUES_FP64 && kind != ALFD_PREC_VALUES_FP32)
    return ctx->err = "alfd_set_preconditioner_values: unknown kind", ALFD_E_INVALID;
  if (kind == ctx->prec_values) return ALFD_OK;   // nothing changes: the setup stays
  ctx->prec_values = kind;
  ctx->is_setup = false;   // as alfd_configure; alfd_setup_coupling answers "needs alfd_setup"
  ctx->needs_full = "the value type of the preconditioner (alfd_set_preconditioner_values) was set";
  HIPC(hipStreamSynchronize(ctx->stream));
  return a32_sync(ctx);
}

int alfd_get_preconditioner_values(alfd_ctx_t ctx, alfd_prec_values_info *out) {
  if (!ctx || !out) return ALFD_E_INVALID;
  const DevCsr &m = ctx->mat[ALFD_A];
  std::memset(out, 0, sizeof(*out));
  out->requested = ctx->prec_values == ALFD_PREC_VALUES_FP32 ? 1 : 0;
  out->stored = m.val32 ? 1 : 0;
  out->used = m.val32 && ctx->is_setup && ctx->a32_used ? 1 : 0;
  if (m.val32) {
    out->reason = out->used ? ALFD_PREC_VALUES_NONE : ALFD_PREC_VALUES_NOT_APPLIED;
    out->family = a32_family(ctx, m);
    out->flushed_to_zero = m.val32_flushed;
    out->copy_bytes = std::max<int64_t>(m.nnz, 1) * (int64_t)sizeof(float);
    out->streamed_bytes_fp32 = m.streamed_bytes32();
  } else {
    const int form = a32_form_reason(ctx);   // an entry out of range is all that the form cannot tell
    out->reason = form == ALFD_PREC_VALUES_NONE ? ctx->a32_reason : form;
  }
  if (m.present) {
    out->nnz = m.nnz;
    out->streamed_bytes_fp64 = m.streamed_bytes(!ctx->vi_off, ctx->vs_enable != 0 && !ctx->vi_off);
  }
  return ALFD_OK;
}

int alfd_spmv_preconditioner(alfd_ctx_t ctx, const double *x, double *y, int mode, double alpha) {
  CHECK_CTX();
  if (!x || !y || (mode != 0 && mode != 1)) return ALFD_E_INVALID;
  DevCsr &m = ctx->mat[ALFD_A];
  if (!m.val32)
    return ctx->err = "alfd_spmv_preconditioner: slot A holds no single-precision copy (alfd_get_preconditioner_values)",
           ALFD_E_UNSUPPORTED;
  double *dx = nullptr, *dy = nullptr;
  HIPC(hipMalloc((void **)&dx, std::max<int64_t>(m.ncols, 1) * sizeof(double)));
  HIPC(hipMalloc((void **)&dy, std::max<int64_t>(m.nrows, 1) * sizeof(double)));
  HIPC(hipMemcpyAsync(dx, x, m.ncols * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(dy, y, m.nrows * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  int rc;
  {
    const A32Scope a32(ctx, true);
    rc = spmv(ctx, ALFD_A, dx, dy, mode, alpha);
  }
  if (rc == ALFD_OK) {
    HIPC(hipMemcpyAsync(y, dy, m.nrows * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
  }
  hipFree(dx);
  hipFree(dy);
  return rc;
}

int alfd_bench_spmv_preconditioner(alfd_ctx_t ctx, int32_t reps, double *ms_per_launch, double *streamed_bytes) {
  CHECK_CTX();
  if (reps < 1) return ALFD_E_INVALID;
  if (!ctx->mat[ALFD_A].val32)
    return ctx->err = "alfd_bench_spmv_preconditioner: slot A holds no single-precision copy", ALFD_E_UNSUPPORTED;
  int rc;
  {
    const A32Scope a32(ctx, true);
    rc = alfd_bench_spmv(ctx, ALFD_A, reps, ms_per_launch, nullptr);
  }
  if (streamed_bytes) *streamed_bytes = ctx->mat[ALFD_A].streamed_bytes32();
  return rc;
}

int alfd_host_window_plan(int64_t nrows, const int64_t *rp, const int32_t *col, const double *val, int32_t lanes,
                          int32_t want_value_index, alfd_window_plan_info *out) {
  if (nrows < 0 || !rp || !out || (rp[nrows] > 0 && (!col || !val))) return ALFD_E_INVALID;
  if (lanes != 4 && lanes != 8 && lanes != 16 && lanes != 32 && lanes != 64) return ALFD_E_INVALID;
  WindowParams wp;
  wp.want_vi = want_value_index != 0;
  WindowPlan pl;
  plan_window(nrows, lanes, rp, col, val, wp, pl);
  std::memset(out, 0, sizeof(*out));
  out->windowed = pl.win;
  out->value_indexed = pl.vi;
  out->row_block = pl.RB;
  out->max_window = pl.maxW;
  out->blocks = pl.nb;
  out->fallback_blocks = pl.fallback;
  out->segments = (int64_t)pl.seg_col.size();
  out->value_indexed_blocks = pl.vi ? pl.vi_blocks : 0;
  out->value_indexed_nnz = pl.vi ? pl.vi_nnz : 0;
  out->value_wide_nnz = pl.vi ? pl.wide_nnz : 0;
  out->dictionary_entries = pl.vi ? (int64_t)pl.dict.size() : 0;
  if (!pl.win) return ALFD_OK;
  // decode the plan back and compare with the CSR it was made from
  int64_t bad = 0, batches = 0;
  std::vector<int32_t> wcol;
  std::vector<int> seen;
  for (int64_t b = 0; b < pl.nb; ++b) {
    const int64_t r0 = b * pl.RB, r1 = std::min<int64_t>(r0 + pl.RB, nrows);
    const int64_t k0 = rp[r0], k1 = rp[r1];
    const int32_t W = pl.blkW[b];
    if (W >= 0) {
      wcol.assign(W, -1);
      for (int32_t sg = pl.seg_begin[b]; sg < pl.seg_begin[b + 1]; ++sg) {
        const int32_t end = (sg + 1 < pl.seg_begin[b + 1]) ? pl.seg_off[sg + 1] : W;
        for (int32_t o = pl.seg_off[sg]; o < end; ++o) wcol[o] = pl.seg_col[sg] + (o - pl.seg_off[sg]);
      }
      for (int64_t k = k0; k < k1; ++k) bad += pl.lcol[k] >= W || wcol[pl.lcol[k]] != col[k];
    }
    if (pl.vi && W >= 0 && pl.blk_dn[b] >= 0) {
      const bool wide = (pl.blk_dn[b] & kDictWide) != 0;
      const int32_t nd = pl.blk_dn[b] & 0xffff;
      for (int64_t k = k0; k < k1; ++k) {
        const int32_t code = wide ? (int32_t)pl.vidw[k] : (int32_t)pl.vidx[k];
        if (code >= nd || std::memcmp(&pl.dict[pl.doff[b] + code], &val[k], 8) != 0) ++bad;
      }
    }
    if (pl.stride > 0) {
      seen.assign(r1 - r0, 0);
      batches += pl.cnt[b];
      for (int32_t q = 0; q < pl.cnt[b]; ++q) {
        const uint64_t *dsc = &pl.tab[((size_t)b * pl.stride + q) * 4];
        const int cls = (int)(dsc[0] >> 56);
        for (int i = 0; i < 4; ++i) {
          const int id = (int)((dsc[i] >> 48) & 0xff);
          const int64_t ks = (int64_t)(dsc[i] & 0xffffffffull), len = (int64_t)((dsc[i] >> 32) & 0xffff);
          if ((int)(dsc[i] >> 56) != cls) ++bad;
          if (id == 0xff) {  // filler repeats the batch's first row
            bad += ks != (int64_t)(dsc[0] & 0xffffffffull) || i == 0;
            continue;
          }
          if (id >= r1 - r0) {
            ++bad;
            continue;
          }
          ++seen[id];
          const int64_t rl = rp[r0 + id + 1] - rp[r0 + id];
          const int64_t want_cls = std::min<int64_t>((rl + 63) / 64, kVibMaxClass + 1);
          bad += ks != rp[r0 + id] - k0 || len != rl || cls != want_cls;
        }
      }
      for (int v : seen) bad += v != 1;
    }
  }
  out->batches = batches;
  out->decode_mismatches = bad;
  return ALFD_OK;
}

static void shape_of(const alfd_ctx *ctx, const DevCsr &m, alfd_batch_major_shape *out) {
  std::memset(out, 0, sizeof(*out));
  const bool on = m.vs.on && ctx->vs_enable, lng = on && m.vs.L == 64;
  out->batch_major = on ? (m.vs.bricks ? 2 : 1) : 0;
  out->lanes = m.L;
  out->nrows = m.nrows;
  out->nnz = m.nnz;
  out->shared_nnz = m.vs.on ? m.vs.shared_nnz : 0;
  out->rows = lng ? m.vs.RB : 0;
  out->waves = lng ? (m.tag == 1 && m.vs.NW > 4 ? 4 : m.vs.NW) : 0;
  out->small = lng && m.vs.small ? 1 : 0;
  out->blocks = m.vs.on ? m.vs.nb : 0;
  out->batches = m.vs.on ? m.vs.nbatch : 0;
  out->compute_units = ctx->vs_cus;
  out->lds_bytes = lng ? (int64_t)(m.vs.wide ? VsFmt<1>::kWinOff : VsFmt<0>::kWinOff) + 8 * (int64_t)m.vs.maxW : 0;
}

int alfd_get_matrix_shape(alfd_ctx_t ctx, int slot, alfd_batch_major_shape *out) {
  CHECK_CTX();
  if (slot < 0 || slot >= ALFD_NSLOTS || !ctx->mat[slot].present || !out) return ALFD_E_INVALID;
  shape_of(ctx, ctx->mat[slot], out);
  return ALFD_OK;
}

int alfd_get_side_rows(alfd_ctx_t ctx, int slot, alfd_side_rows_info *out) {
  CHECK_CTX();
  if (slot < 0 || slot >= ALFD_NSLOTS || !ctx->mat[slot].present || !out) return ALFD_E_INVALID;
  const DevCsr::Vs &v = ctx->mat[slot].vs;
  std::memset(out, 0, sizeof(*out));
  if (!(v.on && ctx->vs_enable) || v.side_n == 0) return ALFD_OK;
  out->rows = v.side_n, out->nnz = v.side_nnz, out->longest = v.side_longest;
  out->interior_rows = v.side_interior, out->grid = side_grid(v.side_n);
  return ALFD_OK;
}

// the operators the library builds for itself (alfd_operator): null when the context has none such
static DevCsr *own_operator(alfd_ctx *ctx, int op, int level) {
  DevCsr *m = nullptr;
  if (op == ALFD_OPERATOR_LEVEL) {
    std::vector<MlLevel> &ml = ctx->hier[0].ml;
    if (level < 1 || level >= (int)ml.size()) return nullptr;
    m = ml[level].rep.A.present ? &ml[level].rep.A : &ml[level].loc.A;
  } else if (op == ALFD_OPERATOR_PATCH_SS || op == ALFD_OPERATOR_PATCH_S) {
    if (!ctx->patch.on) return nullptr;
    m = op == ALFD_OPERATOR_PATCH_SS ? &ctx->patch.Ass : &ctx->patch.As;
  }
  return m && m->present ? m : nullptr;
}

int alfd_get_operator_shape(alfd_ctx_t ctx, int op, int level, alfd_batch_major_shape *out) {
  CHECK_CTX();
  CHECK_SETUP();
  const DevCsr *m = own_operator(ctx, op, level);
  if (!m || !out) return ALFD_E_INVALID;
  shape_of(ctx, *m, out);
  return ALFD_OK;
}

int alfd_host_small_shape(int64_t nrows, int64_t blocks, int64_t batches, int32_t rows, int32_t waves, int32_t compute_units,
                          int32_t *rows_out, int32_t *waves_out) {
  if (!rows_out || !waves_out || rows < 4 || rows > kVsMaxRows || waves < 1 || compute_units < 1) return ALFD_E_INVALID;
  int r = rows, w = waves;
  vs_small_shape(nrows, blocks, batches, rows, waves, compute_units, &r, &w);
  *rows_out = r;
  *waves_out = w;
  return ALFD_OK;
}

int alfd_bench_operator(alfd_ctx_t ctx, int op, int level, int32_t rows, int32_t waves, int32_t reps, double *us_per_launch,
                        alfd_batch_major_shape *info) {
  CHECK_CTX();
  CHECK_SETUP();
  if (ctx->nranks > 1) return ALFD_E_UNSUPPORTED;
  DevCsr *own = own_operator(ctx, op, level);
  if (!own || reps < 1) return ALFD_E_INVALID;
  if (rows != 0 && (rows < 4 || rows > kVsMaxRows || (waves != 1 && waves != 2 && waves != 4))) return ALFD_E_INVALID;
  if (!own->vs.on || own->vs.L != 64 || own->sparse) return ctx->err = "not a long-row batch-major operator", ALFD_E_UNSUPPORTED;
  DevCsr tmp;
  struct Guard {
    DevCsr &t;
    ~Guard() { csr_free(t); }
  } guard{tmp};
  const DevCsr *m = own;
  if (rows != 0) {   // the same operator planned once more at the given shape, beside the one the solver keeps
    HostCsr h;
    RC(download_csr(ctx, *own, h));
    tmp.nrows = tmp.n_list = own->nrows, tmp.ncols = own->ncols, tmp.nnz = own->nnz;
    tmp.L = 64, tmp.tag = own->tag, tmp.n_local_cols = own->n_local_cols, tmp.rep = own->rep;
    ctx->vs_force_RB = rows, ctx->vs_force_NW = waves;
    const int rc = build_vs(ctx, tmp, kScratchSlot, h.rp.data(), h.col.data(), h.val.data());
    ctx->vs_force_RB = ctx->vs_force_NW = 0;
    RC(rc);
    if (!tmp.vs.on) return ctx->err = "the operator does not take the batch-major form at this shape", ALFD_E_UNSUPPORTED;
    tmp.present = true;
    m = &tmp;
  }
  double *dx = nullptr, *dy = nullptr;
  HIPC(hipMalloc((void **)&dx, std::max<int64_t>(m->ncols, 1) * sizeof(double)));
  HIPC(hipMalloc((void **)&dy, std::max<int64_t>(m->nrows, 1) * sizeof(double)));
  hipLaunchKernelGGL(hash_vector_kernel, dim3((unsigned)std::max<int64_t>(1, (m->ncols + 255) / 256)), dim3(256), 0, ctx->stream,
                     m->ncols, (int64_t)0, dx);
  hipEvent_t a = nullptr, b = nullptr;
  float ms = 0;
  bool ok = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess;
  ok = ok && launch_vs(ctx, *m, dx, dy, 0, 0.0, nullptr, nullptr);   // warm-up
  ok = ok && hipEventRecord(a, ctx->stream) == hipSuccess;
  for (int i = 0; ok && i < reps; ++i) ok = launch_vs(ctx, *m, dx, dy, 0, 0.0, nullptr, nullptr);
  ok = ok && hipEventRecord(b, ctx->stream) == hipSuccess && hipEventSynchronize(b) == hipSuccess &&
       hipEventElapsedTime(&ms, a, b) == hipSuccess;
  hipStreamSynchronize(ctx->stream);
  if (a) hipEventDestroy(a);
  if (b) hipEventDestroy(b);
  hipFree(dx);
  hipFree(dy);
  HIPC(hipGetLastError());
  if (!ok) return ctx->err = "alfd_bench_operator: launch or timing failed", ALFD_E_HIP;
  if (us_per_launch) *us_per_launch = 1000.0 * (double)ms / reps;
  if (info) shape_of(ctx, *m, info);
  return ALFD_OK;
}

int alfd_get_last_spmv_launch(alfd_ctx_t ctx, alfd_spmv_launch *out) {
  if (!ctx || !out) return ALFD_E_INVALID;   // host state only: no device call
  if (!ctx->has_last_spmv) return ctx->err = "alfd_get_last_spmv_launch: no SpMV launched yet", ALFD_E_NOT_SETUP;
  *out = ctx->last_spmv;
  return ALFD_OK;
}

int alfd_get_matrix_info(alfd_ctx_t ctx, int slot, alfd_matrix_info *out) {
  CHECK_CTX();
  if (slot < 0 || slot >= ALFD_NSLOTS || !ctx->mat[slot].present || !out) return ALFD_E_INVALID;
  const DevCsr &m = ctx->mat[slot];
  std::memset(out, 0, sizeof(*out));
  out->lanes = m.L;
  out->windowed = (m.win || m.win_deferred) ? 1 : 0;
  out->value_indexed = (m.vi || (m.vs.on && ctx->vs_enable)) ? 1 : 0;
  out->batch_major = (m.vs.on && ctx->vs_enable) ? (m.vs.bricks ? 2 : 1) : 0;
  out->nnz = m.nnz;
  out->window_blocks = m.win_nblocks;
  out->window_fallback_blocks = m.win_fallback_blocks;
  out->value_indexed_blocks = m.vi_blocks;
  out->value_indexed_nnz = m.vs.on && ctx->vs_enable ? m.nnz : m.vi_nnz;   // every entry of a batch-major matrix is dictionary-coded
  out->dictionary_entries = m.vi_dict_total;
  out->value_wide_nnz = m.vi_wide_nnz;
  out->algorithmic_bytes = m.algorithmic_bytes();
  out->streamed_bytes = m.streamed_bytes(true, ctx->vs_enable != 0);
  out->shared_nnz = m.vs.on ? m.vs.shared_nnz : 0;
  out->batch_major_blocks = m.vs.on ? m.vs.nb : 0;
  out->batch_major_wide = m.vs.on ? m.vs.wide : 0;
  out->batch_major_interior_blocks = (m.vs.on && m.vs.L == 64 && ctx->nranks > 1 && !m.rep) ? m.vs.nb_interior : 0;
  return ALFD_OK;
}

// Recursive coordinate bisection of the rows' support points: leaves of at most max_rows rows, cut at the
// median of the axis with the largest (weighted) extent.  The axis along which consecutive rows mostly
// advance -- the fast axis of the numbering -- counts half, so that bricks come out about twice as long
// there: the x window of a block is staged in runs of consecutive columns.
namespace {
struct Rcb {
  int dim;
  const double *xyz;
  int64_t max_rows;
  double weight[3];
  std::vector<int32_t> idx;
  std::vector<std::vector<int64_t>> leaves;   // leaf sizes per top-level task, in order
  void split(int64_t a, int64_t e, std::vector<int64_t> &out) {
    if (e - a <= max_rows) {
      if (e > a) out.push_back(e - a);
      return;
    }
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int64_t i = a; i < e; ++i)
      for (int d = 0; d < dim; ++d) {
        const double c = xyz[(int64_t)idx[i] * dim + d];
        lo[d] = std::min(lo[d], c);
        hi[d] = std::max(hi[d], c);
      }
    int ax = 0;
    for (int d = 1; d < dim; ++d)
      if ((hi[d] - lo[d]) * weight[d] > (hi[ax] - lo[ax]) * weight[ax]) ax = d;
    const int64_t mid = cut(a, e, ax);
    split(a, mid, out);
    split(mid, e, out);
  }
  // Cut [a, e) along axis ax at a coordinate PLANE near the median: every point below the plane goes left, so
  // that leaves are whole boxes of the mesh (their x windows are regular, which is what lets translate rows
  // share a template).  Returns the split position.
  int64_t cut(int64_t a, int64_t e, int ax) {
    const int64_t mid = a + (e - a) / 2;
    auto less = [&](int32_t p, int32_t q) {
      const double cp = xyz[(int64_t)p * dim + ax], cq = xyz[(int64_t)q * dim + ax];
      return cp < cq || (cp == cq && p < q);
    };
    std::nth_element(idx.begin() + a, idx.begin() + mid, idx.begin() + e, less);
    const double cm = xyz[(int64_t)idx[mid] * dim + ax];
    // points with coordinate == cm sit on both sides of mid: move the boundary to the nearer end of that plane
    auto lo = std::partition(idx.begin() + a, idx.begin() + mid, [&](int32_t p) { return xyz[(int64_t)p * dim + ax] < cm; });
    auto hi = std::partition(idx.begin() + mid, idx.begin() + e, [&](int32_t p) { return xyz[(int64_t)p * dim + ax] <= cm; });
    const int64_t l = lo - idx.begin(), h = hi - idx.begin();   // [l, h) = the plane cm
    int64_t pos = (mid - l <= h - mid) ? l : h;
    if (pos == a) pos = h;
    if (pos == e) pos = l;
    if (pos == a || pos == e) pos = mid;   // a single plane (cannot happen: ax has a positive extent)
    return pos;
  }
};
}  // namespace

int alfd_host_row_blocks_from_points(int64_t nrows, int32_t dim, const double *points, int32_t max_rows,
                                     int64_t *n_blocks_out, int64_t *block_ptr_out, int32_t *rows_out) {
  if (nrows < 0 || dim < 1 || dim > 3 || !points || max_rows < 1 || max_rows > kVsMaxRows || !n_blocks_out ||
      !block_ptr_out || !rows_out || nrows > 2147483000LL)
    return ALFD_E_INVALID;
  Rcb r;
  r.dim = dim;
  r.xyz = points;
  r.max_rows = max_rows;
  r.idx.resize(nrows);
  for (int64_t i = 0; i < nrows; ++i) r.idx[i] = (int32_t)i;
  // fast axis of the numbering: the axis along which consecutive rows most often differ
  int64_t moves[3] = {0, 0, 0};
  for (int64_t i = 0; i + 1 < nrows; i += std::max<int64_t>(1, nrows / 100000)) {
    int best = -1;
    double bd = 0;
    for (int d = 0; d < dim; ++d) {
      const double dd = std::fabs(points[(i + 1) * dim + d] - points[i * dim + d]);
      if (dd > bd) bd = dd, best = d;
    }
    if (best >= 0) ++moves[best];
  }
  int fast = 0;
  for (int d = 1; d < dim; ++d)
    if (moves[d] > moves[fast]) fast = d;
  for (int d = 0; d < 3; ++d) r.weight[d] = d == fast ? 0.5 : 1.0;
  // top levels sequentially into 2^k tasks, the tasks in parallel
  std::vector<std::pair<int64_t, int64_t>> tasks(1, {0, nrows});
  const int T = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  while ((int)tasks.size() < T && nrows > (int64_t)max_rows * 64) {
    std::vector<std::pair<int64_t, int64_t>> next;
    for (auto [a, e] : tasks) {
      if (e - a <= max_rows) {
        next.push_back({a, e});
        continue;
      }
      double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
      for (int64_t i = a; i < e; ++i)
        for (int d = 0; d < dim; ++d) {
          const double c = points[(int64_t)r.idx[i] * dim + d];
          lo[d] = std::min(lo[d], c);
          hi[d] = std::max(hi[d], c);
        }
      int ax = 0;
      for (int d = 1; d < dim; ++d)
        if ((hi[d] - lo[d]) * r.weight[d] > (hi[ax] - lo[ax]) * r.weight[ax]) ax = d;
      const int64_t mid = r.cut(a, e, ax);
      next.push_back({a, mid});
      next.push_back({mid, e});
    }
    tasks.swap(next);
  }
  r.leaves.assign(tasks.size(), {});
  {
    std::vector<std::thread> th;
    std::atomic<size_t> nextTask(0);
    for (int t = 0; t < T; ++t)
      th.emplace_back([&]() {
        for (size_t q = nextTask++; q < tasks.size(); q = nextTask++) r.split(tasks[q].first, tasks[q].second, r.leaves[q]);
      });
    for (auto &x : th) x.join();
  }
  int64_t nb = 0;
  block_ptr_out[0] = 0;
  for (auto &lv : r.leaves)
    for (int64_t sz : lv) {
      block_ptr_out[nb + 1] = block_ptr_out[nb] + sz;
      ++nb;
    }
  // rows of a block in ascending order (the order the numbering visits them)
  for (int64_t b = 0; b < nb; ++b) std::sort(r.idx.begin() + block_ptr_out[b], r.idx.begin() + block_ptr_out[b + 1]);
  std::copy(r.idx.begin(), r.idx.end(), rows_out);
  *n_blocks_out = nb;
  return ALFD_OK;
}

// the plan of alfd_host_stream_plan (side: of alfd_host_stream_plan_side), decoded back; seen: the rows the blocks list
static int host_stream_plan(int64_t nrows, const int64_t *rp, const int32_t *col, const double *val, int32_t row_block,
                            int64_t n_blocks, const int64_t *block_ptr, const int32_t *rows, bool side, VsPlan &pl,
                            std::vector<uint8_t> &seen, alfd_stream_plan_info *out) {
  if (!rp || !out || nrows < 0 || row_block < 1 || row_block > kVsMaxRows) return ALFD_E_INVALID;
  std::memset(out, 0, sizeof(*out));
  if (n_blocks > 0) plan_vs(nrows, rp, col, val, row_block, 4096, 8, n_blocks, block_ptr, rows, pl, true, 0, -1, side);
  else plan_vs(nrows, rp, col, val, row_block, 4096, 8, 0, nullptr, nullptr, pl, true, 0, -1, side);
  if (!pl.ok || pl.dict_split) {   // as build_vs: wide codes when the 512-value limit halved blocks
    VsPlan pw;
    if (n_blocks > 0) plan_vs(nrows, rp, col, val, row_block, 4096, 8, n_blocks, block_ptr, rows, pw, true, 1, -1, side);
    else plan_vs(nrows, rp, col, val, row_block, 4096, 8, 0, nullptr, nullptr, pw, true, 1, -1, side);
    if (pw.ok && (!pl.ok || pw.stream.size() + 128 * (size_t)pw.nbatch < pl.stream.size() + 128 * (size_t)pl.nbatch)) pl = std::move(pw);
  }
  const int code_shift = pl.wide ? VsFmt<1>::kCodeShift : VsFmt<0>::kCodeShift;
  out->ok = pl.ok ? 1 : 0;
  if (!pl.ok) return ALFD_OK;
  out->max_window = pl.maxW;
  out->max_rows = pl.rbs;
  out->max_batches = pl.stride;
  out->blocks = pl.nb;
  out->batches = pl.nbatch;
  out->segments = (int64_t)pl.seg_col.size();
  out->dictionary_entries = (int64_t)pl.dict.size();
  out->stream_bytes = (int64_t)pl.stream.size() - 4096;
  out->shared_nnz = pl.shared_nnz;
  seen.assign(nrows, 0);
  int64_t bad = 0, covered = 0;
  std::vector<int32_t> slot_col;
  for (int64_t b = 0; b < pl.nb; ++b) {
    // window slot -> column
    slot_col.assign(pl.blkW[b], -1);
    for (int32_t s = pl.seg_begin[b]; s < pl.seg_begin[b + 1]; ++s) {
      const int32_t end = s + 1 < pl.seg_begin[b + 1] ? pl.seg_off[s + 1] : pl.blkW[b];
      for (int32_t o = pl.seg_off[s]; o < end; ++o) slot_col[o] = pl.seg_col[s] + (o - pl.seg_off[s]);
    }
    const int nbt = pl.cnt[b];
    const uint8_t *sp = pl.stream.data() + pl.sb[b];
    if (pl.sb[b] % 16) ++bad;
    for (int q = 0; q < nbt; ++q) {
      const uint64_t *dsc = &pl.tab[((size_t)b * pl.stride + q) * kVsBatchRows];
      auto off = [](uint64_t dd) { return (uint32_t)dd & 0xfffffu; };
      auto cnt_of = [](uint64_t dd) { return ((uint32_t)dd >> 20) & 0x1ffu; };
      const uint32_t eb = off(dsc[0]);
      const bool shared = (dsc[0] >> 63) != 0;
      const int cls = (int)(((uint32_t)dsc[0] >> 29) & 7u);
      const uint8_t *fb = sp + 16 * (size_t)eb;
      for (int i = 0; i < kVsBatchRows; ++i) {
        const uint32_t rfield = (uint32_t)(dsc[i] >> 32) & (i == 0 ? 0x7fffffffu : 0xffffffffu);
        if (!shared && i >= 4 && (int32_t)rfield >= 0) ++bad;   // plain batches hold 4 rows
        const int64_t r = (int32_t)rfield;
        if (r < 0) continue;  // filler
        if (r >= nrows || seen[r]) { ++bad; continue; }
        seen[r] = 1;
        ++covered;
        const uint32_t n = cnt_of(dsc[shared ? 0 : i]);        // translates share the template's count
        if ((int64_t)n != rp[r + 1] - rp[r] || (int)((n + 63) / 64) != cls) { ++bad; continue; }
        if (!shared && off(dsc[i]) != eb) { ++bad; continue; }
        const int32_t shift = (shared && i > 0) ? (int32_t)(uint32_t)dsc[i] : 0;   // bytes
        if (shift % 8) ++bad;
        for (uint32_t k = 0; k < n; ++k) {
          uint32_t f;
          if (shared) {
            std::memcpy(&f, fb + 256 * (size_t)(k / 64) + 4 * (size_t)(k % 64), 4);
          } else {
            const uint8_t *cell = fb + 768 * (size_t)(k / 64) + 12 * (size_t)(k % 64) + 3 * i;
            f = cell[0] | ((uint32_t)cell[1] << 8) | ((uint32_t)cell[2] << 16);
          }
          if ((f & 7u) || (f >> 24)) ++bad;
          const int32_t lcv = (int32_t)((f >> 3) & ((1u << (code_shift - 3)) - 1u)) + shift / 8;
          const uint32_t vcv = f >> code_shift;
          const double v = (int32_t)vcv < pl.dn[b] ? pl.dict[pl.doff[b] + vcv] : std::nan("");
          const int32_t c = (lcv >= 0 && lcv < pl.blkW[b]) ? slot_col[lcv] : -1;
          if (c != col[rp[r] + k] || std::memcmp(&v, &val[rp[r] + k], 8) != 0) ++bad;
        }
      }
    }
  }
  out->decode_mismatches = bad;
  out->rows_covered = covered;
  return ALFD_OK;
}

int alfd_host_stream_plan(int64_t nrows, const int64_t *rp, const int32_t *col, const double *val, int32_t row_block,
                          int64_t n_blocks, const int64_t *block_ptr, const int32_t *rows,
                          alfd_stream_plan_info *out) {
  VsPlan pl;
  std::vector<uint8_t> seen;
  return host_stream_plan(nrows, rp, col, val, row_block, n_blocks, block_ptr, rows, false, pl, seen, out);
}

int alfd_host_stream_plan_side(int64_t nrows, const int64_t *rp, const int32_t *col, const double *val, int32_t row_block,
                               int64_t n_blocks, const int64_t *block_ptr, const int32_t *rows, int64_t *n_side_out,
                               int32_t *side_rows_out, int64_t *side_nnz_out, alfd_stream_plan_info *out) {
  if (!n_side_out || !side_rows_out || !side_nnz_out) return ALFD_E_INVALID;
  *n_side_out = *side_nnz_out = 0;
  VsPlan pl;
  std::vector<uint8_t> seen;
  RC(host_stream_plan(nrows, rp, col, val, row_block, n_blocks, block_ptr, rows, true, pl, seen, out));
  if (!pl.ok) return ALFD_OK;
  // the side list: every row in the blocks or in the list, never in both; the compact CSR is the row, entry by entry
  int64_t bad = 0;
  const int64_t ns = (int64_t)pl.side_rows.size();
  for (int64_t i = 0; i < ns; ++i) {
    const int32_t r = pl.side_rows[i];
    side_rows_out[i] = r;
    if (r < 0 || r >= nrows || seen[r]) { ++bad; continue; }
    seen[r] = 2;
    const int64_t k0 = pl.side_rp[i], n = pl.side_rp[i + 1] - k0;
    if (n != rp[r + 1] - rp[r]) { ++bad; continue; }
    for (int64_t k = 0; k < n; ++k)
      if (pl.side_col[k0 + k] != col[rp[r] + k] || std::memcmp(&pl.side_val[k0 + k], &val[rp[r] + k], 8) != 0) ++bad;
  }
  for (int64_t r = 0; r < nrows; ++r)
    if (!seen[r]) ++bad;
  *n_side_out = ns;
  *side_nnz_out = (int64_t)pl.side_col.size();
  out->decode_mismatches += bad;
  return ALFD_OK;
}

int alfd_host_stream_plan_short(int64_t nrows, const int64_t *rp, const int32_t *col, const double *val, int32_t lanes,
                                alfd_stream_plan_info *out) {
  if (!rp || !out || nrows < 0 || (lanes != 8 && lanes != 16 && lanes != 32)) return ALFD_E_INVALID;
  std::memset(out, 0, sizeof(*out));
  VsPlan pl;
  const int L = lanes, RBb = 4 * (64 / L), W64 = 1 + RBb;
  plan_vss(nrows, L, rp, col, val, std::min(kVssMaxRows, 96 * 2 * 64 / L), 4096, 8, pl);
  out->ok = pl.ok ? 1 : 0;
  if (!pl.ok) return ALFD_OK;
  out->max_window = pl.maxW;
  out->max_rows = pl.rbs;
  out->max_batches = pl.stride;
  out->blocks = pl.nb;
  out->batches = pl.nbatch;
  out->segments = (int64_t)pl.seg_col.size();
  out->dictionary_entries = (int64_t)pl.dict.size();
  out->stream_bytes = (int64_t)pl.stream.size() - 4096 + 8 * (int64_t)W64 * pl.nbatch;
  out->shared_nnz = pl.shared_nnz;
  std::vector<uint8_t> seen(nrows, 0);
  int64_t bad = 0, covered = 0;
  std::vector<int32_t> slot_col;
  for (int64_t b = 0; b < pl.nb; ++b) {
    slot_col.assign(pl.blkW[b], -1);
    for (int32_t s = pl.seg_begin[b]; s < pl.seg_begin[b + 1]; ++s) {
      const int32_t end = s + 1 < pl.seg_begin[b + 1] ? pl.seg_off[s + 1] : pl.blkW[b];
      for (int32_t o = pl.seg_off[s]; o < end; ++o) slot_col[o] = pl.seg_col[s] + (o - pl.seg_off[s]);
    }
    const uint8_t *sp = pl.stream.data() + pl.sb[b];
    for (int q = 0; q < pl.cnt[b]; ++q) {
      const uint64_t *dsc = &pl.tab[((size_t)b * pl.stride + q) * W64];
      const uint32_t eb = (uint32_t)dsc[0] & 0xfffffu, n = ((uint32_t)dsc[0] >> 20) & 0x1ffu;
      const int cls = (int)(((uint32_t)dsc[0] >> 29) & 7u), nreal = (int)(dsc[0] >> 32);
      if ((int)((n + L - 1) / L) != cls || nreal < 1 || nreal > RBb) ++bad;
      for (int i = 0; i < RBb; ++i) {
        const int64_t r = (int32_t)(uint32_t)dsc[1 + i];
        const int32_t shift = (int32_t)(dsc[1 + i] >> 32);
        if (r < 0) {
          if (i < nreal) ++bad;
          continue;
        }
        if (i >= nreal || r >= nrows || seen[r] || (int64_t)n != rp[r + 1] - rp[r] || shift % 8) { ++bad; continue; }
        seen[r] = 1;
        ++covered;
        for (uint32_t k = 0; k < n; ++k) {
          uint32_t f;
          std::memcpy(&f, sp + 16 * (size_t)eb + 4 * (size_t)k, 4);
          if ((f & 7u) || (f >> 24)) ++bad;
          const int32_t lcv = (int32_t)((f >> 3) & 0xfffu) + shift / 8;
          const uint32_t vcv = f >> 15;
          const double v = (int32_t)vcv < pl.dn[b] ? pl.dict[pl.doff[b] + vcv] : std::nan("");
          const int32_t c = (lcv >= 0 && lcv < pl.blkW[b]) ? slot_col[lcv] : -1;
          if (c != col[rp[r] + k] || std::memcmp(&v, &val[rp[r] + k], 8) != 0) ++bad;
        }
      }
    }
  }
  out->decode_mismatches = bad;
  out->rows_covered = covered;
  return ALFD_OK;
}

int alfd_host_numbering_from_points(int64_t nrows, int32_t dim, const double *points, int64_t *new_to_old) {
  if (nrows < 0 || dim < 1 || dim > 3 || !points || !new_to_old) return ALFD_E_INVALID;
  for (int64_t i = 0; i < nrows; ++i) new_to_old[i] = i;
  std::stable_sort(new_to_old, new_to_old + nrows, [&](int64_t a, int64_t b) {
    for (int d = dim - 1; d >= 0; --d) {
      const double pa = points[a * dim + d], pb = points[b * dim + d];
      if (pa != pb) return pa < pb;
    }
    return false;
  });
  return ALFD_OK;
}

int alfd_host_brick_blocks_from_points(int64_t nrows, int32_t dim, const double *points, const int32_t *brick,
                                       int32_t max_rows, int64_t *n_blocks_out, int64_t *block_ptr_out, int32_t *rows_out) {
  if (nrows < 0 || dim < 1 || dim > 3 || !points || !brick || max_rows < 1 || max_rows > kVsMaxRows || !n_blocks_out ||
      !block_ptr_out || !rows_out || nrows > 2147483000LL)
    return ALFD_E_INVALID;
  for (int d = 0; d < dim; ++d)
    if (brick[d] < 1) return ALFD_E_INVALID;
  // grid index of a point along an axis = rank of its coordinate among the distinct coordinates of the axis
  std::vector<std::vector<int32_t>> gi(dim, std::vector<int32_t>(nrows));
  int64_t span[3] = {1, 1, 1};
  for (int d = 0; d < dim; ++d) {
    std::vector<double> u(nrows);
    for (int64_t i = 0; i < nrows; ++i) u[i] = points[i * dim + d];
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    for (int64_t i = 0; i < nrows; ++i)
      gi[d][i] = (int32_t)(std::lower_bound(u.begin(), u.end(), points[i * dim + d]) - u.begin());
    span[d] = (int64_t)u.size() / brick[d] + 1;
  }
  std::vector<std::pair<int64_t, int32_t>> key(nrows);   // (brick id, row): rows of a brick in ascending order
  for (int64_t i = 0; i < nrows; ++i) {
    int64_t k = 0;
    for (int d = dim - 1; d >= 0; --d) k = k * span[d] + gi[d][i] / brick[d];
    key[i] = {k, (int32_t)i};
  }
  std::sort(key.begin(), key.end());
  int64_t nb = 0;
  block_ptr_out[0] = 0;
  for (int64_t i = 0; i < nrows;) {
    int64_t j = i;
    while (j < nrows && key[j].first == key[i].first) ++j;
    for (int64_t a = i; a < j; a += max_rows) block_ptr_out[++nb] = std::min<int64_t>(a + max_rows, j);
    i = j;
  }
  for (int64_t i = 0; i < nrows; ++i) rows_out[i] = key[i].second;
  *n_blocks_out = nb;
  return ALFD_OK;
}

int alfd_host_permute_csr(int64_t nrows, const int64_t *rp, const int32_t *col, const double *val,
                          const int64_t *row_new_to_old, const int64_t *col_old_to_new, int64_t *orp, int32_t *ocol,
                          double *oval) {
  if (nrows < 0 || !rp || !orp || (rp[nrows] > 0 && (!col || !val || !ocol || !oval))) return ALFD_E_INVALID;
  orp[0] = 0;
  for (int64_t r = 0; r < nrows; ++r) {
    const int64_t src = row_new_to_old ? row_new_to_old[r] : r;
    if (src < 0 || src >= nrows) return ALFD_E_INVALID;
    orp[r + 1] = orp[r] + (rp[src + 1] - rp[src]);
  }
  if (orp[nrows] != rp[nrows]) return ALFD_E_INVALID;   // row_new_to_old is not a permutation
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(16u, std::max(1u, std::thread::hardware_concurrency())),
                                                           (nrows + 8191) / 8192));
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t]() {
      std::vector<std::pair<int32_t, double>> row;
      for (int64_t r = nrows * t / T; r < nrows * (t + 1) / T; ++r) {
        const int64_t src = row_new_to_old ? row_new_to_old[r] : r;
        const int64_t k0 = rp[src], len = rp[src + 1] - k0, o0 = orp[r];
        if (!col_old_to_new) {
          for (int64_t k = 0; k < len; ++k) ocol[o0 + k] = col[k0 + k], oval[o0 + k] = val[k0 + k];
          continue;
        }
        row.resize(len);
        for (int64_t k = 0; k < len; ++k) row[k] = {(int32_t)col_old_to_new[col[k0 + k]], val[k0 + k]};
        std::sort(row.begin(), row.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
        for (int64_t k = 0; k < len; ++k) ocol[o0 + k] = row[k].first, oval[o0 + k] = row[k].second;
      }
    });
  for (auto &x : th) x.join();
  return ALFD_OK;
}

int alfd_host_check_numbering(int64_t n, const int64_t *new_to_old, int64_t *old_to_new) {
  if (n < 0 || (n > 0 && !new_to_old)) return ALFD_E_INVALID;
  std::vector<bool> seen((size_t)n, false);
  for (int64_t k = 0; k < n; ++k) {
    const int64_t o = new_to_old[k];
    if (o < 0 || o >= n || seen[(size_t)o]) return ALFD_E_INVALID;
    seen[(size_t)o] = true;
  }
  if (old_to_new)
    for (int64_t k = 0; k < n; ++k) old_to_new[new_to_old[k]] = k;
  return ALFD_OK;
}

static void numbering_release(alfd_ctx *ctx) {
  alfd_ctx::Numbering &N = ctx->num;
  if (N.perm) hipFree(N.perm);
  if (N.inv) hipFree(N.inv);
  if (N.stage) hipFree(N.stage);
  N = alfd_ctx::Numbering();
}

int alfd_set_numbering(alfd_ctx_t ctx, int64_t n, const int64_t *new_to_old) {
  CHECK_CTX();
  const std::string fn = "alfd_set_numbering: ";
  if (n < 0 || (n > 0 && !new_to_old)) return ctx->err = fn + "bad arguments", ALFD_E_INVALID;
  if (n > 2147483000LL) return ctx->err = fn + "more than 2^31 rows", ALFD_E_INVALID;
  if (ctx->nranks > 1) return ctx->err = fn + "not available on a partitioned context", ALFD_E_UNSUPPORTED;
  // what was taken in under the numbering in force (or under none) would meet vectors translated by the new one
  const int slots[5] = {ALFD_A, ALFD_BT, ALFD_B, ALFD_CT, ALFD_C};
  const char *names[5] = {"A", "BT", "B", "CT", "C"};
  for (int i = 0; i < 5; ++i) {
    if (ctx->mat[slots[i]].present)
      return ctx->err = fn + "slot " + names[i] + " is already uploaded (the numbering must precede it)", ALFD_E_INVALID;
    if (slots[i] != ALFD_B && slots[i] != ALFD_C && !ctx->rb_ptr[slots[i]].empty())
      return ctx->err = fn + "a row-block hint for " + names[i] + " is already set", ALFD_E_INVALID;
  }
  if (!ctx->hier[0].P[0].rp.empty()) return ctx->err = fn + "a level-0 prolongator of block 0 is already set", ALFD_E_INVALID;
  if (!ctx->hier[0].agg[0].empty()) return ctx->err = fn + "level-0 aggregates are already set", ALFD_E_INVALID;
  if (n == 0) {
    HIPC(hipStreamSynchronize(ctx->stream));
    numbering_release(ctx);
    return ALFD_OK;
  }
  std::vector<int64_t> o2n((size_t)n);
  if (alfd_host_check_numbering(n, new_to_old, o2n.data()) != ALFD_OK)
    return ctx->err = fn + "new_to_old is not a permutation of [0, n) (entry out of range or repeated)", ALFD_E_INVALID;
  HIPC(hipStreamSynchronize(ctx->stream));
  numbering_release(ctx);
  alfd_ctx::Numbering &N = ctx->num;
  const int64_t npad = pad_chunk(n);
  std::vector<int32_t> h((size_t)npad, 0);
  int32_t **dst[2] = {&N.perm, &N.inv};
  const int64_t *src[2] = {new_to_old, o2n.data()};
  for (int a = 0; a < 2; ++a) {
    for (int64_t k = 0; k < n; ++k) h[(size_t)k] = (int32_t)src[a][k];
    if (hipMalloc((void **)dst[a], npad * sizeof(int32_t)) != hipSuccess ||
        hipMemcpy(*dst[a], h.data(), npad * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
      numbering_release(ctx);
      return ctx->err = fn + "device allocation failed", ALFD_E_HIP;
    }
  }
  if (hipMalloc((void **)&N.stage, npad * sizeof(double)) != hipSuccess) {
    numbering_release(ctx);
    return ctx->err = fn + "device allocation failed", ALFD_E_HIP;
  }
  N.n2o.assign(new_to_old, new_to_old + n);
  N.o2n.swap(o2n);
  return ALFD_OK;
}

int alfd_set_numbering_from_points(alfd_ctx_t ctx, int64_t n, int32_t dim, const double *points, const int32_t *brick) {
  CHECK_CTX();
  const std::string fn = "alfd_set_numbering_from_points: ";
  if (n < 1 || dim < 1 || dim > 3 || !points) return ctx->err = fn + "bad arguments", ALFD_E_INVALID;
  for (int64_t i = 0; i < n * dim; ++i)
    if (!std::isfinite(points[i])) return ctx->err = fn + "non-finite coordinate", ALFD_E_INVALID;
  static const int32_t default_brick[3] = {16, 4, 1};
  const int32_t *bk = brick ? brick : default_brick;
  for (int d = 0; d < dim; ++d)
    if (bk[d] < 1) return ctx->err = fn + "brick sizes must be positive", ALFD_E_INVALID;
  std::vector<int64_t> n2o((size_t)n), ptr((size_t)n + 1);
  std::vector<double> sorted((size_t)n * dim);
  std::vector<int32_t> rows((size_t)n);
  RC(alfd_host_numbering_from_points(n, dim, points, n2o.data()));
  for (int64_t k = 0; k < n; ++k)
    for (int d = 0; d < dim; ++d) sorted[(size_t)k * dim + d] = points[(size_t)n2o[k] * dim + d];
  int64_t nb = 0;
  if (alfd_host_brick_blocks_from_points(n, dim, sorted.data(), bk, 250, &nb, ptr.data(), rows.data()) != ALFD_OK)
    return ctx->err = fn + "alfd_host_brick_blocks_from_points refused the points", ALFD_E_INVALID;
  RC(alfd_set_numbering(ctx, n, n2o.data()));
  // the blocks come from the sorted points: they are in the new numbering already
  ctx->rb_ptr[ALFD_A].assign(ptr.begin(), ptr.begin() + nb + 1);
  ctx->rb_rows[ALFD_A].assign(rows.begin(), rows.end());
  ctx->needs_full = "a prolongator, aggregates or a row-block hint was set";
  return ALFD_OK;
}

int alfd_get_numbering(alfd_ctx_t ctx, int64_t *new_to_old, int64_t capacity, int64_t *n) {
  if (!ctx) return ALFD_E_INVALID;
  if (n) *n = ctx->num.n();
  if (new_to_old) {
    if (capacity < ctx->num.n()) return ALFD_E_INVALID;
    std::copy(ctx->num.n2o.begin(), ctx->num.n2o.end(), new_to_old);
  }
  return ALFD_OK;
}

int alfd_get_device_memory(alfd_ctx_t ctx, int64_t *free_bytes, int64_t *total_bytes) {
  CHECK_CTX();
  size_t f = 0, t = 0;
  HIPC(hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = (int64_t)f;
  if (total_bytes) *total_bytes = (int64_t)t;
  return ALFD_OK;
}

int alfd_set_tunable(alfd_ctx_t ctx, const char *name, int value) {
  if (!ctx || !name) return ALFD_E_INVALID;
  if (std::strcmp(name, "value_index") == 0) {
    ctx->vi_off = value == 0;
    if (value == 0) RC(ensure_window_plans(ctx));   // the general kernel needs the (deferred) window plans
    return ALFD_OK;
  }
  if (std::strcmp(name, "batch_major") == 0) {   // takes effect at the next alfd_set_matrix
    ctx->vs_enable = value != 0;
    if (value == 0) RC(ensure_window_plans(ctx));
    return ALFD_OK;
  }
  if (std::strcmp(name, "batch_major_share") == 0) {   // 0: no template-shared batches (takes effect at the next alfd_set_matrix)
    ctx->vs_share = value != 0;
    return ALFD_OK;
  }
  if (std::strcmp(name, "batch_major_wide") == 0) {   // 0: never plan 10-bit codes (at the next alfd_set_matrix)
    ctx->vs_wide = value != 0;
    return ALFD_OK;
  }
  if (std::strcmp(name, "batch_major_side_rows") == 0) {   // 1: rows beyond kVsMaxLen entries go to a side list (at the next alfd_set_matrix / alfd_setup)
    if (value != 0 && value != 1) return ctx->err = "batch_major_side_rows: 0 or 1", ALFD_E_INVALID;
    ctx->vs_side = value;
    return ALFD_OK;
  }
  if (std::strcmp(name, "batch_major_waves") == 0) {
    if (value != 1 && value != 2 && value != 4 && value != 8) return ctx->err = "batch_major_waves: 1, 2, 4 or 8", ALFD_E_INVALID;
    ctx->vs_NW = value;
    // the default of every operator whose shape the small-operator rule did not choose: the matrices of the slots follow
    // at once (level and patch operators run their own 4-wave instantiations unless that rule shaped them)
    for (int sl = 0; sl < ALFD_NSLOTS; ++sl) {
      DevCsr::Vs &v = ctx->mat[sl].vs;
      if (v.on && v.L == 64 && !v.small && !v.wide) v.NW = value;
    }
    return ALFD_OK;
  }
  if (std::strcmp(name, "batch_major_small") == 0) {   // 0: level / patch operators keep the context-wide shape (at the next alfd_set_matrix / alfd_setup)
    ctx->vs_small = value != 0;
    return ALFD_OK;
  }
  if (std::strcmp(name, "batch_major_rows") == 0) {
    if (value < 4 || value > kVsMaxRows) return ctx->err = "batch_major_rows: 4..250", ALFD_E_INVALID;
    ctx->vs_RB = value;
    return ALFD_OK;
  }
  if (std::strcmp(name, "batch_major_xcd") == 0) {
    ctx->vs_xcd = value != 0;
    return ALFD_OK;
  }
  if (std::strcmp(name, "ml_fuse") == 0) {   // 0: separate launches; 1: aug_tail; 2: + pair launches; 3: + on the fine level
    ctx->ml_fuse = std::max(0, std::min(3, value));   // as ALFD_ML_FUSE: values outside 0..3 take the nearest level
    return ALFD_OK;
  }
  if (std::strcmp(name, "short_rows_per_thread") == 0) {   // 0: spmv_kernel<L> for every 4- and 8-lane operator (same bits); at the next launch
    if (value != 0 && value != 1) return ctx->err = "short_rows_per_thread: 0 or 1", ALFD_E_INVALID;
    ctx->short_rows_per_thread = value;
    return ALFD_OK;
  }
  if (std::strcmp(name, "ml_tail_side_rows") == 0) {   // 1: "ml_tail_in_spmv" also on operators with side rows; at the next alfd_setup / alfd_setup_coupling
    if (value != 0 && value != 1) return ctx->err = "ml_tail_side_rows: 0 or 1", ALFD_E_INVALID;
    ctx->ml_tail_side_rows = value;
    return ALFD_OK;
  }
  if (std::strcmp(name, "ml_tail_in_spmv") == 0) {   // 1: the element-wise tails of the fused smoother steps at the block end of the A launch
    if (value != 0 && value != 1) return ctx->err = "ml_tail_in_spmv: 0 or 1", ALFD_E_INVALID;
    ctx->ml_tail_in_spmv = value;
    return ALFD_OK;
  }
  if (std::strcmp(name, "ml_gpu_galerkin") == 0) {   // 0: every Galerkin product of the setup / the builder on the host (next alfd_setup / build)
    if (value != 0 && value != 1) return ctx->err = "ml_gpu_galerkin: 0 or 1", ALFD_E_INVALID;
    ctx->ml_gpu_galerkin = value;
    return ALFD_OK;
  }
  if (std::strcmp(name, "ml_tail_rows") == 0) {   // 0: off; levels >= 1 of the immersed hierarchy up to this size in one launch
    if (value < 0) return ctx->err = "ml_tail_rows: >= 0", ALFD_E_INVALID;
    ctx->ml_tail_rows = value;
    return ALFD_OK;
  }
  if (std::strcmp(name, "nested_mp_group") == 0) {   // iterations of the device-stepped nested Mp CG per state read
    if (value < 1 || value > 1000) return ctx->err = "nested_mp_group: 1..1000", ALFD_E_INVALID;
    ctx->nmp_group = value;
    return ALFD_OK;
  }
  if (std::strcmp(name, "nested_mp_host_stepped") == 0) {   // 1: the host-stepped pcg() for the nested Mp CG on one rank
    ctx->nmp_host_stepped = value != 0;
    return ALFD_OK;
  }
  if (std::strcmp(name, "spectrum_group") == 0) {   // iterations of the device-stepped CG on C Ct per state read
    if (value < 1 || value > 1000) return ctx->err = "spectrum_group: 1..1000", ALFD_E_INVALID;
    ctx->spec_group = value;
    return ALFD_OK;
  }
  if (std::strcmp(name, "spectrum_host_stepped") == 0) {   // 1: alfd_estimate_spectrum through the host-stepped pcg()
    ctx->spec_host_stepped = value != 0;
    return ALFD_OK;
  }
  if (std::strcmp(name, "numbering_unpack_scatter") == 0) {   // 1: block 0 leaves through unpack_blocks_perm_scatter_kernel (same bits)
    if (value != 0 && value != 1) return ctx->err = "numbering_unpack_scatter: 0 or 1", ALFD_E_INVALID;
    ctx->num_unpack_scatter = value;
    return ALFD_OK;
  }
  return ctx->err = std::string("unknown tunable ") + name, ALFD_E_INVALID;
}

int alfd_host_tridiagonal_extremes(int32_t k, const double *alpha, const double *beta, double *lambda_min,
                                   double *lambda_max) {
  return host_tridiagonal_extremes(k, alpha, beta, lambda_min, lambda_max);
}

int alfd_estimate_spectrum(alfd_ctx_t ctx, int op, const alfd_control *ctrl, alfd_spectrum *out) {
  CHECK_CTX();
  CHECK_SETUP();
  if (!out) return ALFD_E_INVALID;
  if (op != ALFD_SPECTRUM_CCT) return ctx->err = "alfd_estimate_spectrum: unknown operator", ALFD_E_INVALID;
  if (ctx->nranks > 1) return ctx->err = "alfd_estimate_spectrum: single rank only", ALFD_E_UNSUPPORTED;
  const int64_t nl = ctx->n[ctx->nblocks - 1];
  alfd_control c;
  if (ctrl) {
    c = *ctrl;
  } else {   // SolverControl(lambda.size(), 1e-12)
    c.kind = ALFD_CTRL_ABS;
    c.max_steps = (int32_t)std::min<int64_t>(nl, INT32_MAX);
    c.tol = 1e-12;
    c.reduce = 0.0;
  }
  if (c.kind < ALFD_CTRL_ABS || c.kind > ALFD_CTRL_FIXED_ITERS || c.max_steps < 1)
    return ctx->err = "alfd_estimate_spectrum: bad control (max_steps >= 1)", ALFD_E_INVALID;
  if (nl < 1) return ctx->err = "alfd_estimate_spectrum: no multipliers", ALFD_E_INVALID;
  return estimate_spectrum(ctx, c, out);
}

int alfd_get_cg_coefficients(alfd_ctx_t ctx, double *alpha, double *beta, int32_t capacity, int32_t *count) {
  if (!ctx) return ALFD_E_INVALID;
  if (!ctx->spec.have) return ctx->err = "no spectrum estimate yet", ALFD_E_NOT_SETUP;
  const int32_t k = (int32_t)ctx->spec.alpha.size();
  if (count) *count = k;
  for (int32_t i = 0; i < capacity && i < k; ++i) {
    if (alpha) alpha[i] = ctx->spec.alpha[i];
    if (beta && i + 1 < k) beta[i] = ctx->spec.beta[i];
  }
  return ALFD_OK;
}

int alfd_constraint_residual(alfd_ctx_t ctx, const double *const *x_blocks, const double *g, double *linf) {
  CHECK_CTX();
  CHECK_SETUP();
  if (!x_blocks || !linf) return ALFD_E_INVALID;
  if (ctx->nranks > 1) return ctx->err = "alfd_constraint_residual: single rank only", ALFD_E_UNSUPPORTED;
  return constraint_residual(ctx, x_blocks, g, linf);
}

int alfd_set_row_blocks(alfd_ctx_t ctx, int slot, int64_t n_blocks, const int64_t *block_ptr, const int32_t *rows) {
  if (!ctx || slot < 0 || slot >= ALFD_NSLOTS) return ALFD_E_INVALID;
  ctx->rb_ptr[slot].clear();
  ctx->rb_rows[slot].clear();
  ctx->needs_full = "a prolongator, aggregates or a row-block hint was set";
  if (n_blocks <= 0 || !block_ptr || !rows) return ALFD_OK;   // hint removed
  // the prefix is checked before anything is copied with it (a negative, huge or non-monotone value would be
  // undefined behaviour in vector::assign); that the blocks partition the rows is checked against the matrix at upload
  if (block_ptr[0] != 0) return ctx->err = "alfd_set_row_blocks: block_ptr[0] must be 0", ALFD_E_INVALID;
  for (int64_t b = 0; b < n_blocks; ++b)
    if (block_ptr[b + 1] < block_ptr[b]) return ctx->err = "alfd_set_row_blocks: block_ptr must be monotone", ALFD_E_INVALID;
  if (block_ptr[n_blocks] > 2147483000LL) return ctx->err = "alfd_set_row_blocks: more than 2^31 rows", ALFD_E_INVALID;
  // alfd_set_numbering: the row ids of A / BT / CT are block-0 unknowns in the caller's numbering; a block keeps its order
  const bool renum = ctx->num.on() && (slot == ALFD_A || slot == ALFD_BT || slot == ALFD_CT);
  if (renum)
    for (int64_t i = 0; i < block_ptr[n_blocks]; ++i)
      if (rows[i] < 0 || rows[i] >= ctx->num.n())
        return ctx->err = "alfd_set_row_blocks: row id outside the numbering (alfd_set_numbering)", ALFD_E_INVALID;
  ctx->rb_ptr[slot].assign(block_ptr, block_ptr + n_blocks + 1);
  ctx->rb_rows[slot].assign(rows, rows + block_ptr[n_blocks]);
  if (renum)
    for (int32_t &r : ctx->rb_rows[slot]) r = (int32_t)ctx->num.o2n[r];
  return ALFD_OK;
}

int alfd_enable_timing(alfd_ctx_t ctx, int on) {
  if (!ctx) return ALFD_E_INVALID;
  ctx->timing = on < 0 ? 0 : on;
  for (int i = 0; i < ALFD_T_NCLASSES; ++i) ctx->t_ms[i] = 0, ctx->t_launches[i] = 0, ctx->t_bytes[i] = 0, ctx->t_fbytes[i] = 0;
  return ALFD_OK;
}
int alfd_get_timing_streamed(alfd_ctx_t ctx, double *streamed_bytes) {
  if (!ctx || !streamed_bytes) return ALFD_E_INVALID;
  for (int i = 0; i < ALFD_T_NCLASSES; ++i) streamed_bytes[i] = ctx->t_fbytes[i];
  return ALFD_OK;
}
int alfd_get_setup_seconds(alfd_ctx_t ctx, double *seconds) {
  if (!ctx || !seconds) return ALFD_E_INVALID;
  for (int i = 0; i < ALFD_SETUP_NPHASES; ++i) seconds[i] = ctx->setup_s[i];
  return ALFD_OK;
}

int alfd_get_timing(alfd_ctx_t ctx, double *ms, int64_t *launches, double *bytes) {
  if (!ctx) return ALFD_E_INVALID;
  flush_timers(ctx);
  for (int i = 0; i < ALFD_T_NCLASSES; ++i) {
    if (ms) ms[i] = ctx->t_ms[i];
    if (launches) launches[i] = ctx->t_launches[i];
    if (bytes) bytes[i] = ctx->t_bytes[i];
  }
  return ALFD_OK;
}

}  // extern "C"
