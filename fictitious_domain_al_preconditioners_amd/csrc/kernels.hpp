// kernels.hpp -- hand-written HIP kernels for gfx950 (CDNA4, wave64).
//
// All kernels are HBM-bandwidth-bound fp64 sparse / streaming work (no MFMA by
// design: SURVEY.md 8(d)).  Every reduction follows the fixed evaluation order
// of "ALFD-arith v1"  so that results are bit-identical to
// the CPU oracle:
//   SpMV row : L lanes per row; lane l does fma over entries k0+l, k0+l+L, ..;
//              xor-butterfly over the L lanes (lane 0 == binary tree).
//   dot      : 4096-element chunk per 256-thread block; thread t takes the
//              element pairs base + e*512 + 2t (e=0..7) with fma; 64-lane
//              butterfly; (w0+w1)+(w2+w3); second stage = one block doing
//              thread-strided adds and the same tree.
// Replaces: dealii::SparseMatrix<double>::vmult /
// vmult_add / Tvmult behind linear_operator() (stokes_immersed_boundary.cc:923-929)
// and the Vector dot / add / sadd / equ primitives inside SolverCG / SolverFGMRES.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace alfd {

constexpr int kBlock = 256;          // threads per workgroup (4 waves)
constexpr int64_t kChunk = 4096;     // dot chunk == vector padding granule
constexpr int kMaxBasis = 64;        // max FGMRES basis vectors handled by the batched kernels

// --------------------------------------------------------------------------
// Several 64-lane trees at once, on the vector ALU only (no LDS-pipe shuffles).
// The canonical tree adds partner lanes l^32, l^16, l^8, l^4, l^2, l^1 in that
// order.  v_permlane32_swap / v_permlane16_swap exchange half-waves / 16-lane rows
// between two registers, so the first steps of two (four) rows cost one add and
// leave the rows packed side by side; the last four steps are DPP moves inside
// 16-lane rows and serve all packed rows together.  Same pairs, same order =>
// same bits as group_reduce<64>.
__device__ __forceinline__ double dpp_xor_mov(double v, int which) {
  int lo = __double2loint(v), hi = __double2hiint(v), rl, rh;
  if (which == 8) {
    rl = __builtin_amdgcn_update_dpp(0, lo, 0x128, 0xf, 0xf, true);  // row_ror:8 (bound_ctrl: no "old" operand to set up)
    rh = __builtin_amdgcn_update_dpp(0, hi, 0x128, 0xf, 0xf, true);
  } else if (which == 4) {
    rl = __builtin_amdgcn_update_dpp(0, lo, 0x104, 0xf, 0x5, false);   // row_shl:4 -> banks 0,2
    rl = __builtin_amdgcn_update_dpp(rl, lo, 0x114, 0xf, 0xa, false);  // row_shr:4 -> banks 1,3
    rh = __builtin_amdgcn_update_dpp(0, hi, 0x104, 0xf, 0x5, false);
    rh = __builtin_amdgcn_update_dpp(rh, hi, 0x114, 0xf, 0xa, false);
  } else if (which == 2) {
    rl = __builtin_amdgcn_update_dpp(0, lo, 0x4E, 0xf, 0xf, true);  // quad_perm [2,3,0,1]
    rh = __builtin_amdgcn_update_dpp(0, hi, 0x4E, 0xf, 0xf, true);
  } else {
    rl = __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xf, 0xf, true);  // quad_perm [1,0,3,2]
    rh = __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xf, 0xf, true);
  }
  return __hiloint2double(rh, rl);
}
// a -> [a_lo | b_lo], b -> [a_hi | b_hi]  (32-lane halves)
__device__ __forceinline__ void swap32(double &a, double &b) {
  auto l = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  auto h = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  a = __hiloint2double((int)h[0], (int)l[0]);
  b = __hiloint2double((int)h[1], (int)l[1]);
}
// odd 16-lane rows of a <-> even rows of b
__device__ __forceinline__ void swap16(double &a, double &b) {
  auto l = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  auto h = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  a = __hiloint2double((int)h[0], (int)l[0]);
  b = __hiloint2double((int)h[1], (int)l[1]);
}
// --------------------------------------------------------------------------
// wave / group reductions: the canonical tree adds partner lanes l^(L/2), ..., l^2, l^1 in that
// order (all lanes end with the tree value).  Evaluated on the vector ALU: half-wave and
// 16-lane-row exchanges by v_permlane32_swap / v_permlane16_swap on two copies of the value,
// the last four steps by DPP moves -- no ds_bpermute, same pairs in the same order.
template <int L>
__device__ __forceinline__ double group_reduce(double v) {
  if (L >= 64) {
    double a = v, b = v;
    swap32(a, b);  // a = [lo | lo], b = [hi | hi]
    v = a + b;
  }
  if (L >= 32) {
    double p = v, q = v;
    swap16(p, q);  // p = rows [0,0,2,2], q = rows [1,1,3,3]
    v = p + q;
  }
  if (L >= 16) v = v + dpp_xor_mov(v, 8);
  if (L >= 8) v = v + dpp_xor_mov(v, 4);
  if (L >= 4) v = v + dpp_xor_mov(v, 2);
  if (L >= 2) v = v + dpp_xor_mov(v, 1);
  return v;
}

// lane l <- lane l + N of its 16-lane row (row_shl:N; the top N lanes of a row keep 0)
template <int N>
__device__ __forceinline__ double dpp_shl(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const int rl = __builtin_amdgcn_update_dpp(0, lo, 0x100 + N, 0xf, 0xf, true);   // bound_ctrl: the lanes shifted in read 0
  const int rh = __builtin_amdgcn_update_dpp(0, hi, 0x100 + N, 0xf, 0xf, true);
  return __hiloint2double(rh, rl);
}
// Last four tree steps inside 16-lane rows, valid in lane 0 of every row (the lane that stores): after the
// symmetric l^8 step lane l only takes its partner l + k -- the pairs of the canonical tree, and a + b is
// b + a bit for bit -- which needs one DPP move per word instead of the two masked ones of an exchange.
__device__ __forceinline__ double row16_tree(double v) {
  v = v + dpp_xor_mov(v, 8);
  v = v + dpp_shl<4>(v);
  v = v + dpp_shl<2>(v);
  v = v + dpp_shl<1>(v);
  return v;
}
// Trees of 4 rows; the result of row q sits in the 16-lane row kRow4Pos(q).
__device__ __forceinline__ double reduce_rows4(double a0, double a1, double a2, double a3) {
  swap32(a0, a1);
  double p = a0 + a1;  // [row0 | row1], step l^32 done
  swap32(a2, a3);
  double q = a2 + a3;  // [row2 | row3]
  swap16(p, q);
  return row16_tree(p + q);  // 16-lane rows: row0, row2, row1, row3
}
// Trees of 8 rows, packed as far as the hardware swaps allow: after the l^32 and l^16 steps two registers
// hold 4 rows x 16 lanes each; the l^8 step folds each to 8 lanes per row and the two are merged into ONE
// register (lanes 0..7 of every 16-lane row: rows 0..3, lanes 8..15: rows 4..7); the last three steps only
// feed the lane that stores (lane l takes its partner l + k: same pairs as the canonical tree, and a + b is
// b + a bit for bit).  Result of row {0, 2, 1, 3}[lane >> 4] + 4 * ((lane >> 3) & 1) in lanes with lane % 8 == 0.
__device__ __forceinline__ double reduce_rows8(double a0, double a1, double a2, double a3, double a4, double a5,
                                               double a6, double a7, int lane) {
  swap32(a0, a1);
  double p01 = a0 + a1;
  swap32(a2, a3);
  double p23 = a2 + a3;
  swap32(a4, a5);
  double p45 = a4 + a5;
  swap32(a6, a7);
  double p67 = a6 + a7;
  swap16(p01, p23);
  double u = p01 + p23;  // 16-lane rows: row0, row2, row1, row3
  swap16(p45, p67);
  double w = p45 + p67;  // row4, row6, row5, row7
  u = u + dpp_xor_mov(u, 8);
  w = w + dpp_xor_mov(w, 8);
  double x = (lane & 8) ? w : u;
  x = x + dpp_shl<4>(x);
  x = x + dpp_shl<2>(x);
  x = x + dpp_shl<1>(x);
  return x;
}

// lane l <- lane l - N of its 16-lane row (row_shr:N; the bottom N lanes of a row read 0)
template <int N>
__device__ __forceinline__ double dpp_shr(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const int rl = __builtin_amdgcn_update_dpp(0, lo, 0x110 + N, 0xf, 0xf, true);
  const int rh = __builtin_amdgcn_update_dpp(0, hi, 0x110 + N, 0xf, 0xf, true);
  return __hiloint2double(rh, rl);
}
// Trees of 16 rows in 66 vector instructions: the l^32 and l^16 steps leave four registers of 4 rows x 16 lanes, the l^8
// step folds each to 8 lanes per row and pairs of them merge (lanes 0..7 / 8..15 of a 16-lane row), the l^4 step folds
// to 4 lanes per row -- the first register towards the lanes with bit 2 clear (partner l + 4), the second towards those
// with bit 2 set (partner l - 4; a + b is b + a bit for bit) -- and the two merge into ONE register; the last two steps
// feed the lane that stores.  Result of row {0, 2, 1, 3}[lane >> 4] + 4 * ((lane >> 3) & 1) + 8 * ((lane >> 2) & 1) in
// the lanes with lane % 4 == 0.  Same pairs in the same order as group_reduce<64> for every row.
__device__ __forceinline__ double reduce_rows16(double (&a)[16], int lane) {
  double p[8], u[4];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    swap32(a[2 * j], a[2 * j + 1]);
    p[j] = a[2 * j] + a[2 * j + 1];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    swap16(p[2 * j], p[2 * j + 1]);
    u[j] = p[2 * j] + p[2 * j + 1];   // 16-lane rows: rows 4 j + {0, 2, 1, 3}
    u[j] = u[j] + dpp_xor_mov(u[j], 8);
  }
  const bool h = (lane & 8) != 0;
  double x0 = h ? u[1] : u[0], x1 = h ? u[3] : u[2];
  x0 = x0 + dpp_shl<4>(x0);
  x1 = x1 + dpp_shr<4>(x1);
  double z = (lane & 4) ? x1 : x0;
  z = z + dpp_shl<2>(z);
  z = z + dpp_shl<1>(z);
  return z;
}

// Trees of 2 rows: row 0 in lanes 0..31, row 1 in lanes 32..63.
__device__ __forceinline__ double reduce_rows2(double a0, double a1) {
  swap32(a0, a1);
  double p = a0 + a1, q = p;
  swap16(p, q);  // p = rows [0,0,2,2], q = rows [1,1,3,3] of the old p
  return row16_tree(p + q);
}

// block of 256 threads -> (w0+w1)+(w2+w3), valid in thread 0
__device__ __forceinline__ double block_reduce_256(double v, double *lds4) {
  v = group_reduce<64>(v);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds4[wave] = v;
  __syncthreads();
  return (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
}

// --------------------------------------------------------------------------
// CSR SpMV, L lanes per row, 256/L rows per workgroup, grid-stride over row
// groups so that the resident workgroups sweep a compact moving window of rows
// (x re-use out of L2 / Infinity Cache).
//   EPI 0: y[r]  = s
//   EPI 1: y[r]  = fma(alpha, s, y[r])          (vmult_add with a scalar)
//   EPI 2: y[r]  = d[r] * s                      (diag-scaled: t = invW .* (C x))
//   EPI 3: y[r]  = s and y2[r] = d[r] * s        (C x kept for the constraint row too)
// SPARSE: rows[] lists the non-empty rows, rp[] is indexed by list position.
// Columns >= n_local read the halo buffer (multi-GPU row partition).
// The body is shared with the second party of a pair launch (pair_rows below): workgroup `block` of `nblocks`, of BLK
// threads (a pair launch has the workgroup size of its first party).
template <int L, int EPI, bool SPARSE, int BLK = kBlock, class VT = double>
__device__ __forceinline__ void spmv_rows(int64_t block, int64_t nblocks, int64_t nrows,
                                          const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
                                          const VT *__restrict__ val, const int32_t *__restrict__ rows,
                                          const double *__restrict__ x, const double *__restrict__ x_halo,
                                          int32_t n_local, double *__restrict__ y, double alpha,
                                          const double *__restrict__ d, double *__restrict__ y2) {
  constexpr int RPB = BLK / L;
  const int lane = threadIdx.x % L;
  const int sub = threadIdx.x / L;
  const int64_t ngroups = (nrows + RPB - 1) / RPB;
  for (int64_t g = block; g < ngroups; g += nblocks) {
    const int64_t r = g * RPB + sub;
    if (r < nrows) {  // uniform within the L-lane group
      const int64_t k0 = rp[r], k1 = rp[r + 1];
      double acc = 0.0;
      for (int64_t k = k0 + lane; k < k1; k += L) {
        const int32_t c = col[k];
        const double xv = (c < n_local) ? x[c] : x_halo[c - n_local];
        acc = fma((double)val[k], xv, acc);
      }
      acc = group_reduce<L>(acc);
      if (lane == 0) {
        const int64_t ro = SPARSE ? (int64_t)rows[r] : r;
        if (EPI == 0)
          y[ro] = acc;
        else if (EPI == 1)
          y[ro] = fma(alpha, acc, y[ro]);
        else if (EPI == 2)
          y[ro] = d[ro] * acc;
        else {
          y[ro] = acc;
          y2[ro] = d[ro] * acc;
        }
      }
    }
  }
}

template <int L, int EPI, bool SPARSE, class VT = double>
__global__ __launch_bounds__(kBlock) void spmv_kernel(int64_t nrows, const int64_t *__restrict__ rp,
                                                      const int32_t *__restrict__ col,
                                                      const VT *__restrict__ val,
                                                      const int32_t *__restrict__ rows,
                                                      const double *__restrict__ x,
                                                      const double *__restrict__ x_halo, int32_t n_local,
                                                      double *__restrict__ y, double alpha,
                                                      const double *__restrict__ d,
                                                      double *__restrict__ y2) {
  spmv_rows<L, EPI, SPARSE, kBlock, VT>(blockIdx.x, gridDim.x, nrows, rp, col, val, rows, x, x_halo, n_local, y, alpha, d, y2);
}

// --------------------------------------------------------------------------
// CSR SpMV of very short rows, ONE THREAD per row (L = 4 or 8, rows of at most 2 L entries, EPI 0 or 1): 64 rows per
// wave where spmv_kernel<L> has 64 / L, and the 2 L (col, val) loads of a row are independent of each other, so a wave
// keeps 64 x 2 L entries in flight instead of 64.  The arithmetic is spmv_kernel<L>'s, emulated in registers: accumulator
// a[l] is lane l of the L-lane group (entries l, l + L in that order; a lane without entries keeps +0.0 and is added all
// the same), the tree adds the partners l^(L/2), ..., l^1 as lane 0 of group_reduce<L> sees them.  Same bits.
// One row per thread, no grid stride: gridDim.x * kBlock >= nrows.
// rowlane_row is the row of the kernel below: entry(j, c, v) loads entry j < n of the row.
template <int L, int EPI, class Entry>
__device__ __forceinline__ void rowlane_row(int64_t r, int n, Entry entry, const double *__restrict__ x,
                                            const double *__restrict__ x_halo, int32_t n_local,
                                            double *__restrict__ y, double alpha) {
  static_assert(L == 4 || L == 8, "row-per-thread SpMV: 4 or 8 emulated lanes");
  static_assert(EPI == 0 || EPI == 1, "row-per-thread SpMV: epilogues 0 and 1");
  double y0 = 0.0;
  if (EPI == 1) y0 = y[r];
  int32_t c[2 * L];
  double v[2 * L], xv[2 * L];
#pragma unroll
  for (int j = 0; j < 2 * L; ++j) {
    c[j] = 0;
    v[j] = 0.0;
    if (j < n) entry(j, c[j], v[j]);
  }
#pragma unroll
  for (int j = 0; j < 2 * L; ++j) {
    xv[j] = 0.0;
    if (j < n) xv[j] = (c[j] < n_local) ? x[c[j]] : x_halo[c[j] - n_local];
  }
  double a[L];
#pragma unroll
  for (int l = 0; l < L; ++l) a[l] = 0.0;
#pragma unroll
  for (int j = 0; j < 2 * L; ++j)
    if (j < n) a[j % L] = fma(v[j], xv[j], a[j % L]);   // not fma(0, 0, a): that would turn a -0.0 into +0.0
  double s;
  if constexpr (L == 4)
    s = (a[0] + a[2]) + (a[1] + a[3]);
  else
    s = ((a[0] + a[4]) + (a[2] + a[6])) + ((a[1] + a[5]) + (a[3] + a[7]));
  if (EPI == 0)
    y[r] = s;
  else
    y[r] = fma(alpha, s, y0);
}

// ... on the CSR arrays as uploaded: neighbouring threads read neighbouring CSR segments
template <int L, int EPI>
__global__ __launch_bounds__(kBlock) void spmv_rowlane_kernel(int64_t nrows, const int64_t *__restrict__ rp,
                                                              const int32_t *__restrict__ col,
                                                              const double *__restrict__ val,
                                                              const double *__restrict__ x,
                                                              const double *__restrict__ x_halo, int32_t n_local,
                                                              double *__restrict__ y, double alpha) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= nrows) return;
  const int64_t k0 = rp[r];
  const int n = (int)(rp[r + 1] - k0);   // <= 2 L (the launcher's condition)
  rowlane_row<L, EPI>(r, n, [&](int j, int32_t &c, double &v) { c = col[k0 + j], v = val[k0 + j]; }, x, x_halo, n_local, y,
                      alpha);
}

// --------------------------------------------------------------------------
// Pair launch: t = d .* (C x) of a factored operator A + gamma Ct W^-1 C as extra workgroups of the grid that computes
// y = A x (PAIR instantiations of spmv_vs_kernel and spmv_stream_kernel).  Workgroups [0, nA) are the A kernel as it
// is, with nA where it reads gridDim.x; workgroups [nA, nA + nC) run spmv_rows<L, 2, false> on the CSR arrays of C and
// return.  The parties share x and nothing else.  For 64-lane rows spmv_rows forms the canonical sums that
// spmv_stream_kernel reproduces, so the result is that of the separate launch whatever form C runs on alone.
struct PairC {
  int64_t nrows;
  const int64_t *rp;
  const int32_t *col;
  const double *val, *x_halo, *d;
  double *t;
  int32_t n_local, L;   // lanes per row: 16, 32 or 64
  uint32_t nA, nC;
};
struct NoPair {};

__device__ __forceinline__ uint32_t pair_nA(const NoPair &) { return gridDim.x; }
__device__ __forceinline__ uint32_t pair_nA(const PairC &c) { return c.nA; }

// the second party, or false: this workgroup belongs to the first
template <int BLK = kBlock>
__device__ __forceinline__ bool pair_rows(const NoPair &, const double *) { return false; }
template <int BLK = kBlock>
__device__ __forceinline__ bool pair_rows(const PairC &c, const double *__restrict__ x) {
  if (blockIdx.x < c.nA) return false;
  const int64_t block = blockIdx.x - c.nA;
  switch (c.L) {   // block-uniform
    case 16: spmv_rows<16, 2, false, BLK>(block, c.nC, c.nrows, c.rp, c.col, c.val, nullptr, x, c.x_halo, c.n_local, c.t, 0.0, c.d, nullptr); break;
    case 32: spmv_rows<32, 2, false, BLK>(block, c.nC, c.nrows, c.rp, c.col, c.val, nullptr, x, c.x_halo, c.n_local, c.t, 0.0, c.d, nullptr); break;
    default: spmv_rows<64, 2, false, BLK>(block, c.nC, c.nrows, c.rp, c.col, c.val, nullptr, x, c.x_halo, c.n_local, c.t, 0.0, c.d, nullptr); break;
  }
  return true;
}
template <bool PAIR>
using PairArg = typename std::conditional<PAIR, PairC, NoPair>::type;

// --------------------------------------------------------------------------
// Streaming CSR SpMV for long rows (canonical L = 64).  One wave owns a batch
// of R consecutive rows and streams their CONTIGUOUS nnz range with perfectly
// coalesced, U-way unrolled col/val loads: U*768 B (+ the x gathers) in flight
// per wave instead of one row's worth, and no idle lanes at row tails.
// Bit-compatible with the canonical order: entry k of row i belongs to
// canonical lane (k - k0_i) mod 64; the stream lane that sees it is
// (k - k_begin) mod 64 and stays the same for all later entries of that
// canonical lane (k advances by 64), so each stream lane's per-row accumulator
// IS one canonical lane partial, rotated by d_i = (k0_i - k_begin) mod 64.  One
// ds_bpermute un-rotates before the butterfly.
// PAIR: the grid carries a second party behind its first nA workgroups (pair_rows above).
template <int R, int U, int EPI, bool NT, bool PAIR = false, class VT = double>
__global__ __launch_bounds__(kBlock) void spmv_stream_kernel(
    int64_t nrows, const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
    const VT *__restrict__ val, const double *__restrict__ x, const double *__restrict__ x_halo,
    int32_t n_local, double *__restrict__ y, double alpha, const double *__restrict__ d,
    double *__restrict__ y2, PairArg<PAIR> pc) {
  if (pair_rows(pc, x)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nbatches = (nrows + R - 1) / R;
  for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < nbatches; b += (int64_t)pair_nA(pc) * 4) {
    const int64_t r0 = b * R;
    int64_t kb[R + 1];
#pragma unroll
    for (int i = 0; i <= R; ++i) kb[i] = rp[r0 + i < nrows ? r0 + i : nrows];  // wave-uniform
    const int64_t k_begin = kb[0];
    const int32_t n_batch = (int32_t)(kb[R] - k_begin);
    int32_t rel[R + 1];
#pragma unroll
    for (int i = 0; i <= R; ++i) rel[i] = (int32_t)(kb[i] - k_begin);
    double acc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) acc[i] = 0.0;
    const int32_t *cb = col + k_begin;
    const VT *vb = val + k_begin;
    for (int32_t base = 0; base < n_batch; base += 64 * U) {
      int32_t c[U];
      VT v[U];
      double xv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t o = base + 64 * u + lane;
        if (o < n_batch) {
          c[u] = NT ? __builtin_nontemporal_load(cb + o) : cb[o];
          v[u] = NT ? __builtin_nontemporal_load(vb + o) : vb[o];
        } else {
          c[u] = -1;
          v[u] = VT(0);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        xv[u] = 0.0;
        if (c[u] >= 0) xv[u] = (c[u] < n_local) ? x[c[u]] : x_halo[c[u] - n_local];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t o = base + 64 * u + lane;
        if (c[u] >= 0) {
#pragma unroll
          for (int i = 0; i < R; ++i)
            if (o >= rel[i] && o < rel[i + 1]) acc[i] = fma((double)v[u], xv[u], acc[i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t r = r0 + i;
      if (r < nrows) {  // wave-uniform
        const int dsh = rel[i] & 63;
        double s = __shfl(acc[i], (lane + dsh) & 63, 64);
        s = group_reduce<64>(s);
        if (lane == 0) {
          if (EPI == 0)
            y[r] = s;
          else if (EPI == 1)
            y[r] = fma(alpha, s, y[r]);
          else if (EPI == 2)
            y[r] = d[r] * s;
          else {
            y[r] = s;
            y2[r] = d[r] * s;
          }
        }
      }
    }
  }
}

// --------------------------------------------------------------------------
// LDS-windowed streaming SpMV (the roofline kernel for long-row matrices).
// Rows are grouped in blocks of RB; at upload the host finds, per block, the
// union of column intervals its rows touch (the "x window"), lays the
// intervals out back to back and rewrites every column index as a 16-bit
// offset into that window.  A workgroup then
//   1. stages its window from x into LDS with coalesced loads (each x entry is
//      fetched once per block instead of once per use),
//   2. streams val (8 B) + local col (2 B) = 10 B/nnz instead of 12 B/nnz,
//   3. gathers from LDS.
// Same fma/tree order as spmv_stream_kernel => bit-identical results.
// Blocks whose window exceeds the LDS budget (blk_W < 0) gather from global
// memory with the original 32-bit columns.
// TAG only distinguishes instantiations (fine operator = 0, multigrid level matrices = 1)
// so that profiler summaries report them separately.
template <int R, int U, int EPI, int TAG = 0, class VT = double>
__global__ __launch_bounds__(kBlock) void spmv_window_kernel(
    int64_t nrows, int32_t RB, const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
    const uint16_t *__restrict__ lcol, const VT *__restrict__ val,
    const int32_t *__restrict__ blk_seg_begin, const int32_t *__restrict__ blk_W,
    const int32_t *__restrict__ seg_col, const int32_t *__restrict__ seg_off,
    const double *__restrict__ x, const double *__restrict__ x_halo, int32_t n_local,
    double *__restrict__ y, double alpha, const double *__restrict__ d, double *__restrict__ y2,
    int xcd_remap) {
  extern __shared__ double xs[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // XCD-aware block order: workgroups with equal blockIdx % 8 share an XCD (and its L2),
  // so each XCD is given a CONTIGUOUS run of row blocks -- neighbouring blocks share
  // most of their x window, which then hits in that XCD's L2 (bijective remap for any
  // grid size; affects speed only).
  int64_t b = blockIdx.x;
  if (xcd_remap) {
    const int64_t nwg = gridDim.x, q = nwg / 8, rm = nwg % 8, xcd = b % 8, idx = b / 8;
    b = (xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + idx;
  }
  const int32_t W = blk_W[b];
  if (W >= 0) {
    const int32_t s0 = blk_seg_begin[b], s1 = blk_seg_begin[b + 1];
    for (int32_t s = s0 + wave; s < s1; s += 4) {
      const int32_t c0 = seg_col[s], o0 = seg_off[s];
      const int32_t len = ((s + 1 < s1) ? seg_off[s + 1] : W) - o0;
      for (int32_t i = lane; i < len; i += 64) {
        const int32_t c = c0 + i;
        xs[o0 + i] = (c < n_local) ? x[c] : x_halo[c - n_local];
      }
    }
    __syncthreads();
  }
  const int64_t row_begin = b * RB;
  const int64_t row_end = (row_begin + RB < nrows) ? row_begin + RB : nrows;
  for (int64_t r0 = row_begin + (int64_t)wave * R; r0 < row_end; r0 += 4 * R) {
    int64_t kb[R + 1];
#pragma unroll
    for (int i = 0; i <= R; ++i) kb[i] = rp[r0 + i < row_end ? r0 + i : row_end];  // wave-uniform
    const int64_t k_begin = kb[0];
    const int32_t n_batch = (int32_t)(kb[R] - k_begin);
    int32_t rel[R + 1];
#pragma unroll
    for (int i = 0; i <= R; ++i) rel[i] = (int32_t)(kb[i] - k_begin);
    double acc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) acc[i] = 0.0;
    const VT *vb = val + k_begin;
    if (W >= 0) {
      const uint16_t *cb = lcol + k_begin;
      for (int32_t base = 0; base < n_batch; base += 64 * U) {
        int32_t c[U];
        VT v[U];
        double xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int32_t o = base + 64 * u + lane;
          if (o < n_batch) {
            c[u] = cb[o];
            v[u] = vb[o];
          } else {
            c[u] = -1;
            v[u] = VT(0);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) xv[u] = c[u] >= 0 ? xs[c[u]] : 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int32_t o = base + 64 * u + lane;
          if (c[u] >= 0) {
#pragma unroll
            for (int i = 0; i < R; ++i)
              if (o >= rel[i] && o < rel[i + 1]) acc[i] = fma((double)v[u], xv[u], acc[i]);
          }
        }
      }
    } else {
      const int32_t *cb = col + k_begin;
      for (int32_t base = 0; base < n_batch; base += 64 * U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int32_t o = base + 64 * u + lane;
          if (o < n_batch) {
            const int32_t c = cb[o];
            const double xv = (c < n_local) ? x[c] : x_halo[c - n_local];
            const double v = (double)vb[o];
#pragma unroll
            for (int i = 0; i < R; ++i)
              if (o >= rel[i] && o < rel[i + 1]) acc[i] = fma(v, xv, acc[i]);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t r = r0 + i;
      if (r < row_end) {  // wave-uniform
        const int dsh = rel[i] & 63;
        double s = __shfl(acc[i], (lane + dsh) & 63, 64);
        s = group_reduce<64>(s);
        if (lane == 0) {
          if (EPI == 0)
            y[r] = s;
          else if (EPI == 1)
            y[r] = fma(alpha, s, y[r]);
          else if (EPI == 2)
            y[r] = d[r] * s;
          else {
            y[r] = s;
            y2[r] = d[r] * s;
          }
        }
      }
    }
  }
}

// --------------------------------------------------------------------------
// Value-indexed blocks: finite-element matrices on the reference's uniformly refined
// hyper_cube grids repeat a few hundred distinct entry values.  At upload each row block
// whose entries take <= 256 distinct bit patterns gets a private dictionary (stored once,
// staged into LDS next to the x window) and an 8-bit code per entry, so the stream is
// 2 B (window column) + 1 B (value code) = 3 B/nnz instead of 10.  The looked-up double
// is the stored one bit for bit, so results do not change.  Blocks with 257..512 distinct
// values use 16-bit codes (4 B/nnz); blocks beyond that keep streaming the 8-byte values.
//
// Row-batched window kernel for value-indexed matrices.  With 3 B/nnz the stream
// is no longer HBM-bound but latency-bound, so the kernel is organised to keep
// many independent loads in flight and to spend few instructions per entry:
// a wave takes R consecutive rows; lane l reads entries k0_i + l + 64 j of row i
// -- exactly the canonical lane assignment, so there is no rotation and no
// per-row predication -- and issues the loads of all R rows (J chunks each)
// before the first use.  Idle lanes at row tails cost issue slots, not traffic.
// MODE 0: dictionary values + LDS window; 1: 8-byte values + LDS window;
// MODE 2: 8-byte values, x gathered from global memory (block without a window);
// MODE 3: as 0 with 16-bit value codes (blocks with 257..512 distinct values).
constexpr int32_t kDictWide = 1 << 16;    // blk_dict_n flag: 16-bit codes
constexpr int32_t kDictMaxEntries = 512;  // LDS slots reserved for a block dictionary

// ks[i]: offset of row i's first entry from the block's first entry (the *_b pointers are
// pre-offset to it); len[i]: its entry count.
template <int R, int J, int MODE>
__device__ __forceinline__ void vi_rows(const uint32_t (&ks)[R], const int32_t (&len)[R], int lane,
                                        const uint16_t *__restrict__ lcol_b, const uint8_t *__restrict__ vidx_b,
                                        const uint16_t *__restrict__ vidw_b,
                                        const int32_t *__restrict__ col_b, const double *__restrict__ val_b,
                                        const double *xs, const double *ds, const double *__restrict__ x,
                                        const double *__restrict__ x_halo, int32_t n_local, double (&acc)[R]) {
  int32_t maxlen = 0;
#pragma unroll
  for (int i = 0; i < R; ++i) maxlen = len[i] > maxlen ? len[i] : maxlen;
  for (int32_t base = 0; base < maxlen; base += 64 * J) {  // one pass unless a row has > 64 J entries
    // One wave-uniform guard per row and pass; inside it the J chunks are straight-line code:
    // lanes past the row end re-read the row's first entry (a cache hit) and are masked at
    // the fma.  Everything loaded under a guard is only used under the same guard, so the
    // arrays need no defaults, and all loads of the R rows are in flight before the first use.
    int32_t c[R][J], iv[R][J];
    double v[R][J];
    bool ok[R][J];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (base < len[i]) {  // wave-uniform
#pragma unroll
        for (int j = 0; j < J; ++j) {
          const int32_t o = base + 64 * j + lane;
          ok[i][j] = o < len[i];
          const uint32_t k = ks[i] + (uint32_t)(ok[i][j] ? o : 0);
          if (MODE == 2) c[i][j] = col_b[k];
          else c[i][j] = lcol_b[k];
          if (MODE == 0) iv[i][j] = vidx_b[k];
          else if (MODE == 3) iv[i][j] = vidw_b[k];
          else v[i][j] = val_b[k];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (base < len[i]) {  // wave-uniform
        double xv[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {
          if (MODE == 2) xv[j] = (c[i][j] < n_local) ? x[c[i][j]] : x_halo[c[i][j] - n_local];
          else xv[j] = xs[c[i][j]];
          if (MODE == 0 || MODE == 3) v[i][j] = ds[iv[i][j]];
        }
        // keep the gathers of all J chunks ahead of the masked fmas (the compiler would
        // otherwise sink each ds_read into its exec-masked block and wait on it there)
#pragma unroll
        for (int j = 0; j < J; ++j) asm volatile("" : "+v"(xv[j]), "+v"(v[i][j]));
#pragma unroll
        for (int j = 0; j < J; ++j)
          if (ok[i][j]) acc[i] = fma(v[i][j], xv[j], acc[i]);
      }
    }
  }
}

template <int J0, int JN, int NCH, int MODE>
__device__ __forceinline__ void vib_pass(const uint32_t (&ks)[4], const int32_t (&len)[4], int lane,
                                         const uint16_t *__restrict__ lcol_b,
                                         const uint8_t *__restrict__ vidx_b, const uint16_t *__restrict__ vidw_b,
                                         const double *xs, const double *ds, double (&acc)[4]) {
  // chunks J0 .. J0+JN-1 of every row of the batch; chunk NCH-1 is the only partial one
  int32_t c[4][JN], iv[4][JN];
  bool ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < JN; ++j) {
      const int32_t o = 64 * (J0 + j) + lane;
      uint32_t k = ks[i] + (uint32_t)o;
      if (J0 + j == NCH - 1) {
        ok[i] = o < len[i];
        k = ks[i] + (uint32_t)(ok[i] ? o : 0);
      }
      c[i][j] = lcol_b[k];
      iv[i][j] = MODE == 3 ? (int32_t)vidw_b[k] : (int32_t)vidx_b[k];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double xv[JN], v[JN];
#pragma unroll
    for (int j = 0; j < JN; ++j) {
      xv[j] = xs[c[i][j]];
      v[j] = ds[iv[i][j]];
    }
#pragma unroll
    for (int j = 0; j < JN; ++j) asm volatile("" : "+v"(xv[j]), "+v"(v[j]));
#pragma unroll
    for (int j = 0; j < JN; ++j) {
      if (J0 + j == NCH - 1) {
        if (ok[i]) acc[i] = fma(v[j], xv[j], acc[i]);
      } else {
        acc[i] = fma(v[j], xv[j], acc[i]);
      }
    }
  }
}

// Batch of 4 rows that all have exactly NCH 64-entry chunks (the last one possibly partial):
// no guards at all, and only the last chunk of each row carries a lane mask.  At most 3
// chunks per row are in flight at a time (12 chunk loads, ~56 VGPRs: 8 waves per SIMD).
// MODE 0 (8-bit codes) or 3 (16-bit codes).
template <int NCH, int MODE>
__device__ __forceinline__ void vib_rows(const uint32_t (&ks)[4], const int32_t (&len)[4], int lane,
                                         const uint16_t *__restrict__ lcol_b,
                                         const uint8_t *__restrict__ vidx_b, const uint16_t *__restrict__ vidw_b,
                                         const double *xs, const double *ds, double (&acc)[4]) {
  constexpr int A = NCH <= 3 ? NCH : (NCH + 1) / 2;
  vib_pass<0, A, NCH, MODE>(ks, len, lane, lcol_b, vidx_b, vidw_b, xs, ds, acc);
  if (NCH > A) vib_pass<A, (NCH > A ? NCH - A : 1), NCH, MODE>(ks, len, lane, lcol_b, vidx_b, vidw_b, xs, ds, acc);
}

template <int R, int J, int EPI>
__global__ __launch_bounds__(kBlock) void spmv_window_vi_kernel(
    int64_t nrows, int32_t RB, const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
    const uint16_t *__restrict__ lcol, const double *__restrict__ val,
    const int32_t *__restrict__ blk_seg_begin, const int32_t *__restrict__ blk_W,
    const int32_t *__restrict__ seg_col, const int32_t *__restrict__ seg_off,
    const double *__restrict__ x, const double *__restrict__ x_halo, int32_t n_local,
    double *__restrict__ y, double alpha, const double *__restrict__ d, double *__restrict__ y2,
    const uint8_t *__restrict__ vidx, const uint16_t *__restrict__ vidw,
    const int32_t *__restrict__ blk_dict_off, const int32_t *__restrict__ blk_dict_n,
    const double *__restrict__ dict, int32_t dict_lds_off) {
  extern __shared__ double xs[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t b = blockIdx.x;
  const int32_t W = blk_W[b];
  const double *ds = xs + dict_lds_off;
  int mode = 2;  // block-uniform
  if (W >= 0) {
    const int32_t nd = blk_dict_n[b];
    mode = nd < 0 ? 1 : ((nd & kDictWide) ? 3 : 0);
    const int32_t ndv = nd & 0xffff;
    if (nd >= 0)
      for (int t = threadIdx.x; t < ndv; t += kBlock) xs[dict_lds_off + t] = dict[blk_dict_off[b] + t];
    const int32_t s0 = blk_seg_begin[b], s1 = blk_seg_begin[b + 1];
    for (int32_t s = s0 + wave; s < s1; s += 4) {
      const int32_t c0 = seg_col[s], o0 = seg_off[s];
      const int32_t len = ((s + 1 < s1) ? seg_off[s + 1] : W) - o0;
      for (int32_t i = lane; i < len; i += 64) {
        const int32_t c = c0 + i;
        xs[o0 + i] = (c < n_local) ? x[c] : x_halo[c - n_local];
      }
    }
    __syncthreads();
  }
  const int64_t row_begin = b * RB;
  const int64_t row_end = (row_begin + RB < nrows) ? row_begin + RB : nrows;
  for (int64_t r0 = row_begin + (int64_t)wave * R; r0 < row_end; r0 += 4 * R) {
    int64_t kb[R + 1];
#pragma unroll
    for (int i = 0; i <= R; ++i) kb[i] = rp[r0 + i < row_end ? r0 + i : row_end];  // wave-uniform
    uint32_t ks[R];
    int32_t len[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      ks[i] = (uint32_t)(kb[i] - kb[0]);
      len[i] = (int32_t)(kb[i + 1] - kb[i]);
    }
    const uint16_t *lcol_b = lcol + kb[0];
    const uint8_t *vidx_b = vidx + kb[0];
    const uint16_t *vidw_b = vidw + kb[0];
    const int32_t *col_b = col + kb[0];
    const double *val_b = val + kb[0];
    double acc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) acc[i] = 0.0;
    if (mode == 3) vi_rows<R, J, 3>(ks, len, lane, lcol_b, vidx_b, vidw_b, col_b, val_b, xs, ds, x, x_halo, n_local, acc);
    else if (mode == 0) vi_rows<R, J, 0>(ks, len, lane, lcol_b, vidx_b, vidw_b, col_b, val_b, xs, ds, x, x_halo, n_local, acc);
    else if (mode == 1) vi_rows<R, J, 1>(ks, len, lane, lcol_b, vidx_b, vidw_b, col_b, val_b, xs, ds, x, x_halo, n_local, acc);
    else vi_rows<R, J, 2>(ks, len, lane, lcol_b, vidx_b, vidw_b, col_b, val_b, xs, ds, x, x_halo, n_local, acc);
    // rows past row_end have no entries (acc = 0) and are not written
    static_assert(R == 2 || R == 4, "row batches of 2 or 4");
    double s;
    int64_t r;
    bool writer;
    if (R == 4) {
      s = reduce_rows4(acc[0], acc[1], acc[R - 2], acc[R - 1]);
      const int q = lane >> 4;                         // 16-lane row: holds row {0, 2, 1, 3}[q]
      r = r0 + (((q & 1) << 1) | (q >> 1));
      writer = (lane & 15) == 0;
    } else {
      s = reduce_rows2(acc[0], acc[1]);
      r = r0 + (lane >> 5);
      writer = (lane & 31) == 0;
    }
    if (writer && r < row_end) {
      if (EPI == 0)
        y[r] = s;
      else if (EPI == 1)
        y[r] = fma(alpha, s, y[r]);
      else if (EPI == 2)
        y[r] = d[r] * s;
      else {
        y[r] = s;
        y2[r] = d[r] * s;
      }
    }
  }
}

// Class-batched variant (the default for value-indexed matrices).  At upload the rows of
// every block are grouped by their chunk count ceil(len / 64) into batches of 4 rows (a
// 32-byte descriptor per batch: per row its entry offset, length and block-local row id).
// A wave runs the batch through code specialised for that class -- straight-line, no
// guards -- and writes the four sums to the rows the descriptor names.  Rows keep their
// canonical lane assignment and fma order, so the result is unchanged; only the order in
// which a block's rows are visited differs.
constexpr int kVibMaxClass = 6;   // classes 0..6 are specialised, longer rows take the generic path
// The register budget is capped at 64 VGPRs so that 8 waves fit a SIMD (only the rare
// generic paths spill).  TAG only separates the fine operator (0) from multigrid level
// matrices (1) in profiler summaries.
template <int EPI, int TAG = 0, int NW = 4>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(8, 8))) void spmv_window_vib_kernel(
    int64_t nrows, int32_t RB, const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
    const uint16_t *__restrict__ lcol, const double *__restrict__ val,
    const int32_t *__restrict__ blk_seg_begin, const int32_t *__restrict__ blk_W,
    const int32_t *__restrict__ seg_col, const int32_t *__restrict__ seg_off,
    const double *__restrict__ x, const double *__restrict__ x_halo, int32_t n_local,
    double *__restrict__ y, double alpha, const double *__restrict__ d, double *__restrict__ y2,
    const uint8_t *__restrict__ vidx, const uint16_t *__restrict__ vidw,
    const int32_t *__restrict__ blk_dict_off, const int32_t *__restrict__ blk_dict_n,
    const double *__restrict__ dict, int32_t dict_lds_off,
    const uint64_t *__restrict__ btab, const int32_t *__restrict__ bcnt, int32_t bstride, int xcd_remap) {
  extern __shared__ double xs[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // Workgroups with equal blockIdx % 8 share an XCD and its L2.  With 3 B/nnz the x windows are
  // a third of the traffic, and neighbouring row blocks share most of their window: give each
  // XCD a contiguous run of row blocks so that the overlap hits in that XCD's L2.
  int64_t b = blockIdx.x;
  if (xcd_remap) {
    const int64_t nwg = gridDim.x, q = nwg / 8, rm = nwg % 8, xcd = b % 8, idx = b / 8;
    b = (xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + idx;
  }
  const int32_t W = blk_W[b];
  const double *ds = xs + dict_lds_off;
  int mode = 2;  // block-uniform
  if (W >= 0) {
    const int32_t nd = blk_dict_n[b];
    mode = nd < 0 ? 1 : ((nd & kDictWide) ? 3 : 0);
    const int32_t ndv = nd & 0xffff;
    if (nd >= 0)
      for (int t = threadIdx.x; t < ndv; t += 64 * NW) xs[dict_lds_off + t] = dict[blk_dict_off[b] + t];
    const int32_t s0 = blk_seg_begin[b], s1 = blk_seg_begin[b + 1];
    for (int32_t s = s0 + wave; s < s1; s += NW) {
      const int32_t c0 = seg_col[s], o0 = seg_off[s];
      const int32_t len = ((s + 1 < s1) ? seg_off[s + 1] : W) - o0;
      for (int32_t i = lane; i < len; i += 64) {
        const int32_t c = c0 + i;
        xs[o0 + i] = (c < n_local) ? x[c] : x_halo[c - n_local];
      }
    }
    __syncthreads();
  }
  const int64_t row_begin = b * RB;
  const int64_t k_blk = rp[row_begin];
  const uint16_t *lcol_b = lcol + k_blk;
  const uint8_t *vidx_b = vidx + k_blk;
  const uint16_t *vidw_b = vidw + k_blk;
  const int32_t *col_b = col + k_blk;
  const double *val_b = val + k_blk;
  const int32_t nbatch = bcnt[b];
  // batch descriptor: 4 x uint64 = {entry offset from the block start (32) | entry count (16) |
  // block-local row id, 0xFF = filler (8) | class (8)}; the next batch's descriptor is
  // fetched while the current one is processed (one s_load_dwordx8 each)
  const uint64_t *bt = btab + (b * bstride + wave) * 4;
  uint64_t nx[4] = {0, 0, 0, 0};
  if (wave < nbatch) {
#pragma unroll
    for (int i = 0; i < 4; ++i) nx[i] = bt[i];
  }
  for (int32_t bi = wave; bi < nbatch; bi += NW) {
    uint64_t desc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) desc[i] = nx[i];
    bt += 4 * NW;
    if (bi + NW < nbatch) {
#pragma unroll
      for (int i = 0; i < 4; ++i) nx[i] = bt[i];
    }
    const int cls = (int)(desc[0] >> 56);
    uint32_t ks[4];
    int32_t len[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ks[i] = (uint32_t)desc[i];
      len[i] = (int32_t)((desc[i] >> 32) & 0xffff);
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (mode == 0) {
      switch (cls) {
        case 0: break;
        case 1: vib_rows<1, 0>(ks, len, lane, lcol_b, vidx_b, vidw_b, xs, ds, acc); break;
        case 2: vib_rows<2, 0>(ks, len, lane, lcol_b, vidx_b, vidw_b, xs, ds, acc); break;
        case 3: vib_rows<3, 0>(ks, len, lane, lcol_b, vidx_b, vidw_b, xs, ds, acc); break;
        case 4: vib_rows<4, 0>(ks, len, lane, lcol_b, vidx_b, vidw_b, xs, ds, acc); break;
        case 5: vib_rows<5, 0>(ks, len, lane, lcol_b, vidx_b, vidw_b, xs, ds, acc); break;
        case 6: vib_rows<6, 0>(ks, len, lane, lcol_b, vidx_b, vidw_b, xs, ds, acc); break;
        default: vi_rows<4, 2, 0>(ks, len, lane, lcol_b, vidx_b, vidw_b, col_b, val_b, xs, ds, x, x_halo, n_local, acc);
      }
    } else if (mode == 3) {
      switch (cls) {
        case 0: break;
        case 1: vib_rows<1, 3>(ks, len, lane, lcol_b, vidx_b, vidw_b, xs, ds, acc); break;
        case 2: vib_rows<2, 3>(ks, len, lane, lcol_b, vidx_b, vidw_b, xs, ds, acc); break;
        case 3: vib_rows<3, 3>(ks, len, lane, lcol_b, vidx_b, vidw_b, xs, ds, acc); break;
        case 4: vib_rows<4, 3>(ks, len, lane, lcol_b, vidx_b, vidw_b, xs, ds, acc); break;
        case 5: vib_rows<5, 3>(ks, len, lane, lcol_b, vidx_b, vidw_b, xs, ds, acc); break;
        case 6: vib_rows<6, 3>(ks, len, lane, lcol_b, vidx_b, vidw_b, xs, ds, acc); break;
        default: vi_rows<4, 2, 3>(ks, len, lane, lcol_b, vidx_b, vidw_b, col_b, val_b, xs, ds, x, x_halo, n_local, acc);
      }
    } else if (mode == 1) {
      vi_rows<4, 2, 1>(ks, len, lane, lcol_b, vidx_b, vidw_b, col_b, val_b, xs, ds, x, x_halo, n_local, acc);
    } else {
      vi_rows<4, 2, 2>(ks, len, lane, lcol_b, vidx_b, vidw_b, col_b, val_b, xs, ds, x, x_halo, n_local, acc);
    }
    const double s = reduce_rows4(acc[0], acc[1], acc[2], acc[3]);
    const int q = lane >> 4;  // 16-lane row q holds the tree of batch row {0, 2, 1, 3}[q]
    const uint64_t dq = q == 0 ? desc[0] : (q == 1 ? desc[2] : (q == 2 ? desc[1] : desc[3]));
    const int id = (int)((dq >> 48) & 0xff);
    if ((lane & 15) == 0 && id != 0xff) {
      const int64_t r = row_begin + id;
      if (EPI == 0)
        y[r] = s;
      else if (EPI == 1)
        y[r] = fma(alpha, s, y[r]);
      else if (EPI == 2)
        y[r] = d[r] * s;
      else {
        y[r] = s;
        y2[r] = d[r] * s;
      }
    }
  }
}

// --------------------------------------------------------------------------
// The same LDS-window scheme for short-row matrices (canonical L = 8, 16 or 32:
// Q1 stencils, pressure mass, multigrid level operators).  An L-lane group plays
// the role of the wave: it owns a batch of R consecutive rows of the block and
// streams their contiguous entries L*U at a time; the un-rotation and the tree
// stay inside the group (width-L shuffles), so the result is again the canonical
// one bit for bit.  Row blocks are larger (RB scales with 64/L) so that a window
// is amortised over about as many entries as in the long-row kernel.
template <int L, int R, int U, int EPI, int TAG = 0>
__global__ __launch_bounds__(kBlock) void spmv_window_group_kernel(
    int64_t nrows, int32_t RB, const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
    const uint16_t *__restrict__ lcol, const double *__restrict__ val,
    const int32_t *__restrict__ blk_seg_begin, const int32_t *__restrict__ blk_W,
    const int32_t *__restrict__ seg_col, const int32_t *__restrict__ seg_off,
    const double *__restrict__ x, const double *__restrict__ x_halo, int32_t n_local,
    double *__restrict__ y, double alpha, const double *__restrict__ d, double *__restrict__ y2) {
  extern __shared__ double xs[];
  constexpr int G = kBlock / L;  // groups per workgroup
  const int lane = threadIdx.x % L;
  const int grp = threadIdx.x / L;
  const int wlane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t b = blockIdx.x;
  const int32_t W = blk_W[b];
  if (W >= 0) {
    const int32_t s0 = blk_seg_begin[b], s1 = blk_seg_begin[b + 1];
    for (int32_t s = s0 + wave; s < s1; s += 4) {
      const int32_t c0 = seg_col[s], o0 = seg_off[s];
      const int32_t len = ((s + 1 < s1) ? seg_off[s + 1] : W) - o0;
      for (int32_t i = wlane; i < len; i += 64) {
        const int32_t c = c0 + i;
        xs[o0 + i] = (c < n_local) ? x[c] : x_halo[c - n_local];
      }
    }
    __syncthreads();
  }
  const int64_t row_begin = b * RB;
  const int64_t row_end = (row_begin + RB < nrows) ? row_begin + RB : nrows;
  for (int64_t r0 = row_begin + (int64_t)grp * R; r0 < row_end; r0 += G * R) {
    int64_t kb[R + 1];
#pragma unroll
    for (int i = 0; i <= R; ++i) kb[i] = rp[r0 + i < row_end ? r0 + i : row_end];  // group-uniform
    const int64_t k_begin = kb[0];
    const int32_t n_batch = (int32_t)(kb[R] - k_begin);
    int32_t rel[R + 1];
#pragma unroll
    for (int i = 0; i <= R; ++i) rel[i] = (int32_t)(kb[i] - k_begin);
    double acc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) acc[i] = 0.0;
    const double *vb = val + k_begin;
    const uint16_t *cl = lcol + k_begin;
    const int32_t *cg = col + k_begin;
    for (int32_t base = 0; base < n_batch; base += L * U) {
      int32_t c[U];
      double v[U], xv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t o = base + L * u + lane;
        if (o < n_batch) {
          c[u] = (W >= 0) ? (int32_t)cl[o] : cg[o];
          v[u] = vb[o];
        } else {
          c[u] = -1;
          v[u] = 0.0;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        xv[u] = 0.0;
        if (c[u] >= 0) xv[u] = (W >= 0) ? xs[c[u]] : ((c[u] < n_local) ? x[c[u]] : x_halo[c[u] - n_local]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t o = base + L * u + lane;
        if (c[u] >= 0) {
#pragma unroll
          for (int i = 0; i < R; ++i)
            if (o >= rel[i] && o < rel[i + 1]) acc[i] = fma(v[u], xv[u], acc[i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t r = r0 + i;
      if (r < row_end) {  // group-uniform
        const int dsh = rel[i] & (L - 1);
        double s = __shfl(acc[i], (lane + dsh) & (L - 1), L);
        s = group_reduce<L>(s);
        if (lane == 0) {
          if (EPI == 0)
            y[r] = s;
          else if (EPI == 1)
            y[r] = fma(alpha, s, y[r]);
          else if (EPI == 2)
            y[r] = d[r] * s;
          else {
            y[r] = s;
            y2[r] = d[r] * s;
          }
        }
      }
    }
  }
}

// device scalars -> mapped pinned host mirror (read by the host after a stream sync)
__global__ void mirror_scalars_kernel(const double *__restrict__ sc, double *__restrict__ host, int count) {
  for (int i = threadIdx.x; i < count; i += blockDim.x) host[i] = sc[i];
  __threadfence_system();
}

// --------------------------------------------------------------------------
// Streaming vector kernels. All vectors are padded to a multiple of kChunk with
// zeros, so no bounds checks: one workgroup per chunk, thread t owns the pairs
// base + e*512 + 2t -- the SAME mapping as the canonical dot, which lets the
// fused "update + dot" kernels emit canonical partials.
#define ALFD_FOR_PAIRS(i)                                   \
  const int64_t base__ = (int64_t)blockIdx.x * kChunk;      \
  _Pragma("unroll") for (int e__ = 0; e__ < 8; ++e__)       \
      for (int64_t i = base__ + e__ * 512 + 2 * threadIdx.x, once__ = 1; once__; once__ = 0)

__device__ __forceinline__ double2 ld2(const double *p, int64_t i) {
  return *reinterpret_cast<const double2 *>(p + i);
}
__device__ __forceinline__ void st2(double *p, int64_t i, double2 v) {
  *reinterpret_cast<double2 *>(p + i) = v;
}

// partial[b] = canonical chunk sum of x.y
__global__ __launch_bounds__(kBlock) void dot_partial_kernel(const double *__restrict__ x,
                                                             const double *__restrict__ y,
                                                             double *__restrict__ partial) {
  __shared__ double lds4[4];
  double acc = 0.0;
  ALFD_FOR_PAIRS(i) {
    const double2 a = ld2(x, i), b = ld2(y, i);
    acc = fma(a.x, b.x, acc);
    acc = fma(a.y, b.y, acc);
  }
  const double s = block_reduce_256(acc, lds4);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// Second stage for `count` dots at once: block j reduces partial[j*stride ..+nb).
// post-ops on the device scalar table `sc` (so PCG needs no host round trip for
// alpha / beta):
//   FIN_STORE  : sc[out+j] = sum
//   FIN_ALPHA  : sc[out] = sum (p.Ap); sc[S_ALPHA] = sc[S_RZ]/sum; sc[S_NALPHA] = -alpha
//   FIN_RZ     : sc[S_RZ_OLD] = sc[S_RZ]; sc[S_RZ] = sum; sc[S_BETA] = sum / old
enum { FIN_STORE = 0, FIN_ALPHA = 1, FIN_RZ = 2 };
enum { S_RZ = 0, S_RZ_OLD = 1, S_PAP = 2, S_ALPHA = 3, S_NALPHA = 4, S_BETA = 5, S_RR = 6, S_TMP = 7, S_H = 8 };
constexpr int S_STAGE = S_H + 2 * kMaxBasis;  // multi-rank local sums before the all-gather
constexpr int kNumScalars = S_H + 3 * kMaxBasis + 8;

__global__ __launch_bounds__(kBlock) void dot_final_kernel(const double *__restrict__ partial, int64_t nb,
                                                           int64_t stride, double *__restrict__ sc,
                                                           int out, int fin) {
  __shared__ double lds4[4];
  const double *p = partial + (int64_t)blockIdx.x * stride;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < nb; i += kBlock) acc = acc + p[i];
  const double s = block_reduce_256(acc, lds4);
  if (threadIdx.x == 0) {
    if (fin == FIN_STORE) {
      sc[out + blockIdx.x] = s;
    } else if (fin == FIN_ALPHA) {
      sc[S_PAP] = s;
      const double a = sc[S_RZ] / s;
      sc[S_ALPHA] = a;
      sc[S_NALPHA] = -a;
    } else {
      const double old = sc[S_RZ];
      sc[S_RZ_OLD] = old;
      sc[S_RZ] = s;
      sc[S_BETA] = s / old;
    }
  }
}

// Multi-rank second stage: sums nranks gathered local results in rank order.
// in[r*count + j] -> sc[out + j]
__global__ void rank_sum_kernel(const double *__restrict__ in, int nranks, int count,
                                double *__restrict__ sc, int out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < count) {
    double s = in[j];
    for (int r = 1; r < nranks; ++r) s = s + in[(int64_t)r * count + j];
    sc[out + j] = s;
  }
}

// h_j partials for j < count: partial[j*stride + b] = chunk sum of V_j . w
__global__ __launch_bounds__(kBlock) void multi_dot_partial_kernel(const double *__restrict__ V,
                                                                   int64_t vstride, int count,
                                                                   const double *__restrict__ w,
                                                                   double *__restrict__ partial,
                                                                   int64_t pstride) {
  __shared__ double lds[kMaxBasis + 2][4];
  double2 wr[8];
  const int64_t base = (int64_t)blockIdx.x * kChunk;
#pragma unroll
  for (int e = 0; e < 8; ++e) wr[e] = ld2(w, base + e * 512 + 2 * threadIdx.x);
  const int wave = threadIdx.x >> 6;
  for (int j = 0; j < count; ++j) {
    const double *v = V + (int64_t)j * vstride;
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const double2 a = ld2(v, base + e * 512 + 2 * threadIdx.x);
      acc = fma(a.x, wr[e].x, acc);
      acc = fma(a.y, wr[e].y, acc);
    }
    acc = group_reduce<64>(acc);
    if ((threadIdx.x & 63) == 0) lds[j][wave] = acc;
  }
  __syncthreads();
  if (threadIdx.x < count)
    partial[(int64_t)threadIdx.x * pstride + blockIdx.x] =
        (lds[threadIdx.x][0] + lds[threadIdx.x][1]) + (lds[threadIdx.x][2] + lds[threadIdx.x][3]);
}

// w = fma(-h_j, V_j, w) for j = 0..count-1 in order (h read from sc[hoff+j])
__global__ __launch_bounds__(kBlock) void multi_axpy_neg_kernel(const double *__restrict__ V,
                                                                int64_t vstride, int count,
                                                                const double *__restrict__ sc, int hoff,
                                                                double *__restrict__ w) {
  ALFD_FOR_PAIRS(i) {
    double2 a = ld2(w, i);
    for (int j = 0; j < count; ++j) {
      const double h = -sc[hoff + j];
      const double2 v = ld2(V + (int64_t)j * vstride, i);
      a.x = fma(h, v.x, a.x);
      a.y = fma(h, v.y, a.y);
    }
    st2(w, i, a);
  }
}

// x = fma(y_j, Z_j, x) for j in order, y on the host side -> passed via sc[hoff+j]
__global__ __launch_bounds__(kBlock) void multi_axpy_kernel(const double *__restrict__ Z, int64_t zstride,
                                                            int count, const double *__restrict__ sc,
                                                            int hoff, double *__restrict__ x) {
  ALFD_FOR_PAIRS(i) {
    double2 a = ld2(x, i);
    for (int j = 0; j < count; ++j) {
      const double h = sc[hoff + j];
      const double2 v = ld2(Z + (int64_t)j * zstride, i);
      a.x = fma(h, v.x, a.x);
      a.y = fma(h, v.y, a.y);
    }
    st2(x, i, a);
  }
}

// The element pair i, i + 1 of axpy_kernel, sub_from_kernel, cheb_init_kernel and cheb_step_kernel: the kernels below
// and ml_tail_kernel (one workgroup, its own loop over the pairs) call the same bodies => same bits.
__device__ __forceinline__ void axpy_pair(int64_t i, double a, const double *x, double *y) {
  const double2 xv = ld2(x, i);
  double2 yv = ld2(y, i);
  yv.x = fma(a, xv.x, yv.x);
  yv.y = fma(a, xv.y, yv.y);
  st2(y, i, yv);
}
__device__ __forceinline__ void sub_from_pair(int64_t i, const double *b, double *v) {
  const double2 bv = ld2(b, i);
  double2 vv = ld2(v, i);
  vv.x = bv.x - vv.x;
  vv.y = bv.y - vv.y;
  st2(v, i, vv);
}
__device__ __forceinline__ void cheb_init_pair(int64_t i, double inv_theta, const double *dinv, const double *r, double *d,
                                               double *z, double *res, int keep_res) {
  const double2 dv = ld2(dinv, i), rv = ld2(r, i);
  double2 o;
  o.x = inv_theta * (dv.x * rv.x);
  o.y = inv_theta * (dv.y * rv.y);
  st2(d, i, o);
  st2(z, i, o);
  if (keep_res) st2(res, i, rv);
}
__device__ __forceinline__ void cheb_step_pair(int64_t i, double c1, double c2, const double *dinv, const double *tmp,
                                               double *res, double *d, double *z) {
  const double2 dv = ld2(dinv, i), tv = ld2(tmp, i);
  double2 rv = ld2(res, i), dd = ld2(d, i), zv = ld2(z, i);
  rv.x = rv.x - tv.x;
  rv.y = rv.y - tv.y;
  dd.x = fma(c1, dd.x, c2 * (dv.x * rv.x));
  dd.y = fma(c1, dd.y, c2 * (dv.y * rv.y));
  zv.x = zv.x + dd.x;
  zv.y = zv.y + dd.y;
  st2(res, i, rv);
  st2(d, i, dd);
  st2(z, i, zv);
}

// y = fma(a, x, y); a = sc[ai] when sc != nullptr else aval
__global__ __launch_bounds__(kBlock) void axpy_kernel(const double *__restrict__ sc, int ai, double aval,
                                                      const double *__restrict__ x, double *__restrict__ y) {
  const double a = sc ? sc[ai] : aval;
  ALFD_FOR_PAIRS(i) axpy_pair(i, a, x, y);
}

// x *= a  (a = 1/sc[ai] when inv, for the Arnoldi normalisation v /= ||v||)
__global__ __launch_bounds__(kBlock) void scale_kernel(const double *__restrict__ sc, int ai, int inv_sqrt,
                                                       double aval, double *__restrict__ x) {
  double a = aval;
  if (sc) a = inv_sqrt ? 1.0 / sqrt(sc[ai]) : sc[ai];
  ALFD_FOR_PAIRS(i) {
    double2 v = ld2(x, i);
    v.x = a * v.x;
    v.y = a * v.y;
    st2(x, i, v);
  }
}

// y = a * x
__global__ __launch_bounds__(kBlock) void scale_copy_kernel(double a, const double *__restrict__ x,
                                                            double *__restrict__ y) {
  ALFD_FOR_PAIRS(i) {
    double2 v = ld2(x, i);
    v.x = a * v.x;
    v.y = a * v.y;
    st2(y, i, v);
  }
}

// v = b - v
__global__ __launch_bounds__(kBlock) void sub_from_kernel(const double *__restrict__ b,
                                                          double *__restrict__ v) {
  ALFD_FOR_PAIRS(i) sub_from_pair(i, b, v);
}

// y = a * (d .* x)          (v2 = -gamma invW u2, ...preconditioner.h:32,66)
__global__ __launch_bounds__(kBlock) void pmul_scale_kernel(double a, const double *__restrict__ d,
                                                            const double *__restrict__ x,
                                                            double *__restrict__ y) {
  ALFD_FOR_PAIRS(i) {
    const double2 dv = ld2(d, i), xv = ld2(x, i);
    double2 yv;
    yv.x = a * (dv.x * xv.x);
    yv.y = a * (dv.y * xv.y);
    st2(y, i, yv);
  }
}

// ---- PCG fused kernels (canonical dot partials come out of the same pass)
// z = d .* r ; partial = chunk sum of r.z            (Jacobi + r.z)
__global__ __launch_bounds__(kBlock) void jacobi_dot_kernel(const double *__restrict__ d,
                                                            const double *__restrict__ r,
                                                            double *__restrict__ z,
                                                            double *__restrict__ partial) {
  __shared__ double lds4[4];
  double acc = 0.0;
  ALFD_FOR_PAIRS(i) {
    const double2 dv = ld2(d, i), rv = ld2(r, i);
    double2 zv;
    zv.x = dv.x * rv.x;
    zv.y = dv.y * rv.y;
    st2(z, i, zv);
    acc = fma(rv.x, zv.x, acc);
    acc = fma(rv.y, zv.y, acc);
  }
  const double s = block_reduce_256(acc, lds4);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// p = fma(beta, p, z)  (first: p = z)
__global__ __launch_bounds__(kBlock) void p_update_kernel(const double *__restrict__ sc, int first,
                                                          const double *__restrict__ z,
                                                          double *__restrict__ p) {
  const double beta = first ? 0.0 : sc[S_BETA];
  ALFD_FOR_PAIRS(i) {
    const double2 zv = ld2(z, i);
    if (first) {
      st2(p, i, zv);
    } else {
      double2 pv = ld2(p, i);
      pv.x = fma(beta, pv.x, zv.x);
      pv.y = fma(beta, pv.y, zv.y);
      st2(p, i, pv);
    }
  }
}

// x = fma(alpha, p, x); r = fma(-alpha, Ap, r); partial = chunk sum of r.r
__global__ __launch_bounds__(kBlock) void xr_update_dot_kernel(const double *__restrict__ sc,
                                                               const double *__restrict__ p,
                                                               const double *__restrict__ Ap,
                                                               double *__restrict__ x,
                                                               double *__restrict__ r,
                                                               double *__restrict__ partial) {
  __shared__ double lds4[4];
  const double a = sc[S_ALPHA], na = sc[S_NALPHA];
  double acc = 0.0;
  ALFD_FOR_PAIRS(i) {
    const double2 pv = ld2(p, i), av = ld2(Ap, i);
    double2 xv = ld2(x, i), rv = ld2(r, i);
    xv.x = fma(a, pv.x, xv.x);
    xv.y = fma(a, pv.y, xv.y);
    rv.x = fma(na, av.x, rv.x);
    rv.y = fma(na, av.y, rv.y);
    st2(x, i, xv);
    st2(r, i, rv);
    acc = fma(rv.x, rv.x, acc);
    acc = fma(rv.y, rv.y, acc);
  }
  const double s = block_reduce_256(acc, lds4);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ---- Chebyshev (Saad Alg. 12.1, zero start) on D^-1 Aug
// d = inv_theta * (dinv .* r); z = d; res = r
__global__ __launch_bounds__(kBlock) void cheb_init_kernel(double inv_theta, const double *__restrict__ dinv,
                                                           const double *__restrict__ r,
                                                           double *__restrict__ d, double *__restrict__ z,
                                                           double *__restrict__ res, int keep_res) {
  ALFD_FOR_PAIRS(i) cheb_init_pair(i, inv_theta, dinv, r, d, z, res, keep_res);
}
// res -= tmp; d = fma(c1, d, c2 * (dinv .* res)); z += d
__global__ __launch_bounds__(kBlock) void cheb_step_kernel(double c1, double c2,
                                                           const double *__restrict__ dinv,
                                                           const double *__restrict__ tmp,
                                                           double *__restrict__ res, double *__restrict__ d,
                                                           double *__restrict__ z) {
  ALFD_FOR_PAIRS(i) cheb_step_pair(i, c1, c2, dinv, tmp, res, d, z);
}

// z = inv_theta * (dinv .* r): cheb_init_kernel without its two copies.  The fused sweep (aug_tail_kernel) reads
// the first direction back from z and the first residual from r itself.
__global__ __launch_bounds__(kBlock) void cheb_init_z_kernel(double inv_theta, const double *__restrict__ dinv,
                                                             const double *__restrict__ r, double *__restrict__ z) {
  ALFD_FOR_PAIRS(i) {
    const double2 dv = ld2(dinv, i), rv = ld2(r, i);
    double2 o;
    o.x = inv_theta * (dv.x * rv.x);
    o.y = inv_theta * (dv.y * rv.y);
    st2(z, i, o);
  }
}

// --------------------------------------------------------------------------
// Tail of a factored augmented operator y = A x + gamma Ct t, t = invW .* (C x): ONE launch forms
// y += gamma Ct t (the EPI 1 product of spmv_kernel) and the element-wise kernel that followed it.  The
// expressions are those of spmv_kernel, cheb_step_kernel, sub_from_kernel, cheb_init_kernel and axpy_kernel,
// each element goes through them in the same order => same bits as the separate launches.
//   TAIL_STEP           res = rin - y; d = fma(c1, din, c2 * (dinv .* res)); z += d      stores res, d, z
//   TAIL_LAST           the same                                                        stores z
//   TAIL_LAST_ADD       the same, then zout = fma(1, z, zout)                           stores zout
//   TAIL_RES            res = rin - y                                                   stores res
//   TAIL_RES_INIT       res = rin - y; z = c1 * (dinv .* res)   (c1 = 1 / theta)        stores z (res: store_res)
//   TAIL_RES_INIT_ADD   the same, then zout = fma(1, z, zout)                           stores zout
// rin / din / zin may be the arrays res / d / z themselves (every element is read and written by one thread only); zin is
// where the step modes read the iterate, z where they store it (the hosts of this file set zin = z unless a sweep
// ping-pongs the two, see cheb_fused in alfd.hip).
enum { TAIL_STEP = 0, TAIL_LAST = 1, TAIL_LAST_ADD = 2, TAIL_RES = 3, TAIL_RES_INIT = 4, TAIL_RES_INIT_ADD = 5 };
struct AugTailArgs {
  double gamma = 0, c1 = 0, c2 = 0;
  const double *dinv = nullptr, *y = nullptr, *rin = nullptr, *din = nullptr, *zin = nullptr;
  double *res = nullptr, *d = nullptr, *z = nullptr, *zout = nullptr;
  int store_res = 0;
};

template <int MODE>
__device__ __forceinline__ void aug_tail_math(const AugTailArgs &p, double y, double dinv, double rin, double din,
                                              double zin, double zo, double &res, double &d, double &z, double &zout) {
  res = rin - y;
  if (MODE <= TAIL_LAST_ADD) {
    d = fma(p.c1, din, p.c2 * (dinv * res));
    z = zin + d;
    if (MODE == TAIL_LAST_ADD) zout = fma(1.0, z, zo);
  } else if (MODE >= TAIL_RES_INIT) {
    z = p.c1 * (dinv * res);
    if (MODE == TAIL_RES_INIT_ADD) zout = fma(1.0, z, zo);
  }
}

// element i, whose operator value is y
template <int MODE>
__device__ __forceinline__ void aug_tail_elem(const AugTailArgs &p, int64_t i, double y) {
  constexpr bool kStep = MODE <= TAIL_LAST_ADD, kAdd = MODE == TAIL_LAST_ADD || MODE == TAIL_RES_INIT_ADD;
  const double dinv = MODE != TAIL_RES ? p.dinv[i] : 0.0, rin = p.rin[i];
  const double din = kStep ? p.din[i] : 0.0, zin = kStep ? p.zin[i] : 0.0, zo = kAdd ? p.zout[i] : 0.0;
  double res, d = 0.0, z = 0.0, zout = 0.0;
  aug_tail_math<MODE>(p, y, dinv, rin, din, zin, zo, res, d, z, zout);
  if (MODE == TAIL_STEP || MODE == TAIL_RES || (MODE == TAIL_RES_INIT && p.store_res)) p.res[i] = res;
  if (MODE == TAIL_STEP) p.d[i] = d;
  if (MODE == TAIL_STEP || MODE == TAIL_LAST || MODE == TAIL_RES_INIT) p.z[i] = z;
  if (kAdd) p.zout[i] = zout;
}

// Workgroups [0, nb_rows): the rows of Ct (n_list of them; rows[] lists them when Ct is in row-list form), L lanes
// per row as in spmv_kernel<L, 1, *>, lane 0 goes on with the element-wise tail of its row.
// Workgroups [nb_rows, nb_rows + npad / kChunk): the padded vector in the ALFD_FOR_PAIRS mapping; elements whose
// mask byte is set belong to the first party and are skipped (a row of Ct that is not listed is never touched by
// the separate product either: y_r stays the A x value).
template <int L, int MODE>
__global__ __launch_bounds__(kBlock) void aug_tail_kernel(int64_t n_list, const int64_t *__restrict__ rp,
                                                          const int32_t *__restrict__ col,
                                                          const double *__restrict__ val,
                                                          const int32_t *__restrict__ rows,
                                                          const double *__restrict__ t, int nb_rows,
                                                          const uint8_t *__restrict__ mask, AugTailArgs p) {
  if ((int)blockIdx.x < nb_rows) {
    constexpr int RPB = kBlock / L;
    const int lane = threadIdx.x % L;
    const int sub = threadIdx.x / L;
    const int64_t ngroups = (n_list + RPB - 1) / RPB;
    for (int64_t g = blockIdx.x; g < ngroups; g += nb_rows) {
      const int64_t r = g * RPB + sub;
      if (r < n_list) {  // uniform within the L-lane group
        const int64_t k0 = rp[r], k1 = rp[r + 1];
        double acc = 0.0;
        for (int64_t k = k0 + lane; k < k1; k += L) acc = fma(val[k], t[col[k]], acc);
        acc = group_reduce<L>(acc);
        if (lane == 0) {
          const int64_t ro = rows ? (int64_t)rows[r] : r;
          aug_tail_elem<MODE>(p, ro, fma(p.gamma, acc, p.y[ro]));
        }
      }
    }
    return;
  }
  constexpr bool kStep = MODE <= TAIL_LAST_ADD, kAdd = MODE == TAIL_LAST_ADD || MODE == TAIL_RES_INIT_ADD;
  const int64_t base = (int64_t)((int)blockIdx.x - nb_rows) * kChunk;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int64_t i = base + e * 512 + 2 * threadIdx.x;
    const uchar2 mk = *reinterpret_cast<const uchar2 *>(mask + i);
    if (mk.x | mk.y) {
      if (!mk.x) aug_tail_elem<MODE>(p, i, p.y[i]);
      if (!mk.y) aug_tail_elem<MODE>(p, i + 1, p.y[i + 1]);
      continue;
    }
    const double2 zero = {0.0, 0.0};
    const double2 yv = ld2(p.y, i), rv = ld2(p.rin, i);
    const double2 dv = MODE != TAIL_RES ? ld2(p.dinv, i) : zero;
    const double2 dd = kStep ? ld2(p.din, i) : zero, zi = kStep ? ld2(p.zin, i) : zero;
    const double2 zo = kAdd ? ld2(p.zout, i) : zero;
    double2 res, d = zero, z = zero, zout = zero;
    aug_tail_math<MODE>(p, yv.x, dv.x, rv.x, dd.x, zi.x, zo.x, res.x, d.x, z.x, zout.x);
    aug_tail_math<MODE>(p, yv.y, dv.y, rv.y, dd.y, zi.y, zo.y, res.y, d.y, z.y, zout.y);
    if (MODE == TAIL_STEP || MODE == TAIL_RES || (MODE == TAIL_RES_INIT && p.store_res)) st2(p.res, i, res);
    if (MODE == TAIL_STEP) st2(p.d, i, d);
    if (MODE == TAIL_STEP || MODE == TAIL_LAST || MODE == TAIL_RES_INIT) st2(p.z, i, z);
    if (kAdd) st2(p.zout, i, zout);
  }
}

// mask[row] = 1 for the rows aug_tail_kernel's first party owns
__global__ void mark_rows_kernel(int64_t n_list, const int32_t *__restrict__ rows, uint8_t *__restrict__ mask) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_list) mask[rows ? (int64_t)rows[i] : i] = 1;
}

// --------------------------------------------------------------------------
// The coarse tail of the V-cycle of the immersed hierarchy in ONE launch ("ml_tail_rows"): one
// workgroup of kTailBlock threads runs ml_cycle for the levels first .. nlev - 1 from a table of level descriptors,
// with __syncthreads() where the launches were.  Row sums: L lanes per row, fma over k0 + lane, k0 + lane + L, ..,
// group_reduce<L> -- spmv_kernel's; element-wise steps: the *_pair bodies above.  Every element keeps its arithmetic
// and order => the bits of the launch-per-step path (fused or not: those two agree already).
// The vectors are written and read back by other threads of the workgroup inside the kernel: plain pointers, neither
// const nor __restrict__ (those would license scalar-cache / non-coherent loads of data this kernel stored).
constexpr int kTailBlock = 1024;
constexpr int kTailMaxDegree = 64;   // Chebyshev steps whose coefficients a level descriptor holds
constexpr int kTailMaxLevels = 9;    // ALFD_MAX_LEVELS + 1
struct TailCsr {
  const int64_t *rp;
  const int32_t *col;
  const double *val;
  const int32_t *rows;   // the listed rows when sparse
  int64_t n_list, nrows;
  int32_t L, sparse;
};
struct TailLevel {
  TailCsr A, C, Ct;   // Aug = A + gamma Ct diag(w) C of this level
  TailCsr R, P;       // to / from the next coarser level (unused on the last)
  const double *dinv, *w;
  double *tlam, *r, *z, *t, *cd, *cres, *ctmp;
  double gamma, inv_theta;   // 1 / theta of this level's sweep (the coarsest sweep on the last level)
  int64_t npad;
  int32_t degree, pad_;
  double c1[kTailMaxDegree], c2[kTailMaxDegree];   // ChebCoef::step() in order, computed on the host
};
struct TailTable {
  int32_t nlev, has_inv;
  TailCsr inv;   // explicit inverse of the coarsest operator
  TailLevel lev[kTailMaxLevels];
};

template <int L>
__device__ __forceinline__ void tail_rows(const TailCsr &m, const double *x, double *y, int epi, double alpha,
                                          const double *d) {
  constexpr int RPB = kTailBlock / L;
  const int lane = threadIdx.x % L;
  const int sub = threadIdx.x / L;
  const int64_t ngroups = (m.n_list + RPB - 1) / RPB;
  for (int64_t g = 0; g < ngroups; ++g) {
    const int64_t r = g * RPB + sub;
    if (r < m.n_list) {  // uniform within the L-lane group
      const int64_t k0 = m.rp[r], k1 = m.rp[r + 1];
      double acc = 0.0;
      for (int64_t k = k0 + lane; k < k1; k += L) acc = fma(m.val[k], x[m.col[k]], acc);
      acc = group_reduce<L>(acc);
      if (lane == 0) {
        const int64_t ro = m.sparse ? (int64_t)m.rows[r] : r;
        if (epi == 0)
          y[ro] = acc;
        else if (epi == 1)
          y[ro] = fma(alpha, acc, y[ro]);
        else
          y[ro] = d[ro] * acc;
      }
    }
  }
}

// spmv_m(m, x, y, epi, alpha, d) on one rank, epi 0 / 1 / 2, and the boundary after it
__device__ __forceinline__ void tail_spmv(const TailCsr &m, const double *x, double *y, int epi, double alpha,
                                          const double *d) {
  if (m.sparse && epi != 1) {   // rows outside the list are structurally empty: their result is 0
    for (int64_t i = threadIdx.x; i < m.nrows; i += kTailBlock) y[i] = 0.0;
    __syncthreads();
  }
  switch (m.L) {   // as spmv_launch_local
    case 4: tail_rows<4>(m, x, y, epi, alpha, d); break;
    case 8: tail_rows<8>(m, x, y, epi, alpha, d); break;
    case 16: tail_rows<16>(m, x, y, epi, alpha, d); break;
    case 32: tail_rows<32>(m, x, y, epi, alpha, d); break;
    default: tail_rows<64>(m, x, y, epi, alpha, d); break;
  }
  __syncthreads();
}

// y = Aug x of a level: the three products of aug_apply
__device__ __forceinline__ void tail_aug(const TailLevel &F, const double *x, double *y) {
  tail_spmv(F.A, x, y, 0, 0.0, nullptr);
  tail_spmv(F.C, x, F.tlam, 2, 0.0, F.w);
  tail_spmv(F.Ct, F.tlam, y, 1, F.gamma, nullptr);
}

#define ALFD_TAIL_PAIRS(i, npad) for (int64_t i = 2 * (int64_t)threadIdx.x; i < (npad); i += 2 * kTailBlock)

// t = r - Aug z
__device__ __forceinline__ void tail_residual(const TailLevel &F, const double *r, const double *z, double *t) {
  tail_aug(F, z, t);
  ALFD_TAIL_PAIRS(i, F.npad) sub_from_pair(i, r, t);
  __syncthreads();
}

__global__ __launch_bounds__(kTailBlock) void ml_tail_kernel(const TailTable *__restrict__ tab, int first) {
  const int nl = tab->nlev - first;   // levels of the tail; steps: nl - 1 down, the coarsest, nl - 1 up
  for (int s = 0; s < 2 * nl - 1; ++s) {
    const bool up = s > nl - 1, coarsest = s == nl - 1;
    const int l = first + (up ? 2 * nl - 2 - s : s);
    const TailLevel &F = tab->lev[l];
    if (up) {
      tail_spmv(F.P, tab->lev[l + 1].z, F.z, 1, 1.0, nullptr);   // z += P e_c
      tail_residual(F, F.r, F.z, F.t);
    } else if (coarsest && tab->has_inv) {
      tail_spmv(tab->inv, F.r, F.z, 0, 0.0, nullptr);            // z = Aug_c^-1 r
      continue;
    }
    // cheb_sweep: down and on the coarsest level z = q(r); up the correction F.r = q(t), then z += F.r
    const double *src = up ? F.t : F.r;
    double *dst = up ? F.r : F.z;
    ALFD_TAIL_PAIRS(i, F.npad) cheb_init_pair(i, F.inv_theta, F.dinv, src, F.cd, dst, F.cres, F.degree > 1 ? 1 : 0);
    __syncthreads();
    for (int j = 1; j < F.degree; ++j) {
      tail_aug(F, F.cd, F.ctmp);
      const double c1 = F.c1[j - 1], c2 = F.c2[j - 1];
      ALFD_TAIL_PAIRS(i, F.npad) cheb_step_pair(i, c1, c2, F.dinv, F.ctmp, F.cres, F.cd, dst);
      __syncthreads();
    }
    if (up) {
      ALFD_TAIL_PAIRS(i, F.npad) axpy_pair(i, 1.0, F.r, F.z);
      __syncthreads();
    } else if (!coarsest) {
      tail_residual(F, F.r, F.z, F.t);
      tail_spmv(F.R, F.t, tab->lev[l + 1].r, 0, 0.0, nullptr);   // r_c = P^T t
    }
  }
}
#undef ALFD_TAIL_PAIRS

// ---- batched lock-step CG (RationalPreconditioner: 21 independent SPD solves on
// the immersed matrices, rational_preconditioner.h:41-56).  All systems advance
// together, one workgroup-chunk per 4096 entries; segment s owns chunks
// [s*cps, (s+1)*cps) and its own scalar row scb[s*kBS ..].  A system that has
// met its stop rule is frozen (active flag 0): its x, r, p are never touched
// again, so every system performs exactly the arithmetic of a stand-alone CG.
constexpr int kBS = 8;  // scalars per system: RZ, RZ_OLD, PAP, ALPHA, NALPHA, BETA, RR, ACTIVE
enum { B_RZ = 0, B_RZ_OLD = 1, B_PAP = 2, B_ALPHA = 3, B_NALPHA = 4, B_BETA = 5, B_RR = 6, B_ACTIVE = 7 };

__global__ __launch_bounds__(kBlock) void b_jacobi_dot_kernel(const double *__restrict__ scb, int cps,
                                                              const double *__restrict__ d,
                                                              const double *__restrict__ r,
                                                              double *__restrict__ z,
                                                              double *__restrict__ partial) {
  __shared__ double lds4[4];
  const int seg = blockIdx.x / cps;
  if (scb[seg * kBS + B_ACTIVE] == 0.0) return;
  double acc = 0.0;
  ALFD_FOR_PAIRS(i) {
    const double2 dv = ld2(d, i), rv = ld2(r, i);
    double2 zv;
    zv.x = dv.x * rv.x;
    zv.y = dv.y * rv.y;
    st2(z, i, zv);
    acc = fma(rv.x, zv.x, acc);
    acc = fma(rv.y, zv.y, acc);
  }
  const double sum = block_reduce_256(acc, lds4);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// one workgroup per system: reduce its cps chunk partials, then the CG scalar update
__global__ __launch_bounds__(kBlock) void b_final_kernel(const double *__restrict__ partial, int cps,
                                                         double *__restrict__ scb, int fin) {
  __shared__ double lds4[4];
  const int seg = blockIdx.x;
  double *sc = scb + seg * kBS;
  if (sc[B_ACTIVE] == 0.0) return;
  const double *p = partial + (int64_t)seg * cps;
  double acc = 0.0;
  for (int i = threadIdx.x; i < cps; i += kBlock) acc = acc + p[i];
  const double s = block_reduce_256(acc, lds4);
  if (threadIdx.x == 0) {
    if (fin == FIN_STORE) {
      sc[B_RR] = s;
    } else if (fin == FIN_ALPHA) {
      sc[B_PAP] = s;
      const double a = sc[B_RZ] / s;
      sc[B_ALPHA] = a;
      sc[B_NALPHA] = -a;
    } else {
      const double old = sc[B_RZ];
      sc[B_RZ_OLD] = old;
      sc[B_RZ] = s;
      sc[B_BETA] = s / old;
    }
  }
}

__global__ __launch_bounds__(kBlock) void b_p_update_kernel(const double *__restrict__ scb, int cps, int first,
                                                            const double *__restrict__ z,
                                                            double *__restrict__ p) {
  const int seg = blockIdx.x / cps;
  if (scb[seg * kBS + B_ACTIVE] == 0.0) return;
  const double beta = first ? 0.0 : scb[seg * kBS + B_BETA];
  ALFD_FOR_PAIRS(i) {
    const double2 zv = ld2(z, i);
    if (first) {
      st2(p, i, zv);
    } else {
      double2 pv = ld2(p, i);
      pv.x = fma(beta, pv.x, zv.x);
      pv.y = fma(beta, pv.y, zv.y);
      st2(p, i, pv);
    }
  }
}

__global__ __launch_bounds__(kBlock) void b_xr_update_dot_kernel(const double *__restrict__ scb, int cps,
                                                                 const double *__restrict__ p,
                                                                 const double *__restrict__ Ap,
                                                                 double *__restrict__ x,
                                                                 double *__restrict__ r,
                                                                 double *__restrict__ partial) {
  __shared__ double lds4[4];
  const int seg = blockIdx.x / cps;
  if (scb[seg * kBS + B_ACTIVE] == 0.0) return;
  const double a = scb[seg * kBS + B_ALPHA], na = scb[seg * kBS + B_NALPHA];
  double acc = 0.0;
  ALFD_FOR_PAIRS(i) {
    const double2 pv = ld2(p, i), av = ld2(Ap, i);
    double2 xv = ld2(x, i), rv = ld2(r, i);
    xv.x = fma(a, pv.x, xv.x);
    xv.y = fma(a, pv.y, xv.y);
    rv.x = fma(na, av.x, rv.x);
    rv.y = fma(na, av.y, rv.y);
    st2(x, i, xv);
    st2(r, i, rv);
    acc = fma(rv.x, rv.x, acc);
    acc = fma(rv.y, rv.y, acc);
  }
  const double s = block_reduce_256(acc, lds4);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// r_s = b for every system s (one padded copy of the rhs per segment)
__global__ __launch_bounds__(kBlock) void b_replicate_kernel(int cps, const double *__restrict__ b,
                                                             double *__restrict__ r) {
  const int64_t lbase = (int64_t)(blockIdx.x % cps) * kChunk;
  const int64_t gbase = (int64_t)blockIdx.x * kChunk;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int64_t o = e * 512 + 2 * threadIdx.x;
    st2(r, gbase + o, ld2(b, lbase + o));
  }
}

// out = sum_s coef[s] * X_s, accumulated s = 0..nseg-1 as out = out + coef*x
// (rational_preconditioner.h:59-62)
__global__ __launch_bounds__(kBlock) void b_combine_kernel(int nseg, int64_t seglen,
                                                           const double *__restrict__ coef,
                                                           const double *__restrict__ X,
                                                           double *__restrict__ out) {
  ALFD_FOR_PAIRS(i) {
    double2 a;
    a.x = 0.0;
    a.y = 0.0;
    for (int s = 0; s < nseg; ++s) {
      const double c = coef[s];
      const double2 v = ld2(X + (int64_t)s * seglen, i);
      a.x = a.x + c * v.x;
      a.y = a.y + c * v.y;
    }
    st2(out, i, a);
  }
}

// out = fl32(val), entry by entry (alfd_set_preconditioner_values): round to nearest even; an image below the smallest
// normal binary32 is stored as a zero with the sign of the entry.  The cases are decided by compares on the double, so
// the denormal mode of the conversion instruction never matters:
//   |a| <  (1 - 2^-24) 2^-126   the image is zero or subnormal (the tie at the bound goes to the even 2^-126);
//   |a| >  2^-150               ... and not zero (the tie at 2^-150 goes to the even 0): counts[0], "flushed to zero";
//   |a| >= (2 - 2^-24) 2^127    or a not finite: no finite image (the tie goes to the even infinity): counts[1].
__global__ __launch_bounds__(256) void round_values_kernel(int64_t nnz, const double *__restrict__ val,
                                                           float *__restrict__ out,
                                                           unsigned long long *__restrict__ counts) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  unsigned int flushed = 0, bad = 0;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nnz; k += stride) {
    const double a = val[k], m = fabs(a);
    float f = (float)a;
    if (m < 0x1.fffffep-127) {
      f = signbit(a) ? -0.0f : 0.0f;
      flushed += m > 0x1p-150 ? 1u : 0u;
    }
    if (!(m < 0x1.ffffffp127)) {
      f = 0.0f;
      bad += 1u;
    }
    out[k] = f;
  }
  for (int o = 32; o > 0; o >>= 1) {
    flushed += __shfl_xor(flushed, o, 64);
    bad += __shfl_xor(bad, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (flushed) atomicAdd(&counts[0], (unsigned long long)flushed);
    if (bad) atomicAdd(&counts[1], (unsigned long long)bad);
  }
}

// dinv[i] = 1 / dA[i] (rows < n)
__global__ void inv_diag_kernel(int64_t n, const double *__restrict__ dA, double *__restrict__ dinv) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dinv[i] = 1.0 / dA[i];
}

// ---- setup kernels
// dA[r] = A_rr (exact copy, no arithmetic); diag column = r + row_offset, and
// locally that is column (r) when the matrix's local columns come first.
template <int L>
__global__ __launch_bounds__(kBlock) void extract_diag_kernel(int64_t nrows, const int64_t *__restrict__ rp,
                                                              const int32_t *__restrict__ col,
                                                              const double *__restrict__ val,
                                                              double *__restrict__ dA) {
  constexpr int RPB = kBlock / L;
  const int lane = threadIdx.x % L, sub = threadIdx.x / L;
  const int64_t ngroups = (nrows + RPB - 1) / RPB;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t r = g * RPB + sub;
    if (r < nrows)
      for (int64_t k = rp[r] + lane; k < rp[r + 1]; k += L)
        if (col[k] == (int32_t)r) dA[r] = val[k];
  }
}
// dinv[i] = 1 / fma(gamma, s_i, dA[i]), s_i = sequential fma over row i of Ct of
// (w[c] * v) * v ; one thread per non-empty row of Ct; other rows: 1/dA.
__global__ void aug_diag_rows_kernel(int64_t n_sr, const int64_t *__restrict__ rp,
                                     const int32_t *__restrict__ col, const double *__restrict__ val,
                                     const int32_t *__restrict__ rows, const double *__restrict__ w,
                                     const double *__restrict__ w_halo, int32_t n_local,
                                     double *__restrict__ s_out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n_sr) {
    double s = 0.0;
    for (int64_t k = rp[r]; k < rp[r + 1]; ++k) {
      const int32_t c = col[k];
      const double wv = c < n_local ? w[c] : w_halo[c - n_local];
      s = fma(wv * val[k], val[k], s);
    }
    s_out[rows ? rows[r] : r] = s;
  }
}
// invert = 0: dinv[i] = fma(gamma, s_i, dA[i]) itself (dinv may be dA), for a further term
__global__ void aug_diag_finish_kernel(int64_t n, double gamma, const double *dA, const double *__restrict__ s,
                                       double *dinv, int invert) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const double d = fma(gamma, s[i], dA[i]);
    dinv[i] = invert ? 1.0 / d : d;
  }
}
// power-iteration start vector: v_i = 1 + ((g*2654435761) & 1023)/1024, g = global index
__global__ void hash_vector_kernel(int64_t n, int64_t goff, double *__restrict__ v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    v[i] = 1.0 + (double)(((uint64_t)(i + goff) * 2654435761ull) & 1023ull) * (1.0 / 1024.0);
}

// gather x[idx[i]] -> out[i]   (halo send packing)
__global__ void gather_kernel(int64_t n, const int32_t *__restrict__ idx, const double *__restrict__ x,
                              double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = x[idx[i]];
}

// out[idx[i]] += x[i]   (interface-patch corrections: idx lists distinct rows)
__global__ void scatter_add_kernel(int64_t n, const int32_t *__restrict__ idx, const double *__restrict__ x,
                                   double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[idx[i]] = out[idx[i]] + x[i];
}

// ---------------------------------------------------------------------------------------------------
// Sparse product C = A * P on the device, one 64-lane workgroup per output row (the Galerkin products of the multigrid
// setup: A P, then P^T (A P), and C P).  Deterministic and equal bit for bit to the host / oracle definition: every
// output entry (i, J) is ONE sequential fma chain over the entries k of row i of A in CSR order and the entries of row
// col_k of P in CSR order, acc = fma(a_ik, p_kJ, acc) from 0; the row comes out sorted by column.
//   pass 0 (symbolic): counts[i] = number of distinct columns of row i (LDS hash set of the candidates)
//   pass 1 (numeric):  the same set, compacted and sorted in LDS (bitonic), then lane t owns output column t and walks
//                      the row of A once, looking its column up in every P row it meets (wave-uniform control flow,
//                      broadcast loads).
// kSgTable slots per hash set, at most kSgMaxOut distinct columns per row (overflow[0] is set otherwise: the host falls
// back to its own product).
constexpr int kSgTable = 4096;
constexpr int kSgMaxOut = 1024;
__global__ __launch_bounds__(64) void spgemm_rows_kernel(int64_t nrows, const int64_t *__restrict__ arp,
                                                         const int32_t *__restrict__ acol, const double *__restrict__ aval,
                                                         const int64_t *__restrict__ prp, const int32_t *__restrict__ pcol,
                                                         const double *__restrict__ pval, int pass,
                                                         int32_t *__restrict__ counts, const int64_t *__restrict__ crp,
                                                         int32_t *__restrict__ ccol, double *__restrict__ cval,
                                                         int32_t *__restrict__ overflow) {
  __shared__ int32_t table[kSgTable];
  __shared__ int32_t keys[kSgMaxOut];
  __shared__ int32_t cnt;
  const int lane = threadIdx.x;
  for (int64_t i = blockIdx.x; i < nrows; i += gridDim.x) {
    const int64_t k0 = arp[i], k1 = arp[i + 1];
    if (k0 == k1) {
      if (pass == 0 && lane == 0) counts[i] = 0;
      continue;
    }
    for (int s = lane; s < kSgTable; s += 64) table[s] = -1;
    if (lane == 0) cnt = 0;
    __syncthreads();
    for (int64_t k = k0 + lane; k < k1; k += 64) {
      const int64_t j = acol[k];
      for (int64_t e = prp[j]; e < prp[j + 1]; ++e) {
        const int32_t J = pcol[e];
        uint32_t h = ((uint32_t)J * 2654435761u) >> 20;   // 12 bits
        for (;;) {
          const int32_t old = atomicCAS(&table[h], -1, J);
          if (old == -1) {
            atomicAdd(&cnt, 1);
            break;
          }
          if (old == J) break;
          h = (h + 1) & (kSgTable - 1);
          if (*(volatile int32_t *)&cnt > kSgMaxOut) break;   // overflowing row: stop probing (reported below)
        }
      }
    }
    __syncthreads();
    const int n = cnt;
    if (n > kSgMaxOut) {
      if (lane == 0) overflow[0] = 1;
      if (pass == 0 && lane == 0) counts[i] = 0;
      __syncthreads();
      continue;
    }
    if (pass == 0) {
      if (lane == 0) counts[i] = n;
      __syncthreads();
      continue;
    }
    // compact, pad to a power of two with INT_MAX, bitonic sort
    int n2 = 64;
    while (n2 < n) n2 <<= 1;
    __syncthreads();
    if (lane == 0) cnt = 0;
    __syncthreads();
    for (int s = lane; s < kSgTable; s += 64) {
      const int32_t J = table[s];
      if (J != -1) keys[atomicAdd(&cnt, 1)] = J;
    }
    __syncthreads();
    for (int s = n + lane; s < n2; s += 64) keys[s] = 0x7fffffff;
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int t = lane; t < n2 / 2; t += 64) {
          const int lo = 2 * t - (t & (stride - 1));
          const int hi = lo + stride;
          const bool up = (lo & size) == 0;
          const int32_t a = keys[lo], b = keys[hi];
          if ((a > b) == up) {
            keys[lo] = b;
            keys[hi] = a;
          }
        }
        __syncthreads();
      }
    // numeric: lane t owns output column keys[t]
    const int64_t c0 = crp[i];
    for (int t0 = 0; t0 < n; t0 += 64) {
      const int t = t0 + lane;
      const int32_t J = t < n ? keys[t] : -2;
      double acc = 0.0;
      for (int64_t k = k0; k < k1; ++k) {
        const int64_t j = acol[k];
        const double a = aval[k];
        const int64_t e1 = prp[j + 1];
        for (int64_t e = prp[j]; e < e1; ++e)
          if (pcol[e] == J) acc = fma(a, pval[e], acc);
      }
      if (t < n) {
        ccol[c0 + t] = J;
        cval[c0 + t] = acc;
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------
// The node graph of the algebraic aggregation (alfd_build_strength_graph) from the RESIDENT rows of A, so that a
// row-partitioned context forms the graph rows of its own nodes without downloading A.  The rows are the local ones
// (n_nodes * bs of them, the first is global row node0 * bs); a column c is local: owned (c < nlc, global id c0 + c)
// or a halo column (global id halo_g[c - nlc]); on one rank nlc = ncols, c0 = 0 and halo_g is never read.
//   sa_node_diag_kernel (one thread per node): d_I = max |a_ii| over the node's rows, fixed_I = 1 when the node's
//   rows hold nothing but their diagonals (explicit zeros do not count) -- node_diag_host.
//   sa_node_graph_kernel (one 64-lane workgroup per node, two passes as sa_prolongator_kernel): the neighbour nodes
//   J != I, not fixed, with w_IJ = max |a_ij| > 0 go into an LDS hash set whose value is the running maximum (the
//   bit pattern of a positive double orders like the double, so the maximum is an integer atomicMax); J is strong
//   when w_IJ >= theta * sqrt(d_I d_J) with d / fixed of ALL nn nodes (all-gathered).  Pass 0 counts the strong
//   neighbours, pass 1 sorts them ascending and writes (J, w_IJ).  max, fabs, one product, one correctly rounded
//   sqrt and one comparison: the bits of node_graph_host.  More than kNgMaxOut distinct neighbour nodes:
//   overflow[0] is set and the host forms the graph.  LDS: 26 KiB per workgroup.
constexpr int kNgTable = 2048;
constexpr int kNgMaxOut = 512;
__global__ __launch_bounds__(256) void sa_node_diag_kernel(
    int64_t n_nodes, int bs, int64_t node0, const int64_t *__restrict__ arp, const int32_t *__restrict__ acol,
    const double *__restrict__ aval, int32_t nlc, int64_t c0, const int32_t *__restrict__ halo_g,
    double *__restrict__ d, int32_t *__restrict__ fixed) {
  const int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (I >= n_nodes) return;
  double dm = 0.0;
  int32_t fx = 1;
  for (int64_t i = I * bs; i < (I + 1) * bs; ++i) {
    const int64_t gi = node0 * bs + i;
    for (int64_t k = arp[i]; k < arp[i + 1]; ++k) {
      const int32_t c = acol[k];
      const int64_t g = c < nlc ? c0 + c : (int64_t)halo_g[c - nlc];
      if (g == gi) dm = fmax(dm, fabs(aval[k]));
      else if (aval[k] != 0.0) fx = 0;
    }
  }
  d[I] = dm;
  fixed[I] = fx;
}

__global__ __launch_bounds__(64) void sa_node_graph_kernel(
    int64_t n_nodes, int64_t node0, int64_t nn, int bs, double theta, const int64_t *__restrict__ arp,
    const int32_t *__restrict__ acol, const double *__restrict__ aval, int32_t nlc, int64_t c0,
    const int32_t *__restrict__ halo_g, const double *__restrict__ d, const int32_t *__restrict__ fixed, int pass,
    int32_t *__restrict__ counts, const int64_t *__restrict__ gp, int32_t *__restrict__ gc, double *__restrict__ gw,
    int32_t *__restrict__ overflow) {
  __shared__ int32_t table[kNgTable];
  __shared__ unsigned long long tw[kNgTable];
  __shared__ int32_t keys[kNgMaxOut];
  __shared__ int32_t cnt;
  const int lane = threadIdx.x;
  for (int64_t Il = blockIdx.x; Il < n_nodes; Il += gridDim.x) {
    const int64_t I = node0 + Il;
    if (fixed[I]) {
      if (pass == 0 && lane == 0) counts[Il] = 0;
      continue;
    }
    for (int s = lane; s < kNgTable; s += 64) {
      table[s] = -1;
      tw[s] = 0ull;
    }
    if (lane == 0) cnt = 0;
    __syncthreads();
    const int64_t k0 = arp[Il * bs], k1 = arp[(Il + 1) * bs];   // the node's rows are consecutive
    for (int64_t k = k0 + lane; k < k1; k += 64) {
      const int32_t c = acol[k];
      const int64_t g = c < nlc ? c0 + c : (int64_t)halo_g[c - nlc];
      const int64_t Jl = g / bs;
      if (Jl == I || Jl >= nn || fixed[Jl]) continue;
      const double v = fabs(aval[k]);
      if (v == 0.0) continue;
      const int32_t J = (int32_t)Jl;
      const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
      uint32_t h = ((uint32_t)J * 2654435761u) >> 21;   // 11 bits
      for (;;) {
        if (*(volatile int32_t *)&cnt > kNgMaxOut) break;   // overflowing node: stop inserting (reported below)
        const int32_t old = atomicCAS(&table[h], -1, J);
        if (old == -1) atomicAdd(&cnt, 1);
        if (old == -1 || old == J) {
          atomicMax(&tw[h], bits);
          break;
        }
        h = (h + 1) & (kNgTable - 1);
      }
    }
    __syncthreads();
    const int nd = cnt;
    __syncthreads();
    if (nd > kNgMaxOut) {
      if (lane == 0) overflow[0] = 1;
      if (pass == 0 && lane == 0) counts[Il] = 0;
      continue;
    }
    // the strong ones among the nd distinct neighbours
    if (lane == 0) cnt = 0;
    __syncthreads();
    const double dI = d[I];
    for (int s = lane; s < kNgTable; s += 64) {
      const int32_t J = table[s];
      if (J == -1) continue;
      const double w = __longlong_as_double((long long)tw[s]);
      if (w >= theta * sqrt(dI * d[J])) {
        const int at = atomicAdd(&cnt, 1);
        if (pass == 1) keys[at] = J;
      }
    }
    __syncthreads();
    const int n = cnt;
    if (pass == 0) {
      if (lane == 0) counts[Il] = n;
      __syncthreads();
      continue;
    }
    // pad to a power of two with INT_MAX, bitonic sort (n2 <= kNgMaxOut)
    int n2 = 64;
    while (n2 < n) n2 <<= 1;
    for (int s = n + lane; s < n2; s += 64) keys[s] = 0x7fffffff;
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int t = lane; t < n2 / 2; t += 64) {
          const int lo = 2 * t - (t & (stride - 1));
          const int hi = lo + stride;
          const bool up = (lo & size) == 0;
          const int32_t a = keys[lo], b = keys[hi];
          if ((a > b) == up) {
            keys[lo] = b;
            keys[hi] = a;
          }
        }
        __syncthreads();
      }
    const int64_t e0 = gp[Il];
    for (int t = lane; t < n; t += 64) {
      const int32_t J = keys[t];
      uint32_t h = ((uint32_t)J * 2654435761u) >> 21;
      while (table[h] != J) h = (h + 1) & (kNgTable - 1);   // J is in the table
      gc[e0 + t] = J;
      gw[e0 + t] = __longlong_as_double((long long)tw[h]);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------
// The build-time kernels of alfd_build_smoothed_aggregation on a row-partitioned context.  A partitioned matrix keeps
// every row in the order it was uploaded in (ascending GLOBAL columns) and only renames the columns to local ids
// [owned | halo]; the chains of the builder run in global CSR order, so a view of the resident rows needs new column
// ids and nothing else.
//   sa_global_cols_kernel: out[k] = shift + the global id of col[k].  With shift = the number of local rows and the
//     aggregate array laid out as [agg of the own rows | agg of all unknowns], sa_prolongator_kernel and
//     sa_truncated_prolongator_kernel run unchanged on the view (agg[i] is the row's own id, agg[col] a column's).
//   sa_diag_rows_kernel (one thread per row): d_i = fma(gamma, s_i, a_ii), s_i the sequential fma of (w_k c_ik) c_ik
//     over row i of Ct (global multiplier ids; ctrp == nullptr: a_ii alone) -- the bits of sa_diag.
//   sa_power_t_kernel (one thread per row of the REPLICATED C): t_k = w_k * (sequential fma of c_kj v_j over row k).
//   sa_power_rows_kernel (one thread per row): y_i = (A v + gamma Ct t)_i / d_i, each product one sequential fma chain
//     from 0.0 in CSR order -- the per-row chains of sa_spmv_host, which the 64-lane partial sums of the SpMV kernels
//     are not.  v is the whole (replicated) vector, cols carry `shift`.
__global__ __launch_bounds__(256) void sa_global_cols_kernel(int64_t nnz, const int32_t *__restrict__ col, int32_t nlc,
                                                             int64_t c0, const int32_t *__restrict__ halo_g, int64_t shift,
                                                             int32_t *__restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nnz) return;
  const int32_t c = col[k];
  out[k] = (int32_t)(shift + (c < nlc ? c0 + c : (int64_t)halo_g[c - nlc]));
}

__global__ __launch_bounds__(256) void sa_diag_rows_kernel(
    int64_t nrows, int64_t row0, int64_t shift, const int64_t *__restrict__ arp, const int32_t *__restrict__ acol,
    const double *__restrict__ aval, const int64_t *__restrict__ ctrp, const int32_t *__restrict__ ctcol,
    const double *__restrict__ ctval, const double *__restrict__ w, double gamma, double *__restrict__ d) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrows) return;
  double di = 0.0;
  for (int64_t k = arp[i]; k < arp[i + 1]; ++k)
    if ((int64_t)acol[k] - shift == row0 + i) di = aval[k];
  if (ctrp) {
    double s = 0.0;
    for (int64_t k = ctrp[i]; k < ctrp[i + 1]; ++k) s = fma(w[ctcol[k]] * ctval[k], ctval[k], s);
    di = fma(gamma, s, di);
  }
  d[i] = di;
}

__global__ __launch_bounds__(256) void sa_power_t_kernel(int64_t m, const int64_t *__restrict__ crp,
                                                         const int32_t *__restrict__ ccol, const double *__restrict__ cval,
                                                         const double *__restrict__ w, const double *__restrict__ v,
                                                         double *__restrict__ t) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  double s = 0.0;
  for (int64_t k = crp[r]; k < crp[r + 1]; ++k) s = fma(cval[k], v[ccol[k]], s);
  t[r] = w[r] * s;
}

__global__ __launch_bounds__(256) void sa_power_rows_kernel(
    int64_t nrows, int64_t shift, const int64_t *__restrict__ arp, const int32_t *__restrict__ acol,
    const double *__restrict__ aval, const int64_t *__restrict__ ctrp, const int32_t *__restrict__ ctcol,
    const double *__restrict__ ctval, const double *__restrict__ t, double gamma, const double *__restrict__ v,
    const double *__restrict__ d, double *__restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrows) return;
  double s = 0.0;
  for (int64_t k = arp[i]; k < arp[i + 1]; ++k) s = fma(aval[k], v[(int64_t)acol[k] - shift], s);
  if (ctrp) {
    double u = 0.0;
    for (int64_t k = ctrp[i]; k < ctrp[i + 1]; ++k) u = fma(ctval[k], t[ctcol[k]], u);
    s = fma(gamma, u, s);
  }
  y[i] = s / d[i];
}

// ---------------------------------------------------------------------------------------------------
// Smoothed-aggregation prolongator P = P_tent - omega D^-1 (A P_tent + pen), one 64-lane workgroup per fine row i
// (alfd_build_smoothed_aggregation).  P_tent is never formed: (P_tent)_{j, agg[j]} = 1, so (A P_tent)_{iJ} is the sum
// of the entries of row i of A whose column j has agg[j] == J.  pen = gamma Ct diag(w) C P_tent comes in as a CSR matrix
// with sorted rows (formed beforehand by the generic product; C has few rows).  Canonical order of every entry:
//   s = 0.0;  s = s + a_ik  for the entries k of row i of A in CSR order with agg[col_k] == J;
//   s = s + pen_iJ;  P_iJ = fma(f_i, s, J == agg[i] ? 1 : 0)  with f_i = -omega / d_i (from the host).
// Pattern: the structural union {agg[col_k] >= 0} U pattern(pen row i) U {agg[i]}, columns ascending; rows with
// agg[i] < 0 stay empty.  Two passes as spgemm_rows_kernel: pass 0 counts the distinct coarse ids of every row (LDS
// hash set), pass 1 compacts and bitonic-sorts them, then lane t owns output column t and walks the row of A, staged
// in LDS as (agg[col], val) pairs, in CSR order.  At most kSaMaxOut distinct ids per row (overflow[0] is set
// otherwise: the host builds the level with the same arithmetic).  LDS: 16 KiB per workgroup.
constexpr int kSaTable = 2048;
constexpr int kSaMaxOut = 512;
constexpr int kSaStage = 512;
__global__ __launch_bounds__(64) void sa_prolongator_kernel(
    int64_t nrows, const int64_t *__restrict__ arp, const int32_t *__restrict__ acol, const double *__restrict__ aval,
    const int32_t *__restrict__ agg, const double *__restrict__ f, const int64_t *__restrict__ qrp,
    const int32_t *__restrict__ qcol, const double *__restrict__ qval, int pass, int32_t *__restrict__ counts,
    const int64_t *__restrict__ prp, int32_t *__restrict__ pcol, double *__restrict__ pval,
    int32_t *__restrict__ overflow) {
  __shared__ int32_t table[kSaTable];
  __shared__ int32_t keys[kSaMaxOut];
  __shared__ int32_t sJ[kSaStage];
  __shared__ double sv[kSaStage];
  __shared__ int32_t cnt;
  const int lane = threadIdx.x;
  auto insert = [&](int32_t J) {
    uint32_t h = ((uint32_t)J * 2654435761u) >> 21;   // 11 bits
    for (;;) {
      if (*(volatile int32_t *)&cnt > kSaMaxOut) break;   // overflowing row: stop inserting (reported below)
      const int32_t old = atomicCAS(&table[h], -1, J);
      if (old == -1) {
        atomicAdd(&cnt, 1);
        break;
      }
      if (old == J) break;
      h = (h + 1) & (kSaTable - 1);
    }
  };
  for (int64_t i = blockIdx.x; i < nrows; i += gridDim.x) {
    const int32_t gi = agg[i];
    if (gi < 0) {
      if (pass == 0 && lane == 0) counts[i] = 0;
      continue;
    }
    const int64_t k0 = arp[i], k1 = arp[i + 1];
    const int64_t q0 = qrp ? qrp[i] : 0, q1 = qrp ? qrp[i + 1] : 0;
    for (int s = lane; s < kSaTable; s += 64) table[s] = -1;
    if (lane == 0) cnt = 0;
    __syncthreads();
    if (lane == 0) insert(gi);
    for (int64_t k = k0 + lane; k < k1; k += 64) {
      const int32_t J = agg[acol[k]];
      if (J >= 0) insert(J);
    }
    for (int64_t q = q0 + lane; q < q1; q += 64) insert(qcol[q]);
    __syncthreads();
    const int n = cnt;
    if (n > kSaMaxOut) {
      if (lane == 0) overflow[0] = 1;
      if (pass == 0 && lane == 0) counts[i] = 0;
      __syncthreads();
      continue;
    }
    if (pass == 0) {
      if (lane == 0) counts[i] = n;
      __syncthreads();
      continue;
    }
    // compact, pad to a power of two with INT_MAX, bitonic sort (n2 <= kSaMaxOut)
    int n2 = 64;
    while (n2 < n) n2 <<= 1;
    __syncthreads();
    if (lane == 0) cnt = 0;
    __syncthreads();
    for (int s = lane; s < kSaTable; s += 64) {
      const int32_t J = table[s];
      if (J != -1) keys[atomicAdd(&cnt, 1)] = J;
    }
    __syncthreads();
    for (int s = n + lane; s < n2; s += 64) keys[s] = 0x7fffffff;
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int t = lane; t < n2 / 2; t += 64) {
          const int lo = 2 * t - (t & (stride - 1));
          const int hi = lo + stride;
          const bool up = (lo & size) == 0;
          const int32_t a = keys[lo], b = keys[hi];
          if ((a > b) == up) {
            keys[lo] = b;
            keys[hi] = a;
          }
        }
        __syncthreads();
      }
    const int64_t c0 = prp[i];
    const double fi = f[i];
    for (int t0 = 0; t0 < n; t0 += 64) {
      const int t = t0 + lane;
      const int32_t J = t < n ? keys[t] : -2;
      double s = 0.0;
      for (int64_t kb = k0; kb < k1; kb += kSaStage) {
        const int m = (int)(k1 - kb < kSaStage ? k1 - kb : kSaStage);
        __syncthreads();
        for (int e = lane; e < m; e += 64) {
          sJ[e] = agg[acol[kb + e]];
          sv[e] = aval[kb + e];
        }
        __syncthreads();
        for (int e = 0; e < m; ++e)
          if (sJ[e] == J) s = s + sv[e];
      }
      for (int64_t q = q0; q < q1; ++q)
        if (qcol[q] == J) s = s + qval[q];
      if (t < n) {
        pcol[c0 + t] = J;
        pval[c0 + t] = fma(fi, s, J == gi ? 1.0 : 0.0);
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------
// The truncated smoothed-aggregation prolongator (alfd_build_smoothed_aggregation_truncated): the row of
// sa_prolongator_kernel is computed into LDS and truncated there, so the untruncated P is never stored; counts[] and
// the row pointer hold KEPT entries.  Candidates (J ascending, p_J with the bits of sa_prolongator_kernel), g = agg[i],
// tau = drop tolerance, cap = most entries per row (0: no cap), component of J = J mod bs.  Canonical rule (DESIGN.md
// section 4):
//   m = max |p_J|;  K0 = {J : |p_J| >= tau * m} U {g};
//   |K0| > cap > 0:  K = {g} U the first cap - 1 of K0 \ {g} in the order (|p| descending, J ascending), found by
//                    counting rank (every candidate counts the candidates that precede it: no data-dependent sort);
//   per component c with dropped candidates D_c and kept ones:  t = 0.0; t = t + p_J over D_c, J ascending;  the kept
//                    entry of component c that is first in that order (untruncated values) becomes p + t;
//   the row is K, J ascending.
// Both passes compute the whole row: pass 0 counts the kept entries, pass 1 lumps, compacts and stores.  A row has at
// most kSaMaxOut candidates (overflow[0] otherwise: sa_rows_host, then the host truncation, same bits).
// LDS: 20.6 KiB per workgroup (the 16 KiB of sa_prolongator_kernel, the row's values and its keep flags).
__global__ __launch_bounds__(64) void sa_truncated_prolongator_kernel(
    int64_t nrows, const int64_t *__restrict__ arp, const int32_t *__restrict__ acol, const double *__restrict__ aval,
    const int32_t *__restrict__ agg, const double *__restrict__ f, const int64_t *__restrict__ qrp,
    const int32_t *__restrict__ qcol, const double *__restrict__ qval, int bs, double tau, int cap, int pass,
    int32_t *__restrict__ counts, const int64_t *__restrict__ prp, int32_t *__restrict__ pcol,
    double *__restrict__ pval, int32_t *__restrict__ overflow) {
  __shared__ int32_t table[kSaTable];
  __shared__ int32_t keys[kSaMaxOut];
  __shared__ int32_t sJ[kSaStage];
  __shared__ double sv[kSaStage];
  __shared__ double pv[kSaMaxOut];
  __shared__ uint8_t keep[kSaMaxOut];
  __shared__ int32_t cnt;
  const int lane = threadIdx.x;
  auto insert = [&](int32_t J) {
    uint32_t h = ((uint32_t)J * 2654435761u) >> 21;   // 11 bits
    for (;;) {
      if (*(volatile int32_t *)&cnt > kSaMaxOut) break;   // overflowing row: stop inserting (reported below)
      const int32_t old = atomicCAS(&table[h], -1, J);
      if (old == -1) {
        atomicAdd(&cnt, 1);
        break;
      }
      if (old == J) break;
      h = (h + 1) & (kSaTable - 1);
    }
  };
  for (int64_t i = blockIdx.x; i < nrows; i += gridDim.x) {
    const int32_t gi = agg[i];
    if (gi < 0) {
      if (pass == 0 && lane == 0) counts[i] = 0;
      continue;
    }
    const int64_t k0 = arp[i], k1 = arp[i + 1];
    const int64_t q0 = qrp ? qrp[i] : 0, q1 = qrp ? qrp[i + 1] : 0;
    for (int s = lane; s < kSaTable; s += 64) table[s] = -1;
    if (lane == 0) cnt = 0;
    __syncthreads();
    if (lane == 0) insert(gi);
    for (int64_t k = k0 + lane; k < k1; k += 64) {
      const int32_t J = agg[acol[k]];
      if (J >= 0) insert(J);
    }
    for (int64_t q = q0 + lane; q < q1; q += 64) insert(qcol[q]);
    __syncthreads();
    const int n = cnt;
    if (n > kSaMaxOut) {
      if (lane == 0) overflow[0] = 1;
      if (pass == 0 && lane == 0) counts[i] = 0;
      __syncthreads();
      continue;
    }
    // compact, pad to a power of two with INT_MAX, bitonic sort (n2 <= kSaMaxOut)
    int n2 = 64;
    while (n2 < n) n2 <<= 1;
    __syncthreads();
    if (lane == 0) cnt = 0;
    __syncthreads();
    for (int s = lane; s < kSaTable; s += 64) {
      const int32_t J = table[s];
      if (J != -1) keys[atomicAdd(&cnt, 1)] = J;
    }
    __syncthreads();
    for (int s = n + lane; s < n2; s += 64) keys[s] = 0x7fffffff;
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int t = lane; t < n2 / 2; t += 64) {
          const int lo = 2 * t - (t & (stride - 1));
          const int hi = lo + stride;
          const bool up = (lo & size) == 0;
          const int32_t a = keys[lo], b = keys[hi];
          if ((a > b) == up) {
            keys[lo] = b;
            keys[hi] = a;
          }
        }
        __syncthreads();
      }
    // the candidates' values, in sa_prolongator_kernel's order, and the row maximum
    const double fi = f[i];
    double m = 0.0;
    for (int t0 = 0; t0 < n; t0 += 64) {
      const int t = t0 + lane;
      const int32_t J = t < n ? keys[t] : -2;
      double s = 0.0;
      for (int64_t kb = k0; kb < k1; kb += kSaStage) {
        const int ms = (int)(k1 - kb < kSaStage ? k1 - kb : kSaStage);
        __syncthreads();
        for (int e = lane; e < ms; e += 64) {
          sJ[e] = agg[acol[kb + e]];
          sv[e] = aval[kb + e];
        }
        __syncthreads();
        for (int e = 0; e < ms; ++e)
          if (sJ[e] == J) s = s + sv[e];
      }
      for (int64_t q = q0; q < q1; ++q)
        if (qcol[q] == J) s = s + qval[q];
      if (t < n) {
        const double p = fma(fi, s, J == gi ? 1.0 : 0.0);
        pv[t] = p;
        if (fabs(p) > m) m = fabs(p);
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double u = __shfl_xor(m, o);
      if (u > m) m = u;
    }
    const double thr = tau * m;
    int nk = 0;
    for (int t0 = 0; t0 < n; t0 += 64) {
      const int t = t0 + lane;
      const bool k = t < n && (!(fabs(pv[t]) < thr) || keys[t] == gi);
      if (t < n) keep[t] = (uint8_t)(k ? 1 : 0);
      nk += __popcll(__ballot(k));
    }
    __syncthreads();
    if (cap > 0 && nk > cap) {
      // counting rank among K0 \ {g} under (|p| descending, J ascending); lane t decides candidates t, t + 64, ...
      uint32_t mine = 0;   // bit j: candidate lane + 64 j stays
      for (int j = 0; lane + 64 * j < n; ++j) {
        const int t = lane + 64 * j;
        if (!keep[t]) continue;
        if (keys[t] == gi) {
          mine |= 1u << j;
          continue;
        }
        const double a = fabs(pv[t]);
        int rank = 0;
        for (int u = 0; u < n; ++u) {
          const double b = fabs(pv[u]);
          rank += (keep[u] && keys[u] != gi && (b > a || (b == a && u < t))) ? 1 : 0;
        }
        if (rank < cap - 1) mine |= 1u << j;
      }
      __syncthreads();
      for (int j = 0; lane + 64 * j < n; ++j) keep[lane + 64 * j] = (uint8_t)((mine >> j) & 1u);
      nk = cap;
      __syncthreads();
    }
    if (pass == 0) {
      if (lane == 0) counts[i] = nk;
      __syncthreads();
      continue;
    }
    // lump what was dropped: one lane per component walks the candidates in ascending order
    if (nk < n) {
      for (int c = lane; c < bs; c += 64) {
        double t = 0.0, best = -1.0;
        int at = -1, nd = 0;
        for (int u = 0; u < n; ++u) {
          if (keys[u] % bs != c) continue;
          if (keep[u]) {
            if (fabs(pv[u]) > best) best = fabs(pv[u]), at = u;
          } else {
            t = t + pv[u];
            ++nd;
          }
        }
        if (nd > 0 && at >= 0) pv[at] = pv[at] + t;
      }
      __syncthreads();
    }
    const int64_t c0 = prp[i];
    int base = 0;
    for (int t0 = 0; t0 < n; t0 += 64) {
      const int t = t0 + lane;
      const bool k = t < n && keep[t];
      const unsigned long long mask = __ballot(k);
      if (k) {
        const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
        pcol[c0 + at] = keys[t];
        pval[c0 + at] = pv[t];
      }
      base += __popcll(mask);
    }
    __syncthreads();
  }
}

// flag[i] = 1 if row i of the CSR matrix has a column j with mark[j] >= 0 (rows of A that reach the interface patch)
__global__ void rows_touching_kernel(int64_t nrows, const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
                                     const int32_t *__restrict__ mark, uint8_t *__restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (i >= nrows) return;
  const int lane = threadIdx.x & 63;
  int hit = 0;
  for (int64_t k = rp[i] + lane; k < rp[i + 1]; k += 64) hit |= mark[col[k]] >= 0;
  hit = __any(hit);
  if (lane == 0) flag[i] = (uint8_t)(hit ? 1 : 0);
}

// copies the listed rows of a CSR matrix into a compact CSR whose row pointer orp the host computed
__global__ void gather_rows_kernel(int64_t nlist, const int32_t *__restrict__ rows, const int64_t *__restrict__ rp,
                                   const int32_t *__restrict__ col, const double *__restrict__ val,
                                   const int64_t *__restrict__ orp, int32_t *__restrict__ ocol, double *__restrict__ oval) {
  const int64_t q = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (q >= nlist) return;
  const int lane = threadIdx.x & 63;
  const int64_t k0 = rp[rows[q]], len = rp[rows[q] + 1] - k0, o0 = orp[q];
  for (int64_t k = lane; k < len; k += 64) {
    ocol[o0 + k] = col[k0 + k];
    oval[o0 + k] = val[k0 + k];
  }
}

// ---- device-stepped lumped-Jacobi PCG on Mp (the Bt Mp^-1 B term of Aug when grad_div_in_A = 0)
// The stop rule (Control::check) runs on the device, so the host enqueues a group of iterations and reads
// the state once per group.  Five launches per iteration, in pcg()'s canonical order:
//   P  p = z (first) or fma(beta, p, z)
//   S  Ap = Mp p: spmv_kernel's canonical L-lane rows, grid-stride over all resident workgroups
//   D  the p.Ap chunk partials (dot_partial_kernel)
//   U  alpha = rz / pAp from those partials (every workgroup takes the same second stage), then
//      x = fma(alpha, p, x), r = fma(-alpha, Ap, r), z = l .* r, and the r.r and r.z chunk partials
//   F  rr, rz = second stages; res = sqrt(rr); Control::check(step, res); beta = rz / rz_old
// Every kernel of an iteration returns at once when the state word sc[S_NSTATE] is no longer
// ITERATE (0), so nothing runs past convergence but the launch itself.  All partials use the dot's
// thread<->element map and all second stages dot_final_kernel's order: the bits are those of pcg().
enum { S_NSTATE = S_H, S_NSTEP = S_H + 1, S_NRES = S_H + 2, S_NRTOL = S_H + 3 };

__device__ __forceinline__ bool nmp_stopped(const double *sc) { return sc[S_NSTATE] != 0.0; }

// second stage of dot_final_kernel (thread-strided sequential adds, then the 256-thread tree); every
// thread returns the sum
__device__ __forceinline__ double nmp_second_stage(const double *__restrict__ part, int64_t nb, double *lds4) {
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < nb; i += kBlock) acc = acc + part[i];
  return block_reduce_256(acc, lds4);
}

// U, first = 1: r = b, x = 0, Ap = 0 (pcg()'s start; Ap's padding must stay 0); first = 0: alpha from the
// p.Ap partials (FIN_ALPHA of dot_final_kernel), the x / r update.  Then z = l .* r and the chunk partials of
// r.r (part_rr) and r.z (part_rz).
__global__ __launch_bounds__(kBlock) void nmp_update_kernel(const double *__restrict__ sc, int first,
                                                            const double *__restrict__ part_pap, int64_t nb,
                                                            const double *__restrict__ b,
                                                            const double *__restrict__ l,
                                                            const double *__restrict__ p, double *__restrict__ Ap,
                                                            double *__restrict__ x, double *__restrict__ r,
                                                            double *__restrict__ z, double *__restrict__ part_rr,
                                                            double *__restrict__ part_rz) {
  __shared__ double lds_a[4], lds_rr[4], lds_rz[4];
  if (!first && nmp_stopped(sc)) return;
  double a = 0.0, na = 0.0;
  if (!first) {
    const double pap = nmp_second_stage(part_pap, nb, lds_a);
    a = sc[S_RZ] / pap;
    na = -a;
  }
  double arr = 0.0, arz = 0.0;
  ALFD_FOR_PAIRS(i) {
    double2 rv, xv;
    if (first) {
      rv = ld2(b, i);
      xv = make_double2(0.0, 0.0);
      st2(Ap, i, make_double2(0.0, 0.0));
    } else {
      const double2 pv = ld2(p, i), av = ld2(Ap, i);
      xv = ld2(x, i);
      rv = ld2(r, i);
      xv.x = fma(a, pv.x, xv.x);
      xv.y = fma(a, pv.y, xv.y);
      rv.x = fma(na, av.x, rv.x);
      rv.y = fma(na, av.y, rv.y);
    }
    st2(x, i, xv);
    st2(r, i, rv);
    const double2 lv = ld2(l, i);
    double2 zv;
    zv.x = lv.x * rv.x;
    zv.y = lv.y * rv.y;
    st2(z, i, zv);
    arr = fma(rv.x, rv.x, arr);
    arr = fma(rv.y, rv.y, arr);
    arz = fma(rv.x, zv.x, arz);
    arz = fma(rv.y, zv.y, arz);
  }
  const double srr = block_reduce_256(arr, lds_rr);
  const double srz = block_reduce_256(arz, lds_rz);
  if (threadIdx.x == 0) {
    part_rr[blockIdx.x] = srr;
    part_rz[blockIdx.x] = srz;
  }
}

// F: one workgroup.  Control::check of alfd.hip, step by step (step 0 fixes the reference value of
// the reduction kind); the state word is written last, by an ordinary store of thread 0.
__global__ __launch_bounds__(kBlock) void nmp_finish_kernel(const double *__restrict__ part_rr,
                                                            const double *__restrict__ part_rz, int64_t nb,
                                                            double *__restrict__ sc, int step, int kind,
                                                            int max_steps, double tol, double reduce) {
  __shared__ double lds_rr[4], lds_rz[4];
  if (step > 0 && nmp_stopped(sc)) return;
  const double rr = nmp_second_stage(part_rr, nb, lds_rr);
  const double rz = nmp_second_stage(part_rz, nb, lds_rz);
  if (threadIdx.x == 0) {
    const double v = sqrt(rr);
    if (step == 0) sc[S_NRTOL] = v * reduce;
    const double reduced_tol = step == 0 ? v * reduce : sc[S_NRTOL];
    int state = 0;   // ITERATE
    if (kind == ALFD_CTRL_REDUCTION && v < reduced_tol) state = 1;
    else if (kind == ALFD_CTRL_FIXED_ITERS && step >= max_steps) state = 1;
    else if (v <= tol) state = 1;
    else if (step >= max_steps || isnan(v)) state = 2;
    sc[S_RR] = rr;
    sc[S_NRES] = v;
    sc[S_NSTEP] = (double)step;
    if (state == 0) {   // FIN_RZ of the next iteration
      const double old = sc[S_RZ];
      sc[S_RZ_OLD] = old;
      sc[S_RZ] = rz;
      sc[S_BETA] = rz / old;
    }
    sc[S_NSTATE] = (double)state;
  }
}

// P: p = z on the first iteration, else p = fma(beta, p, z)
__global__ __launch_bounds__(kBlock) void nmp_p_kernel(const double *__restrict__ sc, int first,
                                                       const double *__restrict__ z, double *__restrict__ p) {
  if (nmp_stopped(sc)) return;
  const double beta = first ? 0.0 : sc[S_BETA];
  ALFD_FOR_PAIRS(i) {
    const double2 zv = ld2(z, i);
    if (first) {
      st2(p, i, zv);
    } else {
      double2 pv = ld2(p, i);
      pv.x = fma(beta, pv.x, zv.x);
      pv.y = fma(beta, pv.y, zv.y);
      st2(p, i, pv);
    }
  }
}

// S: Ap = Mp p, spmv_kernel<L, 0, false> behind the state word (single rank: every column is local).
// Rows only; the padding of Ap stays as U (first) left it.
template <int L>
__global__ __launch_bounds__(kBlock) void nmp_spmv_kernel(const double *__restrict__ sc, int64_t nrows,
                                                          const int64_t *__restrict__ rp,
                                                          const int32_t *__restrict__ col,
                                                          const double *__restrict__ val,
                                                          const double *__restrict__ p, double *__restrict__ Ap) {
  if (nmp_stopped(sc)) return;
  constexpr int RPB = kBlock / L;
  const int lane = threadIdx.x % L;
  const int sub = threadIdx.x / L;
  const int64_t ngroups = (nrows + RPB - 1) / RPB;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t row = g * RPB + sub;
    if (row < nrows) {   // uniform within the L-lane group
      const int64_t k0 = rp[row], k1 = rp[row + 1];
      double acc = 0.0;
      for (int64_t k = k0 + lane; k < k1; k += L) acc = fma(val[k], p[col[k]], acc);
      acc = group_reduce<L>(acc);
      if (lane == 0) Ap[row] = acc;
    }
  }
}

// D: the canonical chunk partials of p.Ap (dot_partial_kernel behind the state word)
__global__ __launch_bounds__(kBlock) void nmp_dot_kernel(const double *__restrict__ sc, const double *__restrict__ p,
                                                         const double *__restrict__ Ap, double *__restrict__ part_pap) {
  __shared__ double lds4[4];
  if (nmp_stopped(sc)) return;
  double acc = 0.0;
  ALFD_FOR_PAIRS(i) {
    const double2 a = ld2(p, i), b = ld2(Ap, i);
    acc = fma(a.x, b.x, acc);
    acc = fma(a.y, b.y, acc);
  }
  const double s = block_reduce_256(acc, lds4);
  if (threadIdx.x == 0) part_pap[blockIdx.x] = s;
}

// ---- device-stepped unpreconditioned CG on C Ct that records its coefficients (alfd_estimate_spectrum)
// pcg() with ALFD_PREC_IDENTITY on y = Cs (Cts x), b = 1, from a zero start.  Six launches per iteration, the
// scheme of the Mp solve above with z = r (one dot instead of two):
//   P  nmp_p_kernel with z = r          S  t = Cts p, then Ap = Cs t: nmp_spmv_kernel twice
//   D  nmp_dot_kernel                   U  spc_update_kernel         F  spc_finish_kernel
// sc[S_RZ] holds r.r of the previous step (identity: r.z == r.r, same canonical dot, same bits).

// U, first = 1: r = 1 on the n rows (0 on the padding), x = 0, Ap = 0; first = 0: alpha = rr / pAp from the p.Ap
// partials, x = fma(alpha, p, x), r = fma(-alpha, Ap, r).  Then the chunk partials of r.r.
__global__ __launch_bounds__(kBlock) void spc_update_kernel(const double *__restrict__ sc, int first,
                                                            const double *__restrict__ part_pap, int64_t nb, int64_t n,
                                                            const double *__restrict__ p, double *__restrict__ Ap,
                                                            double *__restrict__ x, double *__restrict__ r,
                                                            double *__restrict__ part_rr) {
  __shared__ double lds_a[4], lds_rr[4];
  if (!first && nmp_stopped(sc)) return;
  double a = 0.0, na = 0.0;
  if (!first) {
    const double pap = nmp_second_stage(part_pap, nb, lds_a);
    a = sc[S_RZ] / pap;
    na = -a;
  }
  double arr = 0.0;
  ALFD_FOR_PAIRS(i) {
    double2 rv, xv;
    if (first) {
      rv = make_double2(i < n ? 1.0 : 0.0, i + 1 < n ? 1.0 : 0.0);
      xv = make_double2(0.0, 0.0);
      st2(Ap, i, make_double2(0.0, 0.0));
    } else {
      const double2 pv = ld2(p, i), av = ld2(Ap, i);
      xv = ld2(x, i);
      rv = ld2(r, i);
      xv.x = fma(a, pv.x, xv.x);
      xv.y = fma(a, pv.y, xv.y);
      rv.x = fma(na, av.x, rv.x);
      rv.y = fma(na, av.y, rv.y);
    }
    st2(x, i, xv);
    st2(r, i, rv);
    arr = fma(rv.x, rv.x, arr);
    arr = fma(rv.y, rv.y, arr);
  }
  const double srr = block_reduce_256(arr, lds_rr);
  if (threadIdx.x == 0) part_rr[blockIdx.x] = srr;
}

// F: one workgroup.  Breakdown test (p.Ap <= 0 or NaN: state FAILURE, step and residual stay those of the step
// before), then Control::check as nmp_finish_kernel.  A step that counts stores alpha_step = rr_old / pAp into
// coef[step - 1]; one that goes on also beta_step = rr / rr_old into coef[max_steps + step - 1].  Plain stores of
// thread 0, the state word last.
__global__ __launch_bounds__(kBlock) void spc_finish_kernel(const double *__restrict__ part_rr,
                                                            const double *__restrict__ part_pap, int64_t nb,
                                                            double *__restrict__ sc, double *__restrict__ coef, int step,
                                                            int kind, int max_steps, double tol, double reduce) {
  __shared__ double lds_rr[4], lds_a[4];
  if (step > 0 && nmp_stopped(sc)) return;
  const double rr = nmp_second_stage(part_rr, nb, lds_rr);
  const double pap = step > 0 ? nmp_second_stage(part_pap, nb, lds_a) : 1.0;
  if (threadIdx.x == 0) {
    if (!(pap > 0.0)) {
      sc[S_PAP] = pap;
      sc[S_NSTATE] = 2.0;
      return;
    }
    const double v = sqrt(rr);
    if (step == 0) sc[S_NRTOL] = v * reduce;
    const double reduced_tol = step == 0 ? v * reduce : sc[S_NRTOL];
    int state = 0;   // ITERATE
    if (kind == ALFD_CTRL_REDUCTION && v < reduced_tol) state = 1;
    else if (kind == ALFD_CTRL_FIXED_ITERS && step >= max_steps) state = 1;
    else if (v <= tol) state = 1;
    else if (step >= max_steps || isnan(v)) state = 2;
    const double old = sc[S_RZ];
    if (step > 0) coef[step - 1] = old / pap;
    sc[S_RR] = rr;
    sc[S_NRES] = v;
    sc[S_NSTEP] = (double)step;
    if (state == 0) {
      sc[S_RZ_OLD] = old;
      sc[S_RZ] = rr;
      if (step > 0) {
        const double beta = rr / old;
        sc[S_BETA] = beta;
        coef[max_steps + step - 1] = beta;
      }
    }
    sc[S_NSTATE] = (double)state;
  }
}

// ---- max-abs reduction of d = y - g (alfd_constraint_residual), two stages, no atomics.  A NaN entry makes the
// result NaN (fmax would drop it): every stage carries a NaN flag beside the maximum.
__device__ __forceinline__ double linf_block(double m, double bad, double *lds) {   // lds[8]
  for (int o = 32; o > 0; o >>= 1) {
    m = fmax(m, __shfl_xor(m, o, 64));
    bad = fmax(bad, __shfl_xor(bad, o, 64));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[wave] = m, lds[4 + wave] = bad;
  __syncthreads();
  m = fmax(fmax(lds[0], lds[1]), fmax(lds[2], lds[3]));
  bad = fmax(fmax(lds[4], lds[5]), fmax(lds[6], lds[7]));
  return bad > 0.0 ? nan("") : m;
}

// stage 1: part[b] = max |y_i - g_i| over chunk b (g == nullptr: 0), i < n
__global__ __launch_bounds__(kBlock) void linf_diff_partial_kernel(int64_t n, const double *__restrict__ y,
                                                                   const double *__restrict__ g,
                                                                   double *__restrict__ part) {
  __shared__ double lds[8];
  double m = 0.0, bad = 0.0;
  const int64_t base = (int64_t)blockIdx.x * kChunk;
  for (int64_t i = base + threadIdx.x; i < base + kChunk && i < n; i += kBlock) {
    const double d = g ? y[i] - g[i] : y[i];
    if (isnan(d)) bad = 1.0;
    m = fmax(m, fabs(d));
  }
  const double s = linf_block(m, bad, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// stage 2: one workgroup, out[0] = max of the nb chunk results
__global__ __launch_bounds__(kBlock) void linf_final_kernel(const double *__restrict__ part, int64_t nb,
                                                            double *__restrict__ out) {
  __shared__ double lds[8];
  double m = 0.0, bad = 0.0;
  for (int64_t i = threadIdx.x; i < nb; i += kBlock) {
    const double d = part[i];
    if (isnan(d)) bad = 1.0;
    m = fmax(m, d);
  }
  const double s = linf_block(m, bad, lds);
  if (threadIdx.x == 0) out[0] = s;
}

// ---- caller block vectors <-> the padded internal vector (the *_device entry points of the C ABI).
// The internal vector concatenates the blocks, each padded to a multiple of kChunk (off[b + 1] - off[b]); the padding
// must be ZERO because the fused dot / update kernels read it.  The table travels by value as a kernel argument.
// One workgroup moves one 4096-double chunk at a time (grid-stride over the chunks); a chunk lies in exactly one
// block, and an empty block (off[b] == off[b + 1], null pointer allowed) owns no chunk, so it is never dereferenced.
// Caller pointers are only 8-byte aligned (a view t[1:]): plain 8-byte accesses there; the internal side is
// chunk-aligned and moves 16 bytes per lane.  Thread t takes the pairs base + e*512 + 2t, e = 0..7: a wave covers
// 1 KiB contiguous on both sides.
static_assert(kChunk == 16 * kBlock, "pack / unpack: 8 passes of 2 doubles per thread cover one chunk");
constexpr int kMaxBlocks = 3;   // == ALFD_MAX_BLOCKS
struct BlockTable {
  double *p[kMaxBlocks];        // caller pointers (read by pack, written by unpack)
  int64_t n[kMaxBlocks];        // block lengths
  int64_t off[kMaxBlocks + 1];  // padded offsets into the internal vector
  int32_t nblocks;
};

// the block that owns the chunk starting at `base` (base < off[nblocks]): the last b with off[b] <= base
__device__ __forceinline__ void block_of_chunk(const BlockTable &tab, int64_t base, double *&p, int64_t &m) {
  p = tab.p[0];
  int64_t n = tab.n[0], o = tab.off[0];
#pragma unroll
  for (int b = 1; b < kMaxBlocks; ++b)
    if (b < tab.nblocks && base >= tab.off[b]) p = tab.p[b], n = tab.n[b], o = tab.off[b];
  p += base - o;          // first caller element of this chunk (not dereferenced when m <= 0)
  m = n - (base - o);     // caller elements from there on; >= kChunk except in the block's last chunk
}

__global__ __launch_bounds__(kBlock) void pack_blocks_kernel(BlockTable tab, double *__restrict__ dst, int64_t nchunks) {
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t base = c * kChunk;
    double *p;
    int64_t m;
    block_of_chunk(tab, base, p, m);
    const double *__restrict__ src = p;
    double2 v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int i = e * 512 + 2 * (int)threadIdx.x;
      v[e].x = i < m ? src[i] : 0.0;
      v[e].y = i + 1 < m ? src[i + 1] : 0.0;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e)
      *reinterpret_cast<double2 *>(dst + base + e * 512 + 2 * (int)threadIdx.x) = v[e];
  }
}

__global__ __launch_bounds__(kBlock) void unpack_blocks_kernel(BlockTable tab, const double *__restrict__ src,
                                                               int64_t nchunks) {
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t base = c * kChunk;
    double *p;
    int64_t m;
    block_of_chunk(tab, base, p, m);
    double *__restrict__ dst = p;
    double2 v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      v[e] = *reinterpret_cast<const double2 *>(src + base + e * 512 + 2 * (int)threadIdx.x);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int i = e * 512 + 2 * (int)threadIdx.x;
      if (i < m) dst[i] = v[e].x;
      if (i + 1 < m) dst[i + 1] = v[e].y;
    }
  }
}

// ---- the same two moves under a block-0 numbering (alfd_set_numbering): internal element k of block 0 is the caller's
// element perm[k].  perm is int32 (block 0 has fewer than 2^31 rows), a bijection of [0, n[0]) checked on the host, and
// its device copy is padded to whole chunks, so the 8-byte index load of a pair never leaves the array; the indices past
// n[0] are not used.  Same chunk and thread map on the internal side as above (16-byte accesses, the whole chunk
// written, zero padding); the chunks of block 0 are those below off[1] (off[0] == 0), the other blocks take the straight
// path.  A thread issues the index loads of its 16 elements before the first gather / scatter, so the 16 dependent
// accesses are in flight together: on the caller side the launch is bound by the latency of a round trip.
__device__ __forceinline__ void perm_pairs(const int32_t *__restrict__ q, int2 (&j)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) j[e] = *reinterpret_cast<const int2 *>(q + e * 512 + 2 * (int)threadIdx.x);
}

__global__ __launch_bounds__(kBlock) void pack_blocks_perm_kernel(BlockTable tab, const int32_t *__restrict__ perm,
                                                                  double *__restrict__ dst, int64_t nchunks) {
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t base = c * kChunk;
    double *p;
    int64_t m;
    block_of_chunk(tab, base, p, m);
    double2 v[8];
    if (base < tab.off[1]) {   // block 0: gather through the numbering
      const double *__restrict__ src = tab.p[0];
      int2 j[8];
      perm_pairs(perm + base, j);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int i = e * 512 + 2 * (int)threadIdx.x;
        v[e].x = i < m ? src[j[e].x] : 0.0;
        v[e].y = i + 1 < m ? src[j[e].y] : 0.0;
      }
    } else {
      const double *__restrict__ src = p;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int i = e * 512 + 2 * (int)threadIdx.x;
        v[e].x = i < m ? src[i] : 0.0;
        v[e].y = i + 1 < m ? src[i + 1] : 0.0;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e)
      *reinterpret_cast<double2 *>(dst + base + e * 512 + 2 * (int)threadIdx.x) = v[e];
  }
}

// Scatter form of the unpack (tunable "numbering_unpack_scatter"; kept for the A/B measurement of profiles/numbering/,
// where it is the slower one): coalesced 16-byte reads of the internal vector, 8-byte writes at perm[k].  perm is a
// bijection, so no two lanes write the same element.
__global__ __launch_bounds__(kBlock) void unpack_blocks_perm_scatter_kernel(BlockTable tab, const int32_t *__restrict__ perm,
                                                                    const double *__restrict__ src, int64_t nchunks) {
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t base = c * kChunk;
    double *p;
    int64_t m;
    block_of_chunk(tab, base, p, m);
    const bool first = base < tab.off[1];
    int2 j[8];
    if (first) perm_pairs(perm + base, j);
    double2 v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      v[e] = *reinterpret_cast<const double2 *>(src + base + e * 512 + 2 * (int)threadIdx.x);
    if (first) {
      double *__restrict__ dst = tab.p[0];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int i = e * 512 + 2 * (int)threadIdx.x;
        if (i < m) dst[j[e].x] = v[e].x;
        if (i + 1 < m) dst[j[e].y] = v[e].y;
      }
    } else {
      double *__restrict__ dst = p;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int i = e * 512 + 2 * (int)threadIdx.x;
        if (i < m) dst[i] = v[e].x;
        if (i + 1 < m) dst[i + 1] = v[e].y;
      }
    }
  }
}

// The unpack that runs by default, in gather form: a chunk of block 0 is a chunk of the CALLER's index space, element
// i <- src[inv[i]] with inv the inverse numbering; coalesced 8-byte writes, scattered 8-byte reads.  The same bits as the
// scatter form, since both copy every element once; measured 0.35 against 0.38 ms per solve call at 6.4 M rows.
__global__ __launch_bounds__(kBlock) void unpack_blocks_perm_kernel(BlockTable tab, const int32_t *__restrict__ inv,
                                                                    const double *__restrict__ src, int64_t nchunks) {
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t base = c * kChunk;
    double *p;
    int64_t m;
    block_of_chunk(tab, base, p, m);
    double *__restrict__ dst = p;
    double2 v[8];
    if (base < tab.off[1]) {
      int2 j[8];
      perm_pairs(inv + base, j);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int i = e * 512 + 2 * (int)threadIdx.x;
        v[e].x = i < m ? src[j[e].x] : 0.0;
        v[e].y = i + 1 < m ? src[j[e].y] : 0.0;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        v[e] = *reinterpret_cast<const double2 *>(src + base + e * 512 + 2 * (int)threadIdx.x);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int i = e * 512 + 2 * (int)threadIdx.x;
      if (i < m) dst[i] = v[e].x;
      if (i + 1 < m) dst[i + 1] = v[e].y;
    }
  }
}

// --------------------------------------------------------------------------
// Side rows of a long-row batch-major operator ("batch_major_side_rows"): the few rows beyond kVsMaxLen entries that
// the planner keeps out of the row blocks, in a compact CSR of their own (rows[i]: global row of list entry i, longest
// first; rp: 64-bit offsets into col / val, the entries in the row's own order).  One wave per row, 4 waves per
// workgroup, list entry 4 blockIdx.x + wave first, so the longest rows start first.  Canonical arithmetic of 64-lane
// rows: entry k belongs to lane k mod 64, one fma chain per lane in ascending k, then group_reduce<64> -- what
// spmv_rows<64, ...> computes, bit for bit.
// A row is 385 .. 65 535 entries, i.e. 7 or more 64-entry chunks of ONE dependent chain (col -> x -> fma), and the launch
// has far fewer waves than the chip has slots: what bounds it is the latency of a round trip, not bandwidth.  So a pass
// issues the column and value loads of kSideU chunks, then their x gathers, then the fmas: 2 kSideU + kSideU independent
// loads per lane and pass instead of 3.  kSideU = 8 (20 VGPRs of loads per lane, 10 KB per wave in flight) covers the
// 807 .. 855-entry rows of the locally refined mesh in two passes; the one accumulator keeps the order of the chain.
constexpr int kSideU = 8;
constexpr int kSideMaxLen = 65535;   // longest side row (the planner refuses the variant beyond)
template <int EPI>
__global__ __launch_bounds__(kBlock) void spmv_side_rows_kernel(
    int64_t n_side, const int32_t *__restrict__ rows, const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
    const double *__restrict__ val, const double *__restrict__ x, const double *__restrict__ x_halo, int32_t n_local,
    double *__restrict__ y, double alpha, const double *__restrict__ d, double *__restrict__ y2) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n_side; i += (int64_t)gridDim.x * 4) {   // wave-uniform
    const int64_t k0 = rp[i];
    const int32_t n = (int32_t)(rp[i + 1] - k0);
    const int32_t *cb = col + k0;
    const double *vb = val + k0;
    double acc = 0.0;
    for (int32_t base = 0; base < n; base += 64 * kSideU) {
      int32_t c[kSideU];
      double v[kSideU], xv[kSideU];
#pragma unroll
      for (int u = 0; u < kSideU; ++u) {
        const int32_t o = base + 64 * u + lane;
        c[u] = -1;
        v[u] = 0.0;
        if (o < n) {
          c[u] = cb[o];
          v[u] = vb[o];
        }
      }
#pragma unroll
      for (int u = 0; u < kSideU; ++u) {
        xv[u] = 0.0;
        if (c[u] >= 0) xv[u] = (c[u] < n_local) ? x[c[u]] : x_halo[c[u] - n_local];
      }
#pragma unroll
      for (int u = 0; u < kSideU; ++u)
        if (c[u] >= 0) acc = fma(v[u], xv[u], acc);
    }
    acc = group_reduce<64>(acc);
    if (lane == 0) {
      const int64_t ro = rows[i];
      if (EPI == 0)
        y[ro] = acc;
      else if (EPI == 1)
        y[ro] = fma(alpha, acc, y[ro]);
      else if (EPI == 2)
        y[ro] = d[ro] * acc;
      else {
        y[ro] = acc;
        y2[ro] = d[ro] * acc;
      }
    }
  }
}

// The side rows behind the launch with the block-end tail ("ml_tail_side_rows", launch_vs_tail): a side row has no
// block end, so its tail runs here, where its sum is formed.  The row sum is spmv_side_rows_kernel's, statement for
// statement; lane 0 then does what vs_tail_row does with a block's row: a row Ct lists (mask) gets its y stored and is
// finished by the rows party of aug_tail_kernel, every other row goes through aug_tail_elem<TM> and y is NOT stored.
// Single-rank operators only (no halo).  No output of p may be x (the host refuses that): other waves still gather it.
template <int TM>
__global__ __launch_bounds__(kBlock) void spmv_side_rows_tail_kernel(
    int64_t n_side, const int32_t *__restrict__ rows, const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
    const double *__restrict__ val, const double *__restrict__ x, double *__restrict__ y,
    const uint8_t *__restrict__ mask, AugTailArgs p) {
  static_assert(TM >= TAIL_STEP && TM <= TAIL_RES_INIT, "the modes of the block-end epilogue");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n_side; i += (int64_t)gridDim.x * 4) {   // wave-uniform
    const int64_t k0 = rp[i];
    const int32_t n = (int32_t)(rp[i + 1] - k0);
    const int32_t *cb = col + k0;
    const double *vb = val + k0;
    double acc = 0.0;
    for (int32_t base = 0; base < n; base += 64 * kSideU) {
      int32_t c[kSideU];
      double v[kSideU], xv[kSideU];
#pragma unroll
      for (int u = 0; u < kSideU; ++u) {
        const int32_t o = base + 64 * u + lane;
        c[u] = -1;
        v[u] = 0.0;
        if (o < n) {
          c[u] = cb[o];
          v[u] = vb[o];
        }
      }
#pragma unroll
      for (int u = 0; u < kSideU; ++u) {
        xv[u] = 0.0;
        if (c[u] >= 0) xv[u] = x[c[u]];
      }
#pragma unroll
      for (int u = 0; u < kSideU; ++u)
        if (c[u] >= 0) acc = fma(v[u], xv[u], acc);
    }
    acc = group_reduce<64>(acc);
    if (lane == 0) {
      const int64_t ro = rows[i];
      if (mask[ro]) y[ro] = acc;
      else aug_tail_elem<TM>(p, ro, acc);
    }
  }
}

}  // namespace alfd
