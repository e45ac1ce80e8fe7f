// diffuse.hip -- one step of the random walk of the kernel matrix on a wide fp64 signal (MAGIC-style diffusion of cell signals).
//
// Reference surface: graphtools' diff_op = normalize(K, "l1", axis=1) with K = W + diag(kd) (DeviceGraph.diff_op builds it on the
// host), applied as [UPSTREAM magic-impute, unpinned: not importable next to this code] applies it: X <- diff_op X, t times.
//
//     y[i, c] = ( sum_{e in row i, storage order} val[e] x[col[e], c]  +  kd[i] x[i, c] ) / s[i],      s = dw + kd
//
// The gather scheme is cheby_step_wide_kernel's (csrc/spmm.hip): lanes = COLUMNS, a wave owns DIFF_ROWS consecutive rows as one
// stream of entries, the (value, column) pairs are loaded a chunk ahead by the first lanes and handed round with v_readlane
// (scalar address arithmetic, the value as a scalar operand of the FMA), the gathers of a chunk are in flight while the previous
// chunk is summed; workgroups are XCD-contiguous.  What is new here:
//   * the epilogue is per row (the kernel's diagonal and ONE true division by the row sum of K), not a scalar combination;
//   * a lane carries NC = 1 or 2 columns (lane and lane + 64: two 8-byte accesses, each coalesced across the wave -- no 16-byte
//     vector access, so x, y and the leading dimensions need 8-byte alignment only), which takes a signal of up to 128 columns
//     through ONE stream of the matrix;
//   * x and y have leading dimensions: a wider signal is processed in column panels without copies.
// Register budget: the gathers in flight are what the kernel spends its registers on (cdna_hip_programming.md guidelines 6 and 7).
// NC = 1 keeps the wide step's 16 gathers per lane and chunk (2 chunks x 16 x 2 VGPRs = 64); NC = 2 halves the chunk to 8 entries so
// that the same 64 VGPRs -- and the same bytes in flight per lane -- serve two columns, next to 32 for the rows' own operands and
// two accumulators.  As compiled: NC = 1 takes 122 VGPRs (4 waves per SIMD, as the wide step), NC = 2 takes 144 (3 waves per SIMD),
// neither touches private memory; capping NC = 2 at 128 registers (__launch_bounds__(256, 4)) spills 20 of them into the loop and is
// not done.
// The accumulation of one output element is written with explicit fma calls, in storage order, the diagonal term last: its value
// is a function of the operands alone -- not of p, of the panel, of the leading dimensions or of the other columns in the launch.
// No atomics, plain vector loads and stores.
#include "common.hpp"

namespace meld {

constexpr int DIFF_ROWS = 8;       // rows per wave (consecutive); 4 waves per workgroup: 32 rows
constexpr int DIFF_MAX_COLS = 128;

template <int NC>
__global__ __launch_bounds__(256) void diffuse_step_kernel(const int64_t* __restrict__ rowptr, const int* __restrict__ col,
                                                           const double* __restrict__ val, const double* __restrict__ kd,
                                                           const double* __restrict__ s, int64_t n_rows,
                                                           const double* __restrict__ x, int64_t ldx, double* __restrict__ y,
                                                           int64_t ldy, int p) {
  constexpr int U = 16 / NC;  // entries per chunk = gathers in flight per lane and column
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nb = gridDim.x;  // (a multiple of 8: the remap below is a bijection)
  const int per = (nb + 7) >> 3;
  const int64_t rb = (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (rb >= nb) return;
  const int64_t row_first = (rb * 4 + wv) * DIFF_ROWS;
  if (row_first >= n_rows) return;  // (uniform)
  const int n_here = (int)min((int64_t)DIFF_ROWS, n_rows - row_first);
  bool on[NC];
  int lc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    on[c] = lane + 64 * c < p;
    lc[c] = on[c] ? lane + 64 * c : 0;  // (an idle lane re-reads column 0: inside the row, never stored)
  }
  // row boundaries, kernel diagonal and row sums of the wave's rows: lane r holds row r, handed round with v_readlane
  const int64_t rp = rowptr[min(row_first + min(lane, n_here), n_rows)];
  const int64_t row_l = min(row_first + min(lane, n_here - 1), n_rows - 1);
  const double kdl = kd[row_l], sl = s[row_l];
  // the rows' own operands, column `lane` and column `lane + 64`: register vectors, read at the (uniform) index of the row that
  // closes -- as arrays the allocator keeps them in private memory once the second column is there
  typedef double row_vec __attribute__((ext_vector_type(DIFF_ROWS)));
  row_vec xi0, xi1;
#pragma unroll
  for (int r = 0; r < DIFF_ROWS; ++r) {
    const int64_t row = min(row_first + r, n_rows - 1);
    xi0[r] = x[row * ldx + lc[0]];
    if constexpr (NC > 1) xi1[r] = x[row * ldx + lc[NC - 1]];
  }
  auto rp_at = [&](int r) __attribute__((always_inline)) {
    return (int64_t)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(rp >> 32), r) << 32) |
                     (unsigned)__builtin_amdgcn_readlane((int)rp, r));
  };
  auto uniform = [&](double v, int r) __attribute__((always_inline)) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), r), __builtin_amdgcn_readlane(__double2loint(v), r));
  };
  const int64_t E0 = rp_at(0), E1 = rp_at(n_here);
  // pairs of the chunk that starts at entry e0 (lane u & (U - 1): entry e0 + u); beyond the wave's stream the value is 0 and the
  // column that of the last entry (row 0 where the wave has no entries at all): always a row of x
  auto fetch_pairs = [&](int64_t e0, double& vv, int& cc) __attribute__((always_inline)) {
    const int64_t e = min(e0 + (lane & (U - 1)), E1 - 1);
    vv = (e0 + (lane & (U - 1)) < E1) ? __builtin_nontemporal_load(val + max(e, (int64_t)0)) : 0.0;
    cc = E1 > E0 ? __builtin_nontemporal_load(col + max(e, (int64_t)0)) : 0;
  };
  auto gather = [&](int cc, double (&xj)[U][NC]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const double* xr = x + (int64_t)__builtin_amdgcn_readlane(cc, u) * ldx;
#pragma unroll
      for (int c = 0; c < NC; ++c) xj[u][c] = xr[lc[c]];
    }
  };
  int r_cur = 0;
  int64_t re_cur = rp_at(1);
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  auto flush_rows_until = [&](int64_t e) __attribute__((always_inline)) {  // (uniform) close every row that ends at or before entry e
    while (r_cur < n_here && e >= re_cur) {
      const double kdr = uniform(kdl, r_cur), sr = uniform(sl, r_cur);
      double xr[2] = {xi0[r_cur], 0.0};
      if constexpr (NC > 1) xr[1] = xi1[r_cur];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (on[c]) __builtin_nontemporal_store(fma(kdr, xr[c], acc[c]) / sr, y + (row_first + r_cur) * ldy + lane + 64 * c);
        acc[c] = 0.0;
      }
      ++r_cur;
      re_cur = r_cur < n_here ? rp_at(r_cur + 1) : E1 + 1;
    }
  };
  auto sum_chunk = [&](int64_t e0, double vv, const double (&xj)[U][NC]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      flush_rows_until(e0 + u);
      const double v = uniform(vv, u);
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] = fma(v, xj[u][c], acc[c]);
    }
  };
  double vA, vB;
  int cA, cB;
  double xA[U][NC], xB[U][NC];
  fetch_pairs(E0, vA, cA);
  fetch_pairs(E0 + U, vB, cB);
  gather(cA, xA);
  for (int64_t e0 = E0; e0 < E1; e0 += 2 * U) {
    // chunk A = [e0, e0 + U), chunk B = [e0 + U, e0 + 2 U); the pairs of the chunk after B and B's gathers go out before A is summed
    gather(cB, xB);
    double vN;
    int cN;
    fetch_pairs(e0 + 2 * U, vN, cN);
    sum_chunk(e0, vA, xA);
    gather(cN, xA);
    double vM;
    int cM;
    fetch_pairs(e0 + 3 * U, vM, cM);
    sum_chunk(e0 + U, vB, xB);
    vA = vN;
    cA = cN;
    vB = vM;
    cB = cM;
  }
  // the rows that are left: the last one, and rows without entries.  (Entries past E1 carry the value 0 and are summed after every
  // row has been closed at entry E1: they reach no output.)
  flush_rows_until(E1 + 1);
}

}  // namespace meld

using namespace meld;

extern "C" int meld_diffuse_max_cols(void) { return DIFF_MAX_COLS; }

extern "C" int meld_diffuse_step(const int64_t* rowptr, const int32_t* col, const double* val, const double* kd, const double* s,
                                 int64_t n_rows, const double* x, int64_t ldx, double* y, int64_t ldy, int p, meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && kd && s && x && y, "meld_diffuse_step: rowptr, kd, s, x and y are required");
  MELD_CHECK_ARG(n_rows >= 0, "meld_diffuse_step: n_rows=%lld is negative", (long long)n_rows);
  MELD_CHECK_ARG(p >= 1 && p <= DIFF_MAX_COLS, "meld_diffuse_step: p=%d columns (1 <= p <= %d per call)", p, DIFF_MAX_COLS);
  MELD_CHECK_ARG(ldx >= p && ldy >= p, "meld_diffuse_step: leading dimensions ldx=%lld, ldy=%lld below p=%d", (long long)ldx,
                 (long long)ldy, p);
  MELD_CHECK_ARG(n_rows == 0 || (col && val), "meld_diffuse_step: col and val are required for a matrix with rows");
  {
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + sizeof(double) * (uintptr_t)n_rows * (uintptr_t)ldx;
    const uintptr_t y0 = (uintptr_t)y, y1 = y0 + sizeof(double) * (uintptr_t)n_rows * (uintptr_t)ldy;
    MELD_CHECK_ARG(n_rows == 0 || x1 <= y0 || y1 <= x0, "meld_diffuse_step: y overlaps x (a step reads rows of x other rows have written)");
  }
  if (n_rows == 0) return MELD_OK;
  const int64_t nblk = ceil_div(n_rows, 4 * DIFF_ROWS);
  const unsigned grid = (unsigned)(ceil_div(nblk, 8) * 8);  // multiple of 8: bijective XCD remap
  if (p <= 64)
    hipLaunchKernelGGL(diffuse_step_kernel<1>, dim3(grid), dim3(256), 0, S(stream), rowptr, col, val, kd, s, n_rows, x, ldx, y, ldy, p);
  else
    hipLaunchKernelGGL(diffuse_step_kernel<2>, dim3(grid), dim3(256), 0, S(stream), rowptr, col, val, kd, s, n_rows, x, ldx, y, ldy, p);
  MELD_LAUNCH_CHECK("diffuse_step_kernel");
  return MELD_OK;
}
