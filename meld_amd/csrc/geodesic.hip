// geodesic.hip -- shortest paths along the fitted graph: one synchronous Bellman-Ford round for up to 128 sources at once, and the
// euclidean lengths of the stored entries.
//
// Reference surface: [UPSTREAM graphtools 1.5.x BaseGraph.shortest_path, unpinned: not importable next to this code] -- scipy's
// graph_shortest_path over -log K, over the data distances or over hop counts.
//
//     y[i, c] = min( x[i, c],  min_{e in row i} ( x[col[e], c] + len[e] ) )                      (meld_minplus_step)
//
// The round is diffuse_step_kernel<NC> (csrc/diffuse.hip) with (min, +) in place of (+, x): lanes = COLUMNS = sources, NC = 1 or 2
// columns per lane (lane and lane + 64), a wave owns GEO_ROWS consecutive rows as one stream of entries, the (length, column)
// pairs are loaded a chunk ahead by the first lanes and handed round with v_readlane, the gathers of a chunk are in flight while
// the previous chunk is reduced, 32 rows per workgroup, workgroups XCD-contiguous, 8-byte accesses only.  What differs:
//   * the epilogue of a row is one exact min with the row's own x (no diagonal, no division);
//   * one device word, *changed: a wave that stored an element below the x it replaced stores the constant 1 there from one lane
//     (a plain vector store; every writer writes the same value).  Nothing else is shared between workgroups: no floating-point
//     atomics, no waiting on memory another workgroup writes, no grid barrier; the end of the launch is the only synchronisation.
// The round is out of place (y never overlaps x): a pure function of x, so the number of rounds to the fixed point is the same
// every run.  +inf is "not reached" (inf + len = inf); lengths are finite and >= 0 and distances >= 0 or +inf (the host side
// validates both), so no NaN arises.  An output element is one fp64 add per entry and an exact min: a function of its operands
// alone -- not of p, of the panel, of the leading dimensions or of the other columns in the launch.
// Register budget: as in diffuse.hip the gathers in flight are what the registers go to; the chunk is 16 / NC entries.  As compiled
// (-Rpass-analysis=kernel-resource-usage): NC = 1 takes 120 VGPRs (4 waves per SIMD), NC = 2 takes 138 (3 waves per SIMD), neither
// touches private memory: the diffusion kernel's figures less the diagonal and the row sums it holds.
#include <math.h>

#include "common.hpp"

namespace meld {

constexpr int GEO_ROWS = 8;  // rows per wave (consecutive); 4 waves per workgroup: 32 rows
constexpr int GEO_MAX_COLS = 128;

template <int NC>
__global__ __launch_bounds__(256) void minplus_step_kernel(const int64_t* __restrict__ rowptr, const int* __restrict__ col,
                                                           const double* __restrict__ len, int64_t n_rows,
                                                           const double* __restrict__ x, int64_t ldx, double* __restrict__ y,
                                                           int64_t ldy, int p, int* __restrict__ changed) {
  constexpr int U = 16 / NC;  // entries per chunk = gathers in flight per lane and column
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nb = gridDim.x;  // (a multiple of 8: the remap below is a bijection)
  const int per = (nb + 7) >> 3;
  const int64_t rb = (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (rb >= nb) return;
  const int64_t row_first = (rb * 4 + wv) * GEO_ROWS;
  if (row_first >= n_rows) return;  // (uniform)
  const int n_here = (int)min((int64_t)GEO_ROWS, n_rows - row_first);
  bool on[NC];
  int lc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    on[c] = lane + 64 * c < p;
    lc[c] = on[c] ? lane + 64 * c : 0;  // (an idle lane re-reads column 0: inside the row, never stored)
  }
  // row boundaries of the wave's rows: lane r holds row r, handed round with v_readlane
  const int64_t rp = rowptr[min(row_first + min(lane, n_here), n_rows)];
  // the rows' own distances, column `lane` and column `lane + 64`: register vectors, read at the (uniform) index of the row that
  // closes
  typedef double row_vec __attribute__((ext_vector_type(GEO_ROWS)));
  row_vec xi0, xi1;
#pragma unroll
  for (int r = 0; r < GEO_ROWS; ++r) {
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
  // pairs of the chunk that starts at entry e0 (lane u & (U - 1): entry e0 + u); beyond the wave's stream the length is +inf (it
  // lowers nothing) and the column that of the last entry (row 0 where the wave has no entries at all): always a row of x
  auto fetch_pairs = [&](int64_t e0, double& vv, int& cc) __attribute__((always_inline)) {
    const int64_t e = min(e0 + (lane & (U - 1)), E1 - 1);
    vv = (e0 + (lane & (U - 1)) < E1) ? __builtin_nontemporal_load(len + max(e, (int64_t)0)) : (double)INFINITY;
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
  for (int c = 0; c < NC; ++c) acc[c] = (double)INFINITY;
  bool lowered = false;
  auto flush_rows_until = [&](int64_t e) __attribute__((always_inline)) {  // (uniform) close every row that ends at or before entry e
    while (r_cur < n_here && e >= re_cur) {
      double xr[2] = {xi0[r_cur], 0.0};
      if constexpr (NC > 1) xr[1] = xi1[r_cur];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const bool below = acc[c] < xr[c];
        if (on[c]) {
          __builtin_nontemporal_store(below ? acc[c] : xr[c], y + (row_first + r_cur) * ldy + lane + 64 * c);
          lowered |= below;
        }
        acc[c] = (double)INFINITY;
      }
      ++r_cur;
      re_cur = r_cur < n_here ? rp_at(r_cur + 1) : E1 + 1;
    }
  };
  auto min_chunk = [&](int64_t e0, double vv, const double (&xj)[U][NC]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      flush_rows_until(e0 + u);
      const double v = uniform(vv, u);
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] = fmin(acc[c], xj[u][c] + v);  // (no operand is a NaN: the exact minimum)
    }
  };
  double vA, vB;
  int cA, cB;
  double xA[U][NC], xB[U][NC];
  fetch_pairs(E0, vA, cA);
  fetch_pairs(E0 + U, vB, cB);
  gather(cA, xA);
  for (int64_t e0 = E0; e0 < E1; e0 += 2 * U) {
    // chunk A = [e0, e0 + U), chunk B = [e0 + U, e0 + 2 U); the pairs of the chunk after B and B's gathers go out before A is reduced
    gather(cB, xB);
    double vN;
    int cN;
    fetch_pairs(e0 + 2 * U, vN, cN);
    min_chunk(e0, vA, xA);
    gather(cN, xA);
    double vM;
    int cM;
    fetch_pairs(e0 + 3 * U, vM, cM);
    min_chunk(e0 + U, vB, xB);
    vA = vN;
    cA = cN;
    vB = vM;
    cB = cM;
  }
  // the rows that are left: the last one, and rows without entries (y = x).  (Entries past E1 carry the length +inf and are
  // reduced after every row has been closed at entry E1: they reach no output.)
  flush_rows_until(E1 + 1);
  if (__any(lowered) && lane == 0) *changed = 1;  // (the same value from every wave that lowered an element)
}

// GEO_LANES lanes per row, one stored entry per lane at a time: a lane walks the d columns of the two rows in order
constexpr int GEO_LANES = 16;
constexpr int GEO_THREADS = 256;
constexpr int GEO_MAX_DIMS = 256;

__global__ __launch_bounds__(GEO_THREADS) void edge_lengths_l2_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                                      long long n_rows, const double* __restrict__ X, long long ldX,
                                                                      int d, double* __restrict__ out) {
  const long long t = (long long)blockIdx.x * GEO_THREADS + threadIdx.x;
  const long long i = t / GEO_LANES;
  const int sub = (int)(t % GEO_LANES);
  if (i >= n_rows) return;
  const double* xi = X + i * ldX;
  const long long e1 = rowptr[i + 1];
  for (long long e = rowptr[i] + sub; e < e1; e += GEO_LANES) {
    const double* xj = X + (long long)col[e] * ldX;
    double acc = 0.0;
    for (int k = 0; k < d; ++k) {
      const double df = xi[k] - xj[k];  // ((a - b)^2 == (b - a)^2 exactly, the order is fixed: len(i, j) and len(j, i) are bit-equal)
      acc = fma(df, df, acc);
    }
    out[e] = sqrt(acc);
  }
}

}  // namespace meld

using namespace meld;

extern "C" int meld_minplus_max_cols(void) { return GEO_MAX_COLS; }

extern "C" int meld_minplus_step(const int64_t* rowptr, const int32_t* col, const double* len, int64_t n_rows, const double* x,
                                 int64_t ldx, double* y, int64_t ldy, int p, int32_t* changed, meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && x && y && changed, "meld_minplus_step: rowptr, x, y and changed are required");
  MELD_CHECK_ARG(n_rows >= 0, "meld_minplus_step: n_rows=%lld is negative", (long long)n_rows);
  MELD_CHECK_ARG(p >= 1 && p <= GEO_MAX_COLS, "meld_minplus_step: p=%d columns (1 <= p <= %d per call)", p, GEO_MAX_COLS);
  MELD_CHECK_ARG(ldx >= p && ldy >= p, "meld_minplus_step: leading dimensions ldx=%lld, ldy=%lld below p=%d", (long long)ldx,
                 (long long)ldy, p);
  MELD_CHECK_ARG(n_rows == 0 || (col && len), "meld_minplus_step: col and len are required for a matrix with rows");
  {
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + sizeof(double) * (uintptr_t)n_rows * (uintptr_t)ldx;
    const uintptr_t y0 = (uintptr_t)y, y1 = y0 + sizeof(double) * (uintptr_t)n_rows * (uintptr_t)ldy;
    MELD_CHECK_ARG(n_rows == 0 || x1 <= y0 || y1 <= x0, "meld_minplus_step: y overlaps x (a round reads rows of x other rows have written)");
  }
  MELD_HIP_CALL(hipMemsetAsync(changed, 0, 4, S(stream)));
  if (n_rows == 0) return MELD_OK;
  const int64_t nblk = ceil_div(n_rows, 4 * GEO_ROWS);
  const unsigned grid = (unsigned)(ceil_div(nblk, 8) * 8);  // multiple of 8: bijective XCD remap
  if (p <= 64)
    hipLaunchKernelGGL(minplus_step_kernel<1>, dim3(grid), dim3(256), 0, S(stream), rowptr, col, len, n_rows, x, ldx, y, ldy, p, changed);
  else
    hipLaunchKernelGGL(minplus_step_kernel<2>, dim3(grid), dim3(256), 0, S(stream), rowptr, col, len, n_rows, x, ldx, y, ldy, p, changed);
  MELD_LAUNCH_CHECK("minplus_step_kernel");
  return MELD_OK;
}

extern "C" int meld_edge_lengths_l2(const int64_t* rowptr, const int32_t* col, int64_t n_rows, const double* X, int64_t ldX, int d,
                                    double* out, meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && X, "meld_edge_lengths_l2: rowptr and X are required");
  MELD_CHECK_ARG(n_rows >= 0 && n_rows < (1ll << 31), "meld_edge_lengths_l2: n_rows=%lld outside [0, 2^31)", (long long)n_rows);
  MELD_CHECK_ARG(d >= 1 && d <= GEO_MAX_DIMS, "meld_edge_lengths_l2: d=%d columns (1 <= d <= %d)", d, GEO_MAX_DIMS);
  MELD_CHECK_ARG(ldX >= d, "meld_edge_lengths_l2: leading dimension ldX=%lld below d=%d", (long long)ldX, d);
  MELD_CHECK_ARG(n_rows == 0 || (col && out), "meld_edge_lengths_l2: col and out are required for a matrix with rows");
  if (n_rows == 0) return MELD_OK;
  edge_lengths_l2_kernel<<<(unsigned)ceil_div(n_rows * GEO_LANES, GEO_THREADS), GEO_THREADS, 0, S(stream)>>>(
      reinterpret_cast<const long long*>(rowptr), col, (long long)n_rows, X, (long long)ldX, d, out);
  MELD_LAUNCH_CHECK("edge_lengths_l2_kernel");
  return MELD_OK;
}
