// geodesic.hip -- shortest paths along the fitted graph: one synchronous Bellman-Ford round for up to 128 sources at once, and the
// euclidean lengths of the stored entries.
//
// Reference surface: [UPSTREAM graphtools 1.5.x BaseGraph.shortest_path, unpinned: not importable next to this code] -- scipy's
// graph_shortest_path over -log K, over the data distances or over hop counts.
//
//     y[i, c] = min( x[i, c],  min_{e in row i} ( x[col[e], c] + len[e] ) )                      (meld_minplus_step)
//
// The round is the pass of csr_wave_stream.hpp with (min, +) in place of (+, x): lanes = COLUMNS = sources, NC = 1 or 2 columns per
// lane, 8 rows per wave as one stream of (length, column) pairs.  What is the kernel's own:
//   * the epilogue of a row is one exact min with the row's own x (no diagonal, no division);
//   * one device word, *changed: a wave that stored an element below the x it replaced stores the constant 1 there from one lane
//     (a plain vector store; every writer writes the same value).  Nothing else is shared between workgroups: no floating-point
//     atomics, no waiting on memory another workgroup writes, no grid barrier; the end of the launch is the only synchronisation.
// The round is out of place (y never overlaps x): a pure function of x, so the number of rounds to the fixed point is the same
// every run.  +inf is "not reached" (inf + len = inf), and the length of an entry past the wave's stream (it lowers nothing);
// lengths are finite and >= 0 and distances >= 0 or +inf (the host side validates both), so no NaN arises.  An output element is
// one fp64 add per entry and an exact min: a function of its operands alone -- not of p, of the panel, of the leading dimensions
// or of the other columns in the launch.
// As compiled (-Rpass-analysis=kernel-resource-usage): NC = 1 takes 120 VGPRs (4 waves per SIMD), NC = 2 takes 137 (3 waves per
// SIMD), neither touches private memory: the diffusion kernel's figures less the diagonal and the row sums it holds.
#include <math.h>

#include "csr_wave_stream.hpp"

namespace meld {

template <int NC>
struct MinPlusOp {
  const double* __restrict__ x;
  int64_t ldx;
  double* __restrict__ y;
  int64_t ldy;
  own_rows<NC> xi;  // the rows' own distances
  bool lowered = false;
  __device__ __forceinline__ void load_rows(const wave_rows<NC>& w) { xi.load(x, ldx, w); }
  static __device__ __forceinline__ double pad() { return (double)INFINITY; }
  static __device__ __forceinline__ double identity() { return (double)INFINITY; }
  // (no operand is a NaN: the exact minimum)
  static __device__ __forceinline__ double combine(double acc, double v, double xj) { return fmin(acc, xj + v); }
  __device__ __forceinline__ void close_row(int r, int64_t row, const double (&acc)[NC], const bool (&on)[NC], int lane) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double xr = xi.v[c][r];
      const bool below = acc[c] < xr;
      if (on[c]) {
        __builtin_nontemporal_store(below ? acc[c] : xr, y + row * ldy + lane + 64 * c);  // (a row without entries: y = x)
        lowered |= below;
      }
    }
  }
};

template <int NC>
__global__ __launch_bounds__(256) void minplus_step_kernel(const int64_t* __restrict__ rowptr, const int* __restrict__ col,
                                                           const double* __restrict__ len, int64_t n_rows,
                                                           const double* __restrict__ x, int64_t ldx, double* __restrict__ y,
                                                           int64_t ldy, int p, int* __restrict__ changed) {
  MinPlusOp<NC> op{x, ldx, y, ldy};
  wave_stream_rows<NC>(rowptr, col, len, n_rows, x, ldx, p, op);
  if (__any(op.lowered) && (threadIdx.x & 63) == 0) *changed = 1;  // (the same value from every wave that lowered an element)
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

extern "C" int meld_minplus_max_cols(void) { return WAVE_STREAM_MAX_COLS; }

extern "C" int meld_minplus_step(const int64_t* rowptr, const int32_t* col, const double* len, int64_t n_rows, const double* x,
                                 int64_t ldx, double* y, int64_t ldy, int p, int32_t* changed, meld_stream_t stream) {
  if (int e = check_panel_step("meld_minplus_step", rowptr && x && y && changed, "rowptr, x, y and changed", "len", "round", col, len,
                               n_rows, x, ldx, y, ldy, p))
    return e;
  MELD_HIP_CALL(hipMemsetAsync(changed, 0, 4, S(stream)));
  if (n_rows == 0) return MELD_OK;
  const unsigned grid = wave_stream_grid(n_rows);
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
