// diffuse.hip -- one step of the random walk of the kernel matrix on a wide fp64 signal (MAGIC-style diffusion of cell signals).
//
// Reference surface: graphtools' diff_op = normalize(K, "l1", axis=1) with K = W + diag(kd) (DeviceGraph.diff_op builds it on the
// host), applied as [UPSTREAM magic-impute, unpinned: not importable next to this code] applies it: X <- diff_op X, t times.
//
//     y[i, c] = ( sum_{e in row i, storage order} val[e] x[col[e], c]  +  kd[i] x[i, c] ) / s[i],      s = dw + kd
//
// The pass over the matrix is wave_stream_rows<NC> (csr_wave_stream.hpp: lanes = COLUMNS, 8 rows per wave as one stream of entries,
// NC = 1 or 2 columns per lane).  What is the kernel's own:
//   * the epilogue is per row (the kernel's diagonal and ONE true division by the row sum of K), not a scalar combination;
//   * x and y have leading dimensions: a wider signal is processed in column panels without copies.
// As compiled: NC = 1 takes 122 VGPRs (4 waves per SIMD), NC = 2 takes 142 (3 waves per SIMD), neither touches private memory;
// capping NC = 2 at 128 registers (__launch_bounds__(256, 4)) spills 20 of them into the loop and is not done.
// The accumulation of one output element is written with explicit fma calls, in storage order, the diagonal term last: its value
// is a function of the operands alone -- not of p, of the panel, of the leading dimensions or of the other columns in the launch.
#include "csr_wave_stream.hpp"

namespace meld {

template <int NC>
struct DiffuseOp {
  const double* __restrict__ kd;
  const double* __restrict__ s;
  const double* __restrict__ x;
  int64_t ldx;
  double* __restrict__ y;
  int64_t ldy;
  double kdl, sl;   // lane r: the kernel's diagonal and the row sum of the wave's row r
  own_rows<NC> xi;  // the rows' own x
  __device__ __forceinline__ void load_rows(const wave_rows<NC>& w) {
    kdl = kd[w.lane_row()];
    sl = s[w.lane_row()];
    xi.load(x, ldx, w);
  }
  static __device__ __forceinline__ double pad() { return 0.0; }
  static __device__ __forceinline__ double identity() { return 0.0; }
  static __device__ __forceinline__ double combine(double acc, double v, double xj) { return fma(v, xj, acc); }
  __device__ __forceinline__ void close_row(int r, int64_t row, const double (&acc)[NC], const bool (&on)[NC], int lane) {
    const double kdr = wave_uniform(kdl, r), sr = wave_uniform(sl, r);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (on[c]) __builtin_nontemporal_store(fma(kdr, xi.v[c][r], acc[c]) / sr, y + row * ldy + lane + 64 * c);
  }
};

template <int NC>
__global__ __launch_bounds__(256) void diffuse_step_kernel(const int64_t* __restrict__ rowptr, const int* __restrict__ col,
                                                           const double* __restrict__ val, const double* __restrict__ kd,
                                                           const double* __restrict__ s, int64_t n_rows,
                                                           const double* __restrict__ x, int64_t ldx, double* __restrict__ y,
                                                           int64_t ldy, int p) {
  DiffuseOp<NC> op{kd, s, x, ldx, y, ldy};
  wave_stream_rows<NC>(rowptr, col, val, n_rows, x, ldx, p, op);
}

}  // namespace meld

using namespace meld;

extern "C" int meld_diffuse_max_cols(void) { return WAVE_STREAM_MAX_COLS; }

extern "C" int meld_diffuse_step(const int64_t* rowptr, const int32_t* col, const double* val, const double* kd, const double* s,
                                 int64_t n_rows, const double* x, int64_t ldx, double* y, int64_t ldy, int p, meld_stream_t stream) {
  if (int e = check_panel_step("meld_diffuse_step", rowptr && kd && s && x && y, "rowptr, kd, s, x and y", "val", "step", col, val, n_rows,
                               x, ldx, y, ldy, p))
    return e;
  if (n_rows == 0) return MELD_OK;
  const unsigned grid = wave_stream_grid(n_rows);
  if (p <= 64)
    hipLaunchKernelGGL(diffuse_step_kernel<1>, dim3(grid), dim3(256), 0, S(stream), rowptr, col, val, kd, s, n_rows, x, ldx, y, ldy, p);
  else
    hipLaunchKernelGGL(diffuse_step_kernel<2>, dim3(grid), dim3(256), 0, S(stream), rowptr, col, val, kd, s, n_rows, x, ldx, y, ldy, p);
  MELD_LAUNCH_CHECK("diffuse_step_kernel");
  return MELD_OK;
}
