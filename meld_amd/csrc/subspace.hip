// subspace.hip -- the tall-block algebra of the partial Fourier basis (meld_amd/spectrum.py): Gram matrix, rotation and
// residual norms of row-major fp64 blocks [n_rows, m], 1 <= m <= 64, leading dimension ld >= m.
//
// Stands for [UPSTREAM pygsp (development line) Graph.compute_fourier_basis(n_eigenvectors=k)], which runs ARPACK on the host;
// here the k smoothest eigenpairs come from a Chebyshev-filtered subspace iteration (Zhou & Saad) whose products with L are
// meld_cheby_step_wide (csrc/spmm.hip) and whose Rayleigh-Ritz step is the three passes below.
//
// Layout: the Gram matrix and the rotation are fp64 matrix-core products (v_mfma_f64_16x16x4_f64: one f64 of A and of B per lane,
// A[l & 15][k = l >> 4], B[k = l >> 4][l & 15]; four results per lane, D[(l >> 4) + 4 q][l & 15]).  A wave owns BLK_ROWS = 16
// consecutive rows at a time.  Gram: k runs over the ROWS, both operands are read as [row i0 + 4 u + (l >> 4)][column 16 t +
// (l & 15)] -- 16 lanes per 128 contiguous bytes.  Rotation: k runs over the columns of A, whose 16 rows a wave reads whole
// (lane: row i0 + (l & 15), columns 4 s + (l >> 4)) before it writes any of them; S comes out of LDS.  The residuals are
// lanes = columns, as in cheby_step_wide_kernel.  The column count is rounded up to 16 T, T in {1, 2, 4}, at compile time so that
// the accumulators stay in registers; columns m .. 16 T - 1 are zeros that are never loaded and never stored.
//
// Determinism: no floating-point atomics.  Workgroup b owns the rows [b per, (b + 1) per), per = ceil(n_rows / n_blocks); its
// four waves take those rows in groups of BLK_ROWS, wave w the groups w, w + 4, ..., each in row order; the waves' sums meet in
// LDS in wave order, the workgroup writes its partial to part[b], and a second launch adds the partials in workgroup order.  The
// result is a function of the operands and of n_blocks alone: the same bits every run.
#include "common.hpp"

namespace meld {

constexpr int BLK_THREADS = 256;
constexpr int BLK_WAVES = BLK_THREADS / 64;
constexpr int BLK_ROWS = 16;  // rows a wave holds in registers at a time
constexpr int BLK_MAX_BLOCKS = 1024;
constexpr int BLK_MMAX = 64;
constexpr int BLK_S_LD = 80;  // row stride of S in LDS (doubles): the four k rows of an operand read fall on disjoint banks

typedef double double4_t __attribute__((ext_vector_type(4)));

// part[b][l][j] = sum over the rows of workgroup b of A[i][l] B[i][j]   (l, j < m; [m, m] row-major per workgroup)
template <int T>
__global__ __launch_bounds__(BLK_THREADS) void block_gram_kernel(const double* __restrict__ A, int64_t lda, const double* __restrict__ B,
                                                                 int64_t ldb, int64_t n_rows, int m, double* __restrict__ part) {
  __shared__ double s_c[16 * T * 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int64_t per = (n_rows + gridDim.x - 1) / gridDim.x;
  const int64_t r_begin = (int64_t)blockIdx.x * per, r_end = min(n_rows, r_begin + per);
  double4_t acc[T][T];
#pragma unroll
  for (int ta = 0; ta < T; ++ta)
#pragma unroll
    for (int tb = 0; tb < T; ++tb) acc[ta][tb] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int64_t i0 = r_begin + (int64_t)wv * BLK_ROWS; i0 < r_end; i0 += BLK_WAVES * BLK_ROWS) {
    double a[BLK_ROWS / 4][T], b[BLK_ROWS / 4][T];
#pragma unroll
    for (int u = 0; u < BLK_ROWS / 4; ++u) {
      const int64_t row = i0 + 4 * u + g;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const bool live = row < r_end && 16 * t + c < m;
        a[u][t] = live ? A[row * lda + 16 * t + c] : 0.0;
        b[u][t] = live ? B[row * ldb + 16 * t + c] : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < BLK_ROWS / 4; ++u)
#pragma unroll
      for (int ta = 0; ta < T; ++ta)
#pragma unroll
        for (int tb = 0; tb < T; ++tb) acc[ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][ta], b[u][tb], acc[ta][tb], 0, 0, 0);
  }
  for (int w = 0; w < BLK_WAVES; ++w) {  // the waves' sums meet in wave order
    if (wv == w) {
#pragma unroll
      for (int ta = 0; ta < T; ++ta)
#pragma unroll
        for (int tb = 0; tb < T; ++tb)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int idx = (16 * ta + g + 4 * q) * 64 + 16 * tb + c;
            s_c[idx] = (w == 0 ? 0.0 : s_c[idx]) + acc[ta][tb][q];
          }
    }
    __syncthreads();
  }
  double* out = part + (size_t)blockIdx.x * m * m;
  for (int e = threadIdx.x; e < m * m; e += BLK_THREADS) out[e] = s_c[(e / m) * 64 + (e % m)];
}

// out[e] = part[0][e] + part[1][e] + ... in workgroup order
__global__ __launch_bounds__(BLK_THREADS) void block_sum_partials_kernel(const double* __restrict__ part, int n_blocks, int len,
                                                                         double* __restrict__ out) {
  const int e = blockIdx.x * BLK_THREADS + threadIdx.x;
  if (e >= len) return;
  double s = 0.0;
  for (int b = 0; b < n_blocks; ++b) s += part[(size_t)b * len + e];
  out[e] = s;
}

// out[i][j] = sum_l A[i][l] S[l][j]; a wave reads its BLK_ROWS rows whole before it writes them (out may alias A)
template <int T>
__global__ __launch_bounds__(BLK_THREADS) void block_rotate_kernel(const double* A, int64_t lda, const double* __restrict__ S,
                                                                   int64_t n_rows, int m, double* out, int64_t ldo) {
  __shared__ double s_s[16 * T * BLK_S_LD];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  for (int e = threadIdx.x; e < 16 * T * 64; e += BLK_THREADS) {
    const int l = e >> 6, j = e & 63;
    s_s[l * BLK_S_LD + j] = (l < m && j < m) ? S[l * m + j] : 0.0;
  }
  __syncthreads();
  const int64_t per = (n_rows + gridDim.x - 1) / gridDim.x;
  const int64_t r_begin = (int64_t)blockIdx.x * per, r_end = min(n_rows, r_begin + per);
  for (int64_t i0 = r_begin + (int64_t)wv * BLK_ROWS; i0 < r_end; i0 += BLK_WAVES * BLK_ROWS) {
    double a[4 * T];
#pragma unroll
    for (int s = 0; s < 4 * T; ++s) a[s] = (i0 + c < r_end && 4 * s + g < m) ? A[(i0 + c) * lda + 4 * s + g] : 0.0;
    double4_t acc[T];
#pragma unroll
    for (int tj = 0; tj < T; ++tj) {
      acc[tj] = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4 * T; ++s)
        acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], s_s[(4 * s + g) * BLK_S_LD + 16 * tj + c], acc[tj], 0, 0, 0);
    }
#pragma unroll
    for (int tj = 0; tj < T; ++tj)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t row = i0 + g + 4 * q;
        if (row < r_end && 16 * tj + c < m) out[row * ldo + 16 * tj + c] = acc[tj][q];
      }
  }
}

// part[b][j] = sum over the rows of workgroup b of (LV[i][j] - theta[j] V[i][j])^2
__global__ __launch_bounds__(BLK_THREADS) void block_residuals_kernel(const double* __restrict__ LV, const double* __restrict__ V,
                                                                      int64_t ld, const double* __restrict__ theta, int64_t n_rows,
                                                                      int m, double* __restrict__ part) {
  __shared__ double s_r[BLK_WAVES * 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool on = lane < m;
  const double th = on ? theta[lane] : 0.0;
  const int64_t per = (n_rows + gridDim.x - 1) / gridDim.x;
  const int64_t r_begin = (int64_t)blockIdx.x * per, r_end = min(n_rows, r_begin + per);
  double acc = 0.0;
  for (int64_t i0 = r_begin + (int64_t)wv * BLK_ROWS; i0 < r_end; i0 += BLK_WAVES * BLK_ROWS) {
    double d[BLK_ROWS];
#pragma unroll
    for (int r = 0; r < BLK_ROWS; ++r) {
      const bool live = on && i0 + r < r_end;
      d[r] = live ? LV[(i0 + r) * ld + lane] - th * V[(i0 + r) * ld + lane] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < BLK_ROWS; ++r) acc = fma(d[r], d[r], acc);
  }
  s_r[wv * 64 + lane] = acc;
  __syncthreads();
  if (wv == 0 && on) {
    double s = s_r[lane];
    for (int w = 1; w < BLK_WAVES; ++w) s += s_r[w * 64 + lane];
    part[(size_t)blockIdx.x * m + lane] = s;
  }
}

static inline int block_tiles(int m) { return m <= 16 ? 1 : m <= 32 ? 2 : 4; }  // 16-column tiles per side

}  // namespace meld

using namespace meld;

extern "C" int meld_block_max_blocks(void) { return BLK_MAX_BLOCKS; }

extern "C" int meld_block_gram_f64(const double* A, int64_t lda, const double* B, int64_t ldb, int64_t n_rows, int m, double* part,
                                   int n_blocks, double* C, meld_stream_t stream) {
  MELD_CHECK_ARG(A && B && part && C && n_rows >= 0 && m >= 1 && m <= BLK_MMAX && lda >= m && ldb >= m && n_blocks >= 1 &&
                     n_blocks <= BLK_MAX_BLOCKS,
                 "meld_block_gram_f64: bad arguments (1 <= m <= %d <= ld, 1 <= n_blocks <= %d)", BLK_MMAX, BLK_MAX_BLOCKS);
  switch (block_tiles(m)) {
#define MELD_GRAM_CASE(T)                                                                                                        \
  case T:                                                                                                                        \
    hipLaunchKernelGGL((block_gram_kernel<T>), dim3(n_blocks), dim3(BLK_THREADS), 0, S(stream), A, lda, B, ldb, n_rows, m, part); \
    break;
    MELD_GRAM_CASE(1)
    MELD_GRAM_CASE(2)
    MELD_GRAM_CASE(4)
#undef MELD_GRAM_CASE
  }
  MELD_LAUNCH_CHECK("block_gram_kernel");
  hipLaunchKernelGGL(block_sum_partials_kernel, dim3((unsigned)ceil_div(m * m, BLK_THREADS)), dim3(BLK_THREADS), 0, S(stream), part,
                     n_blocks, m * m, C);
  MELD_LAUNCH_CHECK("block_sum_partials_kernel");
  return MELD_OK;
}

extern "C" int meld_block_rotate_f64(const double* A, int64_t lda, const double* Smat, int64_t n_rows, int m, double* out, int64_t ldo,
                                     meld_stream_t stream) {
  MELD_CHECK_ARG(A && Smat && out && n_rows >= 0 && m >= 1 && m <= BLK_MMAX && lda >= m && ldo >= m,
                 "meld_block_rotate_f64: bad arguments (1 <= m <= %d <= ld)", BLK_MMAX);
  if (n_rows == 0) return MELD_OK;
  const int64_t groups = ceil_div(n_rows, BLK_WAVES * BLK_ROWS);
  const unsigned grid = (unsigned)(groups < 2 * BLK_MAX_BLOCKS ? groups : 2 * BLK_MAX_BLOCKS);
  switch (block_tiles(m)) {
#define MELD_ROTATE_CASE(T)                                                                                                        \
  case T:                                                                                                                          \
    hipLaunchKernelGGL((block_rotate_kernel<T>), dim3(grid), dim3(BLK_THREADS), 0, S(stream), A, lda, Smat, n_rows, m, out, ldo); \
    break;
    MELD_ROTATE_CASE(1)
    MELD_ROTATE_CASE(2)
    MELD_ROTATE_CASE(4)
#undef MELD_ROTATE_CASE
  }
  MELD_LAUNCH_CHECK("block_rotate_kernel");
  return MELD_OK;
}

extern "C" int meld_block_residuals_f64(const double* LV, const double* V, int64_t ld, const double* theta, int64_t n_rows, int m,
                                        double* part, int n_blocks, double* out, meld_stream_t stream) {
  MELD_CHECK_ARG(LV && V && theta && part && out && n_rows >= 0 && m >= 1 && m <= BLK_MMAX && ld >= m && n_blocks >= 1 &&
                     n_blocks <= BLK_MAX_BLOCKS,
                 "meld_block_residuals_f64: bad arguments (1 <= m <= %d <= ld, 1 <= n_blocks <= %d)", BLK_MMAX, BLK_MAX_BLOCKS);
  hipLaunchKernelGGL(block_residuals_kernel, dim3(n_blocks), dim3(BLK_THREADS), 0, S(stream), LV, V, ld, theta, n_rows, m, part);
  MELD_LAUNCH_CHECK("block_residuals_kernel");
  hipLaunchKernelGGL(block_sum_partials_kernel, dim3(1), dim3(BLK_THREADS), 0, S(stream), part, n_blocks, m, out);
  MELD_LAUNCH_CHECK("block_sum_partials_kernel");
  return MELD_OK;
}
