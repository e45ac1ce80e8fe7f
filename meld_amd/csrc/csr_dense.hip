// csr_dense.hip -- products of a sparse cell-by-gene matrix (CSR) with tall-skinny dense fp64 matrices, the transpose of that
// matrix and its densification: the sparse front end of the graph builder (meld_amd/sparse.py; replaces [UPSTREAM graphtools
// Data._reduce_data -> sklearn TruncatedSVD] on scipy.sparse input, reached from meld/meld.py:273).
//
// Product mapping: one wave per work unit, a unit being a segment of at most MELD_CSR_SEG entries of one row, in storage order.
// The lanes hold two adjacent columns each of a 128-column panel of the dense operand, so one wave instruction moves one
// operand row (64 lanes x 16 B); the unit's column indices and values are loaded 64 at a time, one per lane, and read out
// with v_readlane (scalar registers: the operand row address is scalar).  Four operand rows are in flight per wave; the
// multiply-adds stay in storage order.  A row of more than MELD_CSR_SEG entries has one unit per segment: each writes its
// partial sum to a slot of `partial`, and a second pass adds the partials in segment order.  The result is a function of
// the matrix and the operand alone (no atomics, no dependence on the launch shape).
#include "common.hpp"

using namespace meld;

namespace {

constexpr int PANEL = 128;  // columns of the dense operand per pass of a unit (64 lanes x 2)
constexpr int INFLIGHT = 4; // operand rows in flight per wave

template <bool F32>
__device__ __forceinline__ double load_val(const void* val, int64_t j) {
  if constexpr (F32) return (double)reinterpret_cast<const float*>(val)[j];
  else return reinterpret_cast<const double*>(val)[j];
}

__device__ __forceinline__ double readlane_f64(double v, int l) {
  const int64_t b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffff), l);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
  return __longlong_as_double(((int64_t)(unsigned)lo) | ((int64_t)hi << 32));
}

// the two operand entries of this lane in row `row`; VEC: 16-byte loads (ld and base 16-byte aligned, c even)
template <bool VEC>
__device__ __forceinline__ void load_pair(const double* __restrict__ B, int64_t ldb, int64_t row, int c, int r, double& b0,
                                          double& b1) {
  const double* p = B + row * ldb + c;
  if (VEC && c + 1 < r) {
    const double2 v = *reinterpret_cast<const double2*>(p);
    b0 = v.x;
    b1 = v.y;
  } else {
    b0 = c < r ? p[0] : 0.0;
    b1 = c + 1 < r ? p[1] : 0.0;
  }
}

template <bool VEC>
__device__ __forceinline__ void store_pair(double* __restrict__ Y, int64_t ldy, int64_t row, int c, int r, double a0, double a1) {
  double* p = Y + row * ldy + c;
  if (VEC && c + 1 < r) {
    *reinterpret_cast<double2*>(p) = make_double2(a0, a1);
  } else {
    if (c < r) p[0] = a0;
    if (c + 1 < r) p[1] = a1;
  }
}

// One wave per unit.  unit_row[u]: row of unit u (units of a row consecutive, in segment order); unit_off[i]: first unit of
// row i; part_off[i]: first partial slot of row i (rows of one segment write Y directly).
template <bool F32, bool VEC>
__global__ __launch_bounds__(256) void csr_spmm_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                       const void* __restrict__ val, const int32_t* __restrict__ unit_row,
                                                       const int64_t* __restrict__ unit_off, const int64_t* __restrict__ part_off,
                                                       int64_t n_units, const double* __restrict__ B, int64_t ldb, int r,
                                                       double* __restrict__ Y, int64_t ldy, double* __restrict__ partial) {
  const int64_t u = (int64_t)blockIdx.x * (blockDim.x / WAVE) + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  if (u >= n_units) return;
  const int lane = lane_id();
  const int64_t row = unit_row[u];
  const int64_t seg = u - unit_off[row];
  const int64_t rb = rowptr[row], re = rowptr[row + 1];
  const bool split = (re - rb) > MELD_CSR_SEG;
  const int64_t jb = rb + seg * MELD_CSR_SEG;
  const int64_t je = min(re, jb + (int64_t)MELD_CSR_SEG);
  double* out = split ? partial : Y;
  const int64_t out_row = split ? part_off[row] + seg : row;
  const int64_t ldo = split ? (int64_t)r : ldy;
  for (int c0 = 0; c0 < r; c0 += PANEL) {
    const int c = c0 + 2 * lane;
    double a0 = 0.0, a1 = 0.0;
    for (int64_t base = jb; base < je; base += WAVE) {
      const int cnt = (int)min((int64_t)WAVE, je - base);
      int my_col = 0;
      double my_val = 0.0;
      if (lane < cnt) {
        my_col = col[base + lane];
        my_val = load_val<F32>(val, base + lane);
      }
      int k = 0;
      for (; k + INFLIGHT <= cnt; k += INFLIGHT) {
        double b0[INFLIGHT], b1[INFLIGHT], v[INFLIGHT];
#pragma unroll
        for (int q = 0; q < INFLIGHT; ++q) {
          const int64_t brow = __builtin_amdgcn_readlane(my_col, k + q);
          v[q] = readlane_f64(my_val, k + q);
          load_pair<VEC>(B, ldb, brow, c, r, b0[q], b1[q]);
        }
#pragma unroll
        for (int q = 0; q < INFLIGHT; ++q) {
          a0 = __fma_rn(v[q], b0[q], a0);
          a1 = __fma_rn(v[q], b1[q], a1);
        }
      }
      for (; k < cnt; ++k) {
        const int64_t brow = __builtin_amdgcn_readlane(my_col, k);
        const double v = readlane_f64(my_val, k);
        double b0, b1;
        load_pair<VEC>(B, ldb, brow, c, r, b0, b1);
        a0 = __fma_rn(v, b0, a0);
        a1 = __fma_rn(v, b1, a1);
      }
    }
    store_pair<VEC>(out, ldo, out_row, c, r, a0, a1);
  }
}

// second pass: one wave per split row, its partials added in segment order
__global__ __launch_bounds__(256) void csr_spmm_merge_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ split_rows,
                                                             int64_t n_split_rows, const int64_t* __restrict__ part_off,
                                                             const double* __restrict__ partial, int r, double* __restrict__ Y,
                                                             int64_t ldy) {
  const int64_t w = (int64_t)blockIdx.x * (blockDim.x / WAVE) + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  if (w >= n_split_rows) return;
  const int64_t row = split_rows[w];
  const int64_t nseg = (rowptr[row + 1] - rowptr[row] + MELD_CSR_SEG - 1) / MELD_CSR_SEG;
  const double* p = partial + part_off[row] * (int64_t)r;
  for (int c = lane_id(); c < r; c += WAVE) {
    double s = 0.0;
    for (int64_t q = 0; q < nseg; ++q) s += p[q * r + c];
    Y[row * ldy + c] = s;
  }
}

// keys (column << 32 | row) and fp64 values of every entry, in storage order: the input of the sort that transposes
template <bool F32>
__global__ __launch_bounds__(256) void csr_transpose_keys_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                 const void* __restrict__ val, int64_t n_rows,
                                                                 uint64_t* __restrict__ keys, double* __restrict__ vals) {
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x / WAVE) + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  if (row >= n_rows) return;
  for (int64_t j = rowptr[row] + lane_id(); j < rowptr[row + 1]; j += WAVE) {
    keys[j] = ((uint64_t)(uint32_t)col[j] << 32) | (uint64_t)row;
    vals[j] = load_val<F32>(val, j);
  }
}

template <bool F32>
__global__ __launch_bounds__(256) void csr_rows_to_dense_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                const void* __restrict__ val, int64_t row_begin, int64_t n_rows,
                                                                double* __restrict__ out, int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.x * (blockDim.x / WAVE) + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  if (i >= n_rows) return;
  const int64_t row = row_begin + i;
  for (int64_t j = rowptr[row] + lane_id(); j < rowptr[row + 1]; j += WAVE) out[i * ldo + col[j]] = load_val<F32>(val, j);
}

inline unsigned waves_grid(int64_t n) { return (unsigned)ceil_div(n, 256 / WAVE); }

}  // namespace

extern "C" int meld_csr_seg_length(void) { return MELD_CSR_SEG; }

extern "C" int meld_csr_spmm_f64(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_rows,
                                 const int32_t* unit_row, const int64_t* unit_off, int64_t n_units, const int64_t* part_off,
                                 const int32_t* split_rows, int64_t n_split_rows, double* partial, const double* B, int64_t ldb,
                                 int r, double* Y, int64_t ldy, meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && unit_row && unit_off && part_off && B && Y && n_rows > 0 && n_units >= n_rows && r >= 1 && ldb >= r &&
                     ldy >= r && n_split_rows >= 0 && (n_split_rows == 0 || (split_rows && partial)),
                 "meld_csr_spmm_f64: bad arguments (n_rows=%lld n_units=%lld r=%d ldb=%lld ldy=%lld)", (long long)n_rows,
                 (long long)n_units, r, (long long)ldb, (long long)ldy);
  const bool vec = (ldb % 2 == 0) && (ldy % 2 == 0) && (r % 2 == 0 || n_split_rows == 0) &&
                   ((uintptr_t)B % 16 == 0) && ((uintptr_t)Y % 16 == 0) && ((uintptr_t)partial % 16 == 0);
  const dim3 grid(waves_grid(n_units)), block(256);
  hipStream_t st = S(stream);
#define MELD_SPMM_LAUNCH(F, V)                                                                                                      \
  hipLaunchKernelGGL((csr_spmm_kernel<F, V>), grid, block, 0, st, rowptr, col, val, unit_row, unit_off, part_off, n_units, B, ldb, \
                     r, Y, ldy, partial)
  if (val_f32) {
    if (vec) MELD_SPMM_LAUNCH(true, true);
    else MELD_SPMM_LAUNCH(true, false);
  } else {
    if (vec) MELD_SPMM_LAUNCH(false, true);
    else MELD_SPMM_LAUNCH(false, false);
  }
#undef MELD_SPMM_LAUNCH
  MELD_LAUNCH_CHECK("csr_spmm_kernel");
  if (n_split_rows > 0) {
    hipLaunchKernelGGL(csr_spmm_merge_kernel, dim3(waves_grid(n_split_rows)), block, 0, st, rowptr, split_rows, n_split_rows,
                       part_off, partial, r, Y, ldy);
    MELD_LAUNCH_CHECK("csr_spmm_merge_kernel");
  }
  return MELD_OK;
}

extern "C" int meld_csr_transpose_keys(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_rows,
                                       uint64_t* keys, double* vals, meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && n_rows > 0 && n_rows <= INT32_MAX, "meld_csr_transpose_keys: bad arguments (n_rows=%lld)", (long long)n_rows);
  if (val_f32)
    hipLaunchKernelGGL(csr_transpose_keys_kernel<true>, dim3(waves_grid(n_rows)), dim3(256), 0, S(stream), rowptr, col, val, n_rows, keys, vals);
  else
    hipLaunchKernelGGL(csr_transpose_keys_kernel<false>, dim3(waves_grid(n_rows)), dim3(256), 0, S(stream), rowptr, col, val, n_rows, keys, vals);
  MELD_LAUNCH_CHECK("csr_transpose_keys_kernel");
  return MELD_OK;
}

extern "C" int meld_csr_rows_to_dense_f64(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t row_begin,
                                          int64_t n_rows, int64_t n_cols, double* out, int64_t ldo, meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && out && row_begin >= 0 && n_rows >= 0 && n_cols >= 1 && ldo >= n_cols,
                 "meld_csr_rows_to_dense_f64: bad arguments (n_cols=%lld ldo=%lld)", (long long)n_cols, (long long)ldo);
  if (n_rows == 0) return MELD_OK;
  MELD_HIP_CALL(hipMemset2DAsync(out, (size_t)ldo * sizeof(double), 0, (size_t)n_cols * sizeof(double), (size_t)n_rows, S(stream)));
  if (val_f32)
    hipLaunchKernelGGL(csr_rows_to_dense_kernel<true>, dim3(waves_grid(n_rows)), dim3(256), 0, S(stream), rowptr, col, val, row_begin, n_rows, out, ldo);
  else
    hipLaunchKernelGGL(csr_rows_to_dense_kernel<false>, dim3(waves_grid(n_rows)), dim3(256), 0, S(stream), rowptr, col, val, row_begin, n_rows, out, ldo);
  MELD_LAUNCH_CHECK("csr_rows_to_dense_kernel");
  return MELD_OK;
}
