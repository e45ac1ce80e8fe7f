// extend.hip -- out-of-sample extension: the kernel rows of NEW cells against the fitted cells, and their row-normalised
// product with a signal on the fitted cells.
//
// Replaces [UPSTREAM graphtools 1.5.x kNNGraph.build_kernel_to_data(Y) -> BaseGraph.extend_to_data(Y) (sklearn
// normalize(kernel, "l1", axis=1)) -> BaseGraph.interpolate(transform, transitions)] -- reached through ``meld_op.graph`` of the
// reference, never from meld/meld.py itself.
//
// meld_extend_rows: the query-major half of the COO stream of the search between two point sets (keys (query << 32) | ref, values
// K / 2, rows in no particular order: the rows of the exact sweep come behind the others) -> the rectangular CSR [M, N] with
// sorted rows, values K, and the rows' sums.  Count, scan, scatter, then one wave per row ranks the row's columns (every column
// compared with every other out of LDS: rows hold ~knn to ~130 entries, no merge of equal columns is needed and none is done --
// which is why this is not meld_coo_scatter_rows + meld_csr_rows_sort_merge, whose buckets cost 3 KB per row and whose merge
// would have to be undone) and writes each entry to its place.  The scatter's order inside a row depends on atomics; the ranks do
// not, so the result is the same bits every run.  The sums are meld_csr_row_sums' (diag 0).
//
// meld_extend_apply: out = diag(1 / rowsum) K F for F [N, p] fp64 row-major.  One wave per query row; the 64 lanes are CG lanes
// per entry (CG = the power of two >= p, at most 64: lanes = columns, the p contiguous doubles of a gathered row of F are one
// coalesced request) times 64 / CG entries in flight -- the split of the recurrence kernels (csrc/spmm.hip: lanes = entries for
// narrow signals, lanes = columns for wide ones).  fp64 throughout, the partial sums of the entry slots meet by xor exchanges, the
// division by the row sum is part of the same pass: the transitions are never written.  Rows are independent: no atomics, no
// state between workgroups.  Per row of L entries it moves 12 L bytes of the row, 8 p L gathered bytes of F (at least one 64-B
// sector each), 16 bytes of row pointer, 8 of the sum, and writes 8 p.
#include "common.hpp"

#include <limits.h>

namespace meld {

constexpr int EXT_TILE = 256;  // columns of a row held in LDS at a time (per wave)

static inline size_t ext_align(size_t b) { return (b + 255) & ~(size_t)255; }

__global__ __launch_bounds__(256) void extend_count_kernel(const uint64_t* __restrict__ keys, int64_t n, int64_t row_begin,
                                                           int64_t n_rows, int64_t n_cols, int* __restrict__ cnt) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const uint64_t k = keys[e];
  const int64_t r = (int64_t)(k >> 32) - row_begin;
  const int64_t c = (int64_t)(k & 0xFFFFFFFFull);
  if (r >= 0 && r < n_rows && c < n_cols) atomicAdd(&cnt[r], 1);
}

__global__ __launch_bounds__(256) void extend_scatter_kernel(const uint64_t* __restrict__ keys, const double* __restrict__ half_vals,
                                                             int64_t n, int64_t row_begin, int64_t n_rows, int64_t n_cols,
                                                             const int64_t* __restrict__ rowptr, int* __restrict__ cursor,
                                                             int* __restrict__ tcol, double* __restrict__ tval) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const uint64_t k = keys[e];
  const int64_t r = (int64_t)(k >> 32) - row_begin;
  const int64_t c = (int64_t)(k & 0xFFFFFFFFull);
  if (r >= 0 && r < n_rows && c < n_cols) {
    const int64_t pos = rowptr[r] + atomicAdd(&cursor[r], 1);  // (< rowptr[r + 1]: the count pass saw the same entries)
    tcol[pos] = (int)c;
    tval[pos] = 2.0 * half_vals[e];  // (the stream carries K / 2)
  }
}

// One wave per row: entry i goes to place rank(i) = #{j : col_j < col_i, or col_j == col_i and j < i} -- a permutation whatever
// the columns are.  Rows longer than EXT_TILE entries take several trips through LDS (rare: rows of the exact sweep).
__global__ __launch_bounds__(256) void extend_sort_rows_kernel(const int64_t* __restrict__ rowptr, int64_t n_rows,
                                                               const int* __restrict__ tcol, const double* __restrict__ tval,
                                                               int* __restrict__ col, double* __restrict__ val) {
  __shared__ int s_col[4][EXT_TILE];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + w;
  if (r >= n_rows) return;
  const int64_t rs = rowptr[r];
  const int64_t L = rowptr[r + 1] - rs;
  constexpr int U = EXT_TILE / 64;
  for (int64_t i0 = 0; i0 < L; i0 += EXT_TILE) {
    int myc[U], rank[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + lane + 64 * u;
      myc[u] = i < L ? tcol[rs + i] : INT_MAX;
      rank[u] = 0;
    }
    for (int64_t j0 = 0; j0 < L; j0 += EXT_TILE) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // (one wave: the loads of the last trip precede these stores)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t j = j0 + lane + 64 * u;
        s_col[w][lane + 64 * u] = j < L ? tcol[rs + j] : INT_MAX;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // (one wave: its LDS stores precede its loads)
      const int jn = (int)min((int64_t)EXT_TILE, L - j0);
      for (int jj = 0; jj < jn; ++jj) {
        const int cj = s_col[w][jj];  // (one address for the wave: a broadcast)
        const int64_t gj = j0 + jj;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t i = i0 + lane + 64 * u;
          rank[u] += (cj < myc[u] || (cj == myc[u] && gj < i)) ? 1 : 0;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + lane + 64 * u;
      if (i < L) {  // (rank < L: at most L - 1 entries precede one)
        col[rs + rank[u]] = myc[u];
        val[rs + rank[u]] = tval[rs + i];
      }
    }
  }
}

// out[r, :] = (sum_e val[e] F[col[e], :]) / rowsum[r]; LOG_CG: log2 of the lanes per entry
__global__ __launch_bounds__(256) void extend_apply_kernel(const int64_t* __restrict__ rowptr, const int* __restrict__ col,
                                                           const double* __restrict__ val, const double* __restrict__ rowsum,
                                                           int64_t n_rows, const double* __restrict__ F, int64_t n_f_rows, int p,
                                                           const int64_t* __restrict__ colmap, double* __restrict__ out, int log_cg) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  const int cg = 1 << log_cg;
  const int eg = 64 >> log_cg;  // entries in flight
  const int cl = lane & (cg - 1);
  const int es = lane >> log_cg;
  const int64_t rs = rowptr[r], re = rowptr[r + 1];
  const double sum = rowsum[r];
  for (int c0 = 0; c0 < p; c0 += cg) {  // (one trip unless p > 64)
    const int c = c0 + cl;
    double acc0 = 0.0, acc1 = 0.0;  // two chains: the gathers of two entries in flight per lane
    for (int64_t e = rs + es; e < re; e += 2 * eg) {
      const int64_t e1 = e + eg;
      const bool ok1 = e1 < re;
      int64_t j0 = col[e], j1 = ok1 ? col[e1] : 0;
      const double v0 = val[e], v1 = ok1 ? val[e1] : 0.0;
      if (colmap != nullptr) {  // (F in the graph's device order: caller's index -> device index)
        j0 = (j0 >= 0 && j0 < n_f_rows) ? colmap[j0] : -1;
        j1 = (j1 >= 0 && j1 < n_f_rows) ? colmap[j1] : -1;
      }
      const bool in0 = c < p && j0 >= 0 && j0 < n_f_rows;
      const bool in1 = ok1 && c < p && j1 >= 0 && j1 < n_f_rows;
      const double f0 = in0 ? F[j0 * p + c] : 0.0;
      const double f1 = in1 ? F[j1 * p + c] : 0.0;
      acc0 += v0 * f0;
      acc1 += v1 * f1;
    }
    double acc = acc0 + acc1;
    for (int off = 32; off >= cg; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (es == 0 && c < p) out[r * p + c] = sum > 0.0 ? acc / sum : 0.0;  // (a row without entries stays zero, as sklearn's normalize leaves it)
  }
}

}  // namespace meld

using namespace meld;

extern "C" size_t meld_extend_rows_temp_bytes(int64_t n, int64_t n_rows) {
  if (n < 0 || n_rows < 0) return 0;
  return 2 * ext_align(sizeof(int32_t) * (size_t)n_rows) + ext_align(meld_scan_temp_bytes(n_rows)) + ext_align(sizeof(int32_t) * (size_t)n) +
         ext_align(sizeof(double) * (size_t)n) + 256;
}

extern "C" int meld_extend_rows(const uint64_t* keys, const double* half_vals, int64_t n, int64_t row_begin, int64_t n_rows,
                                int64_t n_cols, int64_t* rowptr, int32_t* col, double* val, double* rowsum, void* temp,
                                size_t temp_bytes, meld_stream_t stream) {
  MELD_CHECK_ARG(n >= 0 && n_rows > 0 && row_begin >= 0 && n_cols > 0 && n_cols <= INT_MAX && rowptr && rowsum && temp &&
                     (n == 0 || (keys && half_vals && col && val)),
                 "meld_extend_rows: bad arguments");
  MELD_CHECK_ARG(temp_bytes >= meld_extend_rows_temp_bytes(n, n_rows) && ((uintptr_t)temp & 7) == 0,
                 "meld_extend_rows: temp buffer too small (%zu bytes) or misaligned", temp_bytes);
  char* t = reinterpret_cast<char*>(((uintptr_t)temp + 255) & ~(uintptr_t)255);
  int* cnt = reinterpret_cast<int*>(t);
  t += ext_align(sizeof(int32_t) * (size_t)n_rows);
  int* cursor = reinterpret_cast<int*>(t);
  t += ext_align(sizeof(int32_t) * (size_t)n_rows);
  void* scan_tmp = t;
  const size_t scan_bytes = meld_scan_temp_bytes(n_rows);
  t += ext_align(scan_bytes);
  int* tcol = reinterpret_cast<int*>(t);
  t += ext_align(sizeof(int32_t) * (size_t)n);
  double* tval = reinterpret_cast<double*>(t);
  hipStream_t st = S(stream);
  MELD_HIP_CALL(hipMemsetAsync(cnt, 0, 2 * ext_align(sizeof(int32_t) * (size_t)n_rows), st));  // (cnt and cursor)
  const int nb = (int)ceil_div(n, 256);
  if (n > 0) {
    extend_count_kernel<<<nb, 256, 0, st>>>(keys, n, row_begin, n_rows, n_cols, cnt);
    MELD_LAUNCH_CHECK("meld_extend_rows(count)");
  }
  const int rc = meld_exclusive_scan_i32_i64(cnt, rowptr, n_rows, scan_tmp, scan_bytes, stream);
  if (rc != 0) return rc;
  if (n == 0) {
    MELD_HIP_CALL(hipMemsetAsync(rowsum, 0, sizeof(double) * (size_t)n_rows, st));
    return MELD_OK;
  }
  {
    extend_scatter_kernel<<<nb, 256, 0, st>>>(keys, half_vals, n, row_begin, n_rows, n_cols, rowptr, cursor, tcol, tval);
    MELD_LAUNCH_CHECK("meld_extend_rows(scatter)");
    extend_sort_rows_kernel<<<(int)ceil_div(n_rows, 4), 256, 0, st>>>(rowptr, n_rows, tcol, tval, col, val);
    MELD_LAUNCH_CHECK("meld_extend_rows(sort)");
  }
  return meld_csr_row_sums(rowptr, val, n_rows, 0.0, rowsum, stream);
}

extern "C" int meld_extend_apply(const int64_t* rowptr, const int32_t* col, const double* val, const double* rowsum, int64_t n_rows,
                                 const double* F, int64_t n_f_rows, int p, const int64_t* colmap, double* out,
                                 meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && rowsum && F && out && n_rows > 0 && n_f_rows > 0 && p >= 1, "meld_extend_apply: bad arguments");
  MELD_CHECK_ARG(col && val, "meld_extend_apply: a matrix without entries has nothing to apply (col / val NULL)");
  int log_cg = 0;
  while ((1 << log_cg) < p && log_cg < 6) ++log_cg;
  extend_apply_kernel<<<(int)ceil_div(n_rows, 4), 256, 0, S(stream)>>>(rowptr, col, val, rowsum, n_rows, F, n_f_rows, p, colmap, out, log_cg);
  MELD_LAUNCH_CHECK("meld_extend_apply");
  return MELD_OK;
}
