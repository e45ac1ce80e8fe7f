// landmark.hip -- the landmark algebra of a fitted graph: rows of a CSR matrix merged by the label of their columns, and the dense
// landmark operator built from the merged matrix and its transpose.
//
// Reference surface: [UPSTREAM graphtools 1.5.x LandmarkGraph.build_landmark_op / _landmarks_to_data / extend_to_data, unpinned: not
// importable next to this code] -- reached through ``n_landmark`` of the reference (meld/meld.py:105,118).  With K = W + diag(kd)
// the symmetric kernel, c[i] in [0, L) the landmark of cell i and C the [N, L] one-hot of c:
//
//     A = K C                                    A[j, l] = sum_{i : c[i] = l} K[j, i]           (merge: count + fill)
//     r = A 1 (the row sums of K),   s = A^T 1
//     landmark_op = diag(1 / s) A^T diag(1 / r) A                                               (meld_landmark_gram)
//
// Merge.  One wave per row, two launches (count, fill) with the output row pointers scanned in between.  Entry i of a row (storage
// order; the diagonal, where given, is the row's last entry) is a LEADER when no earlier entry of the row carries its label.  The
// count launch compares every entry with every earlier one (labels of the row pass through LDS in tiles of 256, one broadcast read
// per comparison), leaves the row's number of leaders, and stores every entry's label with the sign bit set on the non-leaders.
// The fill launch walks all entries j of the row for every entry i: place(i) = number of leaders with a smaller label,
// sum(i) = the values of the entries with i's label added in storage order; leaders store (label, sum) at their place.  So a row of
// the output holds every present label once, ascending, whatever the row's length: a row longer than a tile takes several trips
// through LDS, the work is quadratic in the row's length (typical rows hold 10 to 100 entries; a hub of 4,096 takes about a
// millisecond of one wave).  No atomics, nothing shared between waves; every output element is a function of the operands alone.
//
// Gram.  One workgroup of one wave per landmark l, a dense fp64 accumulator of L elements in LDS (dynamic, 8 L bytes).  The cells j
// of row l of A^T are taken 64 at a time (one per lane: t_j = A[j, l] / r[j], the extent of row j of A), then in groups of 8 in
// ascending order: 8 lanes per cell fetch its row of A, and the cells of the group add fma(t_j, A[j, m], acc[m]) one after the
// other -- labels are distinct inside a merged row, so the lanes of one cell never meet on an address, and cells follow each other
// in program order.  A group with a row of more than 8 entries is walked one cell at a time, 64 entries per instruction.  The row
// is divided by s[l] (lanes add their entries in order, then a xor butterfly) and stored.  No atomics, no second workgroup per row.
// As compiled (-Rpass-analysis=kernel-resource-usage): no kernel of this file touches private memory (tests/test_landmark_host.py).
#include "common.hpp"

#include <limits.h>

namespace meld {

constexpr int LM_TILE = 256;      // entries of a row held in LDS at a time (per wave)
constexpr int LM_MAX = 4096;      // landmarks: a 32 KB accumulator, five workgroups resident per CU (160 KB of LDS)
constexpr int LM_DUP = INT_MIN;   // sign bit of a marked label: not the first entry of its label in the row

// the label of entry i of a row of `len` stored entries (+ the diagonal as entry `len` where has_diag)
__device__ __forceinline__ int lm_label(const int* __restrict__ col, const int* __restrict__ label, const int64_t* __restrict__ colmap,
                                        int64_t rs, int64_t len, int64_t row, int64_t i) {
  int64_t c = i < len ? (int64_t)col[rs + i] : row;
  if (colmap != nullptr) c = colmap[c];
  return label[c];
}

__global__ __launch_bounds__(256) void landmark_count_kernel(const int64_t* __restrict__ rowptr, const int* __restrict__ col,
                                                             int64_t n_rows, const int* __restrict__ label,
                                                             const int64_t* __restrict__ colmap, int has_diag, int* __restrict__ marked,
                                                             int* __restrict__ counts) {
  __shared__ int s_lab[4][LM_TILE];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + w;
  if (r >= n_rows) return;
  const int64_t rs = rowptr[r];
  const int64_t len = rowptr[r + 1] - rs;
  const int64_t L = len + (has_diag ? 1 : 0);
  const int64_t base = rs + (has_diag ? r : 0);  // (the row's place in `marked`)
  constexpr int U = LM_TILE / 64;
  int leaders = 0;
  for (int64_t i0 = 0; i0 < L; i0 += LM_TILE) {
    int my[U];
    bool dup[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + lane + 64 * u;
      my[u] = i < L ? lm_label(col, label, colmap, rs, len, r, i) : -1;
      dup[u] = false;
    }
    for (int64_t j0 = 0; j0 <= i0; j0 += LM_TILE) {  // (only earlier entries matter)
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // (one wave: the loads of the last trip precede these stores)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t j = j0 + lane + 64 * u;
        s_lab[w][lane + 64 * u] = j < L ? lm_label(col, label, colmap, rs, len, r, j) : -2;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // (one wave: its LDS stores precede its loads)
      const int jn = (int)min((int64_t)LM_TILE, L - j0);
      for (int jj = 0; jj < jn; ++jj) {
        const int lj = s_lab[w][jj];  // (one address for the wave: a broadcast)
        const int64_t gj = j0 + jj;
#pragma unroll
        for (int u = 0; u < U; ++u) dup[u] |= (lj == my[u]) && (gj < i0 + lane + 64 * u);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + lane + 64 * u;
      const bool in = i < L;
      if (in) marked[base + i] = dup[u] ? (my[u] | LM_DUP) : my[u];
      leaders += __popcll(__ballot(in && !dup[u]));
    }
  }
  if (lane == 0) counts[r] = leaders;
}

__global__ __launch_bounds__(256) void landmark_fill_kernel(const int64_t* __restrict__ rowptr, const double* __restrict__ val,
                                                            const double* __restrict__ kd, int64_t n_rows,
                                                            const int* __restrict__ marked, const int64_t* __restrict__ out_rowptr,
                                                            int* __restrict__ out_col, double* __restrict__ out_val,
                                                            double* __restrict__ rowsum) {
  __shared__ int s_lab[4][LM_TILE];
  __shared__ double s_val[4][LM_TILE];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + w;
  if (r >= n_rows) return;
  const bool has_diag = kd != nullptr;
  const int64_t rs = rowptr[r];
  const int64_t len = rowptr[r + 1] - rs;
  const int64_t L = len + (has_diag ? 1 : 0);
  const int64_t base = rs + (has_diag ? r : 0);
  const int64_t os = out_rowptr[r];
  constexpr int U = LM_TILE / 64;
  if (L == 0 && lane == 0) rowsum[r] = 0.0;
  for (int64_t i0 = 0; i0 < L; i0 += LM_TILE) {
    int my[U], place[U];
    double sum[U];
    double total = 0.0;  // (the same in every lane: all values of the row in storage order, the diagonal last)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + lane + 64 * u;
      my[u] = i < L ? marked[base + i] : -1;  // (-1: a duplicate of no label, never stored)
      place[u] = 0;
      sum[u] = 0.0;
    }
    for (int64_t j0 = 0; j0 < L; j0 += LM_TILE) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // (one wave: the loads of the last trip precede these stores)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t j = j0 + lane + 64 * u;
        s_lab[w][lane + 64 * u] = j < L ? marked[base + j] : -1;
        s_val[w][lane + 64 * u] = j < len ? val[rs + j] : (j < L ? kd[r] : 0.0);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // (one wave: its LDS stores precede its loads)
      const int jn = (int)min((int64_t)LM_TILE, L - j0);
      for (int jj = 0; jj < jn; ++jj) {
        const int mj = s_lab[w][jj];  // (one address for the wave: a broadcast)
        const double vj = s_val[w][jj];
        const int lj = mj & INT_MAX;
        const bool first = mj >= 0;
        total += vj;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int li = my[u] & INT_MAX;
          place[u] += (first && lj < li) ? 1 : 0;
          sum[u] += (lj == li) ? vj : 0.0;  // (x + 0 == x: the entries of the label in storage order)
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (my[u] >= 0) {  // (a leader; place < the row's count: at most count - 1 leaders carry a smaller label)
        out_col[os + place[u]] = my[u];
        out_val[os + place[u]] = sum[u];
      }
    }
    if (i0 == 0 && lane == 0) rowsum[r] = total;
  }
}

// a wave's view of 64 cells of a landmark's support, one per lane
struct lm_cells {
  long long begin;  // first entry of the cell's row of A
  int n;            // its length
  double t;         // A[j, l] / r[j]
};

__global__ __launch_bounds__(64) void landmark_gram_kernel(const int64_t* __restrict__ a_rowptr, const int* __restrict__ a_col,
                                                           const double* __restrict__ a_val, int64_t n_cells,
                                                           const int64_t* __restrict__ t_rowptr, const int* __restrict__ t_col,
                                                           const double* __restrict__ t_val, int n_lm, const double* __restrict__ r,
                                                           double* __restrict__ op, double* __restrict__ s) {
  extern __shared__ double acc[];  // [n_lm]
  const int lane = threadIdx.x;
  const int l = blockIdx.x;
  for (int m = lane; m < n_lm; m += 64) acc[m] = 0.0;
  __syncthreads();
  const int64_t ts = t_rowptr[l], te = t_rowptr[l + 1];
  double part = 0.0;  // this lane's share of s[l]: entries lane, lane + 64, ... in order
  const int sub = lane >> 3, k = lane & 7;
  for (int64_t e0 = ts; e0 < te; e0 += 64) {
    lm_cells c{0, 0, 0.0};
    if (e0 + lane < te) {
      const int64_t j = t_col[e0 + lane];
      const double a = t_val[e0 + lane];
      part += a;
      if (j >= 0 && j < n_cells) {
        const double rj = r[j];
        c.begin = a_rowptr[j];
        c.n = (int)(a_rowptr[j + 1] - c.begin);
        c.t = rj > 0.0 ? a / rj : 0.0;
      }
    }
    const int cells = (int)min((int64_t)64, te - e0);
    for (int g = 0; g < cells; g += 8) {  // cells g .. g + 7 of the batch, 8 lanes each
      const long long b = __shfl(c.begin, g + sub, 64);
      const int n = __shfl(c.n, g + sub, 64);
      const double t = __shfl(c.t, g + sub, 64);
      const bool longest = __any(n > 8);
      if (!longest) {
        const bool on = k < n;
        const int m = on ? a_col[b + k] : -1;
        const double x = on ? a_val[b + k] : 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {  // (cells in ascending order: one LDS read-modify-write per cell)
          if (sub == q && m >= 0 && m < n_lm) acc[m] = fma(t, x, acc[m]);
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // (one wave: cell q's stores precede cell q + 1's loads)
        }
      } else {
        for (int q = 0; q < 8 && g + q < cells; ++q) {  // one cell at a time, the whole wave on its row
          const long long bq = __shfl(c.begin, g + q, 64);
          const int nq = __shfl(c.n, g + q, 64);
          const double tq = __shfl(c.t, g + q, 64);
          for (int kk = lane; kk < nq; kk += 64) {
            const int m = a_col[bq + kk];
            const double x = a_val[bq + kk];
            if (m >= 0 && m < n_lm) acc[m] = fma(tq, x, acc[m]);
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        }
      }
    }
  }
  __syncthreads();
  const double sl = wave_sum(part);
  if (lane == 0) s[l] = sl;
  double* row = op + (int64_t)l * n_lm;
  for (int m = lane; m < n_lm; m += 64) row[m] = sl > 0.0 ? acc[m] / sl : 0.0;
}

}  // namespace meld

using namespace meld;

extern "C" int meld_landmark_max(void) { return LM_MAX; }

extern "C" int meld_landmark_merge_count(const int64_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_cols, const int32_t* label,
                                         int n_landmark, const int64_t* colmap, int has_diag, int32_t* marked, int32_t* counts,
                                         meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && label && counts, "meld_landmark_merge_count: rowptr, label and counts are required");
  MELD_CHECK_ARG(n_rows >= 0 && n_rows < (1ll << 31) && n_cols >= 0 && n_cols < (1ll << 31),
                 "meld_landmark_merge_count: n_rows=%lld, n_cols=%lld outside [0, 2^31)", (long long)n_rows, (long long)n_cols);
  MELD_CHECK_ARG(n_landmark >= 1 && n_landmark <= LM_MAX, "meld_landmark_merge_count: n_landmark=%d (1 <= n_landmark <= %d)", n_landmark,
                 LM_MAX);
  MELD_CHECK_ARG(!has_diag || n_rows == n_cols, "meld_landmark_merge_count: a diagonal needs a square matrix, got %lld x %lld",
                 (long long)n_rows, (long long)n_cols);
  MELD_CHECK_ARG(n_rows == 0 || (col && marked), "meld_landmark_merge_count: col and marked are required for a matrix with rows");
  if (n_rows == 0) return MELD_OK;
  landmark_count_kernel<<<(unsigned)ceil_div(n_rows, 4), 256, 0, S(stream)>>>(rowptr, col, n_rows, label, colmap, has_diag ? 1 : 0, marked,
                                                                              counts);
  MELD_LAUNCH_CHECK("landmark_count_kernel");
  return MELD_OK;
}

extern "C" int meld_landmark_merge_fill(const int64_t* rowptr, const double* val, const double* kd, int64_t n_rows, const int32_t* marked,
                                        const int64_t* out_rowptr, int32_t* out_col, double* out_val, double* rowsum,
                                        meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && out_rowptr && rowsum, "meld_landmark_merge_fill: rowptr, out_rowptr and rowsum are required");
  MELD_CHECK_ARG(n_rows >= 0 && n_rows < (1ll << 31), "meld_landmark_merge_fill: n_rows=%lld outside [0, 2^31)", (long long)n_rows);
  MELD_CHECK_ARG(n_rows == 0 || (val && marked && out_col && out_val),
                 "meld_landmark_merge_fill: val, marked, out_col and out_val are required for a matrix with rows");
  if (n_rows == 0) return MELD_OK;
  landmark_fill_kernel<<<(unsigned)ceil_div(n_rows, 4), 256, 0, S(stream)>>>(rowptr, val, kd, n_rows, marked, out_rowptr, out_col, out_val,
                                                                             rowsum);
  MELD_LAUNCH_CHECK("landmark_fill_kernel");
  return MELD_OK;
}

extern "C" int meld_landmark_gram(const int64_t* a_rowptr, const int32_t* a_col, const double* a_val, int64_t n_cells,
                                  const int64_t* t_rowptr, const int32_t* t_col, const double* t_val, int n_landmark, const double* r,
                                  double* op, double* s, meld_stream_t stream) {
  MELD_CHECK_ARG(a_rowptr && t_rowptr && r && op && s, "meld_landmark_gram: a_rowptr, t_rowptr, r, op and s are required");
  MELD_CHECK_ARG(n_cells >= 0 && n_cells < (1ll << 31), "meld_landmark_gram: n_cells=%lld outside [0, 2^31)", (long long)n_cells);
  MELD_CHECK_ARG(n_landmark >= 1 && n_landmark <= LM_MAX, "meld_landmark_gram: n_landmark=%d (1 <= n_landmark <= %d)", n_landmark, LM_MAX);
  MELD_CHECK_ARG(n_cells == 0 || (a_col && a_val && t_col && t_val),
                 "meld_landmark_gram: the columns and values of A and of its transpose are required for a matrix with rows");
  landmark_gram_kernel<<<(unsigned)n_landmark, 64, sizeof(double) * (size_t)n_landmark, S(stream)>>>(
      a_rowptr, a_col, a_val, n_cells, t_rowptr, t_col, t_val, n_landmark, r, op, s);
  MELD_LAUNCH_CHECK("landmark_gram_kernel");
  return MELD_OK;
}
