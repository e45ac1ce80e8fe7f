// louvain.hip -- Louvain communities of a device CSR graph: the synchronous local-move round of modularity optimisation, the sums
// over the cells grouped by label, the renumbering of labels by their smallest member, the keys of the contraction C^T A C, and the
// terms of the modularity of any labelling.
//
// Reference surface: the reference clusters cells with scanpy's louvain (comparison/comparison.py, find_n_clusters); the quality
// yardstick here is networkx.community.louvain_communities, the rule itself is restated in tests/louvain_reference.py.
//
// A is symmetric with non-negative entries, stored as CSR; an entry (i, i) is the diagonal A_ii (a contracted graph keeps the inner
// weight of a community there).  k = A 1, 2m = 1^T A 1.  With labels c (community ids are vertex numbers of the level), tot_b the sum
// of k over community b and size_b its number of vertices, one ROUND (meld_louvain_move) reads c and writes c':
//
//     w_b  = sum_{j != i, c_j = b} A_ij                       in storage order
//     g(b) = w_b 2m - (gamma k_i) (tot_b - [b = a] k_i)        every operation rounded once (the file is built with -ffp-contract=off)
//
// for a = c_i and every b in the row.  i moves to the allowed b != a with the largest g(b) (the lowest id among equals) when
// g(b) > g(a).  Allowed: a vertex alone in its community (size_a = 1) may join any community of two or more, and another single
// vertex only if b < a; a vertex of a larger community may move to b < a in even rounds and to b > a in odd ones (two neighbours
// cannot swap, a pair cannot chase each other).  own_i = w_a + A_ii, so that sum_i own_i = sum_c in_c of the labels READ.
//
// Move kernel.  louvain_move_kernel<G> is the row pass of label_rows.hpp (G = 16 or 64 lanes per row; the scheme is stated there)
// with lv_move_op: the label of an entry is c_j, -1 for the diagonal; the first chunk's trips leave w_a and A_ii; every row goes on;
// an entry is scored by g(b) under the allowed test above (size and tot of its community gathered once).  Per workgroup the rows'
// own_i and mover flags go through LDS and are added by one thread in row order; louvain_reduce_kernel adds the workgroups'
// partials: thread t takes the partials t, t + 256, ... in order, then a fixed tree.  fp64 throughout, no atomics, nothing shared
// between workgroups: every output is a function of the operands alone, the same bits every run.
//
// Totals (meld_louvain_totals).  The cells sorted by (label, cell) (meld_sort_pairs_u64_f64 on label << 32 | cell, values k): the
// wave that holds the head of a segment walks it 64 elements at a time (lane l adds the elements l, l + 64, ... of the segment in
// ascending order, then a xor butterfly); a segment of one element is stored by its own lane.  Leaves tot, size and the smallest
// member of every present label, zeros / -1 for the others.
// As compiled (-Rpass-analysis=kernel-resource-usage): no kernel of this file touches private memory (tests/test_louvain_host.py).
#include "label_rows.hpp"

namespace meld {

constexpr double LV_SHORT_MEAN = 64.0;  // mean entries per row up to which LR_SHORT is chosen: what one trip of 16 lanes holds

// the label of entry i of a row of `len` entries: -1 for padding and for the diagonal entry (never a candidate), and for a label
// outside [0, n) (labels become addresses of tot and size)
__device__ __forceinline__ int lv_entry_label(const int* __restrict__ col, const int* __restrict__ label, long long rs, long long len,
                                              long long r, long long n, long long i) {
  if (i >= len) return -1;
  const int c = col[rs + i];
  if (c == r) return -1;
  const int l = label[c];
  return (unsigned long long)l < (unsigned long long)n ? l : -1;
}

// what the move rule adds to the row pass (label_rows.hpp): the row r of community a
struct lv_move_op {
  const int* __restrict__ col;
  const int* __restrict__ labels;
  const double* __restrict__ tot;
  const int* __restrict__ size;
  long long n;
  double two_m;
  int odd;
  long long r;  // the row and its community
  int a;
  long long rs = 0, len = 0;  // set for a live row
  int size_a = 0;
  double gk = 0.0;
  double wa = 0.0, self = 0.0;  // w_a and A_ii
  label_best best{-__builtin_inf(), INT_MAX};
  __device__ __forceinline__ int label(long long i) const { return lv_entry_label(col, labels, rs, len, r, n, i); }
  __device__ __forceinline__ void meet(int lj, double vj) {
    wa += (lj == a) ? vj : 0.0;
    self += (lj < 0) ? vj : 0.0;  // (padding carries 0)
  }
  __device__ __forceinline__ bool go_on() const { return true; }
  __device__ __forceinline__ void score(int b, double w) {
    if (b >= 0 && b != a) {
      const int size_b = size[b];
      const bool allowed = size_a == 1 ? (size_b > 1 || b < a) : (odd ? b > a : b < a);
      const double gb = w * two_m - gk * tot[b];  // (built with -ffp-contract=off: three roundings)
      if (allowed) best.offer(gb, b);
    }
  }
};

template <int G>
__global__ __launch_bounds__(LR_THREADS) void louvain_move_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                                  const double* __restrict__ val, long long n,
                                                                  const int* __restrict__ label, const double* __restrict__ k,
                                                                  const double* __restrict__ tot, const int* __restrict__ size,
                                                                  double two_m, double gamma, int odd, int* __restrict__ new_label,
                                                                  double* __restrict__ own, int* __restrict__ moved,
                                                                  double* __restrict__ part_sum, int* __restrict__ part_moved) {
  constexpr int ROWS = LR_THREADS / G;
  __shared__ label_tiles<G> s_tiles;
  __shared__ double s_own[ROWS];
  __shared__ int s_mov[ROWS];
  const int g = threadIdx.x / G;
  const int sub = threadIdx.x % G;
  const long long r = (long long)blockIdx.x * ROWS + g;
  const int a = r < n ? label[r] : -1;
  const bool live = (unsigned long long)a < (unsigned long long)n;  // (a label is an address of tot and size: outside [0, n) the row stays)
  lv_move_op op{col, label, tot, size, n, two_m, odd, r, a};
  if (live) {
    op.rs = rowptr[r];
    op.len = rowptr[r + 1] - op.rs;
    op.gk = gamma * k[r];
    op.size_a = size[a];
    label_row_pass<G>(s_tiles, val, op);
  }
  op.best.over_lanes<G>();
  if (sub == 0) {
    double mine = 0.0;
    int mv = 0;
    if (live) {
      const double ga = op.wa * two_m - op.gk * (tot[a] - k[r]);
      mv = (op.best.id != INT_MAX && op.best.score > ga) ? 1 : 0;
      mine = op.wa + op.self;
      new_label[r] = mv ? op.best.id : a;
      own[r] = mine;
      moved[r] = mv;
    } else if (r < n) {
      new_label[r] = a;
      own[r] = 0.0;
      moved[r] = 0;
    }
    s_own[g] = mine;
    s_mov[g] = mv;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    int m = 0;
#pragma unroll
    for (int q = 0; q < ROWS; ++q) {
      s += s_own[q];
      m += s_mov[q];
    }
    part_sum[blockIdx.x] = s;
    part_moved[blockIdx.x] = m;
  }
}

// stats[0] = the sum of part_sum, stats[1] = the sum of part_moved (as a double: exact below 2^53)
__global__ __launch_bounds__(LR_THREADS) void louvain_reduce_kernel(const double* __restrict__ part_sum,
                                                                    const int* __restrict__ part_moved, long long n_parts,
                                                                    double* __restrict__ stats) {
  __shared__ double s_sum[LR_THREADS];
  __shared__ double s_mov[LR_THREADS];
  double s = 0.0, m = 0.0;
  for (long long p = threadIdx.x; p < n_parts; p += LR_THREADS) {
    s += part_sum[p];
    m += (double)part_moved[p];
  }
  s_sum[threadIdx.x] = s;
  s_mov[threadIdx.x] = m;
  __syncthreads();
  for (int off = LR_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + off];
      s_mov[threadIdx.x] += s_mov[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    stats[0] = s_sum[0];
    stats[1] = s_mov[0];
  }
}

__device__ __forceinline__ int lv_key_label(const unsigned long long* __restrict__ keys, long long e) { return (int)(keys[e] >> 32); }

__global__ __launch_bounds__(LR_THREADS) void louvain_totals_kernel(const unsigned long long* __restrict__ keys,
                                                                    const double* __restrict__ vals, long long n, long long n_labels,
                                                                    double* __restrict__ tot, int* __restrict__ size,
                                                                    int* __restrict__ minm) {
  const long long t = (long long)blockIdx.x * LR_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool in = t < n;
  const int lab = in ? lv_key_label(keys, t) : -1;
  const bool ok = (unsigned long long)lab < (unsigned long long)n_labels;  // (a label is an address of the outputs)
  const bool head = in && ok && (t == 0 || lv_key_label(keys, t - 1) != lab);
  const bool single = head && (t + 1 == n || lv_key_label(keys, t + 1) != lab);
  if (single) {
    tot[lab] = vals[t];
    size[lab] = 1;
    minm[lab] = (int)(keys[t] & 0xffffffffull);
  }
  unsigned long long todo = __ballot(head && !single);
  while (todo) {  // (uniform over the wave)
    const int leader = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const long long p = t - lane + leader;
    const int l0 = __shfl(lab, leader, 64);
    double part = 0.0;
    int cnt = 0;
    for (long long q = p;; q += 64) {
      const long long e = q + lane;
      const bool mine = e < n && lv_key_label(keys, e) == l0;
      if (mine) {
        part += vals[e];
        ++cnt;
      }
      if (!__all(mine)) break;  // (a segment is contiguous: the first lane outside ends it)
    }
    part = wave_sum(part);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) {
      tot[l0] = part;
      size[l0] = cnt;
      minm[l0] = (int)(keys[p] & 0xffffffffull);
    }
  }
}

// flags[v] = 1 where v is the smallest member of its community
__global__ __launch_bounds__(LR_THREADS) void louvain_heads_kernel(const int* __restrict__ label, const int* __restrict__ minm,
                                                                   long long n, int* __restrict__ flags) {
  const long long v = (long long)blockIdx.x * LR_THREADS + threadIdx.x;
  if (v >= n) return;
  const int b = label[v];
  flags[v] = ((unsigned long long)b < (unsigned long long)n && minm[b] == (int)v) ? 1 : 0;
}

__global__ __launch_bounds__(LR_THREADS) void louvain_renumber_kernel(const int* __restrict__ label, const int* __restrict__ minm,
                                                                      const long long* __restrict__ rank,
                                                                      const int* __restrict__ size, long long n,
                                                                      int* __restrict__ out, long long* __restrict__ sizes) {
  const long long v = (long long)blockIdx.x * LR_THREADS + threadIdx.x;
  if (v >= n) return;
  const int b = label[v];
  if ((unsigned long long)b >= (unsigned long long)n) return;
  const int m = minm[b];
  if ((unsigned long long)m >= (unsigned long long)n) return;  // (the label has no member: minm was not made from these labels)
  const int c = (int)rank[m];
  out[v] = c;
  if (m == (int)v) sizes[c] = size[b];
}

constexpr int LV_ROW = 16;  // lanes per row of the two streaming kernels below

__global__ __launch_bounds__(LR_THREADS) void louvain_keys_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                                  long long n, const int* __restrict__ label,
                                                                  unsigned long long* __restrict__ keys) {
  const long long t = (long long)blockIdx.x * LR_THREADS + threadIdx.x;
  const long long r = t / LV_ROW;
  const int sub = (int)(t % LV_ROW);
  if (r >= n) return;
  const unsigned long long hi = (unsigned long long)(unsigned)label[r] << 32;
  const long long e1 = rowptr[r + 1];
  for (long long e = rowptr[r] + sub; e < e1; e += LV_ROW) keys[e] = hi | (unsigned)label[col[e]];
}

// own[i] = sum_{j : c_j = c_i} A_ij (the diagonal included), k[i] = sum_j A_ij: lane s of the row's 16 adds the entries s, s + 16, ...
// in order, then a xor butterfly
__global__ __launch_bounds__(LR_THREADS) void modularity_terms_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                                      const double* __restrict__ val, long long n,
                                                                      const int* __restrict__ label, double* __restrict__ own,
                                                                      double* __restrict__ k) {
  const long long t = (long long)blockIdx.x * LR_THREADS + threadIdx.x;
  const long long r = t / LV_ROW;
  const int sub = (int)(t % LV_ROW);
  double in = 0.0, all = 0.0;
  if (r < n) {
    const int a = label[r];
    const long long e1 = rowptr[r + 1];
    for (long long e = rowptr[r] + sub; e < e1; e += LV_ROW) {
      const double v = val[e];
      all += v;
      in += (label[col[e]] == a) ? v : 0.0;
    }
  }
#pragma unroll
  for (int off = LV_ROW / 2; off > 0; off >>= 1) {
    in += __shfl_xor(in, off, 64);
    all += __shfl_xor(all, off, 64);
  }
  if (r < n && sub == 0) {
    own[r] = in;
    k[r] = all;
  }
}

}  // namespace meld

using namespace meld;

static inline unsigned lv_blocks(int64_t work) { return (unsigned)ceil_div(work, LR_THREADS); }

extern "C" int meld_louvain_lanes(int64_t n, int64_t nnz) {
  return (n > 0 && (double)nnz <= LV_SHORT_MEAN * (double)n) ? LR_SHORT : LR_LONG;
}

extern "C" int64_t meld_louvain_move_blocks(int64_t n, int lanes) {
  if (n <= 0 || (lanes != LR_SHORT && lanes != LR_LONG)) return 0;
  return ceil_div(n, LR_THREADS / lanes);
}

extern "C" int meld_louvain_move(const int64_t* rowptr, const int32_t* col, const double* val, int64_t n, const int32_t* label,
                                 const double* k, const double* tot, const int32_t* size, double two_m, double gamma, int round,
                                 int lanes, int32_t* new_label, double* own, int32_t* moved, double* part_sum, int32_t* part_moved,
                                 double* stats, meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && label && k && tot && size && new_label && own && moved && part_sum && part_moved && stats,
                 "meld_louvain_move: rowptr, label, k, tot, size, new_label, own, moved, part_sum, part_moved and stats are required");
  MELD_CHECK_ARG(n >= 1 && n < (1ll << 31), "meld_louvain_move: n=%lld outside [1, 2^31)", (long long)n);
  MELD_CHECK_ARG(lanes == LR_SHORT || lanes == LR_LONG, "meld_louvain_move: lanes=%d (%d or %d per row)", lanes, LR_SHORT, LR_LONG);
  MELD_CHECK_ARG(round >= 0, "meld_louvain_move: round=%d is negative", round);
  MELD_CHECK_ARG(two_m >= 0.0 && two_m < __builtin_inf() && gamma > 0.0 && gamma < __builtin_inf(),
                 "meld_louvain_move: two_m=%g, gamma=%g (a finite two_m >= 0 and a finite gamma > 0)", two_m, gamma);
  MELD_CHECK_ARG(new_label != label, "meld_louvain_move: new_label is label (a round reads labels other rows would have written)");
  const long long* rp = reinterpret_cast<const long long*>(rowptr);
  const long long blocks = meld_louvain_move_blocks(n, lanes);
  if (lanes == LR_SHORT) {
    louvain_move_kernel<LR_SHORT><<<(unsigned)blocks, LR_THREADS, 0, S(stream)>>>(rp, col, val, n, label, k, tot, size, two_m, gamma,
                                                                                  round & 1, new_label, own, moved, part_sum, part_moved);
  } else {
    louvain_move_kernel<LR_LONG><<<(unsigned)blocks, LR_THREADS, 0, S(stream)>>>(rp, col, val, n, label, k, tot, size, two_m, gamma,
                                                                                 round & 1, new_label, own, moved, part_sum, part_moved);
  }
  MELD_LAUNCH_CHECK("louvain_move_kernel");
  louvain_reduce_kernel<<<1, LR_THREADS, 0, S(stream)>>>(part_sum, part_moved, blocks, stats);
  MELD_LAUNCH_CHECK("louvain_reduce_kernel");
  return MELD_OK;
}

extern "C" int meld_louvain_totals(const uint64_t* keys_sorted, const double* vals_sorted, int64_t n, int64_t n_labels, double* tot,
                                   int32_t* size, int32_t* minm, meld_stream_t stream) {
  MELD_CHECK_ARG(keys_sorted && vals_sorted && tot && size && minm, "meld_louvain_totals: keys_sorted, vals_sorted, tot, size and minm are required");
  MELD_CHECK_ARG(n >= 1 && n < (1ll << 31) && n_labels >= 1 && n_labels < (1ll << 31),
                 "meld_louvain_totals: n=%lld, n_labels=%lld outside [1, 2^31)", (long long)n, (long long)n_labels);
  MELD_HIP_CALL(hipMemsetAsync(tot, 0, (size_t)n_labels * sizeof(double), S(stream)));
  MELD_HIP_CALL(hipMemsetAsync(size, 0, (size_t)n_labels * 4, S(stream)));
  MELD_HIP_CALL(hipMemsetAsync(minm, 0xff, (size_t)n_labels * 4, S(stream)));
  louvain_totals_kernel<<<lv_blocks(n), LR_THREADS, 0, S(stream)>>>(reinterpret_cast<const unsigned long long*>(keys_sorted), vals_sorted, n,
                                                                    n_labels, tot, size, minm);
  MELD_LAUNCH_CHECK("louvain_totals_kernel");
  return MELD_OK;
}

extern "C" int meld_louvain_heads(const int32_t* label, const int32_t* minm, int64_t n, int32_t* flags, meld_stream_t stream) {
  MELD_CHECK_ARG(label && minm && flags, "meld_louvain_heads: label, minm and flags are required");
  MELD_CHECK_ARG(n >= 1 && n < (1ll << 31), "meld_louvain_heads: n=%lld outside [1, 2^31)", (long long)n);
  louvain_heads_kernel<<<lv_blocks(n), LR_THREADS, 0, S(stream)>>>(label, minm, n, flags);
  MELD_LAUNCH_CHECK("louvain_heads_kernel");
  return MELD_OK;
}

extern "C" int meld_louvain_renumber(const int32_t* label, const int32_t* minm, const int64_t* rank, const int32_t* size, int64_t n,
                                     int32_t* out, int64_t* sizes, meld_stream_t stream) {
  MELD_CHECK_ARG(label && minm && rank && size && out && sizes, "meld_louvain_renumber: label, minm, rank, size, out and sizes are required");
  MELD_CHECK_ARG(n >= 1 && n < (1ll << 31), "meld_louvain_renumber: n=%lld outside [1, 2^31)", (long long)n);
  louvain_renumber_kernel<<<lv_blocks(n), LR_THREADS, 0, S(stream)>>>(label, minm, reinterpret_cast<const long long*>(rank), size, n, out,
                                                                      reinterpret_cast<long long*>(sizes));
  MELD_LAUNCH_CHECK("louvain_renumber_kernel");
  return MELD_OK;
}

extern "C" int meld_louvain_contract_keys(const int64_t* rowptr, const int32_t* col, int64_t n, const int32_t* label, uint64_t* keys,
                                          meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && col && label && keys, "meld_louvain_contract_keys: rowptr, col, label and keys are required");
  MELD_CHECK_ARG(n >= 1 && n < (1ll << 31), "meld_louvain_contract_keys: n=%lld outside [1, 2^31)", (long long)n);
  louvain_keys_kernel<<<lv_blocks(n * LV_ROW), LR_THREADS, 0, S(stream)>>>(reinterpret_cast<const long long*>(rowptr), col, n, label,
                                                                           reinterpret_cast<unsigned long long*>(keys));
  MELD_LAUNCH_CHECK("louvain_keys_kernel");
  return MELD_OK;
}

extern "C" int meld_modularity_terms(const int64_t* rowptr, const int32_t* col, const double* val, int64_t n, const int32_t* label,
                                     double* own, double* k, meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && label && own && k, "meld_modularity_terms: rowptr, label, own and k are required");
  MELD_CHECK_ARG(n >= 1 && n < (1ll << 31), "meld_modularity_terms: n=%lld outside [1, 2^31)", (long long)n);
  modularity_terms_kernel<<<lv_blocks(n * LV_ROW), LR_THREADS, 0, S(stream)>>>(reinterpret_cast<const long long*>(rowptr), col, val, n,
                                                                               label, own, k);
  MELD_LAUNCH_CHECK("modularity_terms_kernel");
  return MELD_OK;
}
