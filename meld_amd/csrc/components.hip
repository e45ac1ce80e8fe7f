// components.hip -- connected components and induced subgraphs of the device CSR (W symmetric, no diagonal, rows in device order).
//
// Reference surface: pygsp's Graph.is_connected / extract_components / subgraph; the labels are those of
// scipy.sparse.csgraph.connected_components(W, directed=False).
//
// Labelling is hook-and-compress on an int32 parent[N], started at parent[v] = v.  One round (meld_cc_round) is two launches:
//   hook      every row u takes the minimum m of parent[v] over its neighbours v (reduced over the row's lanes first: one atomic
//             per row at the most) and, where m is below the root r of u, atomicMin(&parent[r], m);
//   compress  every vertex follows its chain and stores the ancestor it reached.
// INVARIANT: parent[v] <= v at all times, and a stored value only ever decreases (atomicMin with m < r; compress stores an
// ancestor, which is <= the old parent).  A chain therefore strictly descends: it cannot cycle, and a chase ends whatever it
// reads.  A plain load may return a parent another XCD has lowered since, i.e. an OLDER ancestor of the same component: valid,
// it only costs progress.  Chases are capped at CC_HOPS loads on top of that: a chain the cap cuts short is a store, so the round
// is not the last one, and a long chain (a path numbered in order) shortens by that factor per round instead of being walked by
// one lane.  Workgroups never wait for each other: no kernel polls or spins on memory, there is no grid barrier; the end of a
// launch is the only synchronisation.  Every store and every atomic that lowers a value raises *changed; a round that leaves it
// 0 wrote nothing, so every read in it was fresh, every vertex points at a root (compress) and no edge joins two roots (hook):
// the roots are the components, each the smallest device index of its component.  Integer atomics only: the same result every run.
#include <limits.h>

#include "common.hpp"

namespace meld {

constexpr int CC_THREADS = 256;
constexpr int CC_HOPS = 64;  // loads of one chase at the most

// the ancestor of x reached after at most CC_HOPS loads (x itself where it is a root)
__device__ __forceinline__ int cc_chase(const int* parent, int x) {
  for (int h = 0; h < CC_HOPS; ++h) {
    const int p = parent[x];
    if (p == x) break;
    x = p;
  }
  return x;
}

__device__ __forceinline__ void cc_raise(bool wrote, int* changed) {
  if (__any(wrote) && lane_id() == 0) *changed = 1;  // (the same value from every wave that wrote)
}

// CC_LANES lanes per row: the row's columns are read CC_LANES at a time (a kNN row of ~40 entries in three steps), the minimum
// is folded over those lanes
constexpr int CC_LANES = 16;

__global__ __launch_bounds__(CC_THREADS) void cc_hook_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                             long long n_rows, int* parent, int* changed) {
  const long long t = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  const long long u = t / CC_LANES;
  const int sub = (int)(t % CC_LANES);
  bool wrote = false;
  int m = INT_MAX;
  if (u < n_rows) {
    const long long e1 = rowptr[u + 1];
    for (long long e = rowptr[u] + sub; e < e1; e += CC_LANES) m = min(m, parent[col[e]]);
  }
#pragma unroll
  for (int off = CC_LANES / 2; off > 0; off >>= 1) m = min(m, __shfl_xor(m, off, 64));
  if (u < n_rows && sub == 0 && m != INT_MAX) {
    const int r = cc_chase(parent, (int)u);
    if (m < r) wrote = atomicMin(&parent[r], m) > m;
  }
  cc_raise(wrote, changed);
}

__global__ __launch_bounds__(CC_THREADS) void cc_compress_kernel(long long n_rows, int* parent, int* changed) {
  const long long v = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  bool wrote = false;
  if (v < n_rows) {
    const int p = parent[v];
    const int r = cc_chase(parent, p);
    if (r != p) {  // (r < p: only this thread stores parent[v] in this launch)
      parent[v] = r;
      wrote = true;
    }
  }
  cc_raise(wrote, changed);
}

__global__ __launch_bounds__(CC_THREADS) void cc_fill_kernel(int* a, int value, long long n) {
  const long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (i < n) a[i] = value;
}

// min_orig[r] = the smallest caller-order index among the vertices of root r, count[r] = their number.  The lanes of a wave
// that share a root (all of them, mostly: the device order keeps a component's cells together) fold first: one atomicMin and
// one atomicAdd per distinct root and wave.
__global__ __launch_bounds__(CC_THREADS) void cc_minima_kernel(const int* __restrict__ parent, const long long* __restrict__ perm,
                                                               long long n_rows, int* min_orig, int* count) {
  const long long v = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  bool todo = v < n_rows;
  const int r = todo ? parent[v] : -1;
  const int o = todo ? (perm ? (int)perm[v] : (int)v) : INT_MAX;
  while (true) {
    const unsigned long long mask = __ballot(todo);
    if (!mask) break;
    const int leader = __ffsll((long long)mask) - 1;
    const int r0 = __shfl(r, leader, 64);
    const bool mine = todo && r == r0;
    int x = mine ? o : INT_MAX;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = min(x, __shfl_xor(x, off, 64));
    const int cnt = __popcll(__ballot(mine));
    if (lane_id() == leader) {
      atomicMin(&min_orig[r0], x);
      atomicAdd(&count[r0], cnt);
    }
    if (mine) todo = false;
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_flag_kernel(const int* __restrict__ parent, const int* __restrict__ min_orig,
                                                             long long n_rows, int* flags) {
  const long long v = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (v < n_rows && parent[v] == (int)v) flags[min_orig[v]] = 1;
}

__global__ __launch_bounds__(CC_THREADS) void cc_labels_kernel(const int* __restrict__ parent, const long long* __restrict__ perm,
                                                               const int* __restrict__ min_orig, const int* __restrict__ count,
                                                               const long long* __restrict__ rank, long long n_rows,
                                                               int* __restrict__ labels, long long* __restrict__ sizes) {
  const long long v = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (v >= n_rows) return;
  const int r = parent[v];
  const int mo = min_orig[r];
  if ((unsigned)mo >= (unsigned long long)n_rows) return;  // (r is no root: the parents were not brought to their fixed point)
  const int label = (int)rank[mo];
  labels[perm ? perm[v] : v] = label;
  if (r == (int)v) sizes[label] = count[v];
}

// ---- induced subgraph: rows and columns with new_index >= 0, renumbered; SG lanes per row -----------------------------------
constexpr int SG = 16;

__global__ __launch_bounds__(CC_THREADS) void sub_count_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                               const int* __restrict__ new_index, long long n_rows,
                                                               int* __restrict__ counts) {
  const long long t = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  const long long u = t / SG;
  const int sub = (int)(t % SG);
  const int nu = u < n_rows ? new_index[u] : -1;
  int c = 0;
  if (nu >= 0) {
    const long long e1 = rowptr[u + 1];
    for (long long e = rowptr[u] + sub; e < e1; e += SG) c += new_index[col[e]] >= 0;
  }
#pragma unroll
  for (int off = SG / 2; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if (nu >= 0 && sub == 0) counts[nu] = c;
}

__global__ __launch_bounds__(CC_THREADS) void sub_fill_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                              const double* __restrict__ val, const int* __restrict__ new_index,
                                                              long long n_rows, const long long* __restrict__ sub_rowptr,
                                                              int* __restrict__ sub_col, double* __restrict__ sub_val) {
  const long long t = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  const long long u = t / SG;
  const int sub = (int)(t % SG);
  const int nu = u < n_rows ? new_index[u] : -1;
  if (nu < 0) return;  // (the SG lanes of a row leave together)
  const int shift = lane_id() & ~(SG - 1);  // the row's SG bits of a wave ballot
  const long long e0 = rowptr[u], e1 = rowptr[u + 1];
  long long out = sub_rowptr[nu];
  for (long long base = e0; base < e1; base += SG) {  // (uniform over the row's lanes)
    const long long e = base + sub;
    const int nc = e < e1 ? new_index[col[e]] : -1;
    const unsigned bits = (unsigned)(__ballot(nc >= 0) >> shift) & ((1u << SG) - 1u);
    if (nc >= 0) {  // kept entries keep their order: the columns stay sorted
      const long long w = out + __popc(bits & ((1u << sub) - 1u));
      sub_col[w] = nc;
      sub_val[w] = val[e];
    }
    out += __popc(bits);
  }
}

}  // namespace meld

using namespace meld;

static inline unsigned cc_blocks(int64_t work) { return (unsigned)ceil_div(work, CC_THREADS); }

extern "C" int meld_cc_round(const int64_t* rowptr, const int32_t* col, int64_t n_rows, int32_t* parent, int32_t* changed,
                             meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && parent && changed, "meld_cc_round: null argument");
  MELD_CHECK_ARG(n_rows > 0 && n_rows < (1ll << 31), "meld_cc_round: n_rows=%lld outside [1, 2^31)", (long long)n_rows);
  MELD_HIP_CALL(hipMemsetAsync(changed, 0, 4, S(stream)));
  if (col) {  // (a graph without an edge has no column array: every vertex stays its own root)
    cc_hook_kernel<<<cc_blocks(n_rows * CC_LANES), CC_THREADS, 0, S(stream)>>>(reinterpret_cast<const long long*>(rowptr), col, n_rows,
                                                                               parent, changed);
    MELD_LAUNCH_CHECK("cc_hook_kernel");
  }
  cc_compress_kernel<<<cc_blocks(n_rows), CC_THREADS, 0, S(stream)>>>(n_rows, parent, changed);
  MELD_LAUNCH_CHECK("cc_compress_kernel");
  return MELD_OK;
}

extern "C" int meld_cc_minima(const int32_t* parent, const int64_t* perm, int64_t n_rows, int32_t* min_orig, int32_t* count,
                              int32_t* flags, meld_stream_t stream) {
  MELD_CHECK_ARG(parent && min_orig && count && flags, "meld_cc_minima: null argument");
  MELD_CHECK_ARG(n_rows > 0 && n_rows < (1ll << 31), "meld_cc_minima: n_rows=%lld outside [1, 2^31)", (long long)n_rows);
  cc_fill_kernel<<<cc_blocks(n_rows), CC_THREADS, 0, S(stream)>>>(min_orig, INT_MAX, n_rows);
  MELD_LAUNCH_CHECK("cc_fill_kernel");
  MELD_HIP_CALL(hipMemsetAsync(count, 0, (size_t)n_rows * 4, S(stream)));
  MELD_HIP_CALL(hipMemsetAsync(flags, 0, (size_t)n_rows * 4, S(stream)));
  cc_minima_kernel<<<cc_blocks(n_rows), CC_THREADS, 0, S(stream)>>>(parent, reinterpret_cast<const long long*>(perm), n_rows, min_orig, count);
  MELD_LAUNCH_CHECK("cc_minima_kernel");
  cc_flag_kernel<<<cc_blocks(n_rows), CC_THREADS, 0, S(stream)>>>(parent, min_orig, n_rows, flags);
  MELD_LAUNCH_CHECK("cc_flag_kernel");
  return MELD_OK;
}

extern "C" int meld_cc_labels(const int32_t* parent, const int64_t* perm, const int32_t* min_orig, const int32_t* count,
                              const int64_t* rank, int64_t n_rows, int32_t* labels, int64_t* sizes, meld_stream_t stream) {
  MELD_CHECK_ARG(parent && min_orig && count && rank && labels && sizes, "meld_cc_labels: null argument");
  MELD_CHECK_ARG(n_rows > 0 && n_rows < (1ll << 31), "meld_cc_labels: n_rows=%lld outside [1, 2^31)", (long long)n_rows);
  cc_labels_kernel<<<cc_blocks(n_rows), CC_THREADS, 0, S(stream)>>>(parent, reinterpret_cast<const long long*>(perm), min_orig, count,
                                                                   reinterpret_cast<const long long*>(rank), n_rows, labels,
                                                                   reinterpret_cast<long long*>(sizes));
  MELD_LAUNCH_CHECK("cc_labels_kernel");
  return MELD_OK;
}

extern "C" int meld_subgraph_count(const int64_t* rowptr, const int32_t* col, const int32_t* new_index, int64_t n_rows,
                                   int32_t* counts, meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && new_index && counts, "meld_subgraph_count: null argument");
  MELD_CHECK_ARG(n_rows > 0 && n_rows < (1ll << 31), "meld_subgraph_count: n_rows=%lld outside [1, 2^31)", (long long)n_rows);
  sub_count_kernel<<<cc_blocks(n_rows * SG), CC_THREADS, 0, S(stream)>>>(reinterpret_cast<const long long*>(rowptr), col, new_index, n_rows,
                                                                         counts);
  MELD_LAUNCH_CHECK("sub_count_kernel");
  return MELD_OK;
}

extern "C" int meld_subgraph_fill(const int64_t* rowptr, const int32_t* col, const double* val, const int32_t* new_index,
                                  int64_t n_rows, const int64_t* sub_rowptr, int32_t* sub_col, double* sub_val, meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && col && val && new_index && sub_rowptr && sub_col && sub_val, "meld_subgraph_fill: null argument");
  MELD_CHECK_ARG(n_rows > 0 && n_rows < (1ll << 31), "meld_subgraph_fill: n_rows=%lld outside [1, 2^31)", (long long)n_rows);
  sub_fill_kernel<<<cc_blocks(n_rows * SG), CC_THREADS, 0, S(stream)>>>(reinterpret_cast<const long long*>(rowptr), col, val, new_index,
                                                                        n_rows, reinterpret_cast<const long long*>(sub_rowptr), sub_col,
                                                                        sub_val);
  MELD_LAUNCH_CHECK("sub_fill_kernel");
  return MELD_OK;
}
