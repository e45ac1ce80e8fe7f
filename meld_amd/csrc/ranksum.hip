// ranksum.hip -- Wilcoxon rank-sum (Mann-Whitney U) statistics of every gene of a device CSC matrix (the CSR of X^T: one row per
// gene, cells ascending), for k classes of cells at once.  The run is meld_amd/diffexp.py; the scheme is restated with Python
// integers in tests/ranksum_reference.py.
//
// Reference surface: notebooks/MELD_thresholding.Tcell.ipynb, de.test.two_sample(..., test='rank'), one test per gene.
//
// code[c] in {-1, 0 .. k-1} is the class of cell c (-1: the cell takes no part), n_c the class sizes, m their sum.  Of a gene only
// the SELECTED NON-ZERO entries are touched (code >= 0, value != 0; a stored +0.0 / -0.0 is a zero): `cnt` of them, sorted by an
// order-preserving 64-bit image of the value (fp32 values are widened first, which keeps order and ties).  The z = m - cnt zeros are
// one tie group whose ranks follow from the n_neg negatives in front of it.  With lb / ub the first index of an entry's tie run and
// the index behind it (0-based among the sorted non-zeros), twice the mid-rank of the entry is lb + ub + 1, plus 2 z for a positive
// value; twice the mid-rank of a zero is 2 n_neg + z + 1.  Per gene:
//
//   rank2[c] = sum over the entries of class c of twice the mid-rank  +  (n_c - nnz[c]) (2 n_neg + z + 1)
//   tie      = sum over the tie runs of t^3 - t (t = ub - lb)  +  z^3 - z
//   nnz[c]   = the selected non-zero entries of class c
//
// All of it is integer arithmetic: LDS integer atomics into k slots, any order gives the same bits.  t^3 fits int64 up to
// MELD_RANKSUM_MAX_SELECTED selected cells; the entries refuse more.
//
// rs_rank_segment is the one scan, shared by both routes.  An entry finds lb and ub by looking at its neighbours and, inside a
// run, by binary search; the lanes of a wave that sit in one run search the same addresses (one broadcast load per probe).
//
//   short route (stored length <= RS_CAP): one workgroup of 256 per gene gathers the selected non-zero entries into LDS (image
//     8 bytes + class 1 byte per entry), sorts them there with a bitonic network over the next power of two and scans them.
//     RS_CAP = 4096: 36 KiB + the accumulators, four workgroups = 16 waves on a CU's 160 KiB.
//   long route: ranksum_gather_kernel writes (image, slot << 32 | class) for every stored entry of the listed genes (an entry that
//     is not selected gets the image ~0 and sorts behind the gene's live entries), the radix sort orders them by image and then,
//     stably, by slot (meld_sort_pairs_u64_u64), and ranksum_scan_kernel runs rs_rank_segment on each gene's segment in global
//     memory, one workgroup of 1024 per gene.
//
// sum[c] (the class's values, fp64) is one kernel for every gene whatever its route: thread t of 128 adds the entries t, t + 128, ...
// of the gene in storage order into its own LDS slot of the class, then a fixed tree over the 128 slots.  No floating-point atomics.
// As compiled (-Rpass-analysis=kernel-resource-usage): no kernel of this file touches private memory (tests/test_ranksum_reference.py).
#include "common.hpp"

#include <rocprim/rocprim.hpp>

namespace meld {

constexpr int RS_CAP = MELD_RANKSUM_LDS_MAX;
constexpr int RS_MAXK = MELD_RANKSUM_MAX_CLASSES;
constexpr int RS_SHORT_THREADS = 256;
constexpr int RS_LONG_THREADS = 1024;
constexpr int RS_SUM_THREADS = 128;
constexpr int RS_GATHER_THREADS = 256;
constexpr unsigned long long RS_DEAD = ~0ull;        // image of an entry that takes no part (no finite value has it)
constexpr unsigned long long RS_ZERO = 1ull << 63;   // image of +0.0: negatives lie below, positives above

// order-preserving image of a finite fp64 value (unsigned comparison of images == comparison of values; -0.0 and +0.0 differ,
// both are filtered out before)
__device__ __forceinline__ unsigned long long rs_image(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | RS_ZERO);
}

template <bool F32>
__device__ __forceinline__ double rs_value(const void* __restrict__ val, long long i) {
  if (F32) return (double)static_cast<const float*>(val)[i];
  return static_cast<const double*>(val)[i];
}

// the class of the cell in column c: -1 for a column outside [0, n_cells) and for a code outside [0, k) (codes become LDS addresses)
__device__ __forceinline__ int rs_class(const int* __restrict__ code, long long n_cells, int k, int c) {
  if ((unsigned long long)(long long)c >= (unsigned long long)n_cells) return -1;
  const int cd = code[c];
  return (unsigned)cd < (unsigned)k ? cd : -1;
}

// a sorted segment in LDS (short route) and in global memory (long route)
struct RsLds {
  const unsigned long long* key;
  const unsigned char* cls;
  __device__ __forceinline__ unsigned long long k(long long i) const { return key[i]; }
  __device__ __forceinline__ int c(long long i) const { return cls[i]; }
};
struct RsGlobal {
  const unsigned long long* key;
  const unsigned long long* pay;  // slot << 32 | class
  __device__ __forceinline__ unsigned long long k(long long i) const { return key[i]; }
  __device__ __forceinline__ int c(long long i) const { return (int)(unsigned)(pay[i] & 0xFFFFFFFFull); }
};

// first index in [lo, hi) whose image is >= key (hi if none)
template <class A>
__device__ __forceinline__ long long rs_lower(const A& a, long long lo, long long hi, unsigned long long key) {
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (a.k(mid) < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// first index in [lo, hi) whose image is > key (hi if none)
template <class A>
__device__ __forceinline__ long long rs_upper(const A& a, long long lo, long long hi, unsigned long long key) {
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (a.k(mid) <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The scan of one gene: `a` holds its cnt selected non-zero entries ascending by image.  Called by every thread of the workgroup;
// s_r2[RS_MAXK], s_nz[RS_MAXK], s_tie[1] are LDS.  Writes rank2[k], tie[1], nnz[k] of the gene.
template <class A>
__device__ __forceinline__ void rs_rank_segment(const A& a, long long cnt, long long m, int k, const long long* __restrict__ ncls,
                                                unsigned long long* s_r2, int* s_nz, unsigned long long* s_tie,
                                                long long* __restrict__ rank2, long long* __restrict__ tie, int* __restrict__ nnz) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int c = tid; c < k; c += nt) {
    s_r2[c] = 0;
    s_nz[c] = 0;
  }
  if (tid == 0) s_tie[0] = 0;
  __syncthreads();
  const long long z = m - cnt;
  const long long n_neg = rs_lower(a, 0, cnt, RS_ZERO);  // (the same probes in every lane: broadcast loads)
  for (long long i = tid; i < cnt; i += nt) {
    const unsigned long long key = a.k(i);
    const bool head = i == 0 || a.k(i - 1) != key;
    const bool tail = i + 1 == cnt || a.k(i + 1) != key;
    const long long lb = head ? i : rs_lower(a, 0, i, key);
    const long long ub = tail ? i + 1 : rs_upper(a, i + 1, cnt, key);
    const unsigned long long w = (unsigned long long)(lb + ub + 1 + (key > RS_ZERO ? 2 * z : 0));
    const int c = a.c(i);
    if ((unsigned)c < (unsigned)k) {
      atomicAdd(&s_r2[c], w);
      atomicAdd(&s_nz[c], 1);
    }
    if (head) {
      const unsigned long long t = (unsigned long long)(ub - lb);
      if (t > 1) atomicAdd(s_tie, t * t * t - t);
    }
  }
  __syncthreads();
  for (int c = tid; c < k; c += nt) {
    const long long zc = ncls[c] - s_nz[c];
    rank2[c] = (long long)s_r2[c] + zc * (2 * n_neg + z + 1);
    nnz[c] = s_nz[c];
  }
  if (tid == 0) tie[0] = (long long)s_tie[0] + (z * z * z - z);
}

// ---- short route ----------------------------------------------------------------------------------------------------------------
template <bool F32>
__global__ __launch_bounds__(RS_SHORT_THREADS) void ranksum_short_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                                         const void* __restrict__ val, const int* __restrict__ genes,
                                                                         long long n_genes, const int* __restrict__ code, long long n_cells,
                                                                         int k, const long long* __restrict__ ncls, long long m,
                                                                         long long* __restrict__ rank2, long long* __restrict__ tie,
                                                                         int* __restrict__ nnz) {
  __shared__ unsigned long long s_key[RS_CAP];
  __shared__ unsigned char s_cls[RS_CAP];
  __shared__ unsigned long long s_r2[RS_MAXK];
  __shared__ int s_nz[RS_MAXK];
  __shared__ unsigned long long s_tie[1];
  __shared__ int s_cnt;
  const int tid = threadIdx.x;
  const long long g = genes[blockIdx.x];
  if ((unsigned long long)g >= (unsigned long long)n_genes) return;
  const long long rs = rowptr[g];
  const long long len = rowptr[g + 1] - rs;
  if (len < 0 || len > RS_CAP) {  // not a gene of this route: marked, nothing is gathered
    for (int c = tid; c < k; c += RS_SHORT_THREADS) {
      rank2[g * k + c] = -1;
      nnz[g * k + c] = -1;
    }
    if (tid == 0) tie[g] = -1;
    return;
  }
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  // the selected non-zero entries, in any order (the slot is taken with an LDS counter: the sort that follows makes the order moot)
  for (int i = tid; i < (int)len; i += RS_SHORT_THREADS) {
    const int cd = rs_class(code, n_cells, k, col[rs + i]);
    const double v = rs_value<F32>(val, rs + i);
    if (cd >= 0 && v != 0.0) {
      const int p = atomicAdd(&s_cnt, 1);
      s_key[p] = rs_image(v);
      s_cls[p] = (unsigned char)cd;
    }
  }
  __syncthreads();
  const int cnt = s_cnt;
  int P = 2;
  while (P < cnt) P <<= 1;  // (cnt <= len <= RS_CAP, a power of two)
  for (int i = cnt + tid; i < P; i += RS_SHORT_THREADS) {
    s_key[i] = RS_DEAD;
    s_cls[i] = 0xFF;
  }
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (P >> 1); t += RS_SHORT_THREADS) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const unsigned long long ka = s_key[lo], kb = s_key[hi];
        if ((ka > kb) == up && ka != kb) {
          s_key[lo] = kb;
          s_key[hi] = ka;
          const unsigned char ca = s_cls[lo];
          s_cls[lo] = s_cls[hi];
          s_cls[hi] = ca;
        }
      }
      __syncthreads();
    }
  }
  rs_rank_segment(RsLds{s_key, s_cls}, (long long)cnt, m, k, ncls, s_r2, s_nz, s_tie, rank2 + g * k, tie + g, nnz + g * k);
}

// ---- long route -----------------------------------------------------------------------------------------------------------------
// entry e of the gathered arrays belongs to the slot s with off[s] <= e < off[s + 1] (off: the exclusive scan of the listed genes'
// stored lengths); an entry that takes no part, or whose addresses do not fit the matrix, is written dead
template <bool F32>
__global__ __launch_bounds__(RS_GATHER_THREADS) void ranksum_gather_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                                           const void* __restrict__ val, const int* __restrict__ genes,
                                                                           const long long* __restrict__ off, long long n_list,
                                                                           long long total, long long n_genes, const int* __restrict__ code,
                                                                           long long n_cells, int k, unsigned long long* __restrict__ keys,
                                                                           unsigned long long* __restrict__ pay) {
  const long long e = (long long)blockIdx.x * RS_GATHER_THREADS + threadIdx.x;
  if (e >= total) return;
  long long lo = 0, hi = n_list;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (off[mid + 1] <= e) lo = mid + 1; else hi = mid;
  }
  const long long s = lo < n_list ? lo : n_list - 1;
  unsigned long long key = RS_DEAD;
  unsigned cls = 0xFFFFFFFFu;
  const long long g = genes[s];
  if ((unsigned long long)g < (unsigned long long)n_genes) {
    const long long src = rowptr[g] + (e - off[s]);
    if (e >= off[s] && src < rowptr[g + 1]) {
      const int cd = rs_class(code, n_cells, k, col[src]);
      const double v = rs_value<F32>(val, src);
      if (cd >= 0 && v != 0.0) {
        key = rs_image(v);
        cls = (unsigned)cd;
      }
    }
  }
  keys[e] = key;
  pay[e] = ((unsigned long long)s << 32) | cls;
}

__global__ __launch_bounds__(RS_LONG_THREADS) void ranksum_scan_kernel(const unsigned long long* __restrict__ keys,
                                                                       const unsigned long long* __restrict__ pay,
                                                                       const int* __restrict__ genes, const long long* __restrict__ off,
                                                                       long long n_genes, int k, const long long* __restrict__ ncls,
                                                                       long long m, long long* __restrict__ rank2,
                                                                       long long* __restrict__ tie, int* __restrict__ nnz) {
  __shared__ unsigned long long s_r2[RS_MAXK];
  __shared__ int s_nz[RS_MAXK];
  __shared__ unsigned long long s_tie[1];
  const long long s = blockIdx.x;
  const long long g = genes[s];
  if ((unsigned long long)g >= (unsigned long long)n_genes) return;
  const long long b = off[s];
  const long long len = off[s + 1] - b;
  const RsGlobal a{keys + b, pay + b};
  const long long cnt = len > 0 ? rs_lower(a, 0, len, RS_DEAD) : 0;  // the dead entries sort behind the live ones
  rs_rank_segment(a, cnt, m, k, ncls, s_r2, s_nz, s_tie, rank2 + g * k, tie + g, nnz + g * k);
}

// ---- the classes' sums ----------------------------------------------------------------------------------------------------------
template <bool F32>
__global__ __launch_bounds__(RS_SUM_THREADS) void ranksum_sums_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                                      const void* __restrict__ val, const int* __restrict__ code,
                                                                      long long n_cells, int k, double* __restrict__ sum) {
  extern __shared__ double s_acc[];  // [k][RS_SUM_THREADS]
  const int tid = threadIdx.x;
  const long long g = blockIdx.x;
  for (int c = 0; c < k; ++c) s_acc[c * RS_SUM_THREADS + tid] = 0.0;
  const long long rs = rowptr[g];
  const long long len = rowptr[g + 1] - rs;
  for (long long i = tid; i < len; i += RS_SUM_THREADS) {  // (a thread's own slots: its entries in storage order)
    const int cd = rs_class(code, n_cells, k, col[rs + i]);
    const double v = rs_value<F32>(val, rs + i);
    if (cd >= 0) s_acc[cd * RS_SUM_THREADS + tid] += v;
  }
  __syncthreads();
  for (int half = RS_SUM_THREADS / 2; half > 0; half >>= 1) {
    for (int j = tid; j < k * half; j += RS_SUM_THREADS) {
      const int c = j / half, t = j % half;
      s_acc[c * RS_SUM_THREADS + t] += s_acc[c * RS_SUM_THREADS + t + half];
    }
    __syncthreads();
  }
  if (tid < k) sum[g * k + tid] = s_acc[tid * RS_SUM_THREADS];
}

}  // namespace meld

using namespace meld;

extern "C" int meld_ranksum_lds_max(void) { return RS_CAP; }
extern "C" int meld_ranksum_max_classes(void) { return RS_MAXK; }
extern "C" int64_t meld_ranksum_max_selected(void) { return MELD_RANKSUM_MAX_SELECTED; }

// the arguments every entry shares: the matrix, the codes, k
static int rs_check_common(const char* entry, const void* rowptr, const void* col, const void* val, int val_f32, int64_t n_genes,
                           const void* code, int64_t n_cells, int k) {
  MELD_CHECK_ARG(rowptr && col && val && code, "%s: rowptr, col, val and code are required", entry);
  MELD_CHECK_ARG(val_f32 == 0 || val_f32 == 1, "%s: val_f32=%d (0: fp64 values, 1: fp32)", entry, val_f32);
  MELD_CHECK_ARG(n_genes >= 1 && n_genes < (1ll << 31), "%s: n_genes=%lld outside [1, 2^31)", entry, (long long)n_genes);
  MELD_CHECK_ARG(n_cells >= 1 && n_cells < (1ll << 31), "%s: n_cells=%lld outside [1, 2^31)", entry, (long long)n_cells);
  MELD_CHECK_ARG(k >= 1 && k <= RS_MAXK, "%s: k=%d classes (1 <= k <= %d)", entry, k, RS_MAXK);
  return MELD_OK;
}

static int rs_check_selected(const char* entry, int64_t m) {
  MELD_CHECK_ARG(m >= 0 && m <= MELD_RANKSUM_MAX_SELECTED, "%s: m=%lld selected cells (0 <= m <= %lld: t^3 of a tie group in int64)", entry,
                 (long long)m, (long long)MELD_RANKSUM_MAX_SELECTED);
  return MELD_OK;
}

extern "C" int meld_ranksum_sums(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_genes,
                                 const int32_t* code, int64_t n_cells, int k, double* sum, meld_stream_t stream) {
  if (int rc = rs_check_common("meld_ranksum_sums", rowptr, col, val, val_f32, n_genes, code, n_cells, k)) return rc;
  MELD_CHECK_ARG(sum, "meld_ranksum_sums: sum is required");
  const long long* rp = reinterpret_cast<const long long*>(rowptr);
  const size_t lds = sizeof(double) * (size_t)k * RS_SUM_THREADS;
  if (val_f32) {
    ranksum_sums_kernel<true><<<(unsigned)n_genes, RS_SUM_THREADS, lds, S(stream)>>>(rp, col, val, code, n_cells, k, sum);
  } else {
    ranksum_sums_kernel<false><<<(unsigned)n_genes, RS_SUM_THREADS, lds, S(stream)>>>(rp, col, val, code, n_cells, k, sum);
  }
  MELD_LAUNCH_CHECK("ranksum_sums_kernel");
  return MELD_OK;
}

extern "C" int meld_ranksum_short(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_genes,
                                  const int32_t* genes, int64_t n_list, const int32_t* code, int64_t n_cells, int k,
                                  const int64_t* ncls, int64_t m, int64_t* rank2, int64_t* tie, int32_t* nnz, meld_stream_t stream) {
  if (int rc = rs_check_common("meld_ranksum_short", rowptr, col, val, val_f32, n_genes, code, n_cells, k)) return rc;
  if (int rc = rs_check_selected("meld_ranksum_short", m)) return rc;
  MELD_CHECK_ARG(genes && ncls && rank2 && tie && nnz, "meld_ranksum_short: genes, ncls, rank2, tie and nnz are required");
  MELD_CHECK_ARG(n_list >= 0 && n_list <= n_genes, "meld_ranksum_short: n_list=%lld outside [0, n_genes=%lld]", (long long)n_list,
                 (long long)n_genes);
  if (n_list == 0) return MELD_OK;
  const long long* rp = reinterpret_cast<const long long*>(rowptr);
  const long long* nc = reinterpret_cast<const long long*>(ncls);
  long long* r2 = reinterpret_cast<long long*>(rank2);
  long long* ti = reinterpret_cast<long long*>(tie);
  if (val_f32) {
    ranksum_short_kernel<true><<<(unsigned)n_list, RS_SHORT_THREADS, 0, S(stream)>>>(rp, col, val, genes, n_genes, code, n_cells, k, nc, m,
                                                                                    r2, ti, nnz);
  } else {
    ranksum_short_kernel<false><<<(unsigned)n_list, RS_SHORT_THREADS, 0, S(stream)>>>(rp, col, val, genes, n_genes, code, n_cells, k, nc,
                                                                                     m, r2, ti, nnz);
  }
  MELD_LAUNCH_CHECK("ranksum_short_kernel");
  return MELD_OK;
}

extern "C" int meld_ranksum_gather(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_genes,
                                   const int32_t* genes, const int64_t* off, int64_t n_list, int64_t total, const int32_t* code,
                                   int64_t n_cells, int k, uint64_t* keys, uint64_t* payload, meld_stream_t stream) {
  if (int rc = rs_check_common("meld_ranksum_gather", rowptr, col, val, val_f32, n_genes, code, n_cells, k)) return rc;
  MELD_CHECK_ARG(genes && off, "meld_ranksum_gather: genes and off are required");
  MELD_CHECK_ARG(n_list >= 1 && n_list <= n_genes, "meld_ranksum_gather: n_list=%lld outside [1, n_genes=%lld]", (long long)n_list,
                 (long long)n_genes);
  MELD_CHECK_ARG(total >= 0 && total < (1ll << 38), "meld_ranksum_gather: total=%lld entries outside [0, 2^38)", (long long)total);
  if (total == 0) return MELD_OK;
  MELD_CHECK_ARG(keys && payload, "meld_ranksum_gather: keys and payload are required");
  const long long* rp = reinterpret_cast<const long long*>(rowptr);
  const long long* of = reinterpret_cast<const long long*>(off);
  unsigned long long* ky = reinterpret_cast<unsigned long long*>(keys);
  unsigned long long* py = reinterpret_cast<unsigned long long*>(payload);
  const unsigned blocks = (unsigned)ceil_div(total, RS_GATHER_THREADS);
  if (val_f32) {
    ranksum_gather_kernel<true><<<blocks, RS_GATHER_THREADS, 0, S(stream)>>>(rp, col, val, genes, of, n_list, total, n_genes, code, n_cells,
                                                                            k, ky, py);
  } else {
    ranksum_gather_kernel<false><<<blocks, RS_GATHER_THREADS, 0, S(stream)>>>(rp, col, val, genes, of, n_list, total, n_genes, code, n_cells,
                                                                             k, ky, py);
  }
  MELD_LAUNCH_CHECK("ranksum_gather_kernel");
  return MELD_OK;
}

extern "C" int meld_ranksum_scan(const uint64_t* keys_sorted, const uint64_t* payload_sorted, const int32_t* genes, const int64_t* off,
                                 int64_t n_list, int64_t n_genes, int k, const int64_t* ncls, int64_t m, int64_t* rank2, int64_t* tie,
                                 int32_t* nnz, meld_stream_t stream) {
  MELD_CHECK_ARG(genes && off && ncls && rank2 && tie && nnz, "meld_ranksum_scan: genes, off, ncls, rank2, tie and nnz are required");
  MELD_CHECK_ARG(n_genes >= 1 && n_genes < (1ll << 31), "meld_ranksum_scan: n_genes=%lld outside [1, 2^31)", (long long)n_genes);
  MELD_CHECK_ARG(n_list >= 1 && n_list <= n_genes, "meld_ranksum_scan: n_list=%lld outside [1, n_genes=%lld]", (long long)n_list,
                 (long long)n_genes);
  MELD_CHECK_ARG(k >= 1 && k <= RS_MAXK, "meld_ranksum_scan: k=%d classes (1 <= k <= %d)", k, RS_MAXK);
  if (int rc = rs_check_selected("meld_ranksum_scan", m)) return rc;
  // (genes whose segments are all empty pass any address for the sorted arrays; a segment with entries reads them)
  MELD_CHECK_ARG(keys_sorted && payload_sorted, "meld_ranksum_scan: keys_sorted and payload_sorted are required");
  ranksum_scan_kernel<<<(unsigned)n_list, RS_LONG_THREADS, 0, S(stream)>>>(
      reinterpret_cast<const unsigned long long*>(keys_sorted), reinterpret_cast<const unsigned long long*>(payload_sorted), genes,
      reinterpret_cast<const long long*>(off), n_genes, k, reinterpret_cast<const long long*>(ncls), m, reinterpret_cast<long long*>(rank2),
      reinterpret_cast<long long*>(tie), nnz);
  MELD_LAUNCH_CHECK("ranksum_scan_kernel");
  return MELD_OK;
}

extern "C" int meld_sort_pairs_u64_u64(const uint64_t* keys_in, uint64_t* keys_out, const uint64_t* vals_in, uint64_t* vals_out,
                                       int64_t n, int begin_bit, int end_bit, void* temp, size_t temp_bytes, meld_stream_t stream) {
  MELD_CHECK_ARG(keys_in && keys_out && vals_in && vals_out && temp, "meld_sort_pairs_u64_u64: keys, values and temp are required");
  MELD_CHECK_ARG(n >= 0 && begin_bit >= 0 && begin_bit < end_bit && end_bit <= 64,
                 "meld_sort_pairs_u64_u64: n=%lld, bits [%d, %d) (n >= 0, 0 <= begin_bit < end_bit <= 64)", (long long)n, begin_bit, end_bit);
  if (n == 0) return MELD_OK;
  size_t need = 0;
  (void)rocprim::radix_sort_pairs(nullptr, need, keys_in, keys_out, vals_in, vals_out, (size_t)n, (unsigned)begin_bit, (unsigned)end_bit);
  MELD_CHECK_ARG(temp_bytes >= need, "meld_sort_pairs_u64_u64: temp_bytes=%zu below the %zu the sort of %lld pairs needs", temp_bytes, need,
                 (long long)n);
  size_t bytes = temp_bytes;
  MELD_HIP_CALL(rocprim::radix_sort_pairs(temp, bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, (unsigned)begin_bit,
                                          (unsigned)end_bit, S(stream)));
  return MELD_OK;
}
