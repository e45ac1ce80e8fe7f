// preprocess.hip -- the steps in front of the graph on the device CSR of the counts: per-cell statistics, per-gene capture counts and
// the one rewrite of the matrix (rows and columns selected, values normalised by library size and transformed).
//
// Reference surface: scprep.filter.filter_library_size / filter_rare_genes / filter_gene_set_expression,
// scprep.normalize.library_size_normalize (sklearn.preprocessing.normalize(X, "l1") * rescale) and scprep.transform.sqrt / log /
// arcsinh, as the reference's notebooks call them before meld.MELD().
//
// The operand is the CSR a DeviceCSR holds: rowptr int64, col int32, val fp32 (widened on load, exactly) or fp64; stored zeros
// allowed, rows of any length, nnz beyond 2^31.  All arithmetic is fp64, stated operation by operation (the file is compiled with
// -ffp-contract=off: tests/preprocess_reference.py evaluates the same operations with numpy and the tests compare bits).  There are
// no floating-point atomics; the integer atomics of the column counts give the same bits in any order.
//
// ORDER OF A ROW'S SUMS (row_stats_kernel): a wave per row.  Number the row's COUNTED entries (all of them, or those whose column
// the mask keeps) 0, 1, 2 ... in storage order; lane l adds the entries l, l + 64, l + 128 ... into one accumulator in that order,
// then a fixed butterfly over the 64 lanes.  The order is a function of the number of counted entries alone, so the masked sums of
// a row equal, bit for bit, the plain sums of the same row after the columns were dropped (select_fill_kernel keeps storage order):
// the fused route of meld_amd/preprocess.py and the step-by-step calls agree on real-valued data too, not only on counts.  The
// masked kernel gets that numbering from a ballot per 64 entries and a 128-slot ring in LDS per wave: kept values are written to
// ring[rank % 128] and, whenever 64 are pending, lane l takes ring[head + l].
#include "common.hpp"

namespace meld {

constexpr int PREP_THREADS = 256;               // 4 waves, one row each
constexpr int PREP_WAVES = PREP_THREADS / WAVE;
constexpr int PREP_CC_THREADS = 1024;           // column counts: 16 waves share one LDS panel
constexpr int PREP_CC_WAVES = PREP_CC_THREADS / WAVE;
constexpr int PREP_CC_BLOCKS = 256;             // one workgroup per CU (the panel takes 128 of its 160 KiB)

template <bool F32>
__device__ __forceinline__ double prep_load(const void* val, long long e) {
  return F32 ? (double)reinterpret_cast<const float*>(val)[e] : reinterpret_cast<const double*>(val)[e];
}

// orders the LDS accesses of the lanes of ONE wave among themselves (no workgroup barrier: the waves of a block work on different rows)
__device__ __forceinline__ void prep_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- per-row sum, sum of magnitudes and count above the cutoff ---------------------------------------------------------------------
template <bool F32, bool MASKED>
__global__ __launch_bounds__(PREP_THREADS) void row_stats_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                                 const void* __restrict__ val, long long n_rows, int n_cols,
                                                                 const unsigned char* __restrict__ col_mask, double cutoff,
                                                                 double* __restrict__ sum, double* __restrict__ abs_sum,
                                                                 int* __restrict__ count) {
  __shared__ double ring[MASKED ? PREP_WAVES * 2 * WAVE : 1];
  const int lane = lane_id();
  const int w = threadIdx.x / WAVE;
  const long long row = (long long)blockIdx.x * PREP_WAVES + w;
  if (row >= n_rows) return;  // (a whole wave: no barrier follows)
  const long long e0 = rowptr[row], e1 = rowptr[row + 1];
  double s = 0.0, a = 0.0;
  int c = 0;
  if (!MASKED) {
    long long e = e0 + lane;
    for (; e + 3 * WAVE < e1; e += 4 * WAVE) {  // four loads in flight, added in storage order
      const double v0 = prep_load<F32>(val, e), v1 = prep_load<F32>(val, e + WAVE), v2 = prep_load<F32>(val, e + 2 * WAVE),
                   v3 = prep_load<F32>(val, e + 3 * WAVE);
      s += v0; a += fabs(v0); c += v0 > cutoff;
      s += v1; a += fabs(v1); c += v1 > cutoff;
      s += v2; a += fabs(v2); c += v2 > cutoff;
      s += v3; a += fabs(v3); c += v3 > cutoff;
    }
    for (; e < e1; e += WAVE) {
      const double v = prep_load<F32>(val, e);
      s += v; a += fabs(v); c += v > cutoff;
    }
  } else {
    double* my = ring + w * 2 * WAVE;
    int head = 0, pending = 0;  // (wave-uniform) head: 0 or 64, the ring half the next 64 counted entries start in
    bool keep = false;  // of this lane's entry of the current 64; the next 64 columns and their mask bytes are fetched one step ahead
    if (e0 + lane < e1) {
      const int cc = col[e0 + lane];
      keep = (unsigned)cc < (unsigned)n_cols && col_mask[cc] != 0;
    }
    for (long long base = e0; base < e1; base += WAVE) {
      const double v = keep ? prep_load<F32>(val, base + lane) : 0.0;  // (only counted values are read)
      const long long en = base + WAVE + lane;
      bool keep_next = false;
      if (en < e1) {
        const int cc = col[en];
        keep_next = (unsigned)cc < (unsigned)n_cols && col_mask[cc] != 0;
      }
      const unsigned long long bits = __ballot(keep);
      if (keep) {
        const int r = pending + __popcll(bits & ((1ull << lane) - 1ull));  // (< 128: pending < 64 here)
        my[(head + r) & (2 * WAVE - 1)] = v;
        c += v > cutoff;
      }
      pending += __popcll(bits);
      prep_wave_sync();  // the lanes' writes before any lane's read (one wave: LDS operations complete in program order)
      if (pending >= WAVE) {  // (uniform)
        const double x = my[head + lane];
        s += x; a += fabs(x);
        head ^= WAVE;
        pending -= WAVE;
      }
      prep_wave_sync();  // ... and that read before the next 64 entries may wrap into the half it came from
      keep = keep_next;
    }
    if (lane < pending) {
      const double x = my[head + lane];
      s += x; a += fabs(x);
    }
  }
  s = wave_sum(s);
  a = wave_sum(a);
  c = wave_sum_i32(c);
  if (lane == 0) {
    sum[row] = s;
    abs_sum[row] = a;
    count[row] = c;
  }
}

// ---- per-column count of entries above the cutoff over the kept rows ---------------------------------------------------------------
// A workgroup walks rows [row0, row1), a wave per row, and counts the entries of columns [p0, p0 + panel_n) into its LDS panel.
template <bool F32>
__global__ __launch_bounds__(PREP_CC_THREADS) void col_counts_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                                     const void* __restrict__ val, long long n_rows, long long rows_per_block,
                                                                     const unsigned char* __restrict__ row_keep, double cutoff, int p0,
                                                                     int panel_n, int* __restrict__ count) {
  extern __shared__ int panel[];  // [MELD_PREP_PANEL_COLS]
  for (int i = threadIdx.x; i < panel_n; i += PREP_CC_THREADS) panel[i] = 0;
  __syncthreads();
  const int lane = lane_id();
  const int w = threadIdx.x / WAVE;
  const long long row0 = (long long)blockIdx.x * rows_per_block;
  const long long row1 = row0 + rows_per_block < n_rows ? row0 + rows_per_block : n_rows;
  for (long long row = row0 + w; row < row1; row += PREP_CC_WAVES) {
    if (row_keep && row_keep[row] == 0) continue;
    const long long e1 = rowptr[row + 1];
    long long e = rowptr[row] + lane;
    for (; e + 3 * WAVE < e1; e += 4 * WAVE) {  // (16 waves on a CU: four loads each in flight to keep the stream going)
      unsigned local[4];
      double v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        local[u] = (unsigned)(col[e + u * WAVE] - p0);
        v[u] = prep_load<F32>(val, e + u * WAVE);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (local[u] < (unsigned)panel_n && v[u] > cutoff) atomicAdd(&panel[local[u]], 1);
    }
    for (; e < e1; e += WAVE) {
      const unsigned local = (unsigned)(col[e] - p0);
      if (local < (unsigned)panel_n && prep_load<F32>(val, e) > cutoff) atomicAdd(&panel[local], 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < panel_n; i += PREP_CC_THREADS) {
    const int n = panel[i];
    if (n) atomicAdd(&count[p0 + i], n);
  }
}

// the A-B of the panel: every counted entry is one global atomic (development switch MELD_PREP_COLCOUNT_GLOBAL)
template <bool F32>
__global__ __launch_bounds__(PREP_THREADS) void col_counts_global_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                                         const void* __restrict__ val, long long n_rows, int n_cols,
                                                                         const unsigned char* __restrict__ row_keep, double cutoff,
                                                                         int* __restrict__ count) {
  const int lane = lane_id();
  const long long row = (long long)blockIdx.x * PREP_WAVES + threadIdx.x / WAVE;
  if (row >= n_rows || (row_keep && row_keep[row] == 0)) return;
  const long long e1 = rowptr[row + 1];
  for (long long e = rowptr[row] + lane; e < e1; e += WAVE) {
    const int c = col[e];
    if ((unsigned)c < (unsigned)n_cols && prep_load<F32>(val, e) > cutoff) atomicAdd(&count[c], 1);
  }
}

// ---- the rewrite: kept rows (a list), kept columns (a map), values normalised and transformed ------------------------------------------
__device__ __forceinline__ int prep_new_col(const int* __restrict__ col_map, int n_cols, int c) {
  if ((unsigned)c >= (unsigned)n_cols) return -1;
  return col_map ? col_map[c] : c;
}

__global__ __launch_bounds__(PREP_THREADS) void select_count_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                                    long long n_rows, int n_cols, const int* __restrict__ rows,
                                                                    long long n_keep, const int* __restrict__ col_map,
                                                                    int* __restrict__ counts) {
  const int lane = lane_id();
  const long long i = (long long)blockIdx.x * PREP_WAVES + threadIdx.x / WAVE;
  if (i >= n_keep) return;
  const int old = rows[i];
  int c = 0;
  if ((unsigned)old < (unsigned long long)n_rows) {
    const long long e0 = rowptr[old], e1 = rowptr[old + 1];
    if (col_map) {
      long long e = e0 + lane;
      for (; e + 3 * WAVE < e1; e += 4 * WAVE) {  // four column loads, then their four look-ups: two round trips per 256 entries
        const int c0 = col[e], c1 = col[e + WAVE], c2 = col[e + 2 * WAVE], c3 = col[e + 3 * WAVE];
        const int m0 = prep_new_col(col_map, n_cols, c0), m1 = prep_new_col(col_map, n_cols, c1),
                  m2 = prep_new_col(col_map, n_cols, c2), m3 = prep_new_col(col_map, n_cols, c3);
        c += (m0 >= 0) + (m1 >= 0) + (m2 >= 0) + (m3 >= 0);
      }
      for (; e < e1; e += WAVE) c += prep_new_col(col_map, n_cols, col[e]) >= 0;
      c = wave_sum_i32(c);
    } else {
      c = (int)(e1 - e0);  // (column indices are the caller's to have checked: DeviceCSR._validate)
    }
  }
  if (lane == 0) counts[i] = c;
}

__device__ __forceinline__ double prep_transform(double w, int code, double cofactor) {
  switch (code) {
    case MELD_PREP_SQRT: return sqrt(w);
    case MELD_PREP_LOG: return log(w + 1.0);
    case MELD_PREP_LOG2: return log2(w + 1.0);
    case MELD_PREP_LOG10: return log10(w + 1.0);
    case MELD_PREP_ARCSINH: return asinh(w / cofactor);
    default: return w;
  }
}

template <bool F32>
__global__ __launch_bounds__(PREP_THREADS) void select_fill_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                                   const void* __restrict__ val, long long n_rows, int n_cols,
                                                                   const int* __restrict__ rows, long long n_keep,
                                                                   const int* __restrict__ col_map, const double* __restrict__ scale,
                                                                   double rescale, int code, double cofactor,
                                                                   const long long* __restrict__ out_rowptr, int* __restrict__ out_col,
                                                                   double* __restrict__ out_val, double* __restrict__ out_val_norm) {
  const int lane = lane_id();
  const long long i = (long long)blockIdx.x * PREP_WAVES + threadIdx.x / WAVE;
  if (i >= n_keep) return;
  const int old = rows[i];
  if ((unsigned)old >= (unsigned long long)n_rows) return;
  const long long e0 = rowptr[old], e1 = rowptr[old + 1];
  long long out = out_rowptr[i];
  const long long out_end = out_rowptr[i + 1];  // (a row never writes past its own segment, whatever the caller scanned)
  const double s = scale ? scale[i] : 1.0;
  int cc = -1;  // this lane's entry of the current 64 (column -1: none); the next 64 are in flight while these are written
  double v = 0.0;
  if (e0 + lane < e1) {
    cc = col[e0 + lane];
    v = prep_load<F32>(val, e0 + lane);
  }
  for (long long base = e0; base < e1; base += WAVE) {  // (uniform over the wave)
    const long long en = base + WAVE + lane;
    int cn = -1;
    double vn = 0.0;
    if (en < e1) {
      cn = col[en];
      vn = prep_load<F32>(val, en);
    }
    const int nc = prep_new_col(col_map, n_cols, cc);  // (-1 for the column -1)
    const unsigned long long bits = __ballot(nc >= 0);
    if (nc >= 0) {  // kept entries keep their order: the columns stay sorted
      const long long o = out + __popcll(bits & ((1ull << lane) - 1ull));
      if (o < out_end) {
        // sklearn's normalize leaves a row of norm 0 alone (its norm is replaced by 1); rescale still multiplies
        const double wv = scale ? (s == 0.0 ? v : v / s) * rescale : v;
        out_col[o] = nc;
        out_val[o] = prep_transform(wv, code, cofactor);
        if (out_val_norm) out_val_norm[o] = wv;
      }
    }
    out += __popcll(bits);
    cc = cn;
    v = vn;
  }
}

// ---- per-gene count, mean and two-pass variance on the gene-major copy (the CSR of X^T) ---------------------------------------------
// ORDER OF A GENE'S SUMS: number the gene's STORED entries 0, 1, 2 ...; an entry that is not counted (its cell is not kept, or its
// index lies outside the matrix) stands in its place as +0.0.  Up to MELD_PREP_MOMENTS_WAVE_MAX entries one wave takes the gene:
// lane l adds the entries l, l + 64, ... in that order, then the fixed butterfly.  A longer gene takes the workgroup: thread t adds
// the entries t, t + 1024, ..., the butterfly in each wave, a fixed pairwise tree over the 16 wave sums in LDS.  mom_pass is the one
// loop of both routes and both passes (the stride is 64 or 1024); the route is a function of the stored length, so the order is.
// A workgroup owns 16 consecutive genes: each wave does its own if it is short, then all of them walk the long ones together.
constexpr int MOM_THREADS = MELD_PREP_MOMENTS_THREADS;
constexpr int MOM_WAVES = MOM_THREADS / WAVE;
constexpr int MOM_WAVE_MAX = MELD_PREP_MOMENTS_WAVE_MAX;
static_assert(MOM_WAVES == 16, "the tree of mom_tree is written for 16 wave sums");

struct MomOperand {
  const int* col;
  const void* val;
  int n_cells;
  const unsigned char* row_keep;
  const double* row_scale;
  double rescale;
  int code;
  double cofactor;
};

// every load of an entry, none of them conditional (four entries' loads go out together): a cell index outside the matrix reads
// the per-cell vectors at 0 and is not counted
template <bool F32>
__device__ __forceinline__ void mom_fetch(const MomOperand& a, long long e, double& v, double& s, bool& keep) {
  const int c = a.col[e];
  v = prep_load<F32>(a.val, e);
  const bool ok = (unsigned)c < (unsigned)a.n_cells;
  const int ci = ok ? c : 0;
  keep = ok && (!a.row_keep || a.row_keep[ci] != 0);
  s = a.row_scale ? a.row_scale[ci] : 1.0;
}

// the value of select_fill_kernel, operation by operation
__device__ __forceinline__ double mom_value(const MomOperand& a, double v, double s, bool keep) {
  if (!keep) return 0.0;
  const double wv = a.row_scale ? (s == 0.0 ? v : v / s) * a.rescale : v;
  return prep_transform(wv, a.code, a.cofactor);
}

template <bool SECOND>
__device__ __forceinline__ void mom_add(double x, bool keep, double mean, double& acc, int& cnt) {
  if (SECOND) {
    const double d = keep ? x - mean : 0.0;
    acc += d * d;
  } else {
    acc += x;
    cnt += keep;
  }
}

// first pass: acc += x, cnt += counted; second: acc += (x - mean)^2 over the counted entries.  e: this thread's first entry.
template <bool F32, bool SECOND>
__device__ __forceinline__ void mom_pass(const MomOperand& a, long long e, long long e1, int stride, double mean, double& acc, int& cnt) {
  for (; e + 3ll * stride < e1; e += 4ll * stride) {  // four entries in flight, added in storage order
    double v[4], s[4];
    bool keep[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) mom_fetch<F32>(a, e + (long long)u * stride, v[u], s[u], keep[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) mom_add<SECOND>(mom_value(a, v[u], s[u], keep[u]), keep[u], mean, acc, cnt);
  }
  for (; e < e1; e += stride) {
    double v, s;
    bool keep;
    mom_fetch<F32>(a, e, v, s, keep);
    mom_add<SECOND>(mom_value(a, v, s, keep), keep, mean, acc, cnt);
  }
}

__device__ __forceinline__ double mom_tree(const double* part) {  // ((p0 + p8) + (p4 + p12)) + ... : the same in every thread
  double p[MOM_WAVES];
#pragma unroll
  for (int i = 0; i < MOM_WAVES; ++i) p[i] = part[i];
#pragma unroll
  for (int half = MOM_WAVES / 2; half > 0; half >>= 1)
#pragma unroll
    for (int i = 0; i < half; ++i) p[i] += p[i + half];
  return p[0];
}

__device__ __forceinline__ void mom_store(long long g, int c, double m, double ss, long long n_kept, int ddof, int* __restrict__ count,
                                          double* __restrict__ mean, double* __restrict__ var) {
  count[g] = c;
  mean[g] = m;
  var[g] = (ss + (double)(n_kept - c) * (m * m)) / (double)(n_kept - ddof);
}

template <bool F32>
__global__ __launch_bounds__(MOM_THREADS) void gene_moments_kernel(const long long* __restrict__ rowptr, MomOperand a, long long n_genes,
                                                                   const unsigned char* __restrict__ gene_mask, long long n_kept, int ddof,
                                                                   int* __restrict__ count, double* __restrict__ mean,
                                                                   double* __restrict__ var) {
  __shared__ double s_part[MOM_WAVES];
  __shared__ int s_cnt[MOM_WAVES];
  const int lane = lane_id();
  const int w = threadIdx.x / WAVE;
  const long long g0 = (long long)blockIdx.x * MOM_WAVES;
  const double nk = (double)n_kept;
  {  // a wave per gene: masked genes and short ones (no wave leaves: barriers follow)
    const long long g = g0 + w;
    if (g < n_genes) {
      if (gene_mask && gene_mask[g] == 0) {
        if (lane == 0) {
          count[g] = -1;
          mean[g] = 0.0;
          var[g] = 0.0;
        }
      } else {
        const long long e0 = rowptr[g], e1 = rowptr[g + 1];
        if (e1 - e0 <= MOM_WAVE_MAX) {
          double s = 0.0, ss = 0.0;
          int c = 0, unused = 0;
          mom_pass<F32, false>(a, e0 + lane, e1, WAVE, 0.0, s, c);
          s = wave_sum(s);
          c = wave_sum_i32(c);
          const double m = s / nk;
          mom_pass<F32, true>(a, e0 + lane, e1, WAVE, m, ss, unused);
          ss = wave_sum(ss);
          if (lane == 0) mom_store(g, c, m, ss, n_kept, ddof, count, mean, var);
        }
      }
    }
  }
  for (int j = 0; j < MOM_WAVES; ++j) {  // the long genes of the 16, the whole workgroup on each (every branch here is uniform)
    const long long g = g0 + j;
    if (g >= n_genes) break;
    if (gene_mask && gene_mask[g] == 0) continue;
    const long long e0 = rowptr[g], e1 = rowptr[g + 1];
    if (e1 - e0 <= MOM_WAVE_MAX) continue;
    double s = 0.0, ss = 0.0;
    int c = 0, unused = 0;
    mom_pass<F32, false>(a, e0 + threadIdx.x, e1, MOM_THREADS, 0.0, s, c);
    s = wave_sum(s);
    c = wave_sum_i32(c);
    if (lane == 0) {
      s_part[w] = s;
      s_cnt[w] = c;
    }
    __syncthreads();
    const double m = mom_tree(s_part) / nk;
    c = 0;
#pragma unroll
    for (int i = 0; i < MOM_WAVES; ++i) c += s_cnt[i];
    __syncthreads();  // every thread has read the sums before the second pass writes its own
    mom_pass<F32, true>(a, e0 + threadIdx.x, e1, MOM_THREADS, m, ss, unused);
    ss = wave_sum(ss);
    if (lane == 0) s_part[w] = ss;
    __syncthreads();
    if (threadIdx.x == 0) mom_store(g, c, m, mom_tree(s_part), n_kept, ddof, count, mean, var);
    __syncthreads();  // ... and thread 0 before the next gene's
  }
}

}  // namespace meld

using namespace meld;

static inline unsigned prep_row_blocks(int64_t rows) { return (unsigned)ceil_div(rows, PREP_WAVES); }

#define PREP_CHECK_MATRIX(entry)                                                                                                  \
  MELD_CHECK_ARG(rowptr, entry ": rowptr is NULL");                                                                               \
  MELD_CHECK_ARG(val_f32 == 0 || val_f32 == 1, entry ": val_f32=%d outside {0, 1}", val_f32);                                     \
  MELD_CHECK_ARG(n_rows > 0 && n_rows < (1ll << 31), entry ": n_rows=%lld outside [1, 2^31)", (long long)n_rows);                 \
  MELD_CHECK_ARG(n_cols > 0 && n_cols < (1ll << 31), entry ": n_cols=%lld outside [1, 2^31)", (long long)n_cols)

extern "C" int meld_prep_panel_cols(void) { return MELD_PREP_PANEL_COLS; }

extern "C" int meld_prep_row_stats(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_rows,
                                   int64_t n_cols, const uint8_t* col_mask, double cutoff, double* sum, double* abs_sum, int32_t* count,
                                   meld_stream_t stream) {
  PREP_CHECK_MATRIX("meld_prep_row_stats");
  MELD_CHECK_ARG(col && val && sum && abs_sum && count, "meld_prep_row_stats: null argument");
  const long long* rp = reinterpret_cast<const long long*>(rowptr);
  const unsigned grid = prep_row_blocks(n_rows);
#define PREP_RS(F32, MASKED) \
  row_stats_kernel<F32, MASKED><<<grid, PREP_THREADS, 0, S(stream)>>>(rp, col, val, n_rows, (int)n_cols, col_mask, cutoff, sum, abs_sum, count)
  if (col_mask) {
    if (val_f32) PREP_RS(true, true); else PREP_RS(false, true);
  } else {
    if (val_f32) PREP_RS(true, false); else PREP_RS(false, false);
  }
#undef PREP_RS
  MELD_LAUNCH_CHECK("row_stats_kernel");
  return MELD_OK;
}

extern "C" int meld_prep_col_counts(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_rows,
                                    int64_t n_cols, const uint8_t* row_keep, double cutoff, int32_t* count, meld_stream_t stream) {
  PREP_CHECK_MATRIX("meld_prep_col_counts");
  MELD_CHECK_ARG(col && val && count, "meld_prep_col_counts: null argument");
  const long long* rp = reinterpret_cast<const long long*>(rowptr);
  const char* global = meld_dev_getenv("MELD_PREP_COLCOUNT_GLOBAL");
  if (global && global[0] == '1') {
    if (val_f32)
      col_counts_global_kernel<true><<<prep_row_blocks(n_rows), PREP_THREADS, 0, S(stream)>>>(rp, col, val, n_rows, (int)n_cols, row_keep, cutoff, count);
    else
      col_counts_global_kernel<false><<<prep_row_blocks(n_rows), PREP_THREADS, 0, S(stream)>>>(rp, col, val, n_rows, (int)n_cols, row_keep, cutoff, count);
    MELD_LAUNCH_CHECK("col_counts_global_kernel");
    return MELD_OK;
  }
  const size_t lds = (size_t)MELD_PREP_PANEL_COLS * sizeof(int);
  static bool configured[64][2] = {};  // (128 KiB of dynamic LDS is above the default limit of a launch: raised once per device)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (!configured[dev][val_f32]) {
    const void* fn = val_f32 ? reinterpret_cast<const void*>(&col_counts_kernel<true>) : reinterpret_cast<const void*>(&col_counts_kernel<false>);
    MELD_HIP_CALL(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    configured[dev][val_f32] = true;
  }
  // contiguous row ranges, at least one row per wave of a workgroup; at most one workgroup per CU
  const int64_t blocks = ceil_div(n_rows, PREP_CC_WAVES) < PREP_CC_BLOCKS ? ceil_div(n_rows, PREP_CC_WAVES) : PREP_CC_BLOCKS;
  const int64_t rows_per_block = ceil_div(n_rows, blocks);
  for (int64_t p0 = 0; p0 < n_cols; p0 += MELD_PREP_PANEL_COLS) {  // one launch per panel of columns
    const int panel_n = (int)(n_cols - p0 < MELD_PREP_PANEL_COLS ? n_cols - p0 : MELD_PREP_PANEL_COLS);
    if (val_f32)
      col_counts_kernel<true><<<(unsigned)blocks, PREP_CC_THREADS, lds, S(stream)>>>(rp, col, val, n_rows, rows_per_block, row_keep, cutoff, (int)p0, panel_n, count);
    else
      col_counts_kernel<false><<<(unsigned)blocks, PREP_CC_THREADS, lds, S(stream)>>>(rp, col, val, n_rows, rows_per_block, row_keep, cutoff, (int)p0, panel_n, count);
    MELD_LAUNCH_CHECK("col_counts_kernel");
  }
  return MELD_OK;
}

extern "C" int meld_prep_select_count(const int64_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_cols, const int32_t* rows,
                                      int64_t n_keep, const int32_t* col_map, int32_t* counts, meld_stream_t stream) {
  const int val_f32 = 0;
  PREP_CHECK_MATRIX("meld_prep_select_count");
  MELD_CHECK_ARG(col && rows && counts, "meld_prep_select_count: null argument");
  MELD_CHECK_ARG(n_keep > 0 && n_keep < (1ll << 31), "meld_prep_select_count: n_keep=%lld outside [1, 2^31)", (long long)n_keep);
  select_count_kernel<<<prep_row_blocks(n_keep), PREP_THREADS, 0, S(stream)>>>(reinterpret_cast<const long long*>(rowptr), col, n_rows,
                                                                              (int)n_cols, rows, n_keep, col_map, counts);
  MELD_LAUNCH_CHECK("select_count_kernel");
  return MELD_OK;
}

extern "C" int meld_prep_select_fill(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_rows,
                                     int64_t n_cols, const int32_t* rows, int64_t n_keep, const int32_t* col_map, const double* scale,
                                     double rescale, int transform, double cofactor, const int64_t* out_rowptr, int32_t* out_col,
                                     double* out_val, double* out_val_norm, meld_stream_t stream) {
  PREP_CHECK_MATRIX("meld_prep_select_fill");
  MELD_CHECK_ARG(col && val && rows && out_rowptr && out_col && out_val, "meld_prep_select_fill: null argument");
  MELD_CHECK_ARG(n_keep > 0 && n_keep < (1ll << 31), "meld_prep_select_fill: n_keep=%lld outside [1, 2^31)", (long long)n_keep);
  MELD_CHECK_ARG(transform >= MELD_PREP_IDENTITY && transform <= MELD_PREP_ARCSINH, "meld_prep_select_fill: transform=%d outside [0, 5]", transform);
  MELD_CHECK_ARG(transform != MELD_PREP_ARCSINH || cofactor > 0.0, "meld_prep_select_fill: cofactor=%g must be positive", cofactor);
  const long long* rp = reinterpret_cast<const long long*>(rowptr);
  const long long* orp = reinterpret_cast<const long long*>(out_rowptr);
  if (val_f32)
    select_fill_kernel<true><<<prep_row_blocks(n_keep), PREP_THREADS, 0, S(stream)>>>(rp, col, val, n_rows, (int)n_cols, rows, n_keep, col_map, scale,
                                                                                     rescale, transform, cofactor, orp, out_col, out_val, out_val_norm);
  else
    select_fill_kernel<false><<<prep_row_blocks(n_keep), PREP_THREADS, 0, S(stream)>>>(rp, col, val, n_rows, (int)n_cols, rows, n_keep, col_map, scale,
                                                                                      rescale, transform, cofactor, orp, out_col, out_val, out_val_norm);
  MELD_LAUNCH_CHECK("select_fill_kernel");
  return MELD_OK;
}

extern "C" int meld_prep_gene_moments(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_genes,
                                      int64_t n_cells, const uint8_t* row_keep, const double* row_scale, double rescale, int transform,
                                      double cofactor, const uint8_t* gene_mask, int64_t n_kept, int ddof, int32_t* count, double* mean,
                                      double* var, meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && col && val && count && mean && var, "meld_prep_gene_moments: rowptr, col, val, count, mean and var are required");
  MELD_CHECK_ARG(val_f32 == 0 || val_f32 == 1, "meld_prep_gene_moments: val_f32=%d outside {0, 1}", val_f32);
  MELD_CHECK_ARG(n_genes > 0 && n_genes < (1ll << 31), "meld_prep_gene_moments: n_genes=%lld outside [1, 2^31)", (long long)n_genes);
  MELD_CHECK_ARG(n_cells > 0 && n_cells < (1ll << 31), "meld_prep_gene_moments: n_cells=%lld outside [1, 2^31)", (long long)n_cells);
  MELD_CHECK_ARG(transform >= MELD_PREP_IDENTITY && transform <= MELD_PREP_ARCSINH, "meld_prep_gene_moments: transform=%d outside [0, 5]", transform);
  MELD_CHECK_ARG(transform != MELD_PREP_ARCSINH || cofactor > 0.0, "meld_prep_gene_moments: cofactor=%g must be positive", cofactor);
  MELD_CHECK_ARG(ddof == 0 || ddof == 1, "meld_prep_gene_moments: ddof=%d outside {0, 1}", ddof);
  MELD_CHECK_ARG(n_kept >= 1 && n_kept <= n_cells, "meld_prep_gene_moments: n_kept=%lld outside [1, n_cells=%lld]", (long long)n_kept,
                 (long long)n_cells);
  MELD_CHECK_ARG(n_kept - ddof >= 1, "meld_prep_gene_moments: n_kept=%lld leaves no degree of freedom with ddof=%d", (long long)n_kept, ddof);
  const long long* rp = reinterpret_cast<const long long*>(rowptr);
  const MomOperand a{col, val, (int)n_cells, row_keep, row_scale, rescale, transform, cofactor};
  const unsigned grid = (unsigned)ceil_div(n_genes, MOM_WAVES);
  if (val_f32)
    gene_moments_kernel<true><<<grid, MOM_THREADS, 0, S(stream)>>>(rp, a, n_genes, gene_mask, n_kept, ddof, count, mean, var);
  else
    gene_moments_kernel<false><<<grid, MOM_THREADS, 0, S(stream)>>>(rp, a, n_genes, gene_mask, n_kept, ddof, count, mean, var);
  MELD_LAUNCH_CHECK("gene_moments_kernel");
  return MELD_OK;
}
