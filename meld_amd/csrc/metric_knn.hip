// metric_knn.hip -- exact kNN graph for the L1 (manhattan / cityblock / l1) and L-infinity (chebyshev) metrics.
//
// Replaces [UPSTREAM graphtools kNNGraph(distance=...) -> sklearn NearestNeighbors(metric=...)] for the metrics that are no
// function of the euclidean distance of transformed rows, so that the MFMA search of knn16.hip / refine.hip does not apply.
// Net semantics (those of the dense route, meld_amd/dense.py, and of graphtools with the metric handed to sklearn):
//   bw_i = (knn+1)-th smallest distance of row i, self counted, clipped to eps;  K_ij = exp(-(d_ij / bw_i)^decay) >= thresh.
//
// Every distance of this file is computed by ONE arithmetic, metric_acc below, in ONE order: coordinates k = 0 .. d - 1 added
// (L1) or maxed (L-inf) into a running value that starts at +0.  The candidate search, the refinement and the radius sweep
// therefore agree bit for bit: a bandwidth ranked by the search is the one the sweep confirms, and zero padding of the
// coordinate chunks (|0 - 0| = +0 added to / maxed with a non-negative value) changes nothing.
//
// Stages:
//   1. meld_metric_tile_boxes: per tile of MK_TILE rows (in the cells' locality order) the per-coordinate minimum and maximum.
//   2. meld_metric_topk: one wave per query tile, lane = query.  Each query keeps its ksel nearest references by (distance,
//      column) in a max-heap ([slot][query] layout in device memory, so that the lanes' accesses to one slot coalesce).
//      Tiles are visited near-first (the own tile and its index neighbours: the locality order puts them close in space),
//      then every other tile whose box bound does not exceed the largest heap top of the wave.  The bound is computed from the
//      boxes with a margin of 4 d ulps (the L1 bound's summation differs from the distance's), so the pruned search returns
//      exactly what the unpruned one does.
//   3. meld_metric_refine: bandwidth, kernel values, kept count per row; a row is certified when its list holds every cell or
//      its ksel-th distance lies beyond the kernel radius; other rows are flagged.
//   4. meld_metric_radius: count / fill sweep of the flagged rows over all references (the formats of meld_knn_radius_exact).
//
// The same four stages between two point sets -- queries that are not among the references: new cells against a fitted graph,
// DESIGN.md section 4.10 -- are the meld_metric_cross_* entries at the end of the file: a seed pre-pass (nearest reference tile
// per query), the search with the reference tiles optionally split into slices and a merge, a refinement without a self entry,
// a sweep that reads its rows from the queries.  The device code is shared: metric_search / metric_refine_row /
// metric_radius_sweep are the bodies of both families, the CROSS flag selects the differences at compile time.
#include "common.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace meld {

constexpr int MK_TILE = 64;   // rows per tile = queries per wave
constexpr int MK_HALF = 32;   // references held in registers at a time (half a tile)
constexpr int MK_DC = 16;     // coordinates per LDS chunk
constexpr int MK_NEAR = 3;    // index neighbours on either side visited right after the own tile
constexpr int MK_RB = 8;      // flagged rows per workgroup in the radius sweep
constexpr int MK_MAX_SLICES = 16;  // slices of the reference tiles in the search between two point sets

template <int METRIC>
__device__ __forceinline__ double metric_acc(double s, double a, double b) {
  const double t = a - b;
  if constexpr (METRIC == MELD_METRIC_L1) {
    return s + fabs(t);
  } else {
    return fmax(s, fabs(t));
  }
}

template <int METRIC>
__device__ __forceinline__ double metric_dist(const double* __restrict__ xa, const double* __restrict__ xb, int d) {
  double s = 0.0;
  for (int k = 0; k < d; ++k) s = metric_acc<METRIC>(s, xa[k], xb[k]);
  return s;
}

// lower bound of the distance between any two points of two boxes, one coordinate's gap
__device__ __forceinline__ double box_gap(double alo, double ahi, double blo, double bhi) {
  return fmax(0.0, fmax(alo - bhi, blo - ahi));
}

__device__ __forceinline__ double mk_decay_kernel(double dist, double bw, double decay) {
  if (isinf(decay)) return dist <= bw ? 1.0 : 0.0;  // decay=None: connectivity of the cells with d <= bw
  double v = exp(-pow(dist / bw, decay));
  if (v != v) v = 1.0;  // graphtools: NaN -> 1
  return v;
}

// (a, ia) after (b, ib) in the order (distance, column)
__device__ __forceinline__ bool mk_after(double a, int ia, double b, int ib) { return a > b || (a == b && ia > ib); }

// max-heap of `size` entries at hd[s * stride], hi[s * stride]: the root is replaced by (dn, in) and sifted down
__device__ __forceinline__ void mk_heap_sift(double* __restrict__ hd, int* __restrict__ hi, int64_t stride, int size, double dn, int in) {
  int pos = 0;
  for (;;) {
    int c = 2 * pos + 1;
    if (c >= size) break;
    double dc = hd[(int64_t)c * stride];
    int ic = hi[(int64_t)c * stride];
    if (c + 1 < size) {
      const double d2 = hd[(int64_t)(c + 1) * stride];
      const int i2 = hi[(int64_t)(c + 1) * stride];
      if (mk_after(d2, i2, dc, ic)) {
        c += 1;
        dc = d2;
        ic = i2;
      }
    }
    if (!mk_after(dc, ic, dn, in)) break;
    hd[(int64_t)pos * stride] = dc;
    hi[(int64_t)pos * stride] = ic;
    pos = c;
  }
  hd[(int64_t)pos * stride] = dn;
  hi[(int64_t)pos * stride] = in;
}

__global__ __launch_bounds__(64) void metric_tile_boxes_kernel(const double* __restrict__ X, int64_t N, int d, double* __restrict__ box_lo,
                                                               double* __restrict__ box_hi) {
  const int64_t t = blockIdx.x;
  const int64_t r0 = t * MK_TILE, r1 = min(N, r0 + MK_TILE);
  for (int k = threadIdx.x; k < d; k += 64) {
    double lo = INFINITY, hi = -INFINITY;
    for (int64_t r = r0; r < r1; ++r) {
      const double v = X[r * d + k];
      lo = fmin(lo, v);
      hi = fmax(hi, v);
    }
    box_lo[t * d + k] = lo;
    box_hi[t * d + k] = hi;
  }
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// The search of one wave: 64 queries (lane = query) against the reference tiles [t_lo, t_hi).  CROSS = false: the queries are
// the references themselves (Qm == X row-major, M == N), the wave's box is that of tile qt, the own tile is visited first.
// CROSS = true: the queries are another point set, handed over TRANSPOSED (Qm [d][M]: the lanes' reads of one coordinate
// coalesce); the wave's box is computed here, seed[q] names the reference tile nearest to query q (any tile is a valid seed:
// the order of the visits changes the cost, never the lists), blockIdx.y is a slice of the reference tiles with heaps and
// lists of its own (rows slice * M + q of the outputs).  New cells arrive in no spatial order, so a wave's box is wide: a tile
// that passes the box test is visited only if the point-to-box bound of at least one lane does not exceed that lane's heap top.
template <int METRIC, bool CROSS>
__device__ __forceinline__ void metric_search(const double* __restrict__ Qm, int64_t M, const double* __restrict__ X, int64_t N, int d,
                                              int64_t t_lo, int64_t t_hi, const double* __restrict__ box_lo,
                                              const double* __restrict__ box_hi, const int* __restrict__ seed, int ksel, int prune,
                                              double* __restrict__ heap_d, int* __restrict__ heap_i, int64_t stride,
                                              int* __restrict__ cand_idx, double* __restrict__ cand_d, int* __restrict__ cand_cnt,
                                              unsigned long long* __restrict__ tiles_done) {
  __shared__ __attribute__((aligned(16))) double Rs[MK_DC][MK_HALF];
  __shared__ double qlo[256], qhi[256];
  const int lane = threadIdx.x;
  const int64_t qt = blockIdx.x;
  const int64_t q = qt * MK_TILE + lane;
  const bool qv = q < M;
  const int64_t qrow = qv ? q : M - 1;
  const double* __restrict__ xq = CROSS ? Qm + qrow : Qm + qrow * d;  // coordinate k of the lane's query: xq[k * xs]
  const int64_t xs = CROSS ? M : 1;
  const int64_t slice = CROSS ? (int64_t)blockIdx.y : 0;
  double* __restrict__ hd = heap_d + slice * ksel * stride + q;
  int* __restrict__ hi = heap_i + slice * ksel * stride + q;
  if constexpr (CROSS) {
    for (int k = 0; k < d; ++k) {  // (the lanes past M repeat the last query: no effect on a minimum or a maximum)
      const double v = xq[k * xs];
      const double lo = -wave_max(-v), hb = wave_max(v);
      if (lane == 0) {
        qlo[k] = lo;
        qhi[k] = hb;
      }
    }
  } else {
    for (int k = lane; k < d; k += 64) {
      qlo[k] = box_lo[qt * d + k];
      qhi[k] = box_hi[qt * d + k];
    }
  }
  if (qv) {
    for (int s = 0; s < ksel; ++s) {
      hd[(int64_t)s * stride] = INFINITY;
      hi[(int64_t)s * stride] = 0x7fffffff;
    }
  }
  double top_d = INFINITY;
  int top_i = 0x7fffffff;
  __syncthreads();
  // margin of the bound: the L1 bound is summed in another order than the distances (relative error below d ulps either way)
  const double lb_scale = 1.0 - 4.0 * (double)d * DBL_EPSILON;
  unsigned long long done = 0;

  auto wave_threshold = [&]() { return wave_max(qv ? top_d : -INFINITY); };

  // one tile against the wave's 64 queries: distances of two halves of 32 references, each into the heaps
  auto visit = [&](int64_t t) {
    ++done;
    for (int h = 0; h < MK_TILE / MK_HALF; ++h) {
      const int64_t rb = t * MK_TILE + h * MK_HALF;
      if (rb >= N) break;
      double acc[MK_HALF];
#pragma unroll
      for (int j = 0; j < MK_HALF; ++j) acc[j] = 0.0;
      for (int k0 = 0; k0 < d; k0 += MK_DC) {
        __syncthreads();
        {
          const int j = lane & (MK_HALF - 1), kh = (lane >> 5) * (MK_DC / 2);
          const int64_t row = rb + j;
#pragma unroll
          for (int u = 0; u < MK_DC / 2; ++u) {
            const int k = k0 + kh + u;
            Rs[kh + u][j] = (row < N && k < d) ? X[row * d + k] : 0.0;
          }
        }
        double qc[MK_DC];
#pragma unroll
        for (int u = 0; u < MK_DC; ++u) qc[u] = (k0 + u < d) ? xq[(k0 + u) * xs] : 0.0;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MK_DC; ++u) {
          const double2* r2 = reinterpret_cast<const double2*>(&Rs[u][0]);
#pragma unroll
          for (int j = 0; j < MK_HALF; j += 2) {
            const double2 r = r2[j >> 1];
            acc[j] = metric_acc<METRIC>(acc[j], qc[u], r.x);
            acc[j + 1] = metric_acc<METRIC>(acc[j + 1], qc[u], r.y);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < MK_HALF; ++j) {
        const int col = (int)(rb + j);
        const double dj = (rb + j < N) ? acc[j] : INFINITY;
        if (qv && mk_after(top_d, top_i, dj, col)) {
          mk_heap_sift(hd, hi, stride, ksel, dj, col);
          top_d = hd[0];
          top_i = hi[0];
        }
      }
    }
  };

  // bound of tile t against the wave's box, the coordinates split over the lanes (phase 1)
  auto wave_bound = [&](int64_t t) {
    double g = 0.0;
    for (int k = lane; k < d; k += 64) {
      const double gk = box_gap(qlo[k], qhi[k], box_lo[t * d + k], box_hi[t * d + k]);
      g = (METRIC == MELD_METRIC_L1) ? g + gk : fmax(g, gk);
    }
    if (METRIC == MELD_METRIC_L1) return wave_sum(g) * lb_scale;
    return wave_max(g);
  };

  // can any query of the wave still gain from tile t?  The bound of a lane's own query against the tile's box is accumulated like
  // a distance -- coordinates ascending, from +0 -- and every term max(0, lo_k - x_k, x_k - hi_k) is at most |x_k - y_k| as the
  // distance computes it for a y inside the box (subtraction rounds monotonically), so the bound never exceeds a distance: no margin
  auto lane_wants = [&](int64_t t) {
    const double* __restrict__ blo = box_lo + t * d;
    const double* __restrict__ bhi = box_hi + t * d;
    double lb = 0.0;
    for (int k = 0; k < d; ++k) {
      const double x = xq[k * xs];
      const double gk = fmax(0.0, fmax(blo[k] - x, x - bhi[k]));
      lb = (METRIC == MELD_METRIC_L1) ? lb + gk : fmax(lb, gk);
    }
    return __ballot(qv && lb <= top_d) != 0;  // (<=: an equal distance with a lower column still enters)
  };

  // phase 1: the near tiles (near in space in the locality order), nearest index first
  int myseed = 0, smin = 0, smax = 0;
  if constexpr (CROSS) {
    // the seed tile of every lane and its index neighbours; a tile in the window of an earlier lane has had its turn
    myseed = seed[qrow];
    smin = smax = myseed;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      smin = min(smin, __shfl_xor(smin, off, 64));
      smax = max(smax, __shfl_xor(smax, off, 64));
    }
    int prev = -1;
    for (int l = 0; l < 64; ++l) {
      const int s = __shfl(myseed, l, 64);
      if (s == prev) continue;  // (the queries arrive sorted by seed: most lanes repeat their neighbour's)
      prev = s;
      for (int o = 0; o <= MK_NEAR; ++o) {
        for (int sgn = 0; sgn < (o ? 2 : 1); ++sgn) {
          const int64_t t = sgn ? (int64_t)s - o : (int64_t)s + o;
          if (t < t_lo || t >= t_hi) continue;
          if (__ballot(lane < l && t >= (int64_t)myseed - MK_NEAR && t <= (int64_t)myseed + MK_NEAR)) continue;
          if (prune && (wave_bound(t) > wave_threshold() || !lane_wants(t))) continue;
          visit(t);
        }
      }
    }
  } else {
    visit(qt);
    for (int o = 1; o <= MK_NEAR; ++o) {
      for (int sgn = 0; sgn < 2; ++sgn) {
        const int64_t t = sgn ? qt - o : qt + o;
        if (t < 0 || t >= t_hi) continue;
        if (prune && wave_bound(t) > wave_threshold()) continue;
        visit(t);
      }
    }
  }
  // phase 2: every other tile whose bound does not exceed the wave's largest threshold, a lane per tile computing the bound
  for (int64_t g0 = t_lo; g0 < t_hi; g0 += 64) {
    const int64_t t = g0 + lane;
    bool tv;
    if constexpr (CROSS) {
      tv = t < t_hi;
      const bool maybe = tv && t >= (int64_t)smin - MK_NEAR && t <= (int64_t)smax + MK_NEAR;
      if (__ballot(maybe)) {  // (a group of tiles that overlaps the span of the seeds: which of its tiles had their turn in phase 1)
        bool had = false;
        for (int l = 0; l < 64; ++l) {
          const int64_t s = __shfl(myseed, l, 64);
          had = had || (t >= s - MK_NEAR && t <= s + MK_NEAR);
        }
        tv = tv && !had;
      }
    } else {
      tv = t < t_hi && (t < qt - MK_NEAR || t > qt + MK_NEAR);
    }
    double lb = 0.0;
    if (tv && prune) {
      const double* __restrict__ blo = box_lo + t * d;
      const double* __restrict__ bhi = box_hi + t * d;
      for (int k = 0; k < d; ++k) {
        const double gk = box_gap(qlo[k], qhi[k], blo[k], bhi[k]);
        lb = (METRIC == MELD_METRIC_L1) ? lb + gk : fmax(lb, gk);
      }
      lb *= lb_scale;
    }
    double thr = wave_threshold();
    unsigned long long m = __ballot(tv && lb <= thr);
    while (m) {
      const int b = __ffsll((long long)m) - 1;
      m &= m - 1;
      const double lbt = __shfl(lb, b, 64);
      if (lbt > thr) continue;  // (the threshold fell since the ballot)
      if constexpr (CROSS) {
        if (prune && !lane_wants(g0 + b)) continue;
      }
      visit(g0 + b);
      thr = wave_threshold();
    }
  }
  // heap sort into the ascending candidate list of the row
  if (qv) {
    const int64_t o = slice * M + q;
    int cnt = 0;
    for (int s = ksel - 1; s >= 0; --s) {
      const double dr = hd[0];
      const int ir = hi[0];
      cand_d[o * ksel + s] = dr;
      cand_idx[o * ksel + s] = dr < INFINITY ? ir : 0;
      cnt += dr < INFINITY ? 1 : 0;
      if (s > 0) mk_heap_sift(hd, hi, stride, s, hd[(int64_t)s * stride], hi[(int64_t)s * stride]);
    }
    cand_cnt[o] = cnt;
  }
  if (lane == 0) atomicAdd(tiles_done, done);
}

template <int METRIC>
__global__ __launch_bounds__(64) void metric_topk_kernel(const double* __restrict__ X, int64_t N, int d, int64_t n_tiles,
                                                         const double* __restrict__ box_lo, const double* __restrict__ box_hi, int ksel,
                                                         int prune, double* __restrict__ heap_d, int* __restrict__ heap_i, int64_t stride,
                                                         int* __restrict__ cand_idx, double* __restrict__ cand_d, int* __restrict__ cand_cnt,
                                                         unsigned long long* __restrict__ tiles_done) {
  metric_search<METRIC, false>(X, N, X, N, d, 0, n_tiles, box_lo, box_hi, nullptr, ksel, prune, heap_d, heap_i, stride, cand_idx, cand_d,
                               cand_cnt, tiles_done);
}

// the search between two point sets: grid (query tiles, slices of the reference tiles).  (Three waves per SIMD asked for: the
// strided reads of the transposed queries cost a few address registers over the self search's 160.)
template <int METRIC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) void metric_cross_topk_kernel(const double* __restrict__ Qm, int64_t M, const double* __restrict__ X,
                                                               int64_t N, int d, int64_t n_tiles, int64_t tiles_per_slice,
                                                               const double* __restrict__ box_lo, const double* __restrict__ box_hi,
                                                               const int* __restrict__ seed, int ksel, int prune,
                                                               double* __restrict__ heap_d, int* __restrict__ heap_i, int64_t stride,
                                                               int* __restrict__ cand_idx, double* __restrict__ cand_d,
                                                               int* __restrict__ cand_cnt, unsigned long long* __restrict__ tiles_done) {
  const int64_t t_lo = (int64_t)blockIdx.y * tiles_per_slice;
  metric_search<METRIC, true>(Qm, M, X, N, d, t_lo, min(n_tiles, t_lo + tiles_per_slice), box_lo, box_hi, seed, ksel, prune, heap_d, heap_i,
                              stride, cand_idx, cand_d, cand_cnt, tiles_done);
}

// The reference tile nearest to every query by the point-to-box bound, the tiles split over grid.y: seed_key[q] (all ones on
// entry) = min over the tiles of (bound as fp32 bits << 32 | tile).  Rounding the bound to fp32 keeps its order; a seed is a
// place to start from, not a result.
template <int METRIC>
__global__ __launch_bounds__(64) void metric_cross_seed_kernel(const double* __restrict__ Qm, int64_t M, int d,
                                                               const double* __restrict__ box_lo, const double* __restrict__ box_hi,
                                                               int64_t n_tiles, int64_t tiles_per_slice,
                                                               unsigned long long* __restrict__ seed_key) {
  const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const double* __restrict__ xq = Qm + (q < M ? q : M - 1);  // (Qm [d][M]: transposed, as the search takes it)
  const int64_t t_lo = (int64_t)blockIdx.y * tiles_per_slice, t_hi = min(n_tiles, t_lo + tiles_per_slice);
  // (compared AS fp32: with the fp64 minimum of the part rounded afterwards, two tiles whose bounds agree in fp32 went to the later
  // one where its fp64 bound was lower, and the key depended on how the tiles were split over grid.y)
  float best = INFINITY;
  int64_t bt = t_lo;
  for (int64_t t = t_lo; t < t_hi; ++t) {
    const double* __restrict__ blo = box_lo + t * d;
    const double* __restrict__ bhi = box_hi + t * d;
    double lb = 0.0;
    for (int k = 0; k < d; ++k) {
      const double x = xq[(int64_t)k * M];
      const double gk = fmax(0.0, fmax(blo[k] - x, x - bhi[k]));
      lb = (METRIC == MELD_METRIC_L1) ? lb + gk : fmax(lb, gk);
    }
    const float lf = (float)lb;
    if (lf < best) {
      best = lf;
      bt = t;
    }
  }
  if (q < M && t_lo < t_hi)
    atomicMin(&seed_key[q], ((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)(uint32_t)bt);
}

// the ksel smallest by (distance, column) of a query's n_slices ascending lists: one thread per query, a cursor per slice in LDS
__global__ __launch_bounds__(256) void metric_cross_merge_kernel(const int* __restrict__ part_idx, const double* __restrict__ part_d,
                                                                 const int* __restrict__ part_cnt, int64_t M, int ksel, int n_slices,
                                                                 int* __restrict__ cand_idx, double* __restrict__ cand_d,
                                                                 int* __restrict__ cand_cnt) {
  __shared__ unsigned char pos[MK_MAX_SLICES][256];
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= M) return;
  for (int s = 0; s < n_slices; ++s) pos[s][threadIdx.x] = 0;
  int cnt = 0;
  for (int c = 0; c < ksel; ++c) {
    double best = INFINITY;
    int bi = 0x7fffffff, bs = -1;
    for (int s = 0; s < n_slices; ++s) {
      const int p = pos[s][threadIdx.x];
      const int64_t o = (int64_t)s * M + q;
      if (p >= part_cnt[o]) continue;
      const double dd = part_d[o * ksel + p];
      const int ii = part_idx[o * ksel + p];
      if (bs < 0 || mk_after(best, bi, dd, ii)) {
        best = dd;
        bi = ii;
        bs = s;
      }
    }
    if (bs >= 0) {
      pos[bs][threadIdx.x] += 1;
      cnt += 1;
    }
    cand_d[q * ksel + c] = bs >= 0 ? best : INFINITY;
    cand_idx[q * ksel + c] = bs >= 0 ? bi : 0;
  }
  cand_cnt[q] = cnt;
}

// one thread per row: bandwidth, kernel values and the completeness test.  CROSS: the rows are queries that are not among the
// references -- no entry is the row itself, the ranked distance is multiplied by bw_scale, and decay = +inf keeps the first
// knn + 1 entries of the list in (distance, column) order, whatever their distances.
template <bool CROSS>
__device__ __forceinline__ void metric_refine_row(const int* __restrict__ cand_idx, const double* __restrict__ cand_d,
                                                  const int* __restrict__ cand_cnt, int64_t N, int ksel, int knn, double decay, double thresh,
                                                  double radius_factor, double bw_scale, double* __restrict__ bw_out,
                                                  double* __restrict__ cand_val, int* __restrict__ keep_cnt, int* __restrict__ flag_rows,
                                                  int* __restrict__ n_flag) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= N) return;
  const int n = min(cand_cnt[q], ksel);
  const double* __restrict__ dq = cand_d + q * ksel;
  const int* __restrict__ iq = cand_idx + q * ksel;
  const bool first_k = CROSS && isinf(decay);
  const double bw = CROSS ? fmax(bw_scale * dq[min(knn, n - 1)], DBL_EPSILON) : fmax(dq[min(knn, n - 1)], DBL_EPSILON);
  // every reference outside a full list is at least as far as its last entry: beyond the radius (with the sweep's margin, far
  // above the rounding of pow / exp) its kernel value is below thresh
  const bool complete = first_k || n < ksel || dq[ksel - 1] > bw * radius_factor * (1.0 + 1e-9);
  int kept = 0;
  for (int c = 0; c < ksel; ++c) {
    double v = 0.0;
    if (complete && c < n) {
      if (first_k) {
        v = c <= knn ? 1.0 : 0.0;
      } else {
        v = mk_decay_kernel(dq[c], bw, decay);
        if (v < thresh || (!CROSS && (int64_t)iq[c] == q)) v = 0.0;  // diagonal handled analytically (K_ii = 1)
      }
    }
    cand_val[q * ksel + c] = v;
    kept += v > 0.0 ? 1 : 0;
  }
  bw_out[q] = bw;
  keep_cnt[q] = complete ? kept : 0;
  if (!complete) flag_rows[atomicAdd(n_flag, 1)] = (int)q;
}

__global__ __launch_bounds__(256) void metric_refine_kernel(const int* __restrict__ cand_idx, const double* __restrict__ cand_d,
                                                            const int* __restrict__ cand_cnt, int64_t N, int ksel, int knn, double decay,
                                                            double thresh, double radius_factor, double* __restrict__ bw_out,
                                                            double* __restrict__ cand_val, int* __restrict__ keep_cnt,
                                                            int* __restrict__ flag_rows, int* __restrict__ n_flag) {
  metric_refine_row<false>(cand_idx, cand_d, cand_cnt, N, ksel, knn, decay, thresh, radius_factor, 1.0, bw_out, cand_val, keep_cnt, flag_rows,
                           n_flag);
}

__global__ __launch_bounds__(256) void metric_cross_refine_kernel(const int* __restrict__ cand_idx, const double* __restrict__ cand_d,
                                                                  const int* __restrict__ cand_cnt, int64_t M, int ksel, int knn,
                                                                  double decay, double thresh, double radius_factor, double bw_scale,
                                                                  double* __restrict__ bw_out, double* __restrict__ cand_val,
                                                                  int* __restrict__ keep_cnt, int* __restrict__ flag_rows,
                                                                  int* __restrict__ n_flag) {
  metric_refine_row<true>(cand_idx, cand_d, cand_cnt, M, ksel, knn, decay, thresh, radius_factor, bw_scale, bw_out, cand_val, keep_cnt,
                          flag_rows, n_flag);
}

// exact sweep of the flagged rows: MK_RB rows per workgroup, a chunk of the references per grid row, a thread per reference.
// The flagged rows are rows of Qm; CROSS = false: Qm is X and a row does not count itself.
template <int METRIC, bool CROSS>
__device__ __forceinline__ void metric_radius_sweep(const double* __restrict__ Qm, const double* __restrict__ X, int64_t N, int d,
                                                    const int* __restrict__ flag_rows, int n_flag, const double* __restrict__ bw_all,
                                                    double decay, double thresh, double radius_factor, int mode, int* __restrict__ fb_cnt,
                                                    const int64_t* __restrict__ fb_off, int* __restrict__ fb_cursor,
                                                    int* __restrict__ fb_col, double* __restrict__ fb_val, int64_t ref_chunk) {
  extern __shared__ double xq[];  // [MK_RB][d]
  __shared__ int s_cnt[MK_RB];
  const int f0 = blockIdx.x * MK_RB;
  const int nf = min(MK_RB, n_flag - f0);
  const int64_t ref_lo = (int64_t)blockIdx.y * ref_chunk;
  const int64_t ref_hi = min(N, ref_lo + ref_chunk);
  int64_t gi[MK_RB];
  double bw[MK_RB], rad[MK_RB];
#pragma unroll
  for (int f = 0; f < MK_RB; ++f) {
    gi[f] = flag_rows[f0 + (f < nf ? f : 0)];
    bw[f] = bw_all[gi[f]];
    rad[f] = bw[f] * radius_factor * (1.0 + 1e-9);
  }
  for (int u = threadIdx.x; u < MK_RB * d; u += blockDim.x) {
    const int f = u / d, k = u % d;
    xq[u] = Qm[gi[f < nf ? f : 0] * d + k];
  }
  if (threadIdx.x < MK_RB) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  int cnt[MK_RB];
#pragma unroll
  for (int f = 0; f < MK_RB; ++f) cnt[f] = 0;
  for (int64_t ref = ref_lo + threadIdx.x; ref < ref_hi; ref += blockDim.x) {
    const double* __restrict__ xr = X + ref * d;
#pragma unroll
    for (int f = 0; f < MK_RB; ++f) {
      if (f >= nf) continue;
      const double dist = metric_dist<METRIC>(xq + f * d, xr, d);
      if (dist > rad[f] || (!CROSS && ref == gi[f])) continue;
      const double v = mk_decay_kernel(dist, bw[f], decay);
      if (v < thresh) continue;
      if (mode == 0) {
        cnt[f]++;
      } else {
        const int pos = atomicAdd(&fb_cursor[f0 + f], 1);
        fb_col[fb_off[f0 + f] + pos] = (int)ref;
        fb_val[fb_off[f0 + f] + pos] = v;
      }
    }
  }
  if (mode == 0) {
#pragma unroll
    for (int f = 0; f < MK_RB; ++f)
      if (cnt[f]) atomicAdd(&s_cnt[f], cnt[f]);
    __syncthreads();
    if (threadIdx.x < nf && s_cnt[threadIdx.x]) atomicAdd(&fb_cnt[f0 + threadIdx.x], s_cnt[threadIdx.x]);
  }
}

template <int METRIC>
__global__ __launch_bounds__(256) void metric_radius_kernel(const double* __restrict__ X, int64_t N, int d, const int* __restrict__ flag_rows,
                                                            int n_flag, const double* __restrict__ bw_all, double decay, double thresh,
                                                            double radius_factor, int mode, int* __restrict__ fb_cnt,
                                                            const int64_t* __restrict__ fb_off, int* __restrict__ fb_cursor,
                                                            int* __restrict__ fb_col, double* __restrict__ fb_val, int64_t ref_chunk) {
  metric_radius_sweep<METRIC, false>(X, X, N, d, flag_rows, n_flag, bw_all, decay, thresh, radius_factor, mode, fb_cnt, fb_off, fb_cursor, fb_col,
                                     fb_val, ref_chunk);
}

template <int METRIC>
__global__ __launch_bounds__(256) void metric_cross_radius_kernel(const double* __restrict__ Qm, const double* __restrict__ X, int64_t N, int d,
                                                                  const int* __restrict__ flag_rows, int n_flag,
                                                                  const double* __restrict__ bw_all, double decay, double thresh,
                                                                  double radius_factor, int mode, int* __restrict__ fb_cnt,
                                                                  const int64_t* __restrict__ fb_off, int* __restrict__ fb_cursor,
                                                                  int* __restrict__ fb_col, double* __restrict__ fb_val, int64_t ref_chunk) {
  metric_radius_sweep<METRIC, true>(Qm, X, N, d, flag_rows, n_flag, bw_all, decay, thresh, radius_factor, mode, fb_cnt, fb_off, fb_cursor, fb_col,
                                    fb_val, ref_chunk);
}

}  // namespace meld

using namespace meld;

extern "C" int meld_metric_tile_rows(void) { return MK_TILE; }

extern "C" int meld_metric_tile_boxes(const double* X, int64_t N, int d, double* box_lo, double* box_hi, meld_stream_t stream) {
  MELD_CHECK_ARG(X && box_lo && box_hi && N > 0 && d > 0 && d <= 256, "meld_metric_tile_boxes: bad arguments (d=%d must be in [1, 256])", d);
  hipLaunchKernelGGL(metric_tile_boxes_kernel, dim3((unsigned)ceil_div(N, MK_TILE)), dim3(64), 0, S(stream), X, N, d, box_lo, box_hi);
  MELD_LAUNCH_CHECK("metric_tile_boxes_kernel");
  return MELD_OK;
}

extern "C" int meld_metric_topk(const double* X, int64_t N, int d, int metric, int ksel, const double* box_lo, const double* box_hi,
                                int prune, double* heap_d, int32_t* heap_i, int32_t* cand_idx, double* cand_d, int32_t* cand_cnt,
                                unsigned long long* tiles_done, meld_stream_t stream) {
  MELD_CHECK_ARG(X && box_lo && box_hi && heap_d && heap_i && cand_idx && cand_d && cand_cnt && tiles_done && N > 0 && N < INT32_MAX,
                 "meld_metric_topk: bad arguments");
  MELD_CHECK_ARG(d > 0 && d <= 256 && ksel > 0 && ksel <= 128, "meld_metric_topk: d=%d must be in [1, 256], ksel=%d in [1, 128]", d, ksel);
  const int64_t n_tiles = ceil_div(N, MK_TILE);
  const int64_t stride = n_tiles * MK_TILE;  // heap slots: [ksel][stride]
  if (metric == MELD_METRIC_L1) {
    hipLaunchKernelGGL(metric_topk_kernel<MELD_METRIC_L1>, dim3((unsigned)n_tiles), dim3(64), 0, S(stream), X, N, d, n_tiles, box_lo, box_hi,
                       ksel, prune, heap_d, heap_i, stride, cand_idx, cand_d, cand_cnt, tiles_done);
  } else if (metric == MELD_METRIC_LINF) {
    hipLaunchKernelGGL(metric_topk_kernel<MELD_METRIC_LINF>, dim3((unsigned)n_tiles), dim3(64), 0, S(stream), X, N, d, n_tiles, box_lo, box_hi,
                       ksel, prune, heap_d, heap_i, stride, cand_idx, cand_d, cand_cnt, tiles_done);
  } else {
    MELD_CHECK_ARG(false, "meld_metric_topk: unknown metric %d", metric);
  }
  MELD_LAUNCH_CHECK("metric_topk_kernel");
  return MELD_OK;
}

extern "C" int meld_metric_refine(const int32_t* cand_idx, const double* cand_d, const int32_t* cand_cnt, int64_t N, int ksel, int knn,
                                  double decay, double thresh, double* bw, double* cand_val, int32_t* keep_cnt, int32_t* flag_rows,
                                  int32_t* n_flag, meld_stream_t stream) {
  MELD_CHECK_ARG(cand_idx && cand_d && cand_cnt && bw && cand_val && keep_cnt && flag_rows && n_flag && N > 0,
                 "meld_metric_refine: bad arguments");
  MELD_CHECK_ARG(knn >= 0 && knn < ksel && thresh > 0.0, "meld_metric_refine: knn=%d must be below ksel=%d, thresh > 0", knn, ksel);
  const double rf = std::isinf(decay) ? 1.0 : pow(-log(thresh), 1.0 / decay);
  hipLaunchKernelGGL(metric_refine_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, S(stream), cand_idx, cand_d, cand_cnt, N, ksel,
                     knn, decay, thresh, rf, bw, cand_val, keep_cnt, flag_rows, n_flag);
  MELD_LAUNCH_CHECK("metric_refine_kernel");
  return MELD_OK;
}

extern "C" int meld_metric_radius(const double* X, int64_t N, int d, int metric, const int32_t* flag_rows, int32_t n_flag, const double* bw,
                                  double decay, double thresh, int mode, int32_t* fb_cnt, const int64_t* fb_off, int32_t* fb_cursor,
                                  int32_t* fb_col, double* fb_val, meld_stream_t stream) {
  MELD_CHECK_ARG(X && flag_rows && bw && N > 0 && d > 0 && d <= 256 && thresh > 0.0 && (mode == 0 || mode == 1),
                 "meld_metric_radius: bad arguments");
  MELD_CHECK_ARG(mode == 0 ? fb_cnt != nullptr : (fb_off && fb_cursor && fb_col && fb_val), "meld_metric_radius: missing arrays for mode %d", mode);
  if (n_flag <= 0) return MELD_OK;
  const double rf = std::isinf(decay) ? 1.0 : pow(-log(thresh), 1.0 / decay);
  const int64_t n_groups = ceil_div(n_flag, MK_RB);
  // rows x reference chunks: about 4096 workgroups over the device, chunks of at least 1024 references
  const int64_t n_chunks = std::max<int64_t>(1, std::min<int64_t>(ceil_div(4096, n_groups), ceil_div(N, 1024)));
  const int64_t ref_chunk = ceil_div(N, n_chunks);
  const dim3 grid((unsigned)n_groups, (unsigned)ceil_div(N, ref_chunk));
  const size_t lds = sizeof(double) * MK_RB * d;
  if (metric == MELD_METRIC_L1) {
    hipLaunchKernelGGL(metric_radius_kernel<MELD_METRIC_L1>, grid, dim3(256), lds, S(stream), X, N, d, flag_rows, n_flag, bw, decay, thresh, rf,
                       mode, fb_cnt, fb_off, fb_cursor, fb_col, fb_val, ref_chunk);
  } else if (metric == MELD_METRIC_LINF) {
    hipLaunchKernelGGL(metric_radius_kernel<MELD_METRIC_LINF>, grid, dim3(256), lds, S(stream), X, N, d, flag_rows, n_flag, bw, decay, thresh, rf,
                       mode, fb_cnt, fb_off, fb_cursor, fb_col, fb_val, ref_chunk);
  } else {
    MELD_CHECK_ARG(false, "meld_metric_radius: unknown metric %d", metric);
  }
  MELD_LAUNCH_CHECK("metric_radius_kernel");
  return MELD_OK;
}

// ---- new cells against a fitted set ----------------------------------------------------------------

// slices of the reference tiles for M queries: enough (query tile, slice) waves to fill the device, at least 16 tiles a slice
extern "C" int meld_metric_cross_slices(int64_t M, int64_t N, int n_slices) {
  if (M <= 0 || N <= 0 || n_slices < 0) return MELD_ERR_INVALID;
  const int64_t n_tiles = ceil_div(N, MK_TILE), q_tiles = ceil_div(M, MK_TILE);
  if (n_slices == 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    n_slices = (int)std::min<int64_t>(ceil_div(8 * (int64_t)cus, q_tiles), std::max<int64_t>(1, n_tiles / 16));
  }
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_slices, MK_MAX_SLICES), n_tiles));
}

extern "C" int meld_metric_cross_seed(const double* Qt, int64_t M, const double* box_lo, const double* box_hi, int64_t N, int d, int metric,
                                      unsigned long long* seed_key, meld_stream_t stream) {
  MELD_CHECK_ARG(Qt && box_lo && box_hi && seed_key && M > 0 && N > 0 && N < INT32_MAX && d > 0 && d <= 256,
                 "meld_metric_cross_seed: bad arguments (d=%d must be in [1, 256])", d);
  const int64_t n_tiles = ceil_div(N, MK_TILE), q_tiles = ceil_div(M, MK_TILE);
  // about 2048 waves over the device, at least 64 tiles each
  const int64_t n_parts = std::max<int64_t>(1, std::min<int64_t>(ceil_div(2048, q_tiles), ceil_div(n_tiles, 64)));
  const int64_t per = ceil_div(n_tiles, n_parts);
  const dim3 grid((unsigned)q_tiles, (unsigned)ceil_div(n_tiles, per));
  if (metric == MELD_METRIC_L1) {
    hipLaunchKernelGGL(metric_cross_seed_kernel<MELD_METRIC_L1>, grid, dim3(64), 0, S(stream), Qt, M, d, box_lo, box_hi, n_tiles, per, seed_key);
  } else if (metric == MELD_METRIC_LINF) {
    hipLaunchKernelGGL(metric_cross_seed_kernel<MELD_METRIC_LINF>, grid, dim3(64), 0, S(stream), Qt, M, d, box_lo, box_hi, n_tiles, per, seed_key);
  } else {
    MELD_CHECK_ARG(false, "meld_metric_cross_seed: unknown metric %d", metric);
  }
  MELD_LAUNCH_CHECK("metric_cross_seed_kernel");
  return MELD_OK;
}

extern "C" int meld_metric_cross_topk(const double* Qt, int64_t M, const double* X, int64_t N, int d, int metric, int ksel, const double* box_lo,
                                      const double* box_hi, const int32_t* seed, int prune, int n_slices, double* heap_d, int32_t* heap_i,
                                      int32_t* part_idx, double* part_d, int32_t* part_cnt, int32_t* cand_idx, double* cand_d,
                                      int32_t* cand_cnt, unsigned long long* tiles_done, meld_stream_t stream) {
  MELD_CHECK_ARG(Qt && X && box_lo && box_hi && seed && heap_d && heap_i && cand_idx && cand_d && cand_cnt && tiles_done && M > 0 &&
                     M < INT32_MAX && N > 0 && N < INT32_MAX,
                 "meld_metric_cross_topk: bad arguments");
  MELD_CHECK_ARG(d > 0 && d <= 256 && ksel > 0 && ksel <= 128, "meld_metric_cross_topk: d=%d must be in [1, 256], ksel=%d in [1, 128]", d, ksel);
  const int64_t n_tiles = ceil_div(N, MK_TILE), q_tiles = ceil_div(M, MK_TILE);
  MELD_CHECK_ARG(n_slices >= 1 && n_slices <= MK_MAX_SLICES && n_slices <= n_tiles,
                 "meld_metric_cross_topk: n_slices=%d must be what meld_metric_cross_slices returned", n_slices);
  const int64_t per = ceil_div(n_tiles, n_slices);
  const int ny = (int)ceil_div(n_tiles, per);  // (no empty slice)
  MELD_CHECK_ARG(ny == 1 || (part_idx && part_d && part_cnt), "meld_metric_cross_topk: %d slices need the partial lists", ny);
  MELD_CHECK_ARG(q_tiles * ny < INT32_MAX, "meld_metric_cross_topk: too many query tiles");
  const int64_t stride = q_tiles * MK_TILE;  // heap slots: [slice][ksel][stride]
  int32_t* oi = ny == 1 ? cand_idx : part_idx;
  double* od = ny == 1 ? cand_d : part_d;
  int32_t* oc = ny == 1 ? cand_cnt : part_cnt;
  const dim3 grid((unsigned)q_tiles, (unsigned)ny);
  if (metric == MELD_METRIC_L1) {
    hipLaunchKernelGGL(metric_cross_topk_kernel<MELD_METRIC_L1>, grid, dim3(64), 0, S(stream), Qt, M, X, N, d, n_tiles, per, box_lo, box_hi, seed,
                       ksel, prune, heap_d, heap_i, stride, oi, od, oc, tiles_done);
  } else if (metric == MELD_METRIC_LINF) {
    hipLaunchKernelGGL(metric_cross_topk_kernel<MELD_METRIC_LINF>, grid, dim3(64), 0, S(stream), Qt, M, X, N, d, n_tiles, per, box_lo, box_hi, seed,
                       ksel, prune, heap_d, heap_i, stride, oi, od, oc, tiles_done);
  } else {
    MELD_CHECK_ARG(false, "meld_metric_cross_topk: unknown metric %d", metric);
  }
  MELD_LAUNCH_CHECK("metric_cross_topk_kernel");
  if (ny > 1) {
    hipLaunchKernelGGL(metric_cross_merge_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, S(stream), part_idx, part_d, part_cnt, M, ksel,
                       ny, cand_idx, cand_d, cand_cnt);
    MELD_LAUNCH_CHECK("metric_cross_merge_kernel");
  }
  return MELD_OK;
}

extern "C" int meld_metric_cross_refine(const int32_t* cand_idx, const double* cand_d, const int32_t* cand_cnt, int64_t M, int ksel, int knn,
                                        double decay, double thresh, double bw_scale, double* bw, double* cand_val, int32_t* keep_cnt,
                                        int32_t* flag_rows, int32_t* n_flag, meld_stream_t stream) {
  MELD_CHECK_ARG(cand_idx && cand_d && cand_cnt && bw && cand_val && keep_cnt && flag_rows && n_flag && M > 0,
                 "meld_metric_cross_refine: bad arguments");
  MELD_CHECK_ARG(knn >= 0 && knn < ksel && thresh > 0.0 && bw_scale > 0.0,
                 "meld_metric_cross_refine: knn=%d must be below ksel=%d, thresh > 0, bw_scale > 0", knn, ksel);
  const double rf = std::isinf(decay) ? 1.0 : pow(-log(thresh), 1.0 / decay);
  hipLaunchKernelGGL(metric_cross_refine_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, S(stream), cand_idx, cand_d, cand_cnt, M, ksel,
                     knn, decay, thresh, rf, bw_scale, bw, cand_val, keep_cnt, flag_rows, n_flag);
  MELD_LAUNCH_CHECK("metric_cross_refine_kernel");
  return MELD_OK;
}

extern "C" int meld_metric_cross_radius(const double* Q, int64_t M, const double* X, int64_t N, int d, int metric, const int32_t* flag_rows,
                                        int32_t n_flag, const double* bw, double decay, double thresh, int mode, int32_t* fb_cnt,
                                        const int64_t* fb_off, int32_t* fb_cursor, int32_t* fb_col, double* fb_val, meld_stream_t stream) {
  MELD_CHECK_ARG(Q && X && flag_rows && bw && M > 0 && N > 0 && N < INT32_MAX && d > 0 && d <= 256 && thresh > 0.0 && (mode == 0 || mode == 1) &&
                     n_flag <= M,
                 "meld_metric_cross_radius: bad arguments");
  MELD_CHECK_ARG(mode == 0 ? fb_cnt != nullptr : (fb_off && fb_cursor && fb_col && fb_val), "meld_metric_cross_radius: missing arrays for mode %d",
                 mode);
  if (n_flag <= 0) return MELD_OK;
  const double rf = std::isinf(decay) ? 1.0 : pow(-log(thresh), 1.0 / decay);
  const int64_t n_groups = ceil_div(n_flag, MK_RB);
  const int64_t n_chunks = std::max<int64_t>(1, std::min<int64_t>(ceil_div(4096, n_groups), ceil_div(N, 1024)));
  const int64_t ref_chunk = ceil_div(N, n_chunks);
  const dim3 grid((unsigned)n_groups, (unsigned)ceil_div(N, ref_chunk));
  const size_t lds = sizeof(double) * MK_RB * d;
  if (metric == MELD_METRIC_L1) {
    hipLaunchKernelGGL(metric_cross_radius_kernel<MELD_METRIC_L1>, grid, dim3(256), lds, S(stream), Q, X, N, d, flag_rows, n_flag, bw, decay, thresh,
                       rf, mode, fb_cnt, fb_off, fb_cursor, fb_col, fb_val, ref_chunk);
  } else if (metric == MELD_METRIC_LINF) {
    hipLaunchKernelGGL(metric_cross_radius_kernel<MELD_METRIC_LINF>, grid, dim3(256), lds, S(stream), Q, X, N, d, flag_rows, n_flag, bw, decay,
                       thresh, rf, mode, fb_cnt, fb_off, fb_cursor, fb_col, fb_val, ref_chunk);
  } else {
    MELD_CHECK_ARG(false, "meld_metric_cross_radius: unknown metric %d", metric);
  }
  MELD_LAUNCH_CHECK("metric_cross_radius_kernel");
  return MELD_OK;
}
