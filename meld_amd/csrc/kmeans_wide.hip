// kmeans_wide.hip -- the Lloyd step for thousands of centres: nearest-centre assignment and per-cluster sums (meld_amd/kmeans.py).
//
// kmeans.hip keeps at most 64 centres of at most 32 dimensions in LDS.  The landmark features are [N, <= 100] and k is in the
// thousands: here the centres are streamed through LDS in tiles, for any k <= 4096 and d <= 128.
//
// Assignment.  Points are scored as |c_j|^2 - 2 y_i . c_j (the |y_i|^2 every candidate shares is left out of the comparison).
// The products run on v_mfma_f64_16x16x4_f64 (lane layout: csrc/subspace.hip): A[l & 15][l >> 4] = -2 y, B[l >> 4][l & 15] = c, the
// accumulator starts at |c_j|^2, so that D[(l >> 4) + 4 q][l & 15] IS the score of point (l >> 4) + 4 q against centre l & 15 of
// the tile.  A wave keeps the A fragments of two blocks of 16 points in registers across all centre tiles (one block for d > 96,
// where two would spill); a workgroup of 8 waves therefore amortises every staged tile over 256 (128) points.  A tile is 32
// centres; tile t + 1 is fetched into registers before the products of tile t and stored to the other LDS buffer after them (one
// barrier per tile).  LDS layout of a tile:
// [half (16 centres)][coordinate][centre in half], so that a B fragment is 64 consecutive doubles (no bank conflict).
// d is padded with zeros to a multiple of 16 (the template parameter), k to a multiple of 32 with centres whose |c|^2 is +inf:
// their score is +inf and the running minimum only ever takes a strictly smaller score.
//
// Tie rule: the minimum is kept on the pair (score, index).  A lane meets its centres in ascending index and replaces only on a
// strictly smaller score; the 16 lanes of a point then meet in a xor butterfly that takes the other pair if its score is smaller
// or equal with a smaller index.  Equal rows of C get equal bits (the same instruction sequence on the same operands), so the
// lower index of duplicates always wins.
//
// Sums.  One workgroup per cluster, 16 waves = 16 slots; the rows of the cluster (a segment of `order`) are cut into groups of 4,
// slot s adds the groups s, s + 16, ... in sequence, a lane owns columns lane and lane + 64; the slots' partials meet in LDS in slot
// order.  No atomics anywhere: the order of the additions is a function of (order, seg_ptr) and of the constants below.
#include "common.hpp"

namespace meld {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int KW_MAX_D = 128;
constexpr int KW_MAX_K = 4096;
constexpr int KW_THREADS = 512;
constexpr int KW_WAVES = KW_THREADS / 64;
constexpr int KW_KT = 32;  // centres per tile (two halves of 16)
// blocks of 16 points per wave: two while their A fragments (2 x 4 T doubles per lane) leave room for the rest in 256 registers
constexpr int kw_pb(int T) { return T <= 6 ? 2 : 1; }

constexpr int KS_SLOTS = 16;  // waves per cluster
constexpr int KS_GROUP = 4;   // rows a slot adds before the next slot's turn
constexpr int KS_THREADS = KS_SLOTS * 64;

// cn[j] = |c_j|^2, coordinates added in ascending order by one thread (fma chain)
__global__ __launch_bounds__(256) void kmeans_wide_norms_kernel(const double* __restrict__ C, int d, int k, double* __restrict__ cn) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= k) return;
  double s = 0.0;
  for (int c = 0; c < d; ++c) {
    const double v = C[(size_t)j * d + c];
    s = fma(v, v, s);
  }
  cn[j] = s;
}

template <int T>
__global__ __launch_bounds__(KW_THREADS) void kmeans_wide_assign_kernel(const double* __restrict__ Y, int64_t ldy, int64_t n, int d,
                                                                        const double* __restrict__ C, int k,
                                                                        const double* __restrict__ cn, int32_t* __restrict__ labels,
                                                                        double* __restrict__ best_d2) {
  constexpr int KW_PB = kw_pb(T), KW_POINTS = KW_WAVES * KW_PB * 16;
  constexpr int DP = 16 * T;        // padded dimension
  constexpr int STEPS = DP / 4;     // matrix instructions per (point block, half tile)
  constexpr int TILE = KW_KT * DP;  // doubles of a staged tile
  constexpr int PER = TILE / KW_THREADS;  // = T elements of a tile per thread
  __shared__ double s_c[2][TILE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * KW_POINTS + (int64_t)wv * (KW_PB * 16);

  // the points of this wave: A fragments (-2 y) and |y|^2
  double a[KW_PB][STEPS];
  double y2[KW_PB];
#pragma unroll
  for (int pb = 0; pb < KW_PB; ++pb) {
    const int64_t row = row0 + pb * 16 + c;
    const double* yr = Y + (size_t)(row < n ? row : 0) * ldy;
    double s2 = 0.0;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      const int col = 4 * s + g;
      const double v = (row < n && col < d) ? yr[col] : 0.0;
      s2 = fma(v, v, s2);
      a[pb][s] = -2.0 * v;
    }
    s2 += __shfl_xor(s2, 16, 64);
    s2 += __shfl_xor(s2, 32, 64);
    y2[pb] = s2;  // (every lane with l & 15 == c holds |y|^2 of point c of the block)
  }

  // element e = tid + KW_THREADS r of a tile: coordinate 4 (e >> 6) % STEPS + (e & 3) of centre 16 half + ((e >> 2) & 15)
  double stage[PER];
  auto fetch = [&](int j0) {
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int e = tid + KW_THREADS * r;
      const int rest = e >> 6;
      const int half = rest / STEPS, col = 4 * (rest % STEPS) + (e & 3);
      const int j = j0 + 16 * half + ((e >> 2) & 15);
      stage[r] = (j < k && col < d) ? C[(size_t)j * d + col] : 0.0;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int e = tid + KW_THREADS * r;
      const int rest = e >> 6;
      const int half = rest / STEPS, col = 4 * (rest % STEPS) + (e & 3);
      s_c[buf][(half * DP + col) * 16 + ((e >> 2) & 15)] = stage[r];
    }
  };

  double best[KW_PB][4];
  int bidx[KW_PB][4];
#pragma unroll
  for (int pb = 0; pb < KW_PB; ++pb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      best[pb][q] = __builtin_inf();
      bidx[pb][q] = 0;
    }

  const int n_tiles = (k + KW_KT - 1) / KW_KT;
  fetch(0);
  store(0);
  __syncthreads();
  for (int t = 0; t < n_tiles; ++t) {
    const int buf = t & 1, j0 = t * KW_KT;
    if (t + 1 < n_tiles) fetch(j0 + KW_KT);
    const int ja = j0 + c, jb = j0 + 16 + c;
    const double na = ja < k ? cn[ja] : __builtin_inf();
    const double nb = jb < k ? cn[jb] : __builtin_inf();
    double4_t acc[KW_PB][2];
#pragma unroll
    for (int pb = 0; pb < KW_PB; ++pb) {
      acc[pb][0] = double4_t{na, na, na, na};
      acc[pb][1] = double4_t{nb, nb, nb, nb};
    }
    const double* sc = s_c[buf];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      const double b0 = sc[(4 * s + g) * 16 + c];
      const double b1 = sc[(DP + 4 * s + g) * 16 + c];
#pragma unroll
      for (int pb = 0; pb < KW_PB; ++pb) {
        acc[pb][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[pb][s], b0, acc[pb][0], 0, 0, 0);
        acc[pb][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[pb][s], b1, acc[pb][1], 0, 0, 0);
      }
    }
#pragma unroll
    for (int pb = 0; pb < KW_PB; ++pb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {  // ascending index, strictly smaller only: the lowest index of equal scores stays
        if (acc[pb][0][q] < best[pb][q]) {
          best[pb][q] = acc[pb][0][q];
          bidx[pb][q] = ja;
        }
        if (acc[pb][1][q] < best[pb][q]) {
          best[pb][q] = acc[pb][1][q];
          bidx[pb][q] = jb;
        }
      }
    if (t + 1 < n_tiles) store(buf ^ 1);  // (the buffer the products of tile t - 1 read: every wave has passed the barrier since)
    __syncthreads();
  }

  // the 16 lanes of a point meet: (score, index), the lower index among equal scores
#pragma unroll
  for (int pb = 0; pb < KW_PB; ++pb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double bs = best[pb][q];
      int bi = bidx[pb][q];
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
        const double os = __shfl_xor(bs, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (os < bs || (os == bs && oi < bi)) {
          bs = os;
          bi = oi;
        }
      }
      const double yy = __shfl(y2[pb], g + 4 * q, 64);  // |y|^2 of point g + 4 q of the block
      const int64_t row = row0 + pb * 16 + g + 4 * q;
      if (c == 0 && row < n) {
        labels[row] = bi;
        if (best_d2) best_d2[row] = fmax(yy + bs, 0.0);
      }
    }
}

// sums[j][:] = the rows order[seg_ptr[j] .. seg_ptr[j + 1]) of Y, added in the order the header states
__global__ __launch_bounds__(KS_THREADS) void kmeans_wide_sums_kernel(const double* __restrict__ Y, int64_t ldy, int64_t n, int d,
                                                                      const int64_t* __restrict__ order,
                                                                      const int64_t* __restrict__ seg_ptr, double* __restrict__ sums) {
  __shared__ double s_p[KS_SLOTS][KW_MAX_D];
  const int lane = threadIdx.x & 63, slot = threadIdx.x >> 6;
  const int j = blockIdx.x;
  int64_t lo = seg_ptr[j], hi = seg_ptr[j + 1];
  lo = lo < 0 ? 0 : (lo > n ? n : lo);
  hi = hi < lo ? lo : (hi > n ? n : hi);
  const bool on0 = lane < d, on1 = lane + 64 < d;
  double s0 = 0.0, s1 = 0.0;
  for (int64_t r0 = lo + (int64_t)slot * KS_GROUP; r0 < hi; r0 += (int64_t)KS_SLOTS * KS_GROUP) {
    double v0[KS_GROUP], v1[KS_GROUP];
#pragma unroll
    for (int r = 0; r < KS_GROUP; ++r) {
      int64_t row = r0 + r < hi ? order[r0 + r] : -1;
      const bool in = row >= 0 && row < n;
      const double* yr = Y + (size_t)(in ? row : 0) * ldy;
      v0[r] = (in && on0) ? yr[lane] : 0.0;
      v1[r] = (in && on1) ? yr[lane + 64] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < KS_GROUP; ++r) {
      s0 += v0[r];
      s1 += v1[r];
    }
  }
  s_p[slot][lane] = s0;
  s_p[slot][lane + 64] = s1;
  __syncthreads();
  if (threadIdx.x < d) {
    double s = s_p[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < KS_SLOTS; ++w) s += s_p[w][threadIdx.x];
    sums[(size_t)j * d + threadIdx.x] = s;
  }
}

template <int T>
static void launch_assign(const double* Y, int64_t ldy, int64_t n, int d, const double* C, int k, const double* cn, int32_t* labels,
                          double* best_d2, hipStream_t st) {
  hipLaunchKernelGGL(kmeans_wide_assign_kernel<T>, dim3((unsigned)ceil_div(n, KW_WAVES * kw_pb(T) * 16)), dim3(KW_THREADS), 0, st, Y, ldy, n, d, C, k,
                     cn, labels, best_d2);
}

}  // namespace meld

using namespace meld;

extern "C" int meld_kmeans_wide_max_d(void) { return KW_MAX_D; }
extern "C" int meld_kmeans_wide_max_k(void) { return KW_MAX_K; }

extern "C" int meld_kmeans_wide_assign(const double* Y, int64_t ldy, int64_t n, int d, const double* centres, int k, double* centre_norms,
                                       int32_t* labels, double* best_d2, meld_stream_t stream) {
  MELD_CHECK_ARG(d >= 1 && d <= KW_MAX_D, "meld_kmeans_wide_assign: d=%d (1 <= d <= %d)", d, KW_MAX_D);
  MELD_CHECK_ARG(k >= 1 && k <= KW_MAX_K, "meld_kmeans_wide_assign: k=%d (1 <= k <= %d per call)", k, KW_MAX_K);
  MELD_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "meld_kmeans_wide_assign: n=%lld outside [0, 2^31)", (long long)n);
  MELD_CHECK_ARG(ldy >= d, "meld_kmeans_wide_assign: leading dimension ldy=%lld below d=%d", (long long)ldy, d);
  MELD_CHECK_ARG(centres && centre_norms, "meld_kmeans_wide_assign: centres and centre_norms are required");
  if (n == 0) return MELD_OK;
  MELD_CHECK_ARG(Y && labels, "meld_kmeans_wide_assign: Y and labels are required");
  hipStream_t st = S(stream);
  hipLaunchKernelGGL(kmeans_wide_norms_kernel, dim3((unsigned)ceil_div(k, 256)), dim3(256), 0, st, centres, d, k, centre_norms);
  MELD_LAUNCH_CHECK("kmeans_wide_norms_kernel");
  switch ((d + 15) / 16) {
    case 1: launch_assign<1>(Y, ldy, n, d, centres, k, centre_norms, labels, best_d2, st); break;
    case 2: launch_assign<2>(Y, ldy, n, d, centres, k, centre_norms, labels, best_d2, st); break;
    case 3: launch_assign<3>(Y, ldy, n, d, centres, k, centre_norms, labels, best_d2, st); break;
    case 4: launch_assign<4>(Y, ldy, n, d, centres, k, centre_norms, labels, best_d2, st); break;
    case 5: launch_assign<5>(Y, ldy, n, d, centres, k, centre_norms, labels, best_d2, st); break;
    case 6: launch_assign<6>(Y, ldy, n, d, centres, k, centre_norms, labels, best_d2, st); break;
    case 7: launch_assign<7>(Y, ldy, n, d, centres, k, centre_norms, labels, best_d2, st); break;
    default: launch_assign<8>(Y, ldy, n, d, centres, k, centre_norms, labels, best_d2, st); break;
  }
  MELD_LAUNCH_CHECK("kmeans_wide_assign_kernel");
  return MELD_OK;
}

extern "C" int meld_kmeans_wide_sums(const double* Y, int64_t ldy, int64_t n, int d, const int64_t* order, const int64_t* seg_ptr,
                                     int k, double* sums, meld_stream_t stream) {
  MELD_CHECK_ARG(d >= 1 && d <= KW_MAX_D, "meld_kmeans_wide_sums: d=%d (1 <= d <= %d)", d, KW_MAX_D);
  MELD_CHECK_ARG(k >= 1 && k < (1 << 30), "meld_kmeans_wide_sums: k=%d (at least one cluster)", k);
  MELD_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "meld_kmeans_wide_sums: n=%lld outside [0, 2^31)", (long long)n);
  MELD_CHECK_ARG(ldy >= d, "meld_kmeans_wide_sums: leading dimension ldy=%lld below d=%d", (long long)ldy, d);
  if (n == 0) return MELD_OK;
  MELD_CHECK_ARG(Y && order && seg_ptr && sums, "meld_kmeans_wide_sums: Y, order, seg_ptr and sums are required");
  hipLaunchKernelGGL(kmeans_wide_sums_kernel, dim3((unsigned)k), dim3(KS_THREADS), 0, S(stream), Y, ldy, n, d, order, seg_ptr, sums);
  MELD_LAUNCH_CHECK("kmeans_wide_sums_kernel");
  return MELD_OK;
}
