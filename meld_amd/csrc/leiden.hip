// leiden.hip -- the refinement phase of Leiden communities of a device CSR graph: between the move phase of a level (louvain.hip)
// and its contraction, every community P of the move partition is split into sub-communities that are CONNECTED, and the graph is
// contracted by those.  The run is meld_amd/leiden.py; the rule is restated in tests/leiden_reference.py.
//
// Reference surface: the reference clusters cells with scanpy's leiden (comparison/comparison.py, find_n_clusters(adata, k,
// "leiden")); upstream's rule is sequential and randomised, this one is synchronous and deterministic.
//
// A, k, 2m as in louvain.hip.  P_v is the community of v after the move phase (labels in [0, n), totC their sums of k), sub_v its
// sub-community (ids are vertex numbers; the refinement starts from sub = id), tot_t and size_t the sums of k and the sizes of the
// sub-communities.  One ROUND reads sub and writes sub':
//
//   propose.  v proposes only while it is alone (size[sub_v] = 1) and well connected to its community:
//         inC_v 2m >= (gamma k_v) (totC[P_v] - k_v),    inC_v = sum_{j != v, P_j = P_v} A_vj     in storage order
//     Over the entries j != v with P_j = P_v:  w_t = sum_{sub_j = t} A_vj in storage order, g(t) = w_t 2m - (gamma k_v) tot_t (every
//     operation rounded once: the file is built with -ffp-contract=off).  t is allowed if size_t >= 2 or pri(t, round) <
//     pri(v, round), pri a fixed bijection of the 32-bit ids (no ties: of two single neighbours exactly one may ask the other).
//     prop_v = the allowed t with the largest g(t) > 0, the lowest t among equals; -1 otherwise.
//   commit.   v joins t = prop_v iff size_t >= 2 or vertex t proposed nothing (a single vertex that asked to leave is not joined).
//
// Nobody leaves a sub-community of two or more, a non-empty label t contains vertex t, a joiner has an entry to the sub-community
// it joins: every sub-community induces a connected subgraph.
//
// Propose kernel: the shape of louvain_move_kernel<G> -- G = 16 or 64 lanes per row (meld_louvain_lanes), 256 threads, the row taken
// 4 G entries at a time, every chunk meeting all entries of the row through LDS tiles of 4 G (label, value), the argmax a xor
// butterfly on (g, id); a row may have any length, no private memory.  The label of an entry is sub_j where P_j = P_v and -1
// elsewhere (and for the diagonal and the padding), inC_v is summed in the first trip, and a row that is not alone leaves before
// any gather: it costs the loads of sub_v and size[sub_v] (a 16-lane group whose row left idles while its wave's other rows run).
// A row that is not well connected leaves after its first chunk.  Commit kernel: one thread per vertex, the movers of a workgroup
// counted through LDS by a fixed tree, leiden_count_kernel adds the workgroups' counts (integers: any order gives the same).  No
// atomics, nothing shared between workgroups: every output is a function of the operands alone.
// As compiled (-Rpass-analysis=kernel-resource-usage): no kernel of this file touches private memory (tests/test_leiden_host.py).
#include "common.hpp"

#include <limits.h>

namespace meld {

constexpr int LD_THREADS = 256;
constexpr int LD_SHORT = 16;  // lanes per row: the two widths of louvain.hip (meld_louvain_lanes chooses)
constexpr int LD_LONG = 64;
constexpr int LD_U = 4;  // entries of the row a lane holds at a time

// a bijection of the 32-bit ids for every round (xor-shifts and odd multipliers), compared unsigned
__device__ __forceinline__ unsigned ld_pri(unsigned id, unsigned round) {
  unsigned x = id + round * 0x9E3779B9u;
  x = (x ^ (x >> 16)) * 0x45D9F3Bu;
  x = (x ^ (x >> 16)) * 0x45D9F3Bu;
  return x ^ (x >> 16);
}

// the label of entry i of row r (`len` entries, community pr): the sub-community of its column where that lies in the row's
// community; -1 for padding, the diagonal entry, a column of another community and a label outside [0, n) (labels are addresses)
__device__ __forceinline__ int ld_entry_label(const int* __restrict__ col, const int* __restrict__ comm, const int* __restrict__ sub,
                                              long long rs, long long len, long long r, int pr, long long n, long long i) {
  if (i >= len) return -1;
  const int c = col[rs + i];
  if (c == r || comm[c] != pr) return -1;
  const int l = sub[c];
  return (unsigned long long)l < (unsigned long long)n ? l : -1;
}

template <int G>
__global__ __launch_bounds__(LD_THREADS) void leiden_propose_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                                    const double* __restrict__ val, long long n,
                                                                    const int* __restrict__ comm, const int* __restrict__ sub,
                                                                    const double* __restrict__ k, const double* __restrict__ tot,
                                                                    const int* __restrict__ size, const double* __restrict__ tot_comm,
                                                                    double two_m, double gamma, unsigned round, int* __restrict__ prop) {
  constexpr int ROWS = LD_THREADS / G;
  constexpr int TILE = G * LD_U;
  __shared__ int s_lab[ROWS][TILE];
  __shared__ double s_val[ROWS][TILE];
  const int g = threadIdx.x / G;
  const int lane = threadIdx.x % G;
  const long long r = (long long)blockIdx.x * ROWS + g;
  const int a = r < n ? sub[r] : -1;
  const int pr = r < n ? comm[r] : -1;
  // alone in a sub-community, with labels that are addresses of tot, size and tot_comm: every other row leaves before any gather
  const bool live = (unsigned long long)a < (unsigned long long)n && (unsigned long long)pr < (unsigned long long)n && size[a] == 1;
  double best_g = 0.0;
  int best_t = INT_MAX;
  if (live) {
    const long long rs = rowptr[r];
    const long long len = rowptr[r + 1] - rs;
    const double kr = k[r];
    const double gk = gamma * kr;
    const unsigned pri_r = ld_pri((unsigned)r, round);
    double in_c = 0.0;
    for (long long i0 = 0; i0 < len; i0 += TILE) {
      int li[LD_U];
      double vi[LD_U], sum[LD_U];
#pragma unroll
      for (int u = 0; u < LD_U; ++u) {
        const long long i = i0 + lane + G * u;
        li[u] = ld_entry_label(col, comm, sub, rs, len, r, pr, n, i);
        vi[u] = i < len ? val[rs + i] : 0.0;
        sum[u] = 0.0;
      }
      const bool first = i0 == 0;
      for (long long j0 = 0; j0 < len; j0 += TILE) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // (one wave: the loads of the last trip precede these stores)
#pragma unroll
        for (int u = 0; u < LD_U; ++u) {
          if (j0 == i0) {  // (uniform over the group: the tile is the chunk its lanes hold)
            s_lab[g][lane + G * u] = li[u];
            s_val[g][lane + G * u] = vi[u];
          } else {
            const long long j = j0 + lane + G * u;
            s_lab[g][lane + G * u] = ld_entry_label(col, comm, sub, rs, len, r, pr, n, j);
            s_val[g][lane + G * u] = j < len ? val[rs + j] : 0.0;
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // (one wave: its LDS stores precede its loads)
        const int jn = (int)min((long long)TILE, len - j0);
        for (int jj = 0; jj < jn; ++jj) {
          const int lj = s_lab[g][jj];  // (one address for the group: a broadcast)
          const double vj = s_val[g][jj];
#pragma unroll
          for (int u = 0; u < LD_U; ++u) sum[u] += (lj == li[u]) ? vj : 0.0;  // (x + 0 == x: the label's entries in storage order)
          if (first) in_c += (lj >= 0) ? vj : 0.0;                            // (the first chunk meets every entry of the row once)
        }
      }
      if (first) {
        const double need = gk * (tot_comm[pr] - kr);
        if (!(in_c * two_m >= need)) break;  // (uniform over the group; nothing has been scored: the row proposes nothing)
      }
#pragma unroll
      for (int u = 0; u < LD_U; ++u) {
        const int t = li[u];
        if (t >= 0 && t != a) {
          const bool allowed = size[t] >= 2 || ld_pri((unsigned)t, round) < pri_r;
          const double gt = sum[u] * two_m - gk * tot[t];  // (built with -ffp-contract=off: three roundings)
          if (allowed && gt > 0.0 && (gt > best_g || (gt == best_g && t < best_t))) {
            best_g = gt;
            best_t = t;
          }
        }
      }
    }
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    const double og = __shfl_xor(best_g, off, 64);
    const int ot = __shfl_xor(best_t, off, 64);
    if (og > best_g || (og == best_g && ot < best_t)) {
      best_g = og;
      best_t = ot;
    }
  }
  if (lane == 0 && r < n) prop[r] = best_t != INT_MAX ? best_t : -1;
}

// new_sub[v] = prop[v] where the proposal holds, sub[v] elsewhere; part_moved[block] = the movers of the workgroup
__global__ __launch_bounds__(LD_THREADS) void leiden_commit_kernel(const int* __restrict__ sub, const int* __restrict__ prop,
                                                                   const int* __restrict__ size, long long n,
                                                                   int* __restrict__ new_sub, int* __restrict__ part_moved) {
  __shared__ int s_mov[LD_THREADS];
  const long long v = (long long)blockIdx.x * LD_THREADS + threadIdx.x;
  int mv = 0;
  if (v < n) {
    const int t = prop[v];
    if ((unsigned long long)t < (unsigned long long)n) mv = (size[t] >= 2 || prop[t] < 0) ? 1 : 0;
    new_sub[v] = mv ? t : sub[v];
  }
  s_mov[threadIdx.x] = mv;
  __syncthreads();
  for (int off = LD_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s_mov[threadIdx.x] += s_mov[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) part_moved[blockIdx.x] = s_mov[0];
}

// movers[0] = the sum of part_moved: thread t takes the partials t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(LD_THREADS) void leiden_count_kernel(const int* __restrict__ part_moved, long long n_parts,
                                                                  long long* __restrict__ movers) {
  __shared__ long long s_mov[LD_THREADS];
  long long m = 0;
  for (long long p = threadIdx.x; p < n_parts; p += LD_THREADS) m += part_moved[p];
  s_mov[threadIdx.x] = m;
  __syncthreads();
  for (int off = LD_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s_mov[threadIdx.x] += s_mov[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) movers[0] = s_mov[0];
}

}  // namespace meld

using namespace meld;

extern "C" int64_t meld_leiden_commit_blocks(int64_t n) { return n > 0 ? ceil_div(n, LD_THREADS) : 0; }

extern "C" int meld_leiden_propose(const int64_t* rowptr, const int32_t* col, const double* val, int64_t n, const int32_t* comm,
                                   const int32_t* sub, const double* k, const double* tot, const int32_t* size, const double* tot_comm,
                                   double two_m, double gamma, int round, int lanes, int32_t* prop, meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && comm && sub && k && tot && size && tot_comm && prop,
                 "meld_leiden_propose: rowptr, comm, sub, k, tot, size, tot_comm and prop are required");
  MELD_CHECK_ARG(n >= 1 && n < (1ll << 31), "meld_leiden_propose: n=%lld outside [1, 2^31)", (long long)n);
  MELD_CHECK_ARG(lanes == LD_SHORT || lanes == LD_LONG, "meld_leiden_propose: lanes=%d (%d or %d per row)", lanes, LD_SHORT, LD_LONG);
  MELD_CHECK_ARG(round >= 0, "meld_leiden_propose: round=%d is negative", round);
  MELD_CHECK_ARG(two_m >= 0.0 && two_m < __builtin_inf() && gamma > 0.0 && gamma < __builtin_inf(),
                 "meld_leiden_propose: two_m=%g, gamma=%g (a finite two_m >= 0 and a finite gamma > 0)", two_m, gamma);
  MELD_CHECK_ARG(prop != sub && prop != comm && prop != size,
                 "meld_leiden_propose: prop is sub, comm or size (a round reads what other rows would have written)");
  const long long* rp = reinterpret_cast<const long long*>(rowptr);
  const unsigned blocks = (unsigned)ceil_div(n, LD_THREADS / lanes);
  if (lanes == LD_SHORT) {
    leiden_propose_kernel<LD_SHORT><<<blocks, LD_THREADS, 0, S(stream)>>>(rp, col, val, n, comm, sub, k, tot, size, tot_comm, two_m, gamma,
                                                                         (unsigned)round, prop);
  } else {
    leiden_propose_kernel<LD_LONG><<<blocks, LD_THREADS, 0, S(stream)>>>(rp, col, val, n, comm, sub, k, tot, size, tot_comm, two_m, gamma,
                                                                        (unsigned)round, prop);
  }
  MELD_LAUNCH_CHECK("leiden_propose_kernel");
  return MELD_OK;
}

extern "C" int meld_leiden_commit(const int32_t* sub, const int32_t* prop, const int32_t* size, int64_t n, int32_t* new_sub,
                                  int32_t* part_moved, int64_t* movers, meld_stream_t stream) {
  MELD_CHECK_ARG(sub && prop && size && new_sub && part_moved && movers,
                 "meld_leiden_commit: sub, prop, size, new_sub, part_moved and movers are required");
  MELD_CHECK_ARG(n >= 1 && n < (1ll << 31), "meld_leiden_commit: n=%lld outside [1, 2^31)", (long long)n);
  MELD_CHECK_ARG(new_sub != sub && new_sub != prop && new_sub != size,
                 "meld_leiden_commit: new_sub is sub, prop or size (a round reads what other vertices would have written)");
  const long long blocks = meld_leiden_commit_blocks(n);
  leiden_commit_kernel<<<(unsigned)blocks, LD_THREADS, 0, S(stream)>>>(sub, prop, size, n, new_sub, part_moved);
  MELD_LAUNCH_CHECK("leiden_commit_kernel");
  leiden_count_kernel<<<1, LD_THREADS, 0, S(stream)>>>(part_moved, blocks, reinterpret_cast<long long*>(movers));
  MELD_LAUNCH_CHECK("leiden_count_kernel");
  return MELD_OK;
}
