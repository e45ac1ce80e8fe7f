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
// Propose kernel: leiden_propose_kernel<G> is the row pass of label_rows.hpp (the scheme is stated there; meld_louvain_lanes chooses
// G) with ld_propose_op: the label of an entry is sub_j where P_j = P_v and -1 elsewhere (and for the diagonal and the padding); the
// first chunk's trips leave inC_v; a row that is not well connected leaves after them; an entry is scored by g(t) under the allowed
// test above.  A row that is not alone leaves before any gather: it costs the loads of sub_v and size[sub_v] (a 16-lane group whose
// row left idles while its wave's other rows run).  Commit kernel: one thread per vertex, the movers of a workgroup counted through
// LDS by a fixed tree, leiden_count_kernel adds the workgroups' counts (integers: any order gives the same).  No atomics, nothing
// shared between workgroups: every output is a function of the operands alone.
// As compiled (-Rpass-analysis=kernel-resource-usage): no kernel of this file touches private memory (tests/test_leiden_host.py).
#include "label_rows.hpp"

namespace meld {

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

// what the refinement adds to the row pass (label_rows.hpp): the row r of sub-community a in community pr
struct ld_propose_op {
  const int* __restrict__ col;
  const int* __restrict__ comm;
  const int* __restrict__ sub;
  const double* __restrict__ tot;
  const int* __restrict__ size;
  const double* __restrict__ tot_comm;
  long long n;
  double two_m;
  unsigned round;
  long long r;  // the row, its sub-community and its community
  int a, pr;
  long long rs = 0, len = 0;  // set for a live row
  unsigned pri_r = 0;
  double kr = 0.0, gk = 0.0;
  double in_c = 0.0;
  label_best best{0.0, INT_MAX};  // (only a positive score is offered)
  __device__ __forceinline__ int label(long long i) const { return ld_entry_label(col, comm, sub, rs, len, r, pr, n, i); }
  __device__ __forceinline__ void meet(int lj, double vj) { in_c += (lj >= 0) ? vj : 0.0; }
  __device__ __forceinline__ bool go_on() const {  // well connected to its community; otherwise the row proposes nothing
    const double need = gk * (tot_comm[pr] - kr);
    return in_c * two_m >= need;
  }
  __device__ __forceinline__ void score(int t, double w) {
    if (t >= 0 && t != a) {
      const bool allowed = size[t] >= 2 || ld_pri((unsigned)t, round) < pri_r;
      const double gt = w * two_m - gk * tot[t];  // (built with -ffp-contract=off: three roundings)
      if (allowed && gt > 0.0) best.offer(gt, t);
    }
  }
};

template <int G>
__global__ __launch_bounds__(LR_THREADS) void leiden_propose_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                                    const double* __restrict__ val, long long n,
                                                                    const int* __restrict__ comm, const int* __restrict__ sub,
                                                                    const double* __restrict__ k, const double* __restrict__ tot,
                                                                    const int* __restrict__ size, const double* __restrict__ tot_comm,
                                                                    double two_m, double gamma, unsigned round, int* __restrict__ prop) {
  __shared__ label_tiles<G> s_tiles;
  const int lane = threadIdx.x % G;
  const long long r = (long long)blockIdx.x * (LR_THREADS / G) + threadIdx.x / G;
  const int a = r < n ? sub[r] : -1;
  const int pr = r < n ? comm[r] : -1;
  // alone in a sub-community, with labels that are addresses of tot, size and tot_comm: every other row leaves before any gather
  const bool live = (unsigned long long)a < (unsigned long long)n && (unsigned long long)pr < (unsigned long long)n && size[a] == 1;
  ld_propose_op op{col, comm, sub, tot, size, tot_comm, n, two_m, round, r, a, pr};
  if (live) {
    op.rs = rowptr[r];
    op.len = rowptr[r + 1] - op.rs;
    op.kr = k[r];
    op.gk = gamma * op.kr;
    op.pri_r = ld_pri((unsigned)r, round);
    label_row_pass<G, true>(s_tiles, val, op);
  }
  op.best.over_lanes<G>();
  if (lane == 0 && r < n) prop[r] = op.best.id != INT_MAX ? op.best.id : -1;
}

// new_sub[v] = prop[v] where the proposal holds, sub[v] elsewhere; part_moved[block] = the movers of the workgroup
__global__ __launch_bounds__(LR_THREADS) void leiden_commit_kernel(const int* __restrict__ sub, const int* __restrict__ prop,
                                                                   const int* __restrict__ size, long long n,
                                                                   int* __restrict__ new_sub, int* __restrict__ part_moved) {
  __shared__ int s_mov[LR_THREADS];
  const long long v = (long long)blockIdx.x * LR_THREADS + threadIdx.x;
  int mv = 0;
  if (v < n) {
    const int t = prop[v];
    if ((unsigned long long)t < (unsigned long long)n) mv = (size[t] >= 2 || prop[t] < 0) ? 1 : 0;
    new_sub[v] = mv ? t : sub[v];
  }
  s_mov[threadIdx.x] = mv;
  __syncthreads();
  for (int off = LR_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s_mov[threadIdx.x] += s_mov[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) part_moved[blockIdx.x] = s_mov[0];
}

// movers[0] = the sum of part_moved: thread t takes the partials t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(LR_THREADS) void leiden_count_kernel(const int* __restrict__ part_moved, long long n_parts,
                                                                  long long* __restrict__ movers) {
  __shared__ long long s_mov[LR_THREADS];
  long long m = 0;
  for (long long p = threadIdx.x; p < n_parts; p += LR_THREADS) m += part_moved[p];
  s_mov[threadIdx.x] = m;
  __syncthreads();
  for (int off = LR_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s_mov[threadIdx.x] += s_mov[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) movers[0] = s_mov[0];
}

}  // namespace meld

using namespace meld;

extern "C" int64_t meld_leiden_commit_blocks(int64_t n) { return n > 0 ? ceil_div(n, LR_THREADS) : 0; }

extern "C" int meld_leiden_propose(const int64_t* rowptr, const int32_t* col, const double* val, int64_t n, const int32_t* comm,
                                   const int32_t* sub, const double* k, const double* tot, const int32_t* size, const double* tot_comm,
                                   double two_m, double gamma, int round, int lanes, int32_t* prop, meld_stream_t stream) {
  MELD_CHECK_ARG(rowptr && comm && sub && k && tot && size && tot_comm && prop,
                 "meld_leiden_propose: rowptr, comm, sub, k, tot, size, tot_comm and prop are required");
  MELD_CHECK_ARG(n >= 1 && n < (1ll << 31), "meld_leiden_propose: n=%lld outside [1, 2^31)", (long long)n);
  MELD_CHECK_ARG(lanes == LR_SHORT || lanes == LR_LONG, "meld_leiden_propose: lanes=%d (%d or %d per row)", lanes, LR_SHORT, LR_LONG);
  MELD_CHECK_ARG(round >= 0, "meld_leiden_propose: round=%d is negative", round);
  MELD_CHECK_ARG(two_m >= 0.0 && two_m < __builtin_inf() && gamma > 0.0 && gamma < __builtin_inf(),
                 "meld_leiden_propose: two_m=%g, gamma=%g (a finite two_m >= 0 and a finite gamma > 0)", two_m, gamma);
  MELD_CHECK_ARG(prop != sub && prop != comm && prop != size,
                 "meld_leiden_propose: prop is sub, comm or size (a round reads what other rows would have written)");
  const long long* rp = reinterpret_cast<const long long*>(rowptr);
  const unsigned blocks = (unsigned)ceil_div(n, LR_THREADS / lanes);
  if (lanes == LR_SHORT) {
    leiden_propose_kernel<LR_SHORT><<<blocks, LR_THREADS, 0, S(stream)>>>(rp, col, val, n, comm, sub, k, tot, size, tot_comm, two_m, gamma,
                                                                         (unsigned)round, prop);
  } else {
    leiden_propose_kernel<LR_LONG><<<blocks, LR_THREADS, 0, S(stream)>>>(rp, col, val, n, comm, sub, k, tot, size, tot_comm, two_m, gamma,
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
  leiden_commit_kernel<<<(unsigned)blocks, LR_THREADS, 0, S(stream)>>>(sub, prop, size, n, new_sub, part_moved);
  MELD_LAUNCH_CHECK("leiden_commit_kernel");
  leiden_count_kernel<<<1, LR_THREADS, 0, S(stream)>>>(part_moved, blocks, reinterpret_cast<long long*>(movers));
  MELD_LAUNCH_CHECK("leiden_count_kernel");
  return MELD_OK;
}
