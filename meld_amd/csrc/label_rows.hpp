// label_rows.hpp -- the "every entry meets its whole row" pass that louvain_move_kernel<G> (louvain.hip) and
// leiden_propose_kernel<G> (leiden.hip) share: for a row of a CSR matrix whose entries carry a label (an id >= 0, or -1 for an
// entry that is no candidate) and a value,
//
//     w(l) = sum_{j : label_j = l} val_j     in storage order, for the label l of every entry;   score(l, w(l));   argmax over the row
//
// The scheme.  G = 16 or 64 lanes per row (a kNN row of 8 to 14 entries fills a 16-lane group: four rows per wave), 256 threads per
// workgroup.  The row is taken a CHUNK of 4 G entries at a time (four per lane, held in registers with their sums; whatever the
// kernel gathers by label is gathered once per held entry), and every chunk meets ALL entries of the row, which pass through LDS in
// TILES of 4 G (label, value): one broadcast read per four comparisons, sum += (label_j == label_i) ? v_j : 0 in storage order.  The
// tile that is the chunk the lanes hold is stored from their registers, not loaded again.  So every entry knows the whole weight
// of its label, whatever the row's length (a row longer than a tile takes several trips: the work is quadratic in the length),
// duplicates of a label agree, and the argmax over the lanes (a xor butterfly on (score, id)) needs no leader.  The groups of a wave
// have rows of their own lengths; a group's lanes share their control flow and their LDS rows and never leave their wave, so two
// wave-level fences order a tile's LDS traffic (no barrier: the kernels may leave rows early).  fp64, no atomics, plain vector
// loads and stores, no private memory (20 VGPRs per lane hold four labels, values and sums); every sum is a function of the row alone.
//
// What a kernel supplies is an Op (a plain struct of its own) with the row's first entry and length in `rs` and `len`, and
//     int  label(i)          -- the label of entry i of the row, -1 for padding (i >= len) and for an entry that is no candidate
//     void meet(lj, vj)      -- every entry of the row, once, in storage order (during the first chunk's trips): the row's own sums
//     bool go_on()           -- asked once, after the first chunk has met the row and before anything is scored; false: the row leaves
//     void score(l, w)       -- one held entry with the whole weight of its label (called for -1 too: the Op tests it)
// and whatever state it wants to find after the pass.
#pragma once
#include "common.hpp"

#include <limits.h>
#include <type_traits>

namespace meld {

constexpr int LR_THREADS = 256;
constexpr int LR_SHORT = 16;  // lanes per row where the rows are short
constexpr int LR_LONG = 64;   // lanes per row otherwise
constexpr int LR_U = 4;       // entries of the row a lane holds at a time: a trip through LDS serves G * LR_U of them

// the LDS of a workgroup: one tile per row group
template <int G>
struct label_tiles {
  int lab[LR_THREADS / G][G * LR_U];
  double val[LR_THREADS / G][G * LR_U];
};

// the running argmax: a larger score wins, among equal scores the lower id (INT_MAX: nothing yet)
struct label_best {
  double score;
  int id;
  __device__ __forceinline__ void offer(double s, int i) {
    if (s > score || (s == score && i < id)) {
      score = s;
      id = i;
    }
  }
  // the best of the row's G lanes, in all of them: a xor butterfly
  template <int G>
  __device__ __forceinline__ void over_lanes() {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) offer(__shfl_xor(score, off, 64), __shfl_xor(id, off, 64));
  }
};

// the pass over the row of the thread's group: entries [op.rs, op.rs + op.len) of val (uniform over the group's G lanes).  LOCAL: on
// a copy of the Op, handed back at the end -- the compiler then takes the Op's fields apart before this function is inlined and
// not after, and which way a kernel comes out shorter differs: the move kernel is built without, the propose kernel with it.
template <int G, bool LOCAL = false, class Op>
__device__ __forceinline__ void label_row_pass(label_tiles<G>& s, const double* __restrict__ val, Op& op_io) {
  typename std::conditional<LOCAL, Op, Op&>::type op = op_io;
  const long long rs = op.rs, len = op.len;
  static_assert(G == LR_SHORT || G == LR_LONG, "16 or 64 lanes per row: a group never spans waves");
  constexpr int TILE = G * LR_U;
  const int g = threadIdx.x / G;
  const int lane = threadIdx.x % G;
  for (long long i0 = 0; i0 < len; i0 += TILE) {
    int li[LR_U];
    double vi[LR_U], sum[LR_U];
#pragma unroll
    for (int u = 0; u < LR_U; ++u) {
      const long long i = i0 + lane + G * u;
      li[u] = op.label(i);
      vi[u] = i < len ? val[rs + i] : 0.0;
      sum[u] = 0.0;
    }
    const bool first = i0 == 0;
    for (long long j0 = 0; j0 < len; j0 += TILE) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // (one wave: the loads of the last trip precede these stores)
#pragma unroll
      for (int u = 0; u < LR_U; ++u) {
        if (j0 == i0) {  // (uniform over the group: the tile is the chunk its lanes hold)
          s.lab[g][lane + G * u] = li[u];
          s.val[g][lane + G * u] = vi[u];
        } else {
          const long long j = j0 + lane + G * u;
          s.lab[g][lane + G * u] = op.label(j);
          s.val[g][lane + G * u] = j < len ? val[rs + j] : 0.0;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // (one wave: its LDS stores precede its loads)
      const int jn = (int)min((long long)TILE, len - j0);
      for (int jj = 0; jj < jn; ++jj) {
        const int lj = s.lab[g][jj];  // (one address for the group: a broadcast)
        const double vj = s.val[g][jj];
#pragma unroll
        for (int u = 0; u < LR_U; ++u) sum[u] += (lj == li[u]) ? vj : 0.0;  // (x + 0 == x: the label's entries in storage order)
        if (first) op.meet(lj, vj);                                         // (the first chunk meets every entry of the row once)
      }
    }
    if (first && !op.go_on()) break;  // (uniform over the group; nothing has been scored)
#pragma unroll
    for (int u = 0; u < LR_U; ++u) op.score(li[u], sum[u]);
  }
  if (LOCAL) op_io = op;
}

}  // namespace meld
