// csr_wave_stream.hpp -- the "lanes = columns" pass over a CSR matrix that cheby_step_wide_kernel (spmm.hip),
// diffuse_step_kernel<NC> (diffuse.hip) and minplus_step_kernel<NC> (geodesic.hip) share: for every row i and column c of a row-major
// fp64 block x,
//
//     acc = identity;   for e in row i, storage order:  acc = combine(acc, val[e], x[col[e], c]);   close_row(i, acc)
//
// The scheme.  A lane carries NC = 1 or 2 columns (lane and lane + 64: two 8-byte accesses, each coalesced across the wave -- no
// 16-byte vector access, so x and its leading dimension need 8-byte alignment only), which takes a block of up to 128 columns
// through ONE stream of the matrix.  A wave owns WAVE_STREAM_ROWS consecutive rows as ONE stream of entries [E0, E1): the (value,
// column) pairs are loaded a chunk of U = 16 / NC ahead by the first lanes and handed round with v_readlane (scalar address
// arithmetic, the value as a scalar operand of the combine), and the gathers of a chunk are in flight while the previous chunk is
// reduced, so the two dependent memory latencies of a chunk overlap with the previous chunk's work and no bubble opens at a row
// boundary.  For every entry the lanes read 8 p contiguous bytes of the neighbour's row (whole cache lines).  Row boundaries are
// loaded once, up front (lane r: row r).  Four waves per workgroup: 32 consecutive rows, and workgroups are XCD-contiguous, so the
// rows of x a neighbourhood shares are served by that XCD's L2.  No atomics, no LDS, plain vector loads and stores.
// Register budget: the gathers in flight are what the registers go to (2 chunks x U x NC x 2 VGPRs = 64 whatever NC: NC = 2 halves
// the chunk so that the same registers -- and the same bytes in flight per lane -- serve two columns); the rows' own operands come
// next.  NC = 1 compiles to 4 waves per SIMD for the diffusion and min-plus steps and to 3 for the wide recurrence step, which
// also holds a z row; NC = 2 to 3.  The figures are in each kernel's header and held by tests/test_geodesic_host.py.
//
// What a kernel supplies is an Op (a plain struct of its own):
//     void   load_rows(const wave_rows<NC>& w)   -- the per-row operands of the wave's rows, loaded once
//     double pad()                               -- the value an entry past E1 carries
//     double identity()                          -- the value of an empty accumulator
//     double combine(acc, v, xj)                 -- one entry; v is wave-uniform
//     void   close_row(r, row, acc, on, lane)    -- epilogue and store of row `row` (the wave's r-th, r uniform)
// and whatever state it wants to find after the pass.
#pragma once
#include "common.hpp"

namespace meld {

typedef double row_vec __attribute__((ext_vector_type(WAVE_STREAM_ROWS)));

// lane r's value of v, for a uniform r (a scalar operand)
__device__ __forceinline__ double wave_uniform(double v, int r) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), r), __builtin_amdgcn_readlane(__double2loint(v), r));
}

// where a lane stands: the wave's rows [row_first, row_first + n_here) and the lane's columns
template <int NC>
struct wave_rows {
  int lane, n_here;
  int64_t row_first, n_rows;
  bool on[NC];  // column lane + 64 c exists
  int lc[NC];   // ... and is read here (an idle lane re-reads column 0: inside the row, never stored)
  // the row whose per-row scalar this lane holds (lane r: row r; read back with wave_uniform)
  __device__ __forceinline__ int64_t lane_row() const { return min(row_first + min(lane, n_here - 1), n_rows - 1); }
};

// the wave's rows of a row-major block at the lane's columns: register vectors, read at the (uniform) index of the row that closes
// -- as arrays the allocator keeps them in private memory once the second column is there
template <int NC>
struct own_rows {
  row_vec v[NC];
  template <bool STREAMED = false>  // (read once: leave the L2 to the gathered rows)
  __device__ __forceinline__ void load(const double* base, int64_t ld, const wave_rows<NC>& w) {
#pragma unroll
    for (int r = 0; r < WAVE_STREAM_ROWS; ++r) {
      const int64_t row = min(w.row_first + r, w.n_rows - 1);
#pragma unroll
      for (int c = 0; c < NC; ++c) v[c][r] = STREAMED ? __builtin_nontemporal_load(base + row * ld + w.lc[c]) : base[row * ld + w.lc[c]];
    }
  }
};

template <int NC, class Op>
__device__ __forceinline__ void wave_stream_rows(const int64_t* __restrict__ rowptr, const int* __restrict__ col,
                                                 const double* __restrict__ val, int64_t n_rows, const double* __restrict__ x,
                                                 int64_t ldx, int p, Op& op) {
  static_assert(NC == 1 || NC == 2, "a lane carries one or two columns");
  static_assert(WAVE_STREAM_ROWS + 1 <= 64, "row pointers of a wave are held one per lane");
  constexpr int U = 16 / NC;  // entries per chunk = gathers in flight per lane and column
  wave_rows<NC> w;
  w.lane = threadIdx.x & 63;
  w.n_rows = n_rows;
  const int lane = w.lane, wv = threadIdx.x >> 6;
  const int nb = gridDim.x;  // (a multiple of 8, wave_stream_grid: the remap below is a bijection)
  const int per = (nb + 7) >> 3;
  const int64_t rb = (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (rb >= nb) return;
  const int64_t row_first = w.row_first = (rb * 4 + wv) * WAVE_STREAM_ROWS;
  if (row_first >= n_rows) return;  // (uniform)
  const int n_here = w.n_here = (int)min((int64_t)WAVE_STREAM_ROWS, n_rows - row_first);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    w.on[c] = lane + 64 * c < p;
    w.lc[c] = w.on[c] ? lane + 64 * c : 0;
  }
  const int64_t rp = rowptr[min(row_first + min(lane, n_here), n_rows)];
  op.load_rows(w);
  auto rp_at = [&](int r) __attribute__((always_inline)) {
    return (int64_t)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(rp >> 32), r) << 32) |
                     (unsigned)__builtin_amdgcn_readlane((int)rp, r));
  };
  const int64_t E0 = rp_at(0), E1 = rp_at(n_here);
  // pairs of the chunk that starts at entry e0 (lane u & (U - 1): entry e0 + u); beyond the wave's stream the value is the op's
  // padding and the column that of the last entry (row 0 where the wave has no entries at all): always a row of x
  auto fetch_pairs = [&](int64_t e0, double& vv, int& cc) __attribute__((always_inline)) {
    const int64_t e = min(e0 + (lane & (U - 1)), E1 - 1);
    vv = (e0 + (lane & (U - 1)) < E1) ? __builtin_nontemporal_load(val + max(e, (int64_t)0)) : op.pad();
    cc = E1 > E0 ? __builtin_nontemporal_load(col + max(e, (int64_t)0)) : 0;
  };
  auto gather = [&](int cc, double (&xj)[U][NC]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const double* xr = x + (int64_t)__builtin_amdgcn_readlane(cc, u) * ldx;
#pragma unroll
      for (int c = 0; c < NC; ++c) xj[u][c] = xr[w.lc[c]];
    }
  };
  int r_cur = 0;
  int64_t re_cur = rp_at(1);
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = op.identity();
  auto flush_rows_until = [&](int64_t e) __attribute__((always_inline)) {  // (uniform) close every row that ends at or before entry e
    while (r_cur < n_here && e >= re_cur) {
      op.close_row(r_cur, row_first + r_cur, acc, w.on, lane);
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] = op.identity();
      ++r_cur;
      re_cur = r_cur < n_here ? rp_at(r_cur + 1) : E1 + 1;  // (after the last row: no row is left to close)
    }
  };
  auto reduce_chunk = [&](int64_t e0, double vv, const double (&xj)[U][NC]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      flush_rows_until(e0 + u);
      const double v = wave_uniform(vv, u);
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] = op.combine(acc[c], v, xj[u][c]);
    }
  };
  double vA, vB;
  int cA, cB;
  double xA[U][NC], xB[U][NC];
  fetch_pairs(E0, vA, cA);
  fetch_pairs(E0 + U, vB, cB);
  gather(cA, xA);
  for (int64_t e0 = E0; e0 < E1; e0 += 2 * U) {
    // chunk A = [e0, e0 + U), chunk B = [e0 + U, e0 + 2 U); the pairs of the chunk after B and B's gathers go out before A is reduced
    gather(cB, xB);
    double vN;
    int cN;
    fetch_pairs(e0 + 2 * U, vN, cN);
    reduce_chunk(e0, vA, xA);
    gather(cN, xA);
    double vM;
    int cM;
    fetch_pairs(e0 + 3 * U, vM, cM);
    reduce_chunk(e0 + U, vB, xB);
    vA = vN;
    cA = cN;
    vB = vM;
    cB = cM;
  }
  // the rows that are left: the last one, and rows without entries.  (Entries past E1 carry the padding and are reduced after
  // every row has been closed at entry E1: they reach no output.)
  flush_rows_until(E1 + 1);
}

}  // namespace meld
