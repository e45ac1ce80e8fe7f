// mds.hip -- one step of metric multidimensional scaling by SMACOF: the Guttman transform with unit weights and the stress of the
// configuration it starts from (the hot loop of PHATE's embedding, meld_amd/phate.py).
//
// Reference surface: [UPSTREAM phate 1.0.x ``phate.mds.embed_MDS``, unpinned: not importable next to this code]; its metric stage
// is sklearn's SMACOF (de Leeuw 1977), restated here from the textbook definition.  With D [n, n] the target distances, Z [n, dim]
// the configuration and d_ij = |Z[i] - Z[j]|_2 from direct differences:
//
//     Z'[i]         = (1 / n) sum_{j != i, d_ij > 0} (D[i, j] / d_ij) (Z[i] - Z[j])
//     row_stress[i] = sum_{j != i} (d_ij - D[i, j])^2                     stress(Z) = 1/2 sum_i row_stress[i]   (the caller's sum)
//
// Work.  D is the traffic (8 n^2 bytes, read once); Z is small (8 n dim bytes) and every row needs all of it.  A workgroup of four
// waves takes SM_ROWS = 8 consecutive rows, two per wave, and walks the columns in tiles of SM_TILE = 256 points: the tile of Z is
// staged in LDS once for the eight rows (component-major, so that a wave reads 64 consecutive doubles: no bank conflict), lane l of
// a wave takes the columns tile + l, + 64, + 128, + 192, reads each point from LDS once for both of its rows and its two elements
// of D straight from global memory (512 contiguous bytes per wave and instruction).  Z is then read n / 8 times from L2.
// Order of the sums: a lane adds its columns in ascending order into one partial sum per output, the 64 partial sums meet in a xor
// butterfly, one division by n follows.  No atomics, nothing shared between workgroups: every output is a function of the operands
// alone, the same bits every run.  sqrt and the two divisions are the correctly rounded ones (no fast-math in this file).
#include "common.hpp"

namespace meld {

constexpr int SM_MAX_DIM = 8;
constexpr int SM_TILE = 256;       // points of Z in LDS at a time: 2 KB per component, 16 KB at dim 8
constexpr int SM_WAVE_ROWS = 2;    // rows of a wave: a point read from LDS serves both
constexpr int SM_ROWS = 4 * SM_WAVE_ROWS;

template <int DIM>
__global__ __launch_bounds__(256) void smacof_step_kernel(const double* __restrict__ D, int64_t ldD, int n, const double* __restrict__ Z,
                                                          double* __restrict__ Z_out, double* __restrict__ row_stress) {
  __shared__ double s_z[DIM][SM_TILE];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int row0 = blockIdx.x * SM_ROWS + w * SM_WAVE_ROWS;
  int row[SM_WAVE_ROWS];
  const double* drow[SM_WAVE_ROWS];
  double zi[SM_WAVE_ROWS][DIM], acc[SM_WAVE_ROWS][DIM], stress[SM_WAVE_ROWS];
#pragma unroll
  for (int r = 0; r < SM_WAVE_ROWS; ++r) {
    row[r] = row0 + r;
    const int ri = min(row[r], n - 1);  // (a row past the end reads the last one and stores nothing: every wave meets the barriers)
    drow[r] = D + (int64_t)ri * ldD;
    stress[r] = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      zi[r][c] = Z[(int64_t)ri * DIM + c];  // (one address for the wave)
      acc[r][c] = 0.0;
    }
  }
  for (int t0 = 0; t0 < n; t0 += SM_TILE) {
    __syncthreads();  // (the last tile has been read)
    for (int e = threadIdx.x; e < SM_TILE * DIM; e += 256) {  // consecutive elements of Z: a coalesced read, a transposed store
      const int j = e / DIM, c = e - j * DIM;
      s_z[c][j] = t0 + j < n ? Z[(int64_t)(t0 + j) * DIM + c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < SM_TILE / 64; ++q) {
      const int jl = lane + 64 * q;
      const int j = t0 + jl;
      const bool in = j < n;
      double zj[DIM];
#pragma unroll
      for (int c = 0; c < DIM; ++c) zj[c] = s_z[c][jl];
#pragma unroll
      for (int r = 0; r < SM_WAVE_ROWS; ++r) {
        const double dij = in ? drow[r][j] : 0.0;
        double diff[DIM];
        double d2 = 0.0;
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
          diff[c] = zi[r][c] - zj[c];
          d2 = fma(diff[c], diff[c], d2);
        }
        const double d = sqrt(d2);
        const bool pair = in && j != row[r];
        const double ratio = (pair && d > 0.0) ? dij / d : 0.0;
        const double gap = pair ? d - dij : 0.0;
        stress[r] = fma(gap, gap, stress[r]);
#pragma unroll
        for (int c = 0; c < DIM; ++c) acc[r][c] = fma(ratio, diff[c], acc[r][c]);
      }
    }
  }
  const double dn = (double)n;
#pragma unroll
  for (int r = 0; r < SM_WAVE_ROWS; ++r) {
    const double st = wave_sum(stress[r]);
    double out[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) out[c] = wave_sum(acc[r][c]) / dn;
    if (row[r] < n && lane == 0) {
      row_stress[row[r]] = st;
#pragma unroll
      for (int c = 0; c < DIM; ++c) Z_out[(int64_t)row[r] * DIM + c] = out[c];
    }
  }
}

template <int DIM>
static void smacof_launch(const double* D, int64_t ldD, int n, const double* Z, double* Z_out, double* row_stress, hipStream_t st) {
  smacof_step_kernel<DIM><<<(unsigned)ceil_div(n, SM_ROWS), 256, 0, st>>>(D, ldD, n, Z, Z_out, row_stress);
}

}  // namespace meld

using namespace meld;

extern "C" int meld_smacof_max_dim(void) { return SM_MAX_DIM; }

extern "C" int meld_smacof_step(const double* D, int64_t ldD, int n, int dim, const double* Z, double* Z_out, double* row_stress,
                                meld_stream_t stream) {
  MELD_CHECK_ARG(D && Z && Z_out && row_stress, "meld_smacof_step: D, Z, Z_out and row_stress are required");
  MELD_CHECK_ARG(n >= 0, "meld_smacof_step: n=%d is negative", n);
  MELD_CHECK_ARG(dim >= 1 && dim <= SM_MAX_DIM, "meld_smacof_step: dim=%d (1 <= dim <= %d)", dim, SM_MAX_DIM);
  MELD_CHECK_ARG(ldD >= n, "meld_smacof_step: leading dimension ldD=%lld below n=%d", (long long)ldD, n);
  MELD_CHECK_ARG(Z != Z_out, "meld_smacof_step: Z_out is Z (a step reads rows of Z other rows have written)");
  if (n == 0) return MELD_OK;
  hipStream_t st = S(stream);
  switch (dim) {
    case 1: smacof_launch<1>(D, ldD, n, Z, Z_out, row_stress, st); break;
    case 2: smacof_launch<2>(D, ldD, n, Z, Z_out, row_stress, st); break;
    case 3: smacof_launch<3>(D, ldD, n, Z, Z_out, row_stress, st); break;
    case 4: smacof_launch<4>(D, ldD, n, Z, Z_out, row_stress, st); break;
    case 5: smacof_launch<5>(D, ldD, n, Z, Z_out, row_stress, st); break;
    case 6: smacof_launch<6>(D, ldD, n, Z, Z_out, row_stress, st); break;
    case 7: smacof_launch<7>(D, ldD, n, Z, Z_out, row_stress, st); break;
    default: smacof_launch<8>(D, ldD, n, Z, Z_out, row_stress, st); break;
  }
  MELD_LAUNCH_CHECK("smacof_step_kernel");
  return MELD_OK;
}
