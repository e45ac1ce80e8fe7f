// common.hpp -- shared helpers for libmeld_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/meld_hip.h"

namespace meld {

// thread-local last-error string, reported through meld_last_error()
char* err_buf();
void set_err(const char* fmt, ...);

static inline hipStream_t S(meld_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// wave = 64 lanes on CDNA4; hard-coded on purpose (cdna_hip_programming.md section 1)
constexpr int WAVE = 64;

#define MELD_CHECK_ARG(cond, ...)        \
  do {                                   \
    if (!(cond)) {                       \
      meld::set_err(__VA_ARGS__);        \
      return MELD_ERR_INVALID;           \
    }                                    \
  } while (0)

#define MELD_LAUNCH_CHECK(name)                                               \
  do {                                                                        \
    hipError_t e__ = hipGetLastError();                                       \
    if (e__ != hipSuccess) {                                                  \
      meld::set_err("%s: launch failed: %s", name, hipGetErrorString(e__));   \
      return MELD_ERR_HIP;                                                    \
    }                                                                         \
  } while (0)

#define MELD_HIP_CALL(expr)                                                   \
  do {                                                                        \
    hipError_t e__ = (expr);                                                  \
    if (e__ != hipSuccess) {                                                  \
      meld::set_err("%s failed: %s", #expr, hipGetErrorString(e__));          \
      return MELD_ERR_HIP;                                                    \
    }                                                                         \
  } while (0)

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The "lanes = columns" steps over the CSR arrays (csr_wave_stream.hpp): 8 consecutive rows per wave, 4 waves per workgroup, up to
// 2 columns per lane.
constexpr int WAVE_STREAM_ROWS = 8;
constexpr int WAVE_STREAM_MAX_COLS = 128;

// their grid: 32 rows per workgroup, rounded up to a multiple of 8 (the XCD remap of the kernels is then a bijection)
static inline unsigned wave_stream_grid(int64_t n_rows) { return (unsigned)(ceil_div(ceil_div(n_rows, 4 * WAVE_STREAM_ROWS), 8) * 8); }

// The argument contract of a panel step y = step(x) on row-major blocks with leading dimensions (meld_diffuse_step,
// meld_minplus_step); `entry` prefixes the message, `required` names the pointers `required_ok` stands for, `values` the array next
// to col, `pass` what a call is ("step", "round").  MELD_OK, or MELD_ERR_INVALID with the message set: nothing has been launched.
static inline int check_panel_step(const char* entry, bool required_ok, const char* required, const char* values, const char* pass,
                                   const void* col, const void* val, int64_t n_rows, const double* x, int64_t ldx, const double* y,
                                   int64_t ldy, int p) {
  MELD_CHECK_ARG(required_ok, "%s: %s are required", entry, required);
  MELD_CHECK_ARG(n_rows >= 0, "%s: n_rows=%lld is negative", entry, (long long)n_rows);
  MELD_CHECK_ARG(p >= 1 && p <= WAVE_STREAM_MAX_COLS, "%s: p=%d columns (1 <= p <= %d per call)", entry, p, WAVE_STREAM_MAX_COLS);
  MELD_CHECK_ARG(ldx >= p && ldy >= p, "%s: leading dimensions ldx=%lld, ldy=%lld below p=%d", entry, (long long)ldx, (long long)ldy, p);
  MELD_CHECK_ARG(n_rows == 0 || (col && val), "%s: col and %s are required for a matrix with rows", entry, values);
  const uintptr_t x0 = (uintptr_t)x, x1 = x0 + sizeof(double) * (uintptr_t)n_rows * (uintptr_t)ldx;
  const uintptr_t y0 = (uintptr_t)y, y1 = y0 + sizeof(double) * (uintptr_t)n_rows * (uintptr_t)ldy;
  MELD_CHECK_ARG(n_rows == 0 || x1 <= y0 || y1 <= x0, "%s: y overlaps x (a %s reads rows of x other rows have written)", entry, pass);
  return MELD_OK;
}

// slots of a row bucket of the symmetrisation (assemble.hip; refine.hip's emitting kernel writes into the buckets too)
constexpr int CSR_BUCKET = 256;

// Development switches of the library (A-B measurements, ablations, counters): read only under MELD_DEV=1, so that a stray
// variable in a production environment cannot change which kernels run (the same rule as meld_amd/_options.py on the host side)
static inline const char* meld_dev_getenv(const char* name) {
  const char* dev = getenv("MELD_DEV");
  return (dev && dev[0] == '1' && dev[1] == 0) ? getenv(name) : nullptr;
}

// Device-resident Lanczos on the tiled layout without a scalar kernel between the iterations: the SpMV of iteration k derives its
// own scalars from the partial sums the axpy of iteration k - 1 left (beta_{k-1} = sqrt(sum nrm2_prev), s_k = 1 / beta_{k-1},
// y = s_k L u_k - beta_{k-1} s_{k-1} u_{k-1}); block 0 records beta_{k-1} and s_k and clears the slots the next axpy adds into.
struct PtLanczos {
  const double* nrm2_prev;   // DOT_SLOTS partial sums of |w_{k-1}|^2 (k = 0: |u_0|^2 in slot 0)
  double* nrm2_zero;         // DOT_SLOTS slots to clear
  const double* state_prev;  // [0] = s_{k-1} (k = 0: 0)
  double* state_cur;         // [0] <- s_k
  double* betas;             // betas[it - 1] <- beta_{k-1} (it > 0)
  int it;
  const int* stop;  // (optional) nonzero when the launch starts: it does nothing (a stop request of the host's convergence check)
};

// the null-pointer checks of an operator record (include/meld_hip.h): rowptr and dw always, the arrays of the layout when it
// is set, col and val otherwise (a matrix without entries has none)
static inline bool laplacian_ok(const meld_laplacian_t* L) {
  if (!L || !L->rowptr || !L->dw) return false;
  if (const meld_pt_layout_t* t = L->layout)
    return t->blk_row && t->blk_ntile && t->blk_ndist && t->seg && t->list_cols && t->pval && t->pidx;
  return L->nnz == 0 || (L->col && L->val);
}

// one recurrence step on the panel-tiled layout (spmm_tiled.hip); coef_dev: device-resident Lanczos scalars
int pt_step(const meld_pt_layout_t* L, const int64_t* rowptr, const double* dw, int p, const double* x_full,
            int64_t x_row_offset, const double* z, double* y, double* r, double alpha, double beta, double gamma,
            double coef, double* dots, const double* coef_dev, hipStream_t st, double coef_x = 0.0, const PtLanczos* lz = nullptr);

}  // namespace meld
