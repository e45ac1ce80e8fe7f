/* meld_hip.h -- C-ABI of libmeld_hip.so: the MI355X (gfx950) hot path of MELD.fit_transform.
 *
 * The reference (KrishnaswamyLab/MELD v1.0.2) is pure Python and has no FFI; its hot path is the
 * arithmetic that graphtools and pygsp perform under
 *     meld/meld.py:273   self.fit(X)            -> graphtools.Graph(...)   (kNN + alpha-decay kernel)
 *     meld/meld.py:235   filter.filter(...)     -> meld/filter.py:39,56,59 (lmax + Chebyshev filter)
 * Each entry point below names the reference interface (file:line, or the [UPSTREAM] library
 * routine called from that line) whose work it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on that stream;
 *   - no hidden allocation, no global state besides the last-error string (thread local);
 *   - return value: 0 = ok, <0 = error (MELD_ERR_*), message via meld_last_error();
 *   - N, nnz counts are int64_t; column indices int32 (N < 2^31); values are IEEE fp64 wherever
 *     the reference computes in fp64.  fp32 appears only in the candidate search, whose result
 *     is re-evaluated exactly in fp64 before it is used.
 */
#ifndef MELD_HIP_H
#define MELD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MELD_OK 0
#define MELD_ERR_INVALID (-1)     /* bad argument */
#define MELD_ERR_UNSUPPORTED (-2) /* size outside what the kernels are instantiated for */
#define MELD_ERR_HIP (-3)         /* a HIP runtime call failed */

typedef void* meld_stream_t;

/* ---- library info ------------------------------------------------------------------------- */
int meld_abi_version(void);
const char* meld_last_error(void);
/* hipGetDeviceCount-style probe: number of visible devices, or <0 */
int meld_device_count(void);

/* ---- kNN candidate search (replaces [UPSTREAM graphtools kNNGraph.build_kernel_to_data ->
 *      sklearn NearestNeighbors.kneighbors], reached from meld/meld.py:273) ------------------ */

/* Geometry of the search kernel, so that the caller can size its buffers. */
int meld_knn_padded_dim(int d);     /* KP: augmented (d+2) dimension rounded up to an instantiated size; <0 if d unsupported */
int meld_knn_tile_refs(void);       /* TS: reference points per LDS tile (reference array is padded to a multiple) */
int meld_knn_block_queries(void);   /* BQ: queries per workgroup (query arrays are padded to a multiple) */
int meld_knn_row_capacity(int ksel);/* CAP: row stride of the candidate buffers for a given ksel; <0 if unsupported */
double meld_knn_error_coef(int d);  /* fp32 FMA-chain bound KP * 2^-21 of meld_knn_topk */

/* column sums of X[N,d] (fp64) -> sums[d] (zeroed by the call).  Used for centring. */
int meld_col_sums_f64(const double* X, int64_t N, int d, double* sums, meld_stream_t stream);
/* column sums, minima and maxima of X[N,d] in ONE pass (fixed-order reduction: reproducible bits): the centring mean, the
 * front end's NaN / infinity check (graphtools rejects such input before building, reached from meld/meld.py:273) and the
 * extremes meld_knn16_prepare_scaled derives the operand scale from.  temp: meld_col_stats_temp_bytes(d) bytes. */
size_t meld_col_stats_temp_bytes(int d);
int meld_col_stats_f64(const double* X, int64_t N, int d, double* sums, double* mins, double* maxs, void* temp, size_t temp_bytes,
                       meld_stream_t stream);

/* Build the fp32 operands of the distance GEMM from fp64 data (centred by `mean[d]`):
 *   refs:    tile-major augmented reference form  Rt[n_tiles][KP/2][TS][2]  of  [-2x, 1, |x|^2, 0..]
 *            rows >= N are filled so that their distance is huge; norm2[N] = |x|^2 (fp32),
 *            norm2_max[1] = max_i norm2[i] (atomic max; must be zeroed by the caller);
 *   queries: row-major augmented query form  Q[q_pad][KP]  of  [x, |x|^2, 1, 0..]  for rows
 *            q_begin .. q_begin+q_count (rows beyond q_count replicate the last valid row). */
int meld_knn_prepare_refs(const double* X, int64_t N, int d, const double* mean, int KP, float* Rt,
                          float* norm2, float* norm2_max, meld_stream_t stream);
int meld_knn_prepare_queries(const double* X, int64_t N, int d, const double* mean, int KP,
                             int64_t q_begin, int64_t q_count, float* Q, meld_stream_t stream);

/* Brute-force search on the matrix cores: for each of the q_count queries in Q, the ksel
 * references with the smallest fp32 squared distance (self included).  Output rows have stride
 * CAP = meld_knn_row_capacity(ksel); the first min(cand_cnt, ksel) entries of a row are valid and
 * sorted by (d2, idx) ascending.  Buffers must hold q_pad = roundup(q_count, BQ) rows. */
int meld_knn_topk(const float* Q, const float* Rt, int64_t n_ref, int KP, int64_t q_count, int ksel,
                  int32_t* cand_idx, float* cand_d2, int32_t* cand_cnt, meld_stream_t stream);

/* ---- second-generation search: split-fp16 operands on v_mfma_f32_32x32x16_f16 (knn16.hip).
 * Same role and output contract as meld_knn_topk (ksel smallest approximate squared distances,
 * rows of stride CAP sorted by (d2, idx), d2 in input units); ~4x less matrix-pipe time.
 *   meld_knn16_prepare: centre by mean[d], scale into [-1,1], split hi/lo (d2 = |q|^2 + |r|^2 - 2 q.r:
 *       |r|^2 - 2 q.r runs on the matrix cores -- |r|^2 as three exact fp16 pieces in K slots d .. d+2
 *       against 1.0 on the query side -- and |q|^2 is folded into the selection threshold):
 *       Rt16  : ceil(N / TS) * meld_knn16_tile_bytes(d)   (per tile: [kb][half][plane][ref][8 x fp16]
 *               of [-2 x, |x|^2 pieces])
 *       Q16   : roundup(q_count, BQ) * meld_knn16_query_bytes(d);  Qn : roundup(q_count, BQ) fp32 norms
 *       norm2[N], norm2_max[1] (input units), scale_info[4] floats (s, 1/s^2, absmax, pad)
 *   meld_knn16_error_coef: E / max|x~|^2 to pass to meld_knn_refine for this search. */
int meld_knn16_kblocks(int d);           /* KB = ceil((d+3)/16); <0 if d unsupported (d <= 141) */
int meld_knn16_tile_refs(void);          /* TS */
/* SPLIT operand layout (wherever d > 13 and d + 6 K slots fit the K blocks of d + 3): K block 0 holds the first
 * meld_knn16_split_dims(d) = 13 coordinates and the pieces of |r_A|^2 (less a margin that the second set of pieces,
 * behind the other coordinates, gives back), so that the list-driven first pass (meld_knn16_topk_listed) can test a block of 32
 * references on its accumulators behind K block 0 -- a distance over some of the coordinates never exceeds the distance -- and
 * skip the other K blocks where no partial value is within reach of its row.  Results are the same in any orthonormal frame;
 * the test prunes when the leading coordinates carry the distances (the Python host rotates the cells to principal
 * coordinates for the search; PCA-reduced input, the reference's default, already is such a frame).  0: plain layout.
 * The layout is a function of d alone (no process-wide switch). */
int meld_knn16_split_dims(int d);
/* The cells' principal frame for that search (frame.hip; no reference counterpart -- graphtools searches the data as given):
 *   meld_cov_sample_f64:  cov[d*d] (row-major, upper triangle; zeroed by the caller) += the scatter matrix about mean[d] of
 *                         the rows 0, stride, 2 stride, ... of X[N][d]
 *   meld_rotate_rows_f64: out[N][d] = (X - mean) A^T, At[d][meld_frame_max_dims()] = the new axes as rows, zero-padded; out != X
 * d <= meld_frame_max_dims().  The eigenvectors are the caller's business (a d x d problem: host LAPACK). */
int meld_frame_max_dims(void);
int meld_cov_sample_f64(const double* X, int64_t N, int d, const double* mean, int64_t stride, double* cov, meld_stream_t stream);
int meld_rotate_rows_f64(const double* X, int64_t N, int d, const double* mean, const double* At, double* out, meld_stream_t stream);
int meld_knn16_block_queries(void);      /* BQ */
int meld_knn16_row_capacity(int ksel);   /* CAP */
double meld_knn16_error_coef(int nprod, int d);       /* worst case: E <= coef * max|x~|^2 (depends on the dimension:
                                                        the accumulators sum nprod * d + 3 terms) */
double meld_knn16_error_coef_const(int nprod, int d); /* per-row form: E_i = c_const max|x~|^2 + c_lin |x~_i| max|x~| */
double meld_knn16_error_coef_lin(int nprod);
size_t meld_knn16_tile_bytes(int d);     /* bytes of one reference tile (KB * 4096) */
size_t meld_knn16_query_bytes(int d);    /* bytes of one query row of Q16 */
int meld_knn16_prepare(const double* X, int64_t N, int d, const double* mean, int64_t q_begin,
                       int64_t q_count, void* Rt16, void* Q16, float* Qn, float* norm2, float* norm2_max,
                       float* scale_info, meld_stream_t stream);
/* meld_knn16_prepare with the operand scale (max |x - mean| over all entries) taken from the columns' extremes
 * (meld_col_stats_f64) instead of a pass of its own over X; bit-identical operands. */
int meld_knn16_prepare_scaled(const double* X, int64_t N, int d, const double* mean, const double* col_min, const double* col_max,
                              int64_t q_begin, int64_t q_count, void* Rt16, void* Q16, float* Qn, float* norm2, float* norm2_max,
                              float* scale_info, meld_stream_t stream);
/* Queries = all N references (q_begin = 0, q_count = N: every single-GPU build): the operands of meld_knn16_prepare_scaled (of
 * meld_knn16_prepare where col_min and col_max are both NULL) AND the tile spheres of meld_knn16_tile_spheres over all tiles, in
 * temp (meld_knn16_bounds_temp_bytes bytes, zeroed inside), from ONE pass over X: every 64-row tile is read once and written in
 * both layouts, its sphere computed from the same copy in LDS.  Bit-identical to the separate calls.  Afterwards
 * meld_knn16_step_lists_direct_spheres / meld_knn16_bounds_from_spheres take the spheres from temp. */
int meld_knn16_prepare_fused(const double* X, int64_t N, int d, const double* mean, const double* col_min, const double* col_max,
                             void* Rt16, void* Q16, float* Qn, float* norm2, float* norm2_max, float* scale_info, void* temp,
                             meld_stream_t stream);
/* Optional exact pruning.  meld_knn16_bounds fills lb2[n_query_waves][n_tiles] (fp16, rounded towards
 * zero) with a lower bound (scaled space) on the squared distance between any query of a wave of the
 * search kernel (64 consecutive cells = one reference tile) and any reference of a tile (TS consecutive
 * cells): (min over the wave's cells of the distance to the tile centroid - tile radius)^2, the minimum
 * taken point by point by a cells x centroids distance GEMM on the MFMA path (Rt16 = the reference
 * operand of meld_knn16_prepare).  In meld_knn16_topk a wave sits out every tile whose bound exceeds all
 * of its thresholds plus the search-error allowance, and a tile no wave of the workgroup needs is not
 * even loaded -- neither can change the result.  It pays when consecutive cells are spatially close
 * (meld_assign_nearest ordering).  lb2 = NULL disables pruning.  q_begin (a multiple of TS) = global
 * index of query 0 (the scan of every workgroup starts at its own position among the references and
 * wraps around).
 * thr_seed (optional, q_count floats, scaled units) = the thr_init the search of the same queries will be
 * started with (meld_knn16_seed_thresholds_mfma), nprod = that search's products: thresholds only fall, so a tile
 * that no query of the wave can reach from its OWN start threshold (|p - c_t| - rho_t > sqrt(seed_p + E) for
 * all 64 cells p) is marked +inf in the table.  The table is then valid only for a search started from
 * exactly these thresholds (or lower ones).
 * No reference counterpart: graphtools delegates the search to sklearn's trees. */
size_t meld_knn16_bounds_bytes(int64_t n_ref, int64_t q_count);
size_t meld_knn16_bounds_temp_bytes(int64_t n_ref, int d, int64_t q_count);
int meld_knn16_bounds(const double* X, int64_t N, int d, const double* mean, const float* scale_info,
                      const float* norm2_max, const void* Rt16, int64_t q_begin, int64_t q_count,
                      const float* thr_seed, const float* q_norm2 /* optional: Qn of meld_knn16_prepare, per-row allowance */,
                      int nprod, void* temp, void* lb2, meld_stream_t stream);
/* The same in two calls, for a row-sharded build: every rank computes the spheres of a range of tiles into its slots of a zeroed
 * temp (three arrays, meld_knn16_sphere_layout: [rows][row_bytes] centres, [rows] fp32 |c|^2, [rows] fp32 radii), the ranks
 * all-gather them, and the table is built from the complete arrays. */
int meld_knn16_tile_spheres(const double* X, int64_t N, int d, const double* mean, const float* scale_info, void* temp,
                            int64_t tile_begin, int64_t tile_count, meld_stream_t stream);
int meld_knn16_sphere_layout(int64_t n_ref, int d, int64_t* rows, int64_t* row_bytes);
int meld_knn16_bounds_from_spheres(const double* X, int64_t N, int d, const double* mean, const float* scale_info,
                      const float* norm2_max, const void* Rt16, int64_t q_begin, int64_t q_count,
                      const float* thr_seed, const float* q_norm2 /* optional: Qn of meld_knn16_prepare, per-row allowance */,
                      int nprod, void* temp, void* lb2, meld_stream_t stream);
/* nprod selects the precision of the products: 3 = hi.hi + hi.lo + lo.hi (error bound
 * 2^-14 max|x~|^2), 1 = hi.hi only (a third of the MFMAs, bound 2^-9 |x~_q| max|x~|; rows the looser
 * bound cannot certify are searched again / go through meld_knn_radius_exact, so results are
 * identical).  The norm pieces live in the hi plane and are exact in either mode. */
/* meld_knn16_prepare for a search between two point sets (the blocks between two samples of graphtools' MNN kernel,
 * reached through reference meld/meld.py:117-118 with sample_idx=, test/test_meld.py:34): X holds n_total rows, the
 * references are rows [0, n_refs), the queries a range of the rest.  Scaling (and mean) over all n_total rows.  Outputs and
 * their units:
 *   Rt16, Q16     the operands of meld_knn16_prepare: centred coordinates times scale_info[0], fp16 hi / lo planes (scaled units);
 *   Qn            [roundup(q_count, BQ)] the queries' |x~|^2 in the search's SCALED units (input units * scale_info[0]^2);
 *   norm2         [n_total] |x - mean|^2 in INPUT units: rows [0, n_refs) for the references and rows [q_begin, q_begin + q_count)
 *                 for the queries (norm2[q_begin + i] * scale_info[0]^2 == Qn[i]); rows of neither range are not written;
 *   norm2_max     [1] the maximum of those norms over the references AND the queries, input units;
 *   scale_info    [4] {s = 1 / absmax, 1 / s^2, absmax = max |x - mean| over all entries of the n_total rows (input units), 0}.
 * meld_knn_refine, the radius cut of meld_knn16_topk and meld_knn16_research_thresholds read norm2 / norm2_max as input-unit
 * quantities for queries and references alike (tests/test_gpu_cross_search.py pins this). */
int meld_knn16_prepare_cross(const double* X, int64_t n_refs, int64_t n_total, int d, const double* mean, int64_t q_begin,
                             int64_t q_count, void* Rt16, void* Q16, float* Qn, float* norm2, float* norm2_max,
                             float* scale_info, meld_stream_t stream);
/* query operands for a list of local rows (rows[i] + q_begin = global index): the re-search of the
 * rows a reduced-precision first pass could not certify */
int meld_knn16_prepare_rows(const double* X, int64_t N, int d, const double* mean, const float* scale_info,
                            int64_t q_begin, const int32_t* rows, int64_t n_rows, void* Q16, float* Qn,
                            meld_stream_t stream);
/* Start thresholds (scaled units, thr[roundup(n_rows, BQ)]) for the re-search of those rows through
 * meld_knn16_topk(thr_init = thr): a first pass that found ksel references with approximate d2 <= tau bounds the re-search's
 * ksel-th distance by tau + E1 + E3 (both passes' error allowances); rows with a shorter first list start at +inf.
 * cand_cnt / cand_d2 (stride cap): the first pass's lists; err_coef / err_lin: its coefficients, err3: meld_knn16_error_coef(3, d). */
int meld_knn16_research_thresholds(const int32_t* rows, int64_t n_rows, int64_t q_begin, const int32_t* cand_cnt,
                                   const float* cand_d2, int cap, int ksel, const float* norm2, const float* norm2_max,
                                   double err_coef, double err_lin, double err3, const float* scale_info, float* thr,
                                   meld_stream_t stream);
/* thr_init (optional, roundup(q_count, BQ) floats in the SCALED units of the search, i.e. input
 * d2 * scale_info[0]^2): per query, a bound below which all wanted neighbours are known to lie; the
 * selection thresholds start there instead of at +inf (the re-search passes the first pass's
 * ksel-th distance plus both error allowances).  NULL = +inf.
 * n_slices > 1 (small query sets): the references are cut into n_slices ranges, each scanned by its
 * own workgroups into its own candidate rows (buffers of n_slices * roundup(q_count, BQ) rows);
 * meld_knn16_merge_slices then writes the ksel smallest of the union to the final rows. */
/* Start values for the thresholds of meld_knn16_topk's first pass (thr_init, scaled units, roundup(q_count, BQ)
 * floats) from the fp16 operands of meld_knn16_prepare, computed on the matrix pipe: the (knn+1)-th smallest distance of
 * a query among the cells of its block's own tiles and side_tiles on either side in index order (side_tiles <= 0:
 * n_ref / 12500, between 8 and 64 -- the cost grows with N, what tighter seeds save in the search and through
 * meld_knn16_bounds' per-query test with N^2) bounds its bandwidth from above, so nothing beyond radius_factor^2 times
 * that (plus the error allowance) can be wanted.  Spares the scan the wholesale appends of its first tiles.  q_begin
 * must be a multiple of BQ; knn + 1 > 64: every row +inf.  No reference counterpart. */
int meld_knn16_seed_thresholds_mfma(const void* Q16, const float* Qn, const void* Rt16, const float* scale_info,
                                    const float* norm2_max, int64_t n_ref, int d, int64_t q_begin, int64_t q_count,
                                    int knn, double radius_factor, int nprod, int side_tiles, float* thr_init,
                                    meld_stream_t stream);
int meld_knn16_topk(const void* Q16, const float* Qn, const void* Rt16, const float* scale_info,
                    int64_t n_ref, int d, int64_t q_count, int ksel, int nprod, int n_slices, const void* lb2,
                    const float* norm2_max, int64_t q_begin, const float* thr_init, int knn, double radius_factor,
                    int32_t* cand_idx, float* cand_d2, int32_t* cand_cnt, float* cand_thr,
                    uint64_t* tiles_done /* += (wave, tile) pairs actually computed, or NULL */,
                    const int32_t* block_order /* workgroup b searches query block block_order[b]; NULL = b */,
                    meld_stream_t stream);
/* Dispatch order of the pruned search.  Workgroups start in index order as slots free up, and with pruning the tiles a
 * query block has to stage differ by an order of magnitude; meld_knn16_block_work writes, per query block, the number of
 * tiles its four waves cannot rule out at their start thresholds (lb2 from meld_knn16_bounds, thr_seed = the thr_init of
 * the search, NULL = +inf).  Passing the blocks by decreasing work as block_order starts the longest first
 * (1M cells: the last slot finishes 4 % after the mean instead of 12 %).  The result does not depend on the order. */
int meld_knn16_block_work(const void* lb2, const float* thr_seed, int64_t n_ref, int d, int64_t q_count, int nprod,
                          const float* norm2_max, const float* scale_info, int32_t* work, meld_stream_t stream);
/* Step lists of the first pass (replaces the per-step use of the pruning table inside the search; graphtools
 * build_kernel_to_data's kNN query reached from /root/reference/meld/meld.py:273 has no counterpart -- this is how the
 * brute-force scan is cut down).  With start thresholds from meld_knn16_seed_thresholds_mfma the tiles a query block can rule out
 * are known before the search (what the falling thresholds add is 1.5 % of the blocks at 1M cells), so they are written
 * down once: list[b * list_stride + i] = tile | (bit w set: wave w of block b cannot rule the tile out) << 24 for the
 * i-th step of block b in scan order, cnt[b] = its steps (>= 1), which is also the block's work for block_order.
 * list_stride >= ceil(n_ref / 64); q_begin as for meld_knn16_topk (it fixes where a block's scan starts).
 * meld_knn16_topk_listed is meld_knn16_topk(nprod = 1) walking those lists: same candidate rows, counts,
 * thresholds (the lists are a superset of the tiles the table-driven kernel visits; the extra ones hold no candidate). */
int meld_knn16_step_lists(const void* lb2, const float* thr_seed, int64_t n_ref, int d, int64_t q_count, int nprod,
                          const float* norm2_max, const float* scale_info, int64_t q_begin, uint32_t* list,
                          int64_t list_stride, int32_t* cnt, meld_stream_t stream);
/* The same lists straight from the cells when the queries are all the cells (one GPU): tile spheres, bounds, symmetrisation and list
 * building in one call, with the bounds kept as two bits per (wave, tile) instead of the fp16 table (lb2 is never written).
 * temp: meld_knn16_bounds_temp_bytes(n_ref, d, n_ref) bytes; scratch: meld_knn16_list_scratch_bytes(n_ref) bytes;
 * thr_seed / q_norm2: the start thresholds and |q|^2 of the search (both required). */
size_t meld_knn16_list_scratch_bytes(int64_t n_ref);
int meld_knn16_step_lists_direct(const double* X, int64_t N, int d, const double* mean, const float* scale_info, const float* norm2_max,
                                 const void* Rt16, const float* thr_seed, const float* q_norm2, int nprod, void* temp, void* scratch,
                                 uint32_t* list, int64_t list_stride, int32_t* cnt, meld_stream_t stream);
/* ... with the bounds taken from the first K block of the operands alone (lead_only != 0; SPLIT layout, cells in a frame whose
 * leading coordinates carry the distances -- see meld_knn16_split_dims): lower bounds all the same, a quarter of the tile stream. */
int meld_knn16_step_lists_direct_lead(const double* X, int64_t N, int d, const double* mean, const float* scale_info, const float* norm2_max,
                                 const void* Rt16, const float* thr_seed, const float* q_norm2, int nprod, void* temp, void* scratch,
                                 uint32_t* list, int64_t list_stride, int32_t* cnt, int lead_only, meld_stream_t stream);
/* meld_knn16_step_lists_direct_lead with the tile spheres already in temp (meld_knn16_prepare_fused): X and mean are not read. */
int meld_knn16_step_lists_direct_spheres(const double* X, int64_t N, int d, const double* mean, const float* scale_info, const float* norm2_max,
                                 const void* Rt16, const float* thr_seed, const float* q_norm2, int nprod, void* temp, void* scratch,
                                 uint32_t* list, int64_t list_stride, int32_t* cnt, int lead_only, meld_stream_t stream);
int meld_knn16_topk_listed(const void* Q16, const float* Qn, const void* Rt16, const float* scale_info, int64_t n_ref, int d,
                           int64_t q_count, int ksel, const uint32_t* step_list, const int32_t* step_cnt, int64_t list_stride,
                           const float* norm2_max, int64_t q_begin, const float* thr_init, int knn, double radius_factor,
                           int32_t* cand_idx, float* cand_d2, int32_t* cand_cnt, float* cand_thr, uint64_t* tiles_done,
                           const int32_t* block_order, int n_slices /* as meld_knn16_topk: slice y walks the entries y, y + S, ... of a
                           block's list into its own candidate rows; merge with meld_knn16_merge_slices */, meld_stream_t stream);
/* ... with the partial test of the SPLIT layout: partial_test != 0 lets the pass drop a block of 32 references behind its first K
 * block when no partial value is within reach of its row (same rows, counts and thresholds; see meld_knn16_split_dims).
 * tiles_done (optional) holds TWO counters here: [0] (wave, tile) pairs computed, [1] blocks of 32 references that went on. */
int meld_knn16_topk_listed_partial(const void* Q16, const float* Qn, const void* Rt16, const float* scale_info, int64_t n_ref,
                                   int d, int64_t q_count, int ksel, const uint32_t* step_list, const int32_t* step_cnt,
                                   int64_t list_stride, const float* norm2_max, int64_t q_begin, const float* thr_init, int knn,
                                   double radius_factor, int32_t* cand_idx, float* cand_d2, int32_t* cand_cnt, float* cand_thr,
                                   uint64_t* tiles_done, const int32_t* block_order, int n_slices, int partial_test,
                                   meld_stream_t stream);
/* meld_knn16_topk_listed_partial with one slice that leaves the rows RAW: two half-rows [0, cap / 2) and [cap / 2, cap) of n0 and n1
 * unsorted entries, values v = d2 - |q|^2 in scaled units, cand_cnt[q] = n0 | n1 << 16.  meld_knn_refine_sort_emit takes them as they
 * are; meld_knn16_finish_rows turns them, in place, into what every other search entry point returns: the ksel smallest sorted by
 * (d2, index), d2 = (v + Qn[row]) * scale_info[1] in input units, cand_cnt[row] = min(n0 + n1, ksel). */
int meld_knn16_topk_listed_raw(const void* Q16, const float* Qn, const void* Rt16, const float* scale_info, int64_t n_ref, int d,
                               int64_t q_count, int ksel, const uint32_t* step_list, const int32_t* step_cnt, int64_t list_stride,
                               const float* norm2_max, int64_t q_begin, const float* thr_init, int knn, double radius_factor,
                               int32_t* cand_idx, float* cand_d2, int32_t* cand_cnt, float* cand_thr, uint64_t* tiles_done,
                               const int32_t* block_order, int partial_test, meld_stream_t stream);
int meld_knn16_finish_rows(float* cand_d2, int32_t* cand_idx, int32_t* cand_cnt, const float* Qn, const float* scale_info, int64_t n_rows,
                           int ksel, meld_stream_t stream);
/* The partial test as a pass of its own over the step lists (round 6; the default route in the principal frame): every listed
 * (wave, tile) pair is tested on K block 0 alone against the row's START threshold (thr_init, scaled units: the seeds the lists
 * were built for) and loses its bit when no partial distance is within reach; step_list is rewritten in place, emptied entries
 * dropped, cnt_out[block] = the new length (may alias step_cnt), tested (optional) += pairs tested.  meld_knn16_topk_listed over
 * the thinned lists returns the rows the search over the full ones would (no reference counterpart: graphtools searches a tree).
 * list_stride is at least the number of tiles of Rt16, as every list builder requires (a list holds a tile at most once), so it
 * bounds the tile numbers: where list_stride tiles are shorter than 4 GiB the kernel addresses all of them through one buffer
 * descriptor, otherwise through one per staged piece. */
int meld_knn16_partial_filter(const void* Q16, const float* Qn, const void* Rt16, const float* scale_info, const float* norm2_max, int d,
                              int64_t q_count, const float* thr_init, uint32_t* step_list, const int32_t* step_cnt, int64_t list_stride,
                              int32_t* cnt_out, uint64_t* tested, const int32_t* block_order /* optional: workgroup g takes block
                              block_order[g] */, meld_stream_t stream);
/* Radius cut (cand_thr != NULL; knn and radius_factor = (-ln thresh)^(1/decay) of the kernel that will be
 * built from the lists): once a row holds knn + 1 entries, its bandwidth^2 is at most A + E (A = its
 * (knn+1)-th smallest approximate d2, E = the row's search-error allowance), so nothing with approximate d2
 * above R = radius_factor^2 (A + E) + E can lie inside the kernel radius: the row's threshold drops to R, the
 * list stays short (far fewer appends and compactions, tighter pruning) and cand_thr[q] (input units,
 * roundup(q_count, BQ) floats) publishes the final threshold -- the list holds every reference below it --
 * for meld_knn_refine's completeness test.  The graph is the same with or without the cut. */
/* workgroups of meld_knn16_topk resident on the device at once (occupancy x CUs); the host hands a
 * nearly empty last wave of workgroups to a sliced launch instead of letting it run alone */
int meld_knn16_resident_blocks(int d, int nprod);
int meld_knn16_max_slices(int ksel); /* largest n_slices meld_knn16_merge_slices accepts */
int meld_knn16_merge_slices(const int32_t* s_idx, const float* s_d2, const int32_t* s_cnt, int64_t q_count,
                            int ksel, int n_slices, int32_t* out_idx, float* out_d2, int32_t* out_cnt,
                            meld_stream_t stream);

/* ---- exact re-evaluation + alpha-decay kernel (replaces [UPSTREAM graphtools
 *      kNNGraph.build_kernel_to_data, "affinities" block]) ---------------------------------- */

/* For each query row: exact fp64 distances to its candidates, bandwidth bw = (knn+1)-th smallest
 * (self counted), kernel value v = exp(-(d/bw)^decay), kept iff v >= thresh.  A row whose candidate
 * list cannot be proven to contain every reference with v >= thresh ("completeness")
 * is appended to flag_rows (its keep_cnt is set to 0) and must go through meld_knn_radius_exact.
 *   cand_val[q_count][ksel] : kernel value or 0
 *   keep_cnt[q_count]       : number of kept OFF-DIAGONAL entries (0 for flagged rows)
 *   err_coef, err_coef_lin  : search-error allowance of the kernel that produced the candidates,
 *                             E_i = err_coef * norm2_max + err_coef_lin * sqrt(norm2[i] * norm2_max)
 *                             (meld_knn_error_coef(d) / 0 for meld_knn_topk; meld_knn16_error_coef_const /
 *                             _lin for meld_knn16_topk, or the worst case meld_knn16_error_coef with norm2 = NULL)
 *   n_flag[1]               : atomic counter, zeroed by the caller
 *   rows (optional)         : second-stage form -- candidate row q belongs to local row rows[q]:
 *                             bw / cand_val / keep_cnt are written at that row, the candidate indices
 *                             are copied to cand_idx_out (row stride out_cap) and flag_rows receives
 *                             the local row.  NULL = row q is local row q. */
int meld_knn_refine(const double* X, int64_t N, int d, int64_t q_begin, int64_t q_count,
                    const int32_t* cand_idx, const float* cand_d2, const int32_t* cand_cnt,
                    const float* cand_thr /* [q_count] thresholds published by meld_knn16_topk's radius cut, or NULL */,
                    int ksel, int cap /* row stride of the candidate buffers */, int knn, double decay, double thresh,
                    const float* norm2_max, double err_coef,
                    const float* norm2 /* [N] per-row |x~|^2 or NULL */, double err_coef_lin, double* bw,
                    double* cand_val, int32_t* keep_cnt, int32_t* flag_rows, int32_t* n_flag,
                    const int32_t* rows, int out_cap, int32_t* cand_idx_out,
                    double bw_scale /* graphtools' bandwidth_scale: the kernel uses max(bw * bw_scale, eps); bw[] records the unscaled value */,
                    const double* bw_fixed /* [N] graphtools' bandwidth= (a given bandwidth per cell, knn then only sizes the search), or NULL */,
                    int max_rank /* graphtools' knn_max + 1 (self counted): a row keeps its max_rank nearest cells at most; 0 = no limit */,
                    meld_stream_t stream);

/* meld_knn_refine for ALL rows of a single-GPU build (q_begin = 0, q_count = N, no row list; even d <= 256), with the emit fused in:
 * the kept entries of every complete row go straight into the row buckets of the symmetrisation (what meld_coo_emit_scatter would
 * do with cand_val, which is not written) -- the row's own (idx, v / 2) pairs behind ONE atomic claim of cursor[row], every
 * transposed copy behind one of cursor[idx].  cursor[N] is zeroed here; on return it counts what was sent to every bucket (a
 * count above meld_csr_bucket_slots() = overflow: nothing was written beyond the bucket and the caller must rebuild the rows
 * another way).  A row's own entries sit anywhere in its bucket: meld_csr_rows_sort_merge does not depend on the order.  bw,
 * keep_cnt, flag_rows, n_flag as meld_knn_refine writes them.  Flagged rows emit nothing here: see meld_coo_emit_scatter_listed.
 * X must be 16-byte aligned (MELD_ERR_INVALID otherwise): four lanes read 64 contiguous bytes of a row as pairs of doubles.
 * The same holds for meld_knn_refine, meld_knn_radius_exact and meld_knn_pair_distances whenever d is even and <= 256. */
int meld_knn_refine_emit(const double* X, int64_t N, int d, const int32_t* cand_idx, const float* cand_d2, const int32_t* cand_cnt,
                         const float* cand_thr, int ksel, int cap, int knn, double decay, double thresh, const float* norm2_max,
                         double err_coef, const float* norm2, double err_coef_lin, double* bw, int32_t* keep_cnt,
                         int32_t* flag_rows, int32_t* n_flag, double bw_scale, const double* bw_fixed, int max_rank,
                         int32_t* cursor, int32_t* tcol, double* tval, meld_stream_t stream);
/* meld_knn_refine_emit on the RAW rows meld_knn16_topk_listed_raw leaves (cap = meld_knn16_row_capacity(ksel); Qn, scale_info: the
 * search's operands): every row is ranked in registers exactly as meld_knn16_finish_rows ranks it -- the row is judged by the same
 * fp32 values, (v + Qn[row]) * scale_info[1] -- and only the rows that end in flag_rows are written back finished (sorted entries in
 * input units, cand_cnt[row] = min(n0 + n1, ksel)): meld_knn16_research_thresholds, the second-stage meld_knn_refine and the sweep
 * read those.  The rows of complete rows stay raw.  Everything else as meld_knn_refine_emit. */
int meld_knn_refine_sort_emit(const double* X, int64_t N, int d, int32_t* cand_idx, float* cand_d2, int32_t* cand_cnt, const float* Qn,
                              const float* scale_info, const float* cand_thr, int ksel, int cap, int knn, double decay, double thresh,
                              const float* norm2_max, double err_coef, const float* norm2, double err_coef_lin, double* bw,
                              int32_t* keep_cnt, int32_t* flag_rows, int32_t* n_flag, double bw_scale, const double* bw_fixed, int max_rank,
                              int32_t* cursor, int32_t* tcol, double* tval, meld_stream_t stream);

/* Exact fp64 radius search for the flagged rows (the analogue of graphtools' re-search /
 * radius_neighbors fallback), rows x reference chunks over the whole device.  mode 0: fb_cnt[f] = number
 * of off-diagonal references with v >= thresh, and err_flag[0] |= 1 if the row's bandwidth cannot be
 * confirmed (fb_cursor[n_flag] is scratch for that check and is left zeroed);
 * mode 1: write (column, value) at fb_off[f] + running cursor (fb_cursor[f], zero on entry).
 * d <= 2559: the eight rows of a workgroup sit in LDS (beyond 64 KB, d > 1023, the kernel's dynamic-LDS limit is raised); a wider
 * d is refused (MELD_ERR_INVALID) before anything is launched. */
int meld_knn_radius_exact(const double* X, int64_t N, int d, int64_t q_begin, const int32_t* flag_rows,
                          int32_t n_flag, const double* bw, int knn, double decay, double thresh,
                          int mode, int32_t* fb_cnt, const int64_t* fb_off, int32_t* fb_cursor,
                          int32_t* fb_col, double* fb_val, int32_t* err_flag,
                          double bw_scale /* as in meld_knn_refine: bw[] is unscaled; with a fixed bandwidth pass knn = INT32_MAX (nothing to verify) */,
                          meld_stream_t stream);
/* out[i][c] = |X[rows[i]] - X[cand[i][c]]| (rows, cand: global row numbers; cand [n][kk]) in the summation order of meld_knn_refine
 * and meld_knn_radius_exact: a bandwidth ranked from these is one the sweep confirms (it counts the references strictly closer
 * in this arithmetic; a library norm differs by a few ulps at d ~ 50).  The order (csrc/refine.hip): even d <= 256 -- coordinate pair
 * kk in slot kk & 3, an even and an odd FMA chain per slot, d2 = (u0 + u1) + (u2 + u3); any other d -- one even and one odd chain.
 * X must be 16-byte aligned when d is even (rows are read as pairs of doubles). */
int meld_knn_pair_distances(const double* X, int d, const int64_t* rows, const int64_t* cand, int64_t n, int kk, double* out,
                            meld_stream_t stream);

/* ---- exact kNN graph under the L1 / L-infinity metrics (replaces [UPSTREAM graphtools kNNGraph(distance="manhattan" |
 *      "cityblock" | "l1" | "chebyshev") -> sklearn NearestNeighbors(metric=...)], reached from reference meld/meld.py:273;
 *      csrc/metric_knn.hip) ------------------------------------------------------------------------
 * Distances are fp64 in one arithmetic and one order for all four calls: |x_k - y_k| summed (L1) or maxed (L-inf) over
 * k = 0 .. d - 1, starting at +0.  d <= 256, N < 2^31, rows in the order the caller gives (tiles = consecutive rows). */
#define MELD_METRIC_L1 1
#define MELD_METRIC_LINF 2
int meld_metric_tile_rows(void); /* rows per tile (64) */
/* box_lo / box_hi [ceil(N / 64)][d]: per-coordinate minimum / maximum of every tile of rows */
int meld_metric_tile_boxes(const double* X, int64_t N, int d, double* box_lo, double* box_hi, meld_stream_t stream);
/* Every row's ksel nearest rows by (distance, column), exactly, ascending: cand_idx / cand_d [N][ksel], cand_cnt[N] =
 * min(ksel, N).  heap_d / heap_i: scratch of ksel * ceil(N / 64) * 64 entries each.  prune = 0 visits every tile (the
 * result is the same bit for bit).  tiles_done[0] (zeroed by the caller) += (query tile, reference tile) pairs computed. */
int meld_metric_topk(const double* X, int64_t N, int d, int metric, int ksel, const double* box_lo, const double* box_hi, int prune,
                     double* heap_d, int32_t* heap_i, int32_t* cand_idx, double* cand_d, int32_t* cand_cnt,
                     unsigned long long* tiles_done, meld_stream_t stream);
/* meld_knn_refine's outputs from those lists: bw[N] = max((knn+1)-th distance, eps), cand_val[N][ksel] = kernel value or 0
 * (diagonal and values below thresh dropped), keep_cnt[N]; a row whose full list does not reach beyond its kernel radius is
 * appended to flag_rows (n_flag[0] zeroed by the caller) with keep_cnt 0.  decay = +inf: connectivity of d <= bw. */
int meld_metric_refine(const int32_t* cand_idx, const double* cand_d, const int32_t* cand_cnt, int64_t N, int ksel, int knn,
                       double decay, double thresh, double* bw, double* cand_val, int32_t* keep_cnt, int32_t* flag_rows,
                       int32_t* n_flag, meld_stream_t stream);
/* Exact sweep of the flagged rows over all N references (meld_knn_radius_exact's formats): mode 0 fb_cnt[f] (zeroed by the
 * caller) = off-diagonal references with kernel value >= thresh; mode 1 writes them at fb_off[f] + fb_cursor[f] (zero on entry). */
int meld_metric_radius(const double* X, int64_t N, int d, int metric, const int32_t* flag_rows, int32_t n_flag, const double* bw,
                       double decay, double thresh, int mode, int32_t* fb_cnt, const int64_t* fb_off, int32_t* fb_cursor,
                       int32_t* fb_col, double* fb_val, meld_stream_t stream);

/* ---- the same, between two point sets: queries Q [M][d] that are NOT among the references X [N][d] (new cells against a fitted
 *      graph: meld_amd/extend.py).  The arithmetic and the (distance, column) order are those above; a
 *      query has no self entry and nothing is dropped as a diagonal.  X, box_lo, box_hi as meld_metric_tile_boxes takes and
 *      writes them. ------------------------------------------------------------------------------------------------------------
 * Slices of the reference tiles the search of M queries is split into (grid.y; every slice keeps heaps of its own, a merge
 * keeps the ksel smallest: the lists are the same bits for any count).  n_slices = 0: chosen from M and the device's CU count;
 * otherwise n_slices clipped to [1, min(16, tiles)].  Size the scratch of meld_metric_cross_topk with the value returned. */
int meld_metric_cross_slices(int64_t M, int64_t N, int n_slices);
/* seed_key[M] (every bit set on entry) <- (point-to-box bound as fp32 bits << 32) | tile of the reference tile nearest to each
 * query: the low 32 bits are the tile the search starts from.  n_tiles * d operations per query.  Qt [d][M]: the queries
 * TRANSPOSED (lane = query: the reads of one coordinate coalesce). */
int meld_metric_cross_seed(const double* Qt, int64_t M, const double* box_lo, const double* box_hi, int64_t N, int d, int metric,
                           unsigned long long* seed_key, meld_stream_t stream);
/* Every query's ksel nearest references by (distance, column), exactly, ascending: cand_idx / cand_d [M][ksel], cand_cnt[M] =
 * min(ksel, N).  Qt [d][M]: the queries transposed.  One wave per 64 consecutive queries: sort the queries by seed tile for the
 * pruning to bite (any order and any seed in [0, tiles) gives the same lists).  A tile is skipped when the bound of its box
 * against the wave's box exceeds every lane's heap top, or when every lane's own point-to-box bound exceeds that lane's.
 * heap_d / heap_i: n_slices * ksel * ceil(M / 64) * 64 entries each; part_idx /
 * part_d [n_slices][M][ksel] and part_cnt [n_slices][M]: the slices' lists (may be NULL when n_slices == 1).  prune = 0 visits
 * every tile.  tiles_done[0] (zeroed by the caller) += (query tile, reference tile) pairs computed. */
int meld_metric_cross_topk(const double* Qt, int64_t M, const double* X, int64_t N, int d, int metric, int ksel, const double* box_lo,
                           const double* box_hi, const int32_t* seed, int prune, int n_slices, double* heap_d, int32_t* heap_i,
                           int32_t* part_idx, double* part_d, int32_t* part_cnt, int32_t* cand_idx, double* cand_d, int32_t* cand_cnt,
                           unsigned long long* tiles_done, meld_stream_t stream);
/* meld_metric_refine for queries: bw[M] = max(bw_scale * (knn+1)-th distance, eps) (pass knn = knn_c - 1: the knn_c-th nearest
 * reference), no entry is the row itself; decay = +inf keeps the first knn + 1 entries of a list, whatever their distances. */
int meld_metric_cross_refine(const int32_t* cand_idx, const double* cand_d, const int32_t* cand_cnt, int64_t M, int ksel, int knn,
                             double decay, double thresh, double bw_scale, double* bw, double* cand_val, int32_t* keep_cnt,
                             int32_t* flag_rows, int32_t* n_flag, meld_stream_t stream);
/* meld_metric_radius for queries: the flagged rows are rows of Q, bw [M] is final (scaled, floored), every reference counts. */
int meld_metric_cross_radius(const double* Q, int64_t M, const double* X, int64_t N, int d, int metric, const int32_t* flag_rows,
                             int32_t n_flag, const double* bw, double decay, double thresh, int mode, int32_t* fb_cnt,
                             const int64_t* fb_off, int32_t* fb_cursor, int32_t* fb_col, double* fb_val, meld_stream_t stream);

/* ---- symmetrise / anisotropy / Laplacian pieces (replaces [UPSTREAM graphtools
 *      BaseGraph.symmetrize_kernel, apply_anisotropy, PyGSPGraph._build_weight_from_kernel;
 *      pygsp Graph.compute_laplacian]) ------------------------------------------------------- */

/* exclusive prefix sum int32 -> int64 (out has n+1 entries; out[n] = total) */
size_t meld_scan_temp_bytes(int64_t n);
int meld_exclusive_scan_i32_i64(const int32_t* in, int64_t* out, int64_t n, void* temp, size_t temp_bytes,
                                meld_stream_t stream);

/* Emit the directed off-diagonal kernel entries as COO, twice: (i,j,v/2) into slot e and the
 * transposed (j,i,v/2) into slot M + e, keys = (row << 32) | col.  keep_off = exclusive scan of
 * keep_cnt; flagged rows take their entries from the fallback arrays at fb_base + fb_off[f]. */
int meld_coo_emit(int64_t q_begin, int64_t q_count, const int32_t* cand_idx, const double* cand_val,
                  const int32_t* cand_cnt, int ksel, int cap, const int64_t* keep_off, const int32_t* flag_rows,
                  int32_t n_flag, const int64_t* fb_off, const int32_t* fb_col, const double* fb_val,
                  int64_t fb_base, int64_t M, uint64_t* keys, double* vals, meld_stream_t stream);

/* radix sort of (u64 key, f64 value) pairs on bits [0, end_bit) */
size_t meld_sort_temp_bytes(int64_t n);
int meld_sort_pairs_u64_f64(const uint64_t* keys_in, uint64_t* keys_out, const double* vals_in,
                            double* vals_out, int64_t n, int end_bit, void* temp, size_t temp_bytes,
                            meld_stream_t stream);

/* Sum runs of equal keys (K + K^T): unique keys/values and their count. */
size_t meld_merge_temp_bytes(int64_t n);
int meld_coo_merge(const uint64_t* keys_sorted, const double* vals_sorted, int64_t n, uint64_t* ukeys,
                   double* uvals, int64_t* n_unique, void* temp, size_t temp_bytes, meld_stream_t stream);

/* keys of rows [row_begin, row_begin + n_rows) -> CSR: rowptr[n_rows+1] (int64), col[nnz] int32 */
int meld_csr_from_keys(const uint64_t* ukeys, int64_t nnz, int64_t row_begin, int64_t n_rows,
                       int64_t* rowptr, int32_t* col, meld_stream_t stream);

/* The same assembly without a global sort (the default; replaces graphtools' (K + K^T)/2 on scipy.sparse, SURVEY.md
 * section 8a A4, like the calls above).  meld_coo_scatter_rows sends every entry to the bucket of its row -- slots
 * [r * B, (r + 1) * B) of tcol / tval, B = meld_csr_bucket_slots(), n_rows * B entries each; cursor[n_rows] (zeroed
 * inside) ends as the number of entries sent to each row, whether they fitted or not.  meld_csr_rows_sort_merge sorts
 * every bucket by column inside one wave and sums pairs of equal columns in place (ucnt[r] = distinct columns of row r;
 * flags[0] bit 0: a row with more than B entries, bit 1: a column that occurs more than twice -- in either case the
 * caller must use the sort-based calls above, whose summation order is defined), and after an exclusive scan of ucnt
 * (rowptr) meld_csr_compact_rows copies the merged buckets to their final place.  Entries whose row lies outside
 * [row_begin, row_begin + n_rows) are ignored. */
/* Row-sharded build: the transposed entries this rank owes to the other ranks (owner of key k = (k >> 32) / rows_per_rank,
 * clipped to world - 1; entries of self_rank are left out: the caller hands its whole transposed array to
 * meld_coo_scatter_rows, which ignores foreign rows) laid out for ONE equal-split all-to-all with no host round trip:
 * send[world][2][cap] int64 -- [o][0][slot] keys, [o][1][slot] the bits of the values; unused slots hold the key ~0, a row
 * outside every slice.  counts[world] (int32) ends as the number of entries owed to each rank, fitted or not: a count above
 * cap means the caller must fall back to a variable-length exchange. */
int meld_coo_partition_remote(const uint64_t* keys, const double* vals, int64_t n, int64_t rows_per_rank, int world,
                              int self_rank, int64_t cap, int32_t* counts, int64_t* send, meld_stream_t stream);
/* Single-GPU shortcut for meld_coo_emit + meld_coo_scatter_rows (all N rows local, q_begin = 0): the kept candidates of
 * meld_knn_refine go straight into the row buckets -- a row's own entries into its first slots without an atomic, the
 * transposed copies behind one -- instead of through 2 M (key, value) pairs.  cursor[N] holds on entry the number of own
 * entries of every row (keep_cnt; for the rows of the exact sweep its count) and ends as meld_coo_scatter_rows leaves it;
 * ksel <= meld_csr_bucket_slots(). */
int meld_coo_emit_scatter(int64_t q_count, const int32_t* cand_idx, const double* cand_val, int ksel, int cap,
                          const int32_t* keep_cnt, const int32_t* flag_rows, int32_t n_flag, const int64_t* fb_off,
                          const int32_t* fb_col, const double* fb_val, int64_t fb_total, int32_t* cursor, int32_t* tcol,
                          double* tval, meld_stream_t stream);
/* Behind meld_knn_refine_emit: the rows it did not emit, into the same buckets (cursor[] as it stands; every own entry behind an
 * atomic claim, guarded by the bucket size like the transposed copies).  rows[n_rows]: the local rows of a second-stage
 * meld_knn_refine (cand_val [.][ksel] / cand_idx [.][cap] at the local row; rows with keep_cnt 0 -- still flagged, or empty --
 * are skipped); flag_rows / fb_*: the entries of the exact sweep, as for meld_coo_emit_scatter.  Either part may be empty. */
int meld_coo_emit_scatter_listed(const int32_t* rows, int32_t n_rows, const int32_t* cand_idx, const double* cand_val, int ksel,
                                 int cap, const int32_t* keep_cnt, const int32_t* flag_rows, int32_t n_flag, const int64_t* fb_off,
                                 const int32_t* fb_col, const double* fb_val, int64_t fb_total, int32_t* cursor, int32_t* tcol,
                                 double* tval, meld_stream_t stream);
int meld_csr_bucket_slots(void);
int meld_coo_scatter_rows(const uint64_t* keys, const double* vals, int64_t n, int64_t row_begin, int64_t n_rows,
                          int32_t* cursor, int32_t* tcol, double* tval, meld_stream_t stream);
int meld_csr_rows_sort_merge(const int32_t* cursor, int64_t n_rows, int32_t* tcol, double* tval, int32_t* ucnt,
                             int32_t* flags,
                             int symm /* how K and K^T combine [UPSTREAM graphtools kernel_symm]: 0 "+" (K + K^T) / 2, 1 "*" K o K^T, 2 "mnn" */,
                             double theta /* symm 2: theta min(K, K^T) + (1 - theta) max(K, K^T) */, meld_stream_t stream);
/* meld_csr_rows_sort_merge, and sums[r] = diag + the merged row's sum out of the wave that holds the row: bit for bit what
 * meld_csr_compact_rows_sums returns (valid where no flag is set). */
int meld_csr_rows_sort_merge_sums(const int32_t* cursor, int64_t n_rows, int32_t* tcol, double* tval, int32_t* ucnt, int32_t* flags,
                                  int symm, double theta, double diag, double* sums, meld_stream_t stream);
/* The compaction with the anisotropy applied on the way out and the degrees of the result: col / val / dw equal, bit for bit,
 * meld_csr_compact_rows followed by meld_csr_anisotropy_degrees(ksum, offset 0).  n_rows = all rows of the graph (the columns
 * index ksum, the sums of meld_csr_rows_sort_merge_sums); anisotropy 0: the plain copy. */
int meld_csr_compact_rows_anisotropy(const int64_t* rowptr, int64_t n_rows, const int32_t* tcol, const double* tval, int32_t* col,
                                     double* val, const double* ksum, double anisotropy, double* dw, meld_stream_t stream);
int meld_csr_compact_rows(const int64_t* rowptr, int64_t n_rows, const int32_t* tcol, const double* tval,
                          int32_t* col, double* val, meld_stream_t stream);
/* The same, and sums[r] = diag + the row's sum on the way out: bit for bit what meld_csr_row_sums returns for the compacted rows. */
int meld_csr_compact_rows_sums(const int64_t* rowptr, int64_t n_rows, const int32_t* tcol, const double* tval, int32_t* col,
                               double* val, double diag, double* sums, meld_stream_t stream);

/* ksum[i] = diag + sum_j val[i,j]   (row sums of the symmetrised kernel; diag = K_ii = 1) */
int meld_csr_row_sums(const int64_t* rowptr, const double* val, int64_t n_rows, double diag,
                      double* out, meld_stream_t stream);
/* W_ij = K_ij / (ksum_i * ksum_j)^anisotropy, in place; ksum_all is indexed by global column,
 * ksum_row_offset = global index of local row 0. */
int meld_csr_anisotropy(const int64_t* rowptr, const int32_t* col, double* val, int64_t n_rows,
                        const double* ksum_all, int64_t ksum_row_offset, double anisotropy,
                        meld_stream_t stream);
/* The same, and the degrees dw[r] = sum_j W_rj of the result in the same pass: equal, bit for bit, to meld_csr_row_sums(diag = 0)
 * called afterwards (same lanes, same order). */
int meld_csr_anisotropy_degrees(const int64_t* rowptr, const int32_t* col, double* val, int64_t n_rows,
                                const double* ksum_all, int64_t ksum_row_offset, double anisotropy, double* dw,
                                meld_stream_t stream);

/* ---- out-of-sample extension (csrc/extend.hip; replaces [UPSTREAM graphtools 1.5.x kNNGraph.build_kernel_to_data(Y),
 *      BaseGraph.extend_to_data(Y), BaseGraph.interpolate(transform, transitions)], reached through `meld_op.graph`) ---- */

/* The query-major half of the COO stream of a search between two point sets (meld_coo_emit: keys (row << 32) | ref, values
 * K / 2, rows in any order) -> the rectangular CSR of rows [row_begin, row_begin + n_rows): rowptr[n_rows + 1] (int64), col[n]
 * (int32, sorted inside a row), val[n] = K, rowsum[n_rows] = the rows' sums (meld_csr_row_sums' bits, diag 0).  Entries of other
 * rows, or with a column >= n_cols, are ignored (rowptr[n_rows] <= n entries are written).  Equal columns inside a row are NOT
 * merged (the stream has none).  The same bits every run.  temp: meld_extend_rows_temp_bytes(n, n_rows) bytes, 8-byte aligned. */
size_t meld_extend_rows_temp_bytes(int64_t n, int64_t n_rows);
int meld_extend_rows(const uint64_t* keys, const double* half_vals, int64_t n, int64_t row_begin, int64_t n_rows, int64_t n_cols,
                     int64_t* rowptr, int32_t* col, double* val, double* rowsum, void* temp, size_t temp_bytes,
                     meld_stream_t stream);
/* out[n_rows, p] = diag(1 / rowsum) K F: the transitions of the new cells applied to a signal on the fitted cells, fp64, without
 * writing the transitions.  F: [n_f_rows, p] row-major, p >= 1.  colmap (optional, int64[n_f_rows]): row of F that holds column
 * j of K (F in the graph's device order: the inverse of its permutation); NULL: row j.  A column outside [0, n_f_rows) adds
 * nothing; a row whose sum is not positive gives zeros.  One wave per row, no atomics: the same bits every run. */
int meld_extend_apply(const int64_t* rowptr, const int32_t* col, const double* val, const double* rowsum, int64_t n_rows,
                      const double* F, int64_t n_f_rows, int p, const int64_t* colmap, double* out, meld_stream_t stream);

/* ---- Laplacian operator: lmax and the Chebyshev recurrence (replaces [UPSTREAM pygsp
 *      Graph.estimate_lmax] at meld/filter.py:39 and [UPSTREAM pygsp
 *      filters.approximations.cheby_op] at meld/filter.py:59) ------------------------------- */

/* The operator L = diag(dw) - W on the local rows [0, n_rows) of a row shard (all rows on one GPU), as every recurrence entry
 * below takes it: the CSR arrays of W, the degrees, and optionally the panel-tiled copy of W (meld_pt_build, further down).
 * layout != NULL selects the panel-tiled kernel (csrc/spmm_tiled.hip), NULL the CSR-stream kernel (csrc/spmm.hip); the entry
 * points, their contracts and their call sites are the same.  rowptr and dw are always required; col and val when layout is
 * NULL (and nnz > 0); every array of the layout otherwise.  nnz (total nonzeros of the local rows) sizes the CSR-stream
 * kernel's LDS staging area.  The record and the layout it points to are HOST memory, read during the call only. */
struct meld_pt_layout;
typedef struct meld_laplacian {
  const int64_t* rowptr; const int32_t* col; const double* val; const double* dw;
  int64_t n_rows, nnz;
  const struct meld_pt_layout* layout;   /* NULL: CSR-stream kernel; col/val may be NULL when set */
} meld_laplacian_t;

/* One step of the three-term recurrence on the local rows of L:
 *     y      = alpha * (dw .* x_loc - W x_full) + beta * x_loc + gamma * z
 *     r     += coef * y                      (if r != NULL)
 *     dots   = per-slot partial sums of [ <y, x_loc>, <y, y> ]   (if dots != NULL; p == 1 only;
 *              dots has 2 * meld_spmm_dot_slots() entries: slot-major per quantity; the caller
 *              sums the slots.  Used by the Lanczos lmax estimate.)
 * x_full is the full-length gathered vector ([n_cols, p] row-major), x_loc = x_full + x_row_offset*p,
 * z, y, r are local ([n_rows, p]); y may alias z.  z may be NULL when gamma == 0.  Any p >= 1 (the CSR-stream kernel in
 * passes of 4 / 2 / 1 columns, the tiled one in passes of 2 + 1).
 *   T1 = (L s - a2 s)/a1          : alpha = 1/a1, beta = -a2/a1, gamma = 0
 *   Tk = (2/a1)(L - a2) T - Told  : alpha = 2/a1, beta = -2 a2/a1, gamma = -1  */
int meld_spmm_dot_slots(void);
int meld_cheby_step(const meld_laplacian_t* L, int p, const double* x_full, int64_t x_row_offset, const double* z, double* y,
                    double* r, double alpha, double beta, double gamma, double coef, double* dots, meld_stream_t stream);

/* One step of the same recurrence for a WIDE signal (the probe block of the filter-bank VertexFrequencyCluster, stands in for the
 * dense window products of /root/reference/meld/cluster.py:98-156,179-194): 1 <= p <= 64 columns, row-major [rows, p], lanes =
 * columns -- the matrix is streamed once for all columns instead of once per column pair.  No accumulator, no dot products:
 *   y = alpha (dw .* x - W x) + beta x + gamma z     (y and z may alias)
 * Reads the CSR arrays of the record whatever its layout: col and val are required. */
int meld_cheby_step_wide(const meld_laplacian_t* L, int p, const double* x_full, int64_t x_row_offset, const double* z, double* y,
                         double alpha, double beta, double gamma, meld_stream_t stream);

/* ---- tall-block algebra of the partial Fourier basis (csrc/subspace.hip; the Rayleigh-Ritz step of the Chebyshev-filtered
 *      subspace iteration that stands for [UPSTREAM pygsp (development line) Graph.compute_fourier_basis(n_eigenvectors=k)]) ----
 * Tall operands are fp64, row-major [n_rows, m] with a leading dimension ld >= m (in doubles), 1 <= m <= 64; the entries of a row
 * beyond column m are neither read nor written.  No floating-point atomics: workgroup b < n_blocks sums the rows
 * [b per, (b + 1) per), per = ceil(n_rows / n_blocks), into part[b] and a second launch adds the partials in workgroup order --
 * the result is a function of the operands and of n_blocks alone, the same bits every run.  1 <= n_blocks <=
 * meld_block_max_blocks().
 *   meld_block_gram_f64:      C[m, m] (row-major, tight) = A^T B;               part: n_blocks * m * m doubles
 *   meld_block_rotate_f64:    out = A S, S [m, m] row-major, tight, on the device (staged in LDS); out may alias A (then
 *                             ldo == lda): a row is read whole before it is written
 *   meld_block_residuals_f64: out[j] = sum_i (LV[i][j] - theta[j] V[i][j])^2;   part: n_blocks * m doubles */
int meld_block_max_blocks(void);
int meld_block_gram_f64(const double* A, int64_t lda, const double* B, int64_t ldb, int64_t n_rows, int m, double* part, int n_blocks,
                        double* C, meld_stream_t stream);
int meld_block_rotate_f64(const double* A, int64_t lda, const double* S, int64_t n_rows, int m, double* out, int64_t ldo,
                          meld_stream_t stream);
int meld_block_residuals_f64(const double* LV, const double* V, int64_t ld, const double* theta, int64_t n_rows, int m, double* part,
                             int n_blocks, double* out, meld_stream_t stream);

/* r = a * x  (n doubles) -- initialises r = c0/2 * T0 */
/* Device-resident Lanczos iterations [it_begin, it_begin + n_iter) of L (single GPU: all n_rows rows local), for the lmax
 * estimate ([UPSTREAM pygsp Graph.estimate_lmax], reference meld/filter.py:39).  v0/v1/v2 [n_rows]: the three rotating
 * vectors -- before iteration 0, v1 holds the (un-normalised) start vector and v0 zeros; state[8]: state[0] = state[3] =
 * 1 / |start|, the rest zero.  alphas[it] / betas[it] receive the tridiagonal entries; nothing is synchronised -- read them
 * back when a convergence check is due.
 *   CSR-stream kernel: scratch = 3 * meld_spmm_dot_slots() doubles, zero before iteration 0; stop is ignored.
 *   tiled layout: scratch = 8 * meld_spmm_dot_slots() doubles (partial sums and scalars in parity buffers: two launches per
 *     iteration, the SpMV derives its own scalars; only state[0] = 1 / |start| is read, before iteration 0); betas[it] of the
 *     LAST iteration of a call is written by a closing one-wave launch.  stop (optional, device memory): a launch of the call
 *     that finds *stop != 0 when it starts does nothing -- the caller checks convergence on the host while the NEXT batch
 *     already runs and voids what is left of it once it has its answer (the vectors and the entries of that batch are then
 *     undefined). */
int meld_lanczos_steps(const meld_laplacian_t* L, double* v0, double* v1, double* v2, double* state, double* alphas,
                       double* betas, int it_begin, int n_iter, double* scratch, const int32_t* stop, meld_stream_t stream);
/* The same iteration as four stream-ordered phases, for the row-sharded driver (it all-reduces dots after
 * the SpMV and nrm2 after the axpy, and all-gathers the new vector): x_full is the gathered iterate,
 * x_row_offset the first local row in it; z_local / y_local / x_local are local rows; state / dots
 * (2 * slots) / nrm2 (slots) as in meld_lanczos_steps (CSR-stream form).  On the tiled layout the SpMV streams the fp32
 * copy of the values (pval32) when the layout keeps one. */
int meld_lanczos_spmv(const meld_laplacian_t* L, const double* x_full, int64_t x_row_offset, const double* z_local,
                      double* y_local, const double* state, double* dots, meld_stream_t stream);
int meld_lanczos_alpha(double* state, const double* dots, double* nrm2, double* alphas, int it, meld_stream_t stream);
int meld_lanczos_axpy(const double* x_local, double* y_local, int64_t n_rows, const double* state, double* nrm2,
                      meld_stream_t stream);
int meld_lanczos_beta(double* state, const double* nrm2, double* dots, double* betas, int it, meld_stream_t stream);
/* One-reduction form of the sharded iteration (one all-reduce + one all-gather per iteration instead of two + one):
 * the iterate stays un-normalised, u_{k+1} = w_k, so meld_lanczos_spmv (with state[3] = 1, state[4] = 0) computes
 * z = L u_k without a scalar and adds the partial sums of <z, u_k> to acc[0 .. slots); meld_lanczos_axpy3 of the previous
 * iteration has added |u_k|^2 to acc[2 slots .. 3 slots).  The caller all-reduces acc (3 * slots doubles, ONCE), then
 *   meld_lanczos_fold:  alpha_k = <z, u_k> / |u_k|^2 -> alphas[it]; n_k = |u_k| -> betas[it - 1] (it > 0); coefficients
 *                       of the update into state[5..7], n_k into state[2]; acc zeroed;
 *   meld_lanczos_axpy3: y <- y / n_k - (alpha_k / n_k) u - (n_k / n_{k-1}) u_prev  (= u_{k+1}, local rows, in place of z)
 *                       and acc[2 slots ..) += |u_{k+1}|^2 (pass nrm2 = acc + 2 * slots).
 * Before iteration 0: acc[2 slots ..) holds the partial sums of |u_0|^2, the rest of acc and state[2] are zero.
 * beta_{k} (= n_{k+1}) is written one iteration late. */
int meld_lanczos_fold(double* state, double* acc, double* alphas, double* betas, int it, meld_stream_t stream);
int meld_lanczos_axpy3(double* y_local, const double* u_local, const double* u_prev_local, int64_t n_rows,
                       const double* state, double* nrm2, meld_stream_t stream);
int meld_scale_f64(const double* x, double a, double* r, int64_t n, meld_stream_t stream);
/* y = a * x + b * y  (n doubles) -- Lanczos vector update.  If nrm2 != NULL it receives
 * meld_spmm_dot_slots() partial sums of <y, y> (zeroed by the call; the caller adds them up). */
int meld_axpby_f64(double a, const double* x, double b, double* y, int64_t n, double* nrm2,
                   meld_stream_t stream);

/* ---- panel-tiled, symmetry-folded layout of W for the recurrence (csrc/spmm_tiled.hip) ----------
 * The `layout` of meld_laplacian_t: same operator and same entry points ([UPSTREAM pygsp cheby_op /
 * estimate_lmax] at reference meld/filter.py:59 / :39), on a copy of W laid out so that the iterate is
 * staged in LDS instead of being gathered per nonzero: rows in nb nnz-balanced blocks (one per CU); the
 * nonzeros whose column lies inside the block's own row range are stored once per symmetric pair (IN
 * part: 12 instead of 24 bytes per pair); the distinct columns outside it are listed, cut into tiles of
 * tile_cols columns and staged through a ring of LDS buffers (OUT part); every consumer wave streams its
 * own contiguous slice of the block in whole chunks of 64 entries.  Built once per graph.  The fold needs
 * a bitwise symmetric W: the builder verifies it (status 5) and can be told not to fold.  Results are
 * reproducible to rounding, not bit for bit (several waves add into one LDS accumulator).
 * All arrays are device memory owned by the caller:
 *   blk_row   [nb + 1]  int32   first row of every block
 *   blk_ntile [nb]      int32   tiles of the block (-1: the block could not be laid out, see status)
 *   blk_ndist [nb]      int32   distinct OUT columns of the block
 *   seg       [meld_pt_seg_len(nb)] int32  per (block, wave) chunk schedule and segment offsets
 *   list_cols [nnz]     int32   block b's sorted distinct OUT columns start at rowptr[blk_row[b]]
 *   pval      [meld_pt_stream_len(nnz, nb)] fp64  values in stream order (+ optional pval32, fp32, same length)
 *   pidx      [meld_pt_stream_len(nnz, nb)] uint32  LDS offsets of the entry's column slot and row   */
typedef struct meld_pt_layout {
  const int32_t* blk_row;
  const int32_t* blk_ntile;
  const int32_t* blk_ndist;
  const int32_t* seg;
  const int32_t* list_cols;
  const double* pval;
  const uint32_t* pidx;
  int32_t nb;
  const float* pval32; /* optional: pval rounded to fp32, streamed by the Lanczos SpMV of the lmax estimate
                          (meld_lanczos_steps / meld_lanczos_spmv) instead of pval; NULL = not kept */
  int64_t stream_len;  /* entries of pval / pidx / pval32 (= meld_pt_stream_len(nnz, nb)) */
  const uint16_t* cdesc; /* [meld_pt_desc_len(nb)] chunk descriptors of every consumer wave's stream */
} meld_pt_layout_t;
int meld_pt_geometry(int* consumer_waves, int* rows_max, int* tile_cols, int* tiles_max);
int meld_pt_num_blocks(int64_t n_rows); /* nb the builder wants for n_rows local rows */
int64_t meld_pt_seg_len(int nb);
int64_t meld_pt_stream_len(int64_t nnz, int nb);
int64_t meld_pt_desc_len(int nb);
/* Build the layout of the local rows [0, n_rows) of a CSR matrix with n_cols columns (the arrays of
 * `layout` are written); local row r is column col_base + r of the matrix (0 on one GPU, the shard's first
 * row on a row shard); symmetric != 0 folds the in-block pairs.  status[0] (device) receives 0, or the
 * reason the layout cannot be used:
 * 1 = (no longer raised: a block's column panels are handled in groups), 2 = too many distinct columns in a block,
 * 3 = n_cols beyond the builder's index range, 4 = a segment / a wave's pairs / its padding beyond the
 * builder's ranges, 5 = W is not bitwise symmetric inside a block (build again with symmetric = 0),
 * 6 = a diagonal entry -- the caller then leaves `layout` of its operator record NULL. */
int meld_pt_build(const int64_t* rowptr, const int32_t* col, const double* val, int64_t n_rows, int64_t n_cols,
                  int64_t col_base, int symmetric, const meld_pt_layout_t* layout,
                  uint32_t* codes /* scratch, nnz entries */, int32_t* status, meld_stream_t stream);

/* ---- row-sharded recurrences with the host out of the loop (csrc/sharded.hip) ----------
 * One process per GPU, cells row-sharded: rank g owns rows [g * rows_pad, (g + 1) * rows_pad) of every full-length vector.
 * RCCL is reached through dlopen("librccl.so.1") (no link-time dependency: the library loads without it and
 * meld_rccl_available() says 0); the communicator is the library's own, built from a unique id the ranks share.
 *   meld_rccl_unique_id: 128 bytes on the HOST (rank 0 calls it, the bytes travel by any means, e.g. torch.distributed);
 *   meld_rccl_comm_create: collective over the `world` ranks, the calling thread's current device = the rank's GPU;
 *   meld_rccl_all_gather / _all_reduce_sum_f64: the two collectives of the path, on `stream`. */
int meld_rccl_available(void);
int meld_rccl_unique_id(void* id_host);
int meld_rccl_comm_create(const void* id_host, int world, int rank, void** comm);
int meld_rccl_comm_destroy(void* comm);
int meld_rccl_all_gather(void* comm, const void* send, void* recv, size_t bytes_per_rank, meld_stream_t stream);
int meld_rccl_all_reduce_sum_f64(void* comm, double* buf, size_t count, meld_stream_t stream);
/* Steps 2 .. n_coef - 1 of the Chebyshev recurrence in ONE call:
 *   T_k = alpha2 L T_{k-1} + beta2 T_{k-1} - T_{k-2},   r += coeffs[k] T_k      [UPSTREAM pygsp cheby_op, reference meld/filter.py:59]
 * t_a / t_b are the FULL-length iterates [world * rows_pad, p] holding the gathered T_0 / T_1 on entry, used as ping-pong
 * buffers (T_k overwrites the local rows of T_{k-2}); r [rows_pad, p]: the local rows of the result, holding c_0/2 T_0 + c_1 T_1
 * on entry; coeffs: n_coef doubles on the HOST.  comm: the rank's communicator (meld_rccl_comm_create) -- the new local slice
 * is all-gathered in place behind every step, row_begin = rank * rows_pad -- or NULL on a single GPU: no collective, row_begin
 * must be 0.  Replaces one kernel call (+ one torch.distributed all-gather) per step issued from Python.  On the tiled layout
 * the accumulator is read and written every other step only (a step adds c_k T_k + c_{k-1} T_{k-1} at once), which removes 16
 * of the 80 vector bytes per row and step at p = 2; the CSR-stream kernel adds c_k T_k at every step.
 * *last (optional) = 1 if t_b holds the last T, 0 if t_a does. */
int meld_cheby_run(void* comm, const meld_laplacian_t* L, int64_t rows_pad, int64_t row_begin, int p, double* t_a, double* t_b,
                   double* r, const double* coeffs, int n_coef, double alpha2, double beta2, int* last, meld_stream_t stream);
/* Iterations [it_begin, it_begin + n_iter) of the one-reduction Lanczos recurrence (meld_lanczos_spmv with state[3] = 1,
 * state[4] = 0; ONE all-reduce of acc [3 * meld_spmm_dot_slots()]; meld_lanczos_fold; meld_lanczos_axpy3; all-gather of
 * the new vector) on a row shard in one call.  v0 / v1 / v2: FULL-length rotating vectors [world * rows_pad]. */
int meld_lanczos_steps_sharded(void* comm, const meld_laplacian_t* L, int64_t rows_pad, int64_t row_begin, double* v0, double* v1,
                               double* v2, double* state, double* acc, double* alphas, double* betas, int it_begin, int n_iter,
                               meld_stream_t stream);

/* ---- KMeans step of VertexFrequencyCluster.predict (reference meld/cluster.py:315-345 -> [UPSTREAM
 *      sklearn.cluster.KMeans], Lloyd iteration; csrc/kmeans.hip) ---------------------------------------
 * One pass over X[n, d] (fp64, d <= 32): labels[i] = nearest of the k <= 64 centroids (ties: lowest index),
 * and per workgroup b < n_blocks the partial sums part_sum[b][k][d], counts part_cnt[b][k] (as fp64) and
 * inertia part_inertia[b]; the caller reduces the partials over b (fixed order) and divides. */
int meld_kmeans_max_blocks(void);
int meld_kmeans_assign(const double* X, int64_t n, int d, const double* centroids, int k, int32_t* labels,
                       double* part_sum, double* part_cnt, double* part_inertia, int n_blocks, meld_stream_t stream);

/* ---- Lloyd step for thousands of centres (csrc/kmeans_wide.hip; meld_amd.KMeans, the reference's k-means baseline
 *      comparison/comparison.py::run_geometry_clustering -> [UPSTREAM sklearn.cluster.KMeans]) -----------------------------
 * Everything is fp64; no atomics; the same operands give the same bits every run.
 * meld_kmeans_wide_assign: labels[i] (int32 [n]) = the centre nearest to row i of Y [n, d] (row-major, leading dimension
 *   ldy >= d) among centres [k, d] (row-major, dense); best_d2[i] (NULL: not wanted) = the squared distance to it, clamped at 0.
 *   Candidates are compared on |c_j|^2 - 2 y_i . c_j (fp64 matrix instruction); among equal scores the lowest index wins.
 *   centre_norms [k] is written by the call (|c_j|^2) and read by its second launch.  1 <= d <= meld_kmeans_wide_max_d() = 128,
 *   1 <= k <= meld_kmeans_wide_max_k() = 4096 per call (more centres: call per chunk and combine the minima).
 * meld_kmeans_wide_sums: sums[j][:] (fp64 [k, d]) = the sum of the rows order[seg_ptr[j] .. seg_ptr[j + 1]) of Y; order int64 [n]
 *   (a permutation of the rows grouped by label), seg_ptr int64 [k + 1] ascending in [0, n].  Any k >= 1.  The additions of a
 *   cluster run in an order that depends on (order, seg_ptr) alone: 16 slots, slot s adds the groups s, s + 16, ... of 4
 *   consecutive entries of the segment in sequence, the slots meet in slot order.  An empty segment gives zeros.
 * Both return -1 before any launch for d or k out of range, ldy < d, n outside [0, 2^31) or a NULL required pointer;
 * n == 0 is a successful no-op. */
int meld_kmeans_wide_max_d(void);
int meld_kmeans_wide_max_k(void);
int meld_kmeans_wide_assign(const double* Y, int64_t ldy, int64_t n, int d, const double* centres, int k, double* centre_norms,
                            int32_t* labels, double* best_d2, meld_stream_t stream);
int meld_kmeans_wide_sums(const double* Y, int64_t ldy, int64_t n, int d, const int64_t* order, const int64_t* seg_ptr, int k,
                          double* sums, meld_stream_t stream);

/* ---- cache-locality ordering helper (no reference counterpart; csrc/reorder.hip) ---------- */
/* out[i] = index (within its group) of the centroid nearest to X[i]; cents holds n_per_group
 * centroids per group, group[i] selects the group of point i (NULL = one shared set).  order
 * (optional, grouped form only) = the points sorted by group: the traversal order that keeps a
 * wave inside one group. */
int meld_assign_nearest(const double* X, int64_t N, int d, const double* cents, int n_per_group,
                        const int32_t* group, const int64_t* order, int32_t* out, meld_stream_t stream);
/* Greedy nearest-neighbour chain over the m (<= 64) rows of every group P[g] ([n_groups][m][d] fp64),
 * starting at the row with the smallest first coordinate: rank[g][i] = position of row i along the chain
 * (orders the centroids of the locality permutation so that consecutive groups are close in space). */
int meld_chain_order(const double* P, int64_t n_groups, int m, int d, int32_t* rank, meld_stream_t stream);
/* out[i][:] = X[perm[i]][:] (rows of d doubles; out must not alias X): the cells brought into the device order. */
int meld_gather_rows_f64(const double* X, const int64_t* perm, int64_t N, int d, double* out, meld_stream_t stream);
/* Glue of the ordering levels, one launch each (meld_amd/reorder.py): stable argsort of 32-bit keys below 2^end_bit
 * (order[i] = index of the i-th smallest key; keys_sorted alongside); starts[g] = first position of key g among the sorted
 * keys, g = 0 .. n_groups; cents[(g f + c) d ..] = the cell at fraction (c + 1/2) / f of group g's sorted members;
 * key[i] <- key[i] f + rank[key[i] f + child[i]] (position of the cell's child along its group's chain). */
size_t meld_argsort_u32_temp_bytes(int64_t n);
int meld_argsort_u32(const uint32_t* keys, int64_t n, int end_bit, int64_t* order, uint32_t* keys_sorted, void* temp,
                     size_t temp_bytes, meld_stream_t stream);
int meld_order_starts(const uint32_t* keys_sorted, int64_t n, int n_groups, int64_t* starts, meld_stream_t stream);
int meld_order_pick_centroids(const double* X, int64_t N, int d, const int64_t* order, const int64_t* starts, int n_groups, int f,
                              double* cents, meld_stream_t stream);
int meld_order_update_keys(uint32_t* key, const int32_t* child, const int32_t* rank, int64_t n, int f, meld_stream_t stream);


/* ---- sample labels -> codes, counts and the indicator signal (replaces MELD._create_sample_indicators,
 *      meld/meld.py:143-191: np.unique + LabelBinarizer, and the column normalisation of meld/meld.py:229-232;
 *      csrc/labels.hip) ------------------------------------------------------------------------------------
 * Labels arrive as fixed-width words (numpy 'U' / 'S' / 64-bit integer arrays viewed as int32 [n_rows, n_words],
 * n_words <= meld_factorize_max_words()).  Two labels get the same group iff all their words are equal (a dictionary
 * of whole labels in LDS: no hashing).  meld_factorize_labels leaves in head (int64 [2 + 2 G], G =
 * meld_factorize_max_groups()): [0] status (1: more than G distinct labels, nothing else valid), [1] number of groups,
 * [2 .. 2 + G) the first row of every group, [2 + G ..) the group sizes; the per-row group numbers stay in temp.
 * meld_factorize_codes then writes codes[i] = rank[group of row i] (rank: int32 on the device, the position of every
 * group among the SORTED labels as np.unique orders them -- only the host can compare label strings; NULL: the group
 * numbers themselves). */
int meld_factorize_max_groups(void);
int meld_factorize_max_words(void);
size_t meld_factorize_temp_bytes(int64_t n_rows);
int meld_factorize_labels(const int32_t* words, int64_t n_rows, int n_words, void* temp, size_t temp_bytes, int64_t* head,
                          meld_stream_t stream);
int meld_factorize_codes(const void* temp, int64_t n_rows, const int32_t* rank, int64_t* codes, meld_stream_t stream);
/* out[n_pad, p] (fp64): row i = scale[c] at column c = codes[perm[i]], 0 elsewhere (scale NULL: 1; perm NULL: i);
 * rows n_rows .. n_pad are zero.  The filter's input signal in the device's row order, one pass. */
int meld_indicator_signal(const int64_t* codes, const double* scale, const int64_t* perm, int64_t n_rows, int64_t n_pad, int p,
                          double* out, meld_stream_t stream);
/* out[perm[i]][:] = in[i][:] for i < n_rows (rows of p doubles): the densities back in the caller's cell order
 * (meld/meld.py:246-250 wraps them with the labels' index). */
int meld_scatter_rows_f64(const double* in, const int64_t* perm, int64_t n_rows, int p, double* out, meld_stream_t stream);

/* ---- connectivity (csrc/components.hip; replaces [UPSTREAM pygsp Graph.is_connected / extract_components / subgraph] and
 *      scipy.sparse.csgraph.connected_components on the exported W) ----------------------------------------------------------
 * The operand is the CSR of a single-GPU graph: W symmetric without diagonal, rowptr[n_rows + 1] int64, col[nnz] int32 in
 * [0, n_rows), rows in device order; 1 <= n_rows < 2^31 everywhere.  Integer atomics only: the same output every run.
 *
 * meld_cc_round: one round of hook-and-compress on parent[n_rows] (int32; the caller starts it at parent[v] = v).  Hook: every
 *   row tries atomicMin(parent[root of the row], min of parent[] over its columns); compress: every vertex stores the ancestor
 *   its chain leads to.  parent[v] <= v always and values only decrease, so chains descend and every chase ends (each is capped
 *   at 64 loads besides).  *changed (device word) is cleared first and set to 1 when the round stored anything.  The caller
 *   repeats rounds until one leaves *changed == 0: then parent[v] is the smallest device index of v's component.  Launch ends
 *   are the only synchronisation between workgroups.  col may be NULL for a graph without entries.
 * meld_cc_minima (parents at their fixed point): min_orig[r] = the smallest caller-order index of root r's component (perm[v]
 *   for device row v, v itself where perm is NULL), count[r] = its size (both int32 [n_rows], defined at roots only), and
 *   flags[i] = 1 where i is such a minimum, 0 elsewhere (int32 [n_rows]: the input of meld_exclusive_scan_i32_i64, whose output
 *   is `rank`, rank[n_rows] the number of components).
 * meld_cc_labels: labels[perm[v]] = rank[min_orig[parent[v]]] (int32 [n_rows], the caller's order: components numbered by their
 *   smallest caller-order index, as scipy numbers them) and sizes[label] = count (int64 [number of components]). */
int meld_cc_round(const int64_t* rowptr, const int32_t* col, int64_t n_rows, int32_t* parent, int32_t* changed,
                  meld_stream_t stream);
int meld_cc_minima(const int32_t* parent, const int64_t* perm, int64_t n_rows, int32_t* min_orig, int32_t* count, int32_t* flags,
                   meld_stream_t stream);
int meld_cc_labels(const int32_t* parent, const int64_t* perm, const int32_t* min_orig, const int32_t* count, const int64_t* rank,
                   int64_t n_rows, int32_t* labels, int64_t* sizes, meld_stream_t stream);
/* Induced subgraph.  new_index[n_rows] (int32, device order): the new row / column number of a kept vertex, -1 for a dropped
 * one; kept vertices are numbered in ascending device order, so the kept columns of a row stay sorted.
 * meld_subgraph_count: counts[new_index[u]] = kept entries of kept row u (int32 [number kept]; scanned by the caller into
 *   sub_rowptr).  meld_subgraph_fill: sub_col / sub_val [sub_rowptr[number kept]] = the kept entries, columns renumbered, values
 *   copied bit for bit. */
int meld_subgraph_count(const int64_t* rowptr, const int32_t* col, const int32_t* new_index, int64_t n_rows, int32_t* counts,
                        meld_stream_t stream);
int meld_subgraph_fill(const int64_t* rowptr, const int32_t* col, const double* val, const int32_t* new_index, int64_t n_rows,
                       const int64_t* sub_rowptr, int32_t* sub_col, double* sub_val, meld_stream_t stream);

/* ---- diffusion of cell signals (csrc/diffuse.hip; replaces the product with graphtools' diff_op = normalize(K, "l1", axis=1)
 *      that [UPSTREAM magic-impute, unpinned: not importable next to this code] repeats t times) ------------------------------
 * One step of the random walk of the kernel matrix K = W + diag(kd) on a wide fp64 signal, rows in the graph's device order:
 *     y[i, c] = ( sum_{e in row i, storage order} val[e] * x[col[e], c]  +  kd[i] * x[i, c] ) / s[i]         c < p
 * rowptr[n_rows + 1] int64, col[nnz] int32 in [0, n_rows), val[nnz] fp64: the CSR of W (no diagonal); kd[n_rows] the kernel's
 * diagonal, s[n_rows] = dw + kd the row sums of K (s[i] != 0 is the caller's to check: the kernel divides).
 * x and y are [n_rows, ld] row-major with ldx, ldy >= p (in doubles); columns beyond p are neither read nor written, so a
 * wider signal is processed in column panels without copies.  1 <= p <= meld_diffuse_max_cols() = 128 per call; lanes =
 * columns, with p > 64 a lane carries column `lane` and column `lane + 64` (8-byte accesses only: x, y and the leading
 * dimensions need no alignment beyond 8 bytes).  The matrix is streamed once per call, whatever p.
 * One output element is: acc = 0; acc = fma(val[e], x[col[e], c], acc) over the row's entries in storage order;
 * acc = fma(kd[i], x[i, c], acc); one true division by s[i] -- a function of the operands alone: the other columns of the launch,
 * p, the panel, the leading dimensions and the run do not change a bit of it.  No atomics.  A row without entries gives
 * kd x / s.
 * y must not overlap x: a call whose ranges [x, x + n_rows*ldx) and [y, y + n_rows*ldy) intersect returns -1.  So do, before any
 * launch: a NULL rowptr / kd / s / x / y; a NULL col or val for a matrix with rows (one without entries passes any address: they
 * are not read); p out of range; ld < p; n_rows < 0.  n_rows == 0 is a successful no-op. */
int meld_diffuse_max_cols(void);
int meld_diffuse_step(const int64_t* rowptr, const int32_t* col, const double* val, const double* kd, const double* s,
                      int64_t n_rows, const double* x, int64_t ldx, double* y, int64_t ldy, int p, meld_stream_t stream);

/* ---- geodesic distances (csrc/geodesic.hip; replaces scipy.sparse.csgraph.dijkstra on the exported graph, what [UPSTREAM
 *      graphtools 1.5.x BaseGraph.shortest_path, unpinned: not importable next to this code] calls) ---------------------------
 * meld_minplus_step: one synchronous Bellman-Ford round on a row-major fp64 distance block, rows in the graph's device order:
 *     y[i, c] = min( x[i, c],  min_{e in row i} ( x[col[e], c] + len[e] ) )                                c < p
 * rowptr[n_rows + 1] int64, col[nnz] int32 in [0, n_rows): the CSR of W; len[nnz] fp64, finite and >= 0, aligned with col (the
 * solver presumes len symmetric).  x holds distances >= 0 or +inf ("not reached": inf + len = inf); with such operands no NaN
 * arises -- validating them is the caller's (meld_amd/geodesic.py does).
 * x and y are [n_rows, ld] row-major with ldx, ldy >= p (in doubles); columns beyond p are neither read nor written, so a wider
 * source set is processed in column panels without copies.  1 <= p <= meld_minplus_max_cols() = 128 per call; lanes = columns
 * (sources), with p > 64 a lane carries column `lane` and column `lane + 64` (8-byte accesses only).  The matrix is streamed
 * once per call, whatever p.
 * One output element is one fp64 add per entry and an exact minimum -- a function of the operands alone: the other columns of
 * the launch, p, the panel, the leading dimensions and the run do not change a bit of it.  A row without entries copies x to y.
 * changed: one device int32.  The entry clears it on the stream before the launch; a wave in which any stored element is lower
 * than the x it replaced stores 1 there (a plain store of the constant from one lane).  Nothing else is shared between
 * workgroups: no floating-point atomics, no waiting on memory another workgroup writes, no grid barrier; the end of the launch
 * is the only synchronisation.  The caller repeats rounds (x and y taking turns) until one leaves *changed == 0: that round's
 * output equals its input.  Round r has every shortest path of at most r edges right, so n_rows rounds always suffice.
 * y must not overlap x (a round is a pure function of x: the number of rounds is the same every run): a call whose ranges
 * [x, x + n_rows*ldx) and [y, y + n_rows*ldy) intersect returns -1.  So do, before any launch: a NULL rowptr / x / y / changed; a
 * NULL col or len for a matrix with rows (one without entries passes any address: they are not read); p out of range; ld < p;
 * n_rows < 0.  n_rows == 0 launches nothing and still clears *changed.
 *
 * meld_edge_lengths_l2: out[e] = sqrt( sum_k (X[i, k] - X[col[e], k])^2 ) for every stored entry e of row i; X [n_rows, ldX]
 * row-major fp64 in the same row order as the CSR, 1 <= d <= 256, ldX >= d.  The sum is acc = 0; acc = fma(t, t, acc), t =
 * X[i, k] - X[col[e], k], k ascending: (a - b)^2 == (b - a)^2 exactly and the order is fixed, so the lengths of (i, j) and (j, i)
 * are bit-equal.  Returns -1 before any launch for a NULL rowptr / X, a NULL col / out for a matrix with rows, d out of range,
 * ldX < d, n_rows outside [0, 2^31); n_rows == 0 is a successful no-op. */
int meld_minplus_max_cols(void);
int meld_minplus_step(const int64_t* rowptr, const int32_t* col, const double* len, int64_t n_rows, const double* x, int64_t ldx,
                      double* y, int64_t ldy, int p, int32_t* changed, meld_stream_t stream);
int meld_edge_lengths_l2(const int64_t* rowptr, const int32_t* col, int64_t n_rows, const double* X, int64_t ldX, int d,
                         double* out, meld_stream_t stream);

/* ---- landmark operator (csrc/landmark.hip; replaces [UPSTREAM graphtools 1.5.x LandmarkGraph.build_landmark_op,
 *      _landmarks_to_data and LandmarkGraph.extend_to_data, unpinned: not importable next to this code], which the reference reaches
 *      by forwarding n_landmark at meld/meld.py:105,118) -------------------------------------------------------------------------
 * Everything is fp64; no atomics; no workgroup waits on memory another writes; every output is a function of the operands alone,
 * the same bits every run.  meld_landmark_max() = 4096 is the largest number of landmarks L (the Gram's LDS accumulator: 32 KB).
 *
 * Merge by label: B = M C for a CSR matrix M [n_rows, n_cols] and the one-hot C [n_cols, L] of label[] -- graphtools' per-cluster
 * sums of the kernel's columns (``pmn`` before its normalisation, by the kernel's symmetry), and for the kernel rows of new cells
 * the sums extend_to_data normalises.  Two launches with a scan of the caller's in between:
 * meld_landmark_merge_count: counts[i] (int32 [n_rows]) = the number of distinct labels in row i, and marked[] (int32 scratch:
 *   one element per stored entry, plus one per row with has_diag; row i starts at rowptr[i] + (has_diag ? i : 0)) = every entry's
 *   label, the sign bit set where an earlier entry of the row carries the same label.  rowptr[n_rows + 1] int64, col[nnz] int32 in
 *   [0, n_cols); label[n_cols] int32 in [0, L) (the caller's to check: labels are stored, never used as addresses); colmap NULL or
 *   int64 [n_cols]: label[colmap[c]] is the label of column c (a graph in its device order with labels in the caller's order:
 *   colmap = perm).  has_diag != 0 (square matrices only) adds the entry (i, label of column i) behind the stored entries of row i.
 * meld_landmark_merge_fill: with out_rowptr[n_rows + 1] = the exclusive scan of counts (meld_exclusive_scan_i32_i64), writes the
 *   CSR [n_rows, L]: out_col / out_val [out_rowptr[n_rows]] hold every label present in the row once, ascending; a value is the sum
 *   of the merged entries in storage order, the diagonal kd[i] (kd NULL: none; it must be given exactly where has_diag was) last.
 *   rowsum[i] = all values of row i in storage order, the diagonal last.  A row without entries and without a diagonal is empty,
 *   its rowsum 0.  Rows may have any length (the work is quadratic in it: every entry is compared with every other, in LDS tiles
 *   of 256).
 *
 * meld_landmark_gram: op[L, L] row-major = diag(1 / s) A^T diag(1 / r) A and s[L] = the column sums of A, for A [n_cells, L] as the
 *   merged CSR above (labels distinct and ascending inside a row) and its transpose t_* [L, n_cells] with the cells ascending inside
 *   a landmark (meld_csr_transpose_keys + meld_sort_pairs_u64_f64 + meld_csr_from_keys), r[n_cells] the row sums.  One workgroup
 *   per landmark l: acc[m] = fma(A[j, l] / r[j], A[j, m], acc[m]) over the cells j of the landmark in ascending order (r[j] <= 0
 *   contributes nothing), op[l, m] = acc[m] / s[l] (one true division; a row with s[l] <= 0 is zeros); s[l] adds the entries
 *   e, e + 64, ... of row l of the transpose per lane, then the 64 lanes by a xor butterfly.
 *
 * Each entry returns -1 before any launch for a NULL required pointer (a matrix without rows passes any address for its columns
 * and values), n_landmark outside [1, meld_landmark_max()], sizes outside [0, 2^31), has_diag on a matrix that is not square.
 * n_rows == 0 is a successful no-op; meld_landmark_gram with n_cells == 0 stores zeros. */
int meld_landmark_max(void);
int meld_landmark_merge_count(const int64_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_cols, const int32_t* label,
                              int n_landmark, const int64_t* colmap, int has_diag, int32_t* marked, int32_t* counts,
                              meld_stream_t stream);
int meld_landmark_merge_fill(const int64_t* rowptr, const double* val, const double* kd, int64_t n_rows, const int32_t* marked,
                             const int64_t* out_rowptr, int32_t* out_col, double* out_val, double* rowsum, meld_stream_t stream);
int meld_landmark_gram(const int64_t* a_rowptr, const int32_t* a_col, const double* a_val, int64_t n_cells, const int64_t* t_rowptr,
                       const int32_t* t_col, const double* t_val, int n_landmark, const double* r, double* op, double* s,
                       meld_stream_t stream);

/* ---- metric MDS of the PHATE embedding (csrc/mds.hip; replaces the metric stage of [UPSTREAM phate 1.0.x phate.mds.embed_MDS,
 *      unpinned: not importable next to this code], which every notebook of the reference and Benchmarker.fit_phate
 *      (meld/benchmark.py) reach through phate.PHATE) -----------------------------------------------------------------------------
 * Everything is fp64; one launch per step; no atomics; no workgroup waits on memory another writes; every output is a function of
 * the operands alone, the same bits every run.  meld_smacof_max_dim() = 8 is the largest number of embedding dimensions.
 *
 * meld_smacof_step: one SMACOF step (the Guttman transform with unit weights) from the configuration Z [n, dim] towards the target
 *   distances D [n, n] (row-major, leading dimension ldD >= n; row i reads D[i, 0:n] only, D need not be symmetric), and the
 *   stress terms of Z itself.  With d_ij = |Z[i] - Z[j]|_2 from direct differences (fma chain over the components, one sqrt):
 *     Z_out[i]      = (1 / n) sum_{j != i, d_ij > 0} (D[i, j] / d_ij) (Z[i] - Z[j])
 *     row_stress[i] = sum_{j != i} (d_ij - D[i, j])^2          (a pair with d_ij == 0 contributes D[i, j]^2 here, nothing above)
 *   so that stress(Z) = 1/2 sum_i row_stress[i] (the caller's sum).  Z and Z_out [n, dim] row-major, distinct buffers (the caller
 *   ping-pongs them); row_stress [n].  Order of the sums: lane l of a wave adds the columns l, l + 64, l + 128, ... in ascending
 *   order, then the 64 lanes by a xor butterfly; one true division by n.  A workgroup takes 8 consecutive rows and stages Z in LDS
 *   in tiles of 256 points its rows share; D is read once.
 *
 * Returns -1 before any launch for a NULL pointer, dim outside [1, meld_smacof_max_dim()], ldD < n, n < 0 and Z == Z_out.  n == 0
 * is a successful no-op; n == 1 stores zeros. */
int meld_smacof_max_dim(void);
int meld_smacof_step(const double* D, int64_t ldD, int n, int dim, const double* Z, double* Z_out, double* row_stress,
                     meld_stream_t stream);

/* ---- Louvain communities of a CSR graph (csrc/louvain.hip; the reference clusters its cells with scanpy's louvain in
 *      comparison/comparison.py, find_n_clusters) --------------------------------------------------------------------------------
 * The graph: rowptr[n + 1] int64, col[nnz] int32 in [0, n), val[nnz] fp64 >= 0, symmetric; an entry (i, i) is the diagonal A_ii.
 * k = A 1, two_m = 1^T A 1.  Labels are int32 in [0, n): community ids are vertex numbers.  Everything is fp64, there are no
 * floating-point atomics, every output is a function of the operands alone.
 *
 * meld_louvain_move: one synchronous round.  For vertex i in community a = label[i], with w_b = the entries A_ij, j != i, of the row
 *   whose column carries label b, added in storage order, and g(b) = w_b two_m - (gamma k[i]) (tot[b] - [b = a] k[i]) (every
 *   operation rounded once): new_label[i] = the allowed b != a of the row with the largest g(b), the lowest id among equals, where
 *   g(b) > g(a); a otherwise.  Allowed: with size[a] == 1, any b with size[b] > 1, and b < a with size[b] == 1; with size[a] > 1,
 *   b < a when round is even, b > a when it is odd.  own[i] = w_a + A_ii, moved[i] = 1 where new_label[i] != a.  stats[0] = the sum
 *   of own, stats[1] = the number of movers: per workgroup in row order (part_sum, part_moved: meld_louvain_move_blocks(n, lanes)
 *   elements each), then partial t, t + 256, ... per thread of one workgroup and a fixed tree.  tot[n], size[n]: the communities'
 *   sums of k and numbers of vertices (meld_louvain_totals).  lanes: 16 or 64 per row (meld_louvain_lanes(n, nnz) picks 16 up to a
 *   mean of 64 entries per row, one trip of a 16-lane group); a row of any length is served by either (quadratic in its length).  new_label must not be label.
 * meld_louvain_totals: keys_sorted[n] = label << 32 | vertex ascending (meld_sort_pairs_u64_f64), vals_sorted[n] the vertices' k in
 *   that order.  tot[b] = the sum over community b (element l, l + 64, ... of the segment per lane in order, then a xor butterfly; a
 *   segment of one element is that element), size[b] its length, minm[b] its smallest vertex; 0 / 0 / -1 for a label in
 *   [0, n_labels) that does not occur.
 * meld_louvain_heads: flags[v] = 1 where minm[label[v]] == v (v is the smallest member of its community), else 0.
 * meld_louvain_renumber: with rank[n + 1] the exclusive scan of flags, out[v] = rank[minm[label[v]]]: communities numbered by their
 *   smallest member; sizes[out[v]] = size[label[v]] (int64, one store per community).
 * meld_louvain_contract_keys: keys[e] = label[row of e] << 32 | label[col[e]] for every stored entry: sorted with the values next
 *   to them (meld_sort_pairs_u64_f64), summed by key (meld_coo_merge) and assembled (meld_csr_from_keys) they are C^T A C.
 * meld_modularity_terms: own[i] = the entries of row i whose column carries label[i] (the diagonal included), k[i] = all of them:
 *   entry s, s + 16, ... per lane of 16 in order, then a xor butterfly.
 *
 * Each entry returns -1 before any launch for a NULL required pointer (a graph without entries passes any address for col and
 * val), n outside [1, 2^31), lanes other than 16 and 64, a negative round, two_m or gamma not finite, gamma <= 0,
 * new_label == label. */
int meld_louvain_lanes(int64_t n, int64_t nnz);
int64_t meld_louvain_move_blocks(int64_t n, int lanes);
int meld_louvain_move(const int64_t* rowptr, const int32_t* col, const double* val, int64_t n, const int32_t* label, const double* k,
                      const double* tot, const int32_t* size, double two_m, double gamma, int round, int lanes, int32_t* new_label,
                      double* own, int32_t* moved, double* part_sum, int32_t* part_moved, double* stats, meld_stream_t stream);
int meld_louvain_totals(const uint64_t* keys_sorted, const double* vals_sorted, int64_t n, int64_t n_labels, double* tot,
                        int32_t* size, int32_t* minm, meld_stream_t stream);
int meld_louvain_heads(const int32_t* label, const int32_t* minm, int64_t n, int32_t* flags, meld_stream_t stream);
int meld_louvain_renumber(const int32_t* label, const int32_t* minm, const int64_t* rank, const int32_t* size, int64_t n,
                          int32_t* out, int64_t* sizes, meld_stream_t stream);
int meld_louvain_contract_keys(const int64_t* rowptr, const int32_t* col, int64_t n, const int32_t* label, uint64_t* keys,
                               meld_stream_t stream);
int meld_modularity_terms(const int64_t* rowptr, const int32_t* col, const double* val, int64_t n, const int32_t* label, double* own,
                          double* k, meld_stream_t stream);

/* ---- Leiden communities: the refinement of a level's move partition (csrc/leiden.hip; the reference clusters its cells with
 *      scanpy's leiden in comparison/comparison.py, find_n_clusters) ------------------------------------------------------------
 * The graph, k and two_m as for Louvain.  comm[n]: the communities of the move partition, int32 in [0, n), tot_comm[n] their sums of
 * k addressed by label; sub[n]: the sub-communities, int32 in [0, n) (ids are vertex numbers, a label that occurs contains the
 * vertex of that number), tot[n] and size[n] their sums of k and sizes (meld_louvain_totals for both).
 *
 * meld_leiden_propose: prop[v] = -1 unless size[sub[v]] == 1 and inC_v two_m >= (gamma k[v]) (tot_comm[comm[v]] - k[v]), inC_v the
 *   entries A_vj, j != v, comm[j] == comm[v], added in storage order.  Otherwise, over those entries, w_t = the ones with
 *   sub[j] == t added in storage order, g(t) = w_t two_m - (gamma k[v]) tot[t] (every operation rounded once), and t is allowed if
 *   size[t] >= 2 or pri(t, round) < pri(v, round) with pri(x, r): x += r 0x9E3779B9; twice x = (x ^ x >> 16) 0x45D9F3B; x ^= x >> 16
 *   (mod 2^32, unsigned).  prop[v] = the allowed t != sub[v] with the largest g(t) > 0, the lowest t among equals; -1 if none.
 *   lanes: 16 or 64 per row (meld_louvain_lanes); a row of any length is served by either.
 * meld_leiden_commit: new_sub[v] = prop[v] where prop[v] is in [0, n) and (size[prop[v]] >= 2 or prop[prop[v]] < 0), sub[v]
 *   elsewhere.  movers[0] = how many moved: per workgroup (part_moved: meld_leiden_commit_blocks(n) elements) by a fixed tree,
 *   then the workgroups' counts by one workgroup in a fixed order.
 *
 * Each entry returns -1 before any launch for a NULL required pointer (a graph without entries passes any address for col and
 * val), n outside [1, 2^31), lanes other than 16 and 64, a negative round, two_m or gamma not finite, gamma <= 0, and an output
 * that is one of the int32 inputs. */
int64_t meld_leiden_commit_blocks(int64_t n);
int meld_leiden_propose(const int64_t* rowptr, const int32_t* col, const double* val, int64_t n, const int32_t* comm,
                        const int32_t* sub, const double* k, const double* tot, const int32_t* size, const double* tot_comm,
                        double two_m, double gamma, int round, int lanes, int32_t* prop, meld_stream_t stream);
int meld_leiden_commit(const int32_t* sub, const int32_t* prop, const int32_t* size, int64_t n, int32_t* new_sub, int32_t* part_moved,
                       int64_t* movers, meld_stream_t stream);

/* ---- next#1: normalize_densities (meld/utils.py:35-47) ------------------------------------ */
/* out[i,:] = in[i,:] / sum_j |in[i,j]|  (rows of zeros are copied unchanged, as sklearn does) */
int meld_normalize_rows_l1(const double* in, double* out, int64_t n_rows, int p, meld_stream_t stream);

/* ---- sparse input: truncated SVD of a cell-by-gene CSR matrix (csr_dense.hip; replaces [UPSTREAM graphtools
 *      Data._reduce_data -> sklearn TruncatedSVD] on scipy.sparse input, reached from meld/meld.py:273) --------------------
 * The CSR operand: rowptr[n_rows + 1] int64 (rowptr[0] = 0), col[nnz] int32, val[nnz] fp32 (val_f32 = 1, widened in the
 * kernel) or fp64; columns of a row need not be sorted, but the summation order is their storage order.
 *
 * meld_csr_spmm_f64: Y[i][0:r] = sum_j val[j] B[col[j]][0:r] for every row i, B[*][ldb] and Y[n_rows][ldy] row-major fp64.
 *   The sum runs in fp64 in storage order inside a segment of MELD_CSR_SEG entries of a row; a row of more entries is
 *   split into segments whose partial sums (partial[part_off[i] + s][r]) are added in segment order by a second pass.
 *   No atomics: the result is a function of the operands alone.  The work plan (built by the caller from rowptr):
 *     unit_row[n_units]: the row of each unit (a unit = one segment; max(1, ceil(len / MELD_CSR_SEG)) units per row,
 *                        consecutive, in segment order); unit_off[n_rows]: the first unit of each row;
 *     part_off[n_rows]: the first partial slot of each row of more than one segment; split_rows[n_split_rows]: those rows.
 *   Every col[j] must be < the number of rows of B (checked by the caller). */
#define MELD_CSR_SEG 1024
int meld_csr_seg_length(void);
int meld_csr_spmm_f64(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_rows,
                      const int32_t* unit_row, const int64_t* unit_off, int64_t n_units, const int64_t* part_off,
                      const int32_t* split_rows, int64_t n_split_rows, double* partial, const double* B, int64_t ldb,
                      int r, double* Y, int64_t ldy, meld_stream_t stream);
/* keys[j] = col[j] << 32 | row of entry j, vals[j] = val[j] as fp64: sorted by meld_sort_pairs_u64_f64 and assembled by
 * meld_csr_from_keys they are the CSR of the transpose, rows ascending inside each column (n_rows < 2^31). */
int meld_csr_transpose_keys(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_rows,
                            uint64_t* keys, double* vals, meld_stream_t stream);
/* out[i][0:n_cols] (row stride ldo) = row row_begin + i of the CSR matrix, zeros elsewhere, i < n_rows (no duplicate columns) */
int meld_csr_rows_to_dense_f64(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t row_begin,
                               int64_t n_rows, int64_t n_cols, double* out, int64_t ldo, meld_stream_t stream);

/* ---- rank-sum differential expression on the CSC copy of the data (csrc/ranksum.hip; the reference ends its analyses with
 *      de.test.two_sample(..., test='rank') per gene, notebooks/MELD_thresholding.Tcell.ipynb) ------------------------------------
 * The operand is the CSR of X^T: rowptr[n_genes + 1] int64, col[nnz] int32 cell indices (no cell twice in a gene), val[nnz] fp32
 * (val_f32 = 1, widened exactly) or fp64, finite.  code[n_cells] int32: the class of each cell in [0, k), anything else (-1): the
 * cell takes no part.  ncls[k] int64: the class sizes, m their sum (at most MELD_RANKSUM_MAX_SELECTED: the cube of a tie group's
 * size is taken in int64; every entry that takes m refuses more).  Stored entries equal to zero (+0.0, -0.0) count as zeros.
 *
 * Per gene g, over the m selected cells ranked with mid-ranks (implicit zeros included, negatives below them):
 *   rank2[g * k + c] int64: twice the rank sum of class c;      tie[g] int64: the sum of t^3 - t over all tie groups;
 *   nnz[g * k + c] int32: the selected non-zero entries of class c;      sum[g * k + c] fp64: the sum of the class's values.
 * rank2, tie and nnz are integer arithmetic throughout (integer LDS atomics: any order gives the same bits), the same whichever
 * route computes them.  sum: thread t of 128 adds the entries t, t + 128, ... of the gene in storage order, then a fixed tree over
 * the 128 partial sums; one kernel for every gene.  No floating-point atomics.
 *
 * meld_ranksum_short: the genes genes[n_list] (int32, each of stored length <= meld_ranksum_lds_max(); a longer one is not
 *   computed, its outputs are set to -1): gathered, sorted and scanned in LDS, one workgroup per gene.
 * meld_ranksum_gather: for the genes genes[n_list] of any length, with off[n_list + 1] the exclusive scan of their stored lengths
 *   and total = off[n_list]: keys[e] = the order-preserving 64-bit image of the value (sign bit set for positives, all bits
 *   flipped for negatives), payload[e] = slot << 32 | class for entry e - off[slot] of gene genes[slot]; an entry that takes no
 *   part has the image ~0 and the class 0xFFFFFFFF.
 * meld_sort_pairs_u64_u64: stable radix sort of (u64 key, u64 value) pairs on the key bits [begin_bit, end_bit); temp as for
 *   meld_sort_pairs_u64_f64 (meld_sort_temp_bytes(n); checked).  Sorting the gathered pairs by image and then, payload as key, on
 *   the slot bits [32, 64) leaves every gene's segment at off[slot], ascending by value, the dead entries last.
 * meld_ranksum_scan: rank2, tie and nnz of the genes genes[n_list] from those sorted arrays, one workgroup per gene.
 * meld_ranksum_sums: sum of every gene.
 *
 * Each entry returns -1 before any launch, naming itself, for a NULL required pointer, val_f32 outside {0, 1}, n_genes or n_cells
 * outside [1, 2^31), k outside [1, meld_ranksum_max_classes()], m outside [0, MELD_RANKSUM_MAX_SELECTED], n_list outside its range,
 * total outside [0, 2^38), a sort whose temp is too small.  Cell indices and classes are range-checked inside the kernels before
 * they address anything. */
#define MELD_RANKSUM_LDS_MAX 4096
#define MELD_RANKSUM_MAX_CLASSES 64
#define MELD_RANKSUM_MAX_SELECTED 2097151ll
int meld_ranksum_lds_max(void);
int meld_ranksum_max_classes(void);
int64_t meld_ranksum_max_selected(void);
int meld_ranksum_sums(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_genes, const int32_t* code,
                      int64_t n_cells, int k, double* sum, meld_stream_t stream);
int meld_ranksum_short(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_genes, const int32_t* genes,
                       int64_t n_list, const int32_t* code, int64_t n_cells, int k, const int64_t* ncls, int64_t m, int64_t* rank2,
                       int64_t* tie, int32_t* nnz, meld_stream_t stream);
int meld_ranksum_gather(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_genes, const int32_t* genes,
                        const int64_t* off, int64_t n_list, int64_t total, const int32_t* code, int64_t n_cells, int k, uint64_t* keys,
                        uint64_t* payload, meld_stream_t stream);
int meld_sort_pairs_u64_u64(const uint64_t* keys_in, uint64_t* keys_out, const uint64_t* vals_in, uint64_t* vals_out, int64_t n,
                            int begin_bit, int end_bit, void* temp, size_t temp_bytes, meld_stream_t stream);
int meld_ranksum_scan(const uint64_t* keys_sorted, const uint64_t* payload_sorted, const int32_t* genes, const int64_t* off,
                      int64_t n_list, int64_t n_genes, int k, const int64_t* ncls, int64_t m, int64_t* rank2, int64_t* tie, int32_t* nnz,
                      meld_stream_t stream);

/* ---- preprocessing of the counts on the device CSR (csrc/preprocess.hip; the reference's notebooks call scprep.filter.
 *      filter_library_size / filter_rare_genes / filter_gene_set_expression, scprep.normalize.library_size_normalize and
 *      scprep.transform.sqrt in front of meld.MELD()) -----------------------------------------------------------------------------------
 * The operand is the CSR of the cells-by-genes matrix: rowptr[n_rows + 1] int64, col[nnz] int32 in [0, n_cols), val[nnz] fp32
 * (val_f32 = 1, widened exactly) or fp64; stored zeros allowed, rows of any length, nnz beyond 2^31.  All arithmetic is fp64, no
 * floating-point atomics: every output is a function of the operands alone.  A column index outside [0, n_cols) is skipped by every
 * kernel before it addresses anything.
 *
 * meld_prep_row_stats: per row i over its COUNTED entries -- all of them, or with col_mask (uint8 [n_cols]) those with
 *   col_mask[col] != 0 --: sum[i] = the sum of v, abs_sum[i] = the sum of |v|, count[i] (int32) = the number with v > cutoff.
 *   Order of the sums: a wave per row; the counted entries numbered 0, 1, 2 ... in storage order, lane l adds the entries l, l + 64,
 *   ... in that order, then a fixed tree over the 64 lanes: a function of the number of counted entries alone, so the masked sums
 *   of a row have the bits of the plain sums of the row meld_prep_select_fill leaves when it drops the same columns.
 * meld_prep_col_counts: count[c] (int32 [n_cols], ZEROED BY THE CALLER) += the number of entries of column c with v > cutoff in
 *   the rows with row_keep[row] != 0 (uint8 [n_rows]; NULL: every row).  A workgroup walks a contiguous range of rows, counts into a
 *   panel of MELD_PREP_PANEL_COLS int32 counters in LDS (integer LDS atomics) and adds the non-zero ones to count with integer
 *   global atomics; a matrix of more columns takes one launch per panel, entries outside the panel are skipped.
 * meld_prep_select_count / meld_prep_select_fill: the matrix of the rows rows[n_keep] (int32, ascending: new row -> old row) and the
 *   columns with col_map[c] >= 0 (int32 [n_cols]: old column -> new column, the kept columns numbered ascending; NULL: every
 *   column keeps its index).  count: counts[i] (int32 [n_keep]) = the kept entries of new row i; the caller scans them
 *   (meld_exclusive_scan_i32_i64) into out_rowptr[n_keep + 1].  fill: out_col / out_val [out_rowptr[n_keep]] in storage order (a
 *   stored zero that survives the column selection stays stored; a row never writes past out_rowptr[i + 1]).  The value, in this
 *   order of operations:  w = scale ? (v / scale[i]) * rescale : v  (scale fp64 [n_keep] or NULL; a row with scale[i] == 0 keeps v,
 *   rescale still multiplies: sklearn's normalize), then out_val = f(w) for transform MELD_PREP_IDENTITY w, _SQRT sqrt(w), _LOG
 *   log(w + 1), _LOG2 log2(w + 1), _LOG10 log10(w + 1), _ARCSINH asinh(w / cofactor).  out_val_norm (NULL: not wanted) receives w.
 *
 * meld_prep_gene_moments: per-gene count, mean and variance over the kept cells, on the CSR of X^T (one row per gene, as the
 *   rank-sum entries take it: rowptr[n_genes + 1], col = cell indices in [0, n_cells)).  row_keep (uint8 [n_cells]; NULL: every
 *   cell), n_kept = the number of kept cells (the caller knows it), gene_mask (uint8 [n_genes]; NULL: every gene), ddof 0 or 1.
 *   The value of a stored entry v of a kept cell i is the rewrite's, same operations in the same order:  w = row_scale ?
 *   (v / row_scale[i]) * rescale : v  (row_scale fp64 [n_cells], indexed by the INPUT's cell; a cell with row_scale[i] == 0 keeps v,
 *   rescale still multiplies), x = f(w).  Implicit zeros and the entries of cells that are not kept contribute nothing (f(0) = 0).
 *     count[g] (int32) = the stored entries of kept cells;  mean[g] = (sum of x) / n_kept;
 *     var[g] = (sum over those entries of (x - mean)^2 + (n_kept - count) * mean^2) / (n_kept - ddof)   -- two passes over the gene.
 *   A gene with gene_mask[g] == 0 gets count = -1, mean = var = 0 and its entries are not read.
 *   Order of the sums: number the gene's STORED entries 0, 1, 2 ... (an entry that is not counted stands in its place as +0.0).  A
 *   gene of at most MELD_PREP_MOMENTS_WAVE_MAX stored entries: lane l of one wave adds the entries l, l + 64, ... in that order,
 *   then a fixed butterfly over the 64 lanes.  A longer gene: thread t of a workgroup of MELD_PREP_MOMENTS_THREADS adds the entries
 *   t, t + 1024, ... in that order, the same butterfly in each of the 16 waves, then a fixed pairwise tree over the 16 wave sums.
 *   Either way a function of the gene's stored length alone: not of the grid, not of what else ran.  Two calls give the same bits.
 *
 * Each entry returns -1 before any launch, naming itself, for a NULL required pointer, val_f32 outside {0, 1}, n_rows, n_cols,
 * n_genes, n_cells or n_keep outside [1, 2^31), a transform outside [0, 5], a cofactor <= 0 with MELD_PREP_ARCSINH; the moments
 * also for ddof outside {0, 1}, n_kept < 1 and n_kept - ddof < 1. */
#define MELD_PREP_PANEL_COLS 32768
#define MELD_PREP_MOMENTS_WAVE_MAX 2048 /* stored entries of a gene up to which one wave takes it; above, a workgroup */
#define MELD_PREP_MOMENTS_THREADS 1024
#define MELD_PREP_IDENTITY 0
#define MELD_PREP_SQRT 1
#define MELD_PREP_LOG 2
#define MELD_PREP_LOG2 3
#define MELD_PREP_LOG10 4
#define MELD_PREP_ARCSINH 5
int meld_prep_panel_cols(void);
int meld_prep_row_stats(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_rows, int64_t n_cols,
                        const uint8_t* col_mask, double cutoff, double* sum, double* abs_sum, int32_t* count, meld_stream_t stream);
int meld_prep_col_counts(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_rows, int64_t n_cols,
                         const uint8_t* row_keep, double cutoff, int32_t* count, meld_stream_t stream);
int meld_prep_select_count(const int64_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_cols, const int32_t* rows,
                           int64_t n_keep, const int32_t* col_map, int32_t* counts, meld_stream_t stream);
int meld_prep_select_fill(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_rows, int64_t n_cols,
                          const int32_t* rows, int64_t n_keep, const int32_t* col_map, const double* scale, double rescale,
                          int transform, double cofactor, const int64_t* out_rowptr, int32_t* out_col, double* out_val,
                          double* out_val_norm, meld_stream_t stream);
int meld_prep_gene_moments(const int64_t* rowptr, const int32_t* col, const void* val, int val_f32, int64_t n_genes, int64_t n_cells,
                           const uint8_t* row_keep, const double* row_scale, double rescale, int transform, double cofactor,
                           const uint8_t* gene_mask, int64_t n_kept, int ddof, int32_t* count, double* mean, double* var,
                           meld_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MELD_HIP_H */
