"""The route of the kNN build, decided before anything is allocated.

``plan_knn_search`` is a pure function of the shape of the call, the search options and the library's geometry (host-only queries
of libmeld_hip.so, no device needed): which search back end runs, whether the cells move to their principal frame, which start
thresholds, pruning table, step lists and dispatch order the first pass gets, whether the partial test runs as a pass of its own,
and whether uncertified rows are searched again at full precision.  ``HipOps.directed_kernel_coo`` follows the plan; what
depends on the data (the frame's variance test, flagged-row counts, bucket overflow, free memory) is decided there.

The ``MELD_KNN_*`` / ``MELD_KNN16_*`` switches the Python side reads are read here and nowhere else.
"""
from __future__ import annotations

import ctypes
import dataclasses
from dataclasses import dataclass
from typing import Optional

from ._lib import check
from ._options import opt


@dataclass(frozen=True)
class SearchOptions:
    """Options of the search (``HipOps`` attributes of the same names).  Every route gives the same graph."""

    # candidate-search kernel: "f16x3" (split-fp16 MFMA) or "f32" (fp32 MFMA)
    search: str = "f16x3"
    # precision of the f16x3 first pass on the coordinate K blocks: 1 = fp16 hi parts only (half the MFMAs, error bound
    # 2^-9 max|x|^2), 3 = full hi/lo split (2^-16); rows the bound cannot certify go through the re-search or the exact sweep
    nprod: int = 1
    # exact tile pruning (bounds table or step lists); the unpruned pass of bench.py --full switches it off
    prune: bool = True
    # rows cut at the kernel radius their (knn+1)-th neighbour so far implies; the final thresholds are published
    radius_cut: bool = True
    # start thresholds of the first pass from every row's own block (meld_knn16_seed_thresholds_mfma)
    seed: bool = True
    # per-query test of the pruning table against those seeds (meld_knn16_bounds, thr_seed)
    seeded_bounds: bool = True
    # pruned search: query blocks dispatched by decreasing work
    block_order: bool = True
    # the search runs in the cells' principal frame where that concentrates the distances in the leading coordinates ...
    rotate: bool = True
    # ... from this many cells on: the frame costs ~0.9 ms whatever the size (a read-back and a 50 x 50 eigenproblem on the host
    # among it) and pays from ~250k cells (200k: 10.0 vs 9.8 ms per step without it; 350k: 14.6 vs 15.4; 500k: 21.0 vs 22.5)
    rotate_min_cells: int = 262144

    @classmethod
    def from_env(cls, search=None, prune=None, nprod=None):
        out = cls(search=search or opt("MELD_KNN_SEARCH", "f16x3"), nprod=1 if nprod is None else int(nprod),
                  prune=(opt("MELD_KNN_PRUNE", "1") != "0") if prune is None else bool(prune),
                  rotate=opt("MELD_KNN_ROTATE", "1") != "0", rotate_min_cells=int(opt("MELD_KNN_ROTATE_MIN", "262144")))
        if out.search not in ("f16x3", "f32"):
            raise ValueError("unknown search kernel {!r}".format(out.search))
        return out


@dataclass(frozen=True)
class KnnPlan:
    search: str              # "f16x3" (split-fp16 MFMA), "f32" (fp32 MFMA) or "wide" (library GEMMs, d > 141)
    nprod: int               # products of the f16x3 first pass (1 or 3)
    frame: bool              # cells in their principal frame (without_frame() where principal_frame declines)
    radius_cut: bool         # rows cut at the kernel radius, final thresholds published
    prune: bool              # tiles pruned, by a bounds table or by step lists
    seed: str                # start thresholds: "none", "mfma" (each row's own block) or "bandwidth" (the given radius)
    knn_cut: int             # the neighbour whose distance cuts a row (0: the radius is given, nothing is cut)
    bounds: str              # pruning table: "none", "bounds" or "bounds_from_spheres" (tile spheres shared by the ranks)
    seeded_bounds: bool      # the table tested against the start thresholds
    lists: str               # step lists: "none", "direct" (from the cells, no table) or "table"
    block_order: str         # dispatch order of the query blocks by: "none", "lists" (list lengths) or "work" (meld_knn16_block_work)
    main_slices: int         # reference slices of the first pass (few query blocks)
    two_pass: bool           # the partial test as a filter pass of its own (meld_knn16_partial_filter)
    partial_in_search: bool  # the K-block-0 partial test inside the search
    stage2: bool             # uncertified rows searched again with the full hi/lo split
    # the direct step lists take their bounds from K block 0 alone (None: as the route implies, i.e. direct lists in the frame)
    lead_bounds: Optional[bool] = None
    partial_forced: bool = False  # partial_in_search set by MELD_KNN16_EE, not by the frame: without_frame() keeps it
    # queries = all the references, pruned: Rt, Q and the tile spheres from ONE pass over the cells (meld_knn16_prepare_fused)
    # (how the operands are written, not which route the search takes: same bits either way, so two plans that differ in this alone
    # compare equal)
    fused_operands: bool = dataclasses.field(default=False, compare=False)
    # the row passes behind the search: "off" (finish, refinement and emit as three kernels), "emit" (the refinement sends the
    # kept entries of complete rows straight to the row buckets, meld_knn_refine_emit) or "sort+emit" (it also takes the rows raw
    # from the search and ranks them in registers, meld_knn_refine_sort_emit); same graph bit for bit
    fused_rows: str = dataclasses.field(default="off", compare=False)

    def __post_init__(self):
        if self.lead_bounds is None:
            object.__setattr__(self, "lead_bounds", self.lists == "direct" and self.frame)

    def without_frame(self):
        """The same route with the cells as given (the frame's leading coordinates carry less than half the variance)."""
        return dataclasses.replace(self, frame=False, two_pass=False, lead_bounds=False,
                                   partial_in_search=self.partial_in_search and self.partial_forced)


def search_nprod(nprod, d):
    """Products of the f16x3 first pass.  In very low dimension the neighbours are so close (relative to max|x|^2) that the
    fp16-hi first pass certifies almost nothing (1M x 3: 968k of 1M rows re-searched); there the full split costs next to
    nothing (one K block), so it is used from the start.  Same result either way."""
    return 3 if (nprod == 1 and d <= 6) else nprod


def sphere_layout(lib, N, d):
    """(rows, bytes per row) of the tile-sphere arrays (``meld_knn16_sphere_layout``)."""
    rows, row_bytes = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib.meld_knn16_sphere_layout(N, d, ctypes.byref(rows), ctypes.byref(row_bytes)), "meld_knn16_sphere_layout")
    return int(rows.value), int(row_bytes.value)


def bucket_route(lib, N, q_begin, q_count, ksel, *, cross, assemble, free_bytes):
    """Whether the kept entries go straight into the row buckets of the symmetrisation (``HipOps._emit``), as far as that is known
    before the search: a single GPU that holds every row and is asked for the assembled rows, the bucket assembly selected, a
    candidate list that fits a bucket, and a quarter of the free memory (``free_bytes``) enough for the buckets."""
    if not assemble or cross or q_begin != 0 or q_count != N:
        return False
    if opt("MELD_ASSEMBLE", "bucket") != "bucket" or opt("MELD_ASSEMBLE_FUSED", "1") == "0":
        return False
    B = int(lib.meld_csr_bucket_slots())
    return ksel <= B and q_count * B * 12 <= int(free_bytes) // 4


def plan_fused_rows(lib, N, d, q_begin, q_count, ksel, *, search, cross=False, world=1, assemble=False, free_bytes=0, x_aligned=True,
                    raw_rows=False):
    """"emit" where the refinement may send its rows straight to the buckets (``meld_knn_refine_emit``), else "off": the bucket
    route, the split-fp16 search, the four-chain refinement (even d <= 256, rows 16-byte aligned) and a list of at most two entries
    per lane.  "sort+emit" where the search can also leave its rows raw (``raw_rows``: the list-driven first pass in one slice --
    sliced searches are merged into finished rows).  MELD_ROWS_FUSED (development) = 0: always the three kernels, a: "emit" at most."""
    if search != "f16x3" or world != 1 or not bucket_route(lib, N, q_begin, q_count, ksel, cross=cross, assemble=assemble, free_bytes=free_bytes):
        return "off"
    if d % 2 != 0 or d > 256 or not x_aligned or ksel > 128 or ksel > int(lib.meld_csr_bucket_slots()):
        return "off"
    want = opt("MELD_ROWS_FUSED", "b")
    if want == "0":
        return "off"
    return "sort+emit" if raw_rows and want != "a" else "emit"


def plan_knn_search(lib, N, d, q_begin, q_count, knn, ksel, *, options, cross=False, bandwidth=False, world=1, resident=0, assemble=False,
                    free_bytes=0, x_aligned=True):
    """Route of ``directed_kernel_coo`` for rows [q_begin, q_begin + q_count) of N cells in d dimensions.

    ``options``: a ``SearchOptions`` (or ``HipOps``); ``cross``: a search between two point sets (``n_refs``); ``bandwidth``: the
    kernel radius is given; ``world``: ranks that share the tile spheres (1: none); ``resident``: workgroups of the search
    resident on the device at once (``meld_knn16_resident_blocks(d, search_nprod(nprod, d))``, the one query that needs a device);
    ``assemble`` / ``free_bytes`` / ``x_aligned``: the caller wants the assembled rows, the device's free memory, the cells are
    16-byte aligned -- what ``plan_fused_rows`` decides the row passes behind the search on."""
    search = options.search
    if search == "f16x3" and lib.meld_knn16_kblocks(d) < 0:
        search = "wide"  # d beyond the instantiated MFMA kernels (d > 141)
    if cross and search != "f16x3":
        raise NotImplementedError("the search between two point sets runs on the split-fp16 MFMA kernel only (d <= 141)")
    if search != "f16x3":
        return KnnPlan(search, options.nprod, False, False, False, "none", knn, "none", False, "none", "none", 1, False, False, False)
    nprod = search_nprod(options.nprod, d)
    TS, BQ = lib.meld_knn16_tile_refs(), lib.meld_knn16_block_queries()
    n_blocks, n_tiles = -(-q_count // BQ), -(-N // TS)
    radius_cut = bool(options.radius_cut) and knn < ksel
    frame = bool(options.rotate and lib.meld_knn16_split_dims(d) > 0 and nprod == 1 and not cross and options.prune and options.seed
                 and N >= max(16384, options.rotate_min_cells) and q_begin % BQ == 0 and not bandwidth)
    prune = bool(options.prune) and q_begin % TS == 0 and N >= 16384 and not cross
    seed = "none"
    if bandwidth and radius_cut:
        seed = "bandwidth"  # every row's radius is known: the thresholds start there and the search cuts nothing itself
    elif options.seed and radius_cut and q_begin % BQ == 0 and not cross:
        seed = "mfma"
    bounds, lists, block_order, seeded_bounds, main_slices = "none", "none", "none", False, 1
    if prune:
        seeded_bounds = seed != "none" and bool(options.seeded_bounds)
        shared = world > 1 and sphere_layout(lib, N, d)[0] % world == 0
        want_lists = seed != "none" and radius_cut and nprod == 1
        if want_lists and seeded_bounds and not shared and q_begin == 0 and q_count == N and opt("MELD_KNN_LIST_DIRECT", "1") != "0":
            lists = "direct"  # queries = all the cells: the lists come straight from the cells, no table
        else:
            bounds = "bounds_from_spheres" if shared else "bounds"
            lists = "table" if want_lists else "none"
        if options.block_order and n_blocks > 1:
            block_order = "lists" if lists != "none" else "work"
        # Few query blocks (a row shard, a mid-sized data set): with pruning the work of a block varies 12-fold and a launch that
        # fills the chip less than twice over ends when its heaviest block does.  The references are then cut into slices --
        # blocks x slices workgroups, each with its own candidate rows, merged afterwards -- so that the heavy blocks are shared
        # out (more slices cost more in merging than they balance).
        if radius_cut and resident > 0 and n_blocks < 2 * resident:
            main_slices = int(max(1, min(4, lib.meld_knn16_max_slices(ksel), -(-2 * resident // n_blocks), n_tiles // 64)))
    # The partial test (K block 0 first, the other blocks only where it passes) pays in the principal frame, whose leading
    # coordinates carry the distances.  MELD_KNN16_EE=0 / 1 forces it off / on inside the search, frame or not, with no filter pass.
    ee = opt("MELD_KNN16_EE")
    partial = frame if ee is None else ee != "0"
    # ... as a pass of its own: every listed (wave, tile) pair is tested on K block 0 and the lists are thinned in place before the
    # search.  Sliced launches (few query blocks) keep the one-kernel form: a workgroup of the filter walks its block's whole list.
    # MELD_KNN_TWO_PHASE=0: always the one-kernel form, =2: also when sliced.
    two = opt("MELD_KNN_TWO_PHASE", "1")
    two_pass = lists != "none" and frame and (main_slices == 1 or two == "2") and two != "0" and ee is None
    # the direct lists in the frame take their bounds from K block 0 alone (lower bounds all the same, for a quarter of the tile
    # stream); MELD_KNN16_LEAD_BOUNDS=0: from all K blocks
    lead_bounds = lists == "direct" and frame and opt("MELD_KNN16_LEAD_BOUNDS", "1") != "0"
    # One pass over the cells for both operand layouts and the tile spheres where the queries are all the references and the
    # spheres are wanted here (pruned, not shared between ranks).  MELD_KNN_FUSED_OPERANDS=0: the three separate passes (same bits).
    fused = prune and bounds != "bounds_from_spheres" and q_begin == 0 and q_count == N and opt("MELD_KNN_FUSED_OPERANDS", "1") != "0"
    fused_rows = plan_fused_rows(lib, N, d, q_begin, q_count, ksel, search=search, cross=cross, world=world, assemble=assemble,
                                 free_bytes=free_bytes, x_aligned=x_aligned, raw_rows=lists != "none" and main_slices == 1)
    return KnnPlan(search, nprod, frame, radius_cut, prune, seed, 0 if seed == "bandwidth" else knn, bounds, seeded_bounds, lists,
                   block_order, main_slices, two_pass, partial, nprod == 1, lead_bounds, ee is not None, fused, fused_rows)
