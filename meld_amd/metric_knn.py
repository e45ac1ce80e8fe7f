"""Sparse kNN graphs under the L1 and L-infinity metrics on the GPU (csrc/metric_knn.hip).

``distance="manhattan" | "cityblock" | "l1" | "chebyshev"`` [UPSTREAM graphtools kNNGraph(distance=...) -> sklearn
``NearestNeighbors(metric=...)``]: no function of the euclidean distance of transformed rows, so the euclidean search does not
apply.  Up to ``dense.DENSE_MAX_N`` cells ``dense.build_dense_knn_graph`` builds them; beyond it this module does, with an exact
fp64 candidate search of its own (tile boxes, near-first visiting order, box-bound pruning), an exact refinement and a radius
sweep for the rows whose candidate list does not reach past the kernel radius.  Everything downstream of the candidate lists --
the COO emit, the symmetrisation (``kernel_symm`` / ``theta``), anisotropy and degrees -- is the euclidean builder's.

New cells (``cross_kernel_rows``): the same search between two point sets -- the fitted cells in their
locality order with their tile boxes cached on the graph's extension state, the new cells sorted by their nearest tile -- for the
graphs of both routes.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from ._device_ops import scan_i32, stream
from ._lib import check, ptr
from ._options import opt
from .dense import DENSE_MAX_N
from .graph import DeviceGraph, HipOps, _EventSpan, _Timer, default_ksel, resolve_graph_params, symm_code

__all__ = ["build_metric_knn_graph", "cross_kernel_rows", "metric_route", "METRICS", "MAX_KNN"]

# metric name -> the library's code (include/meld_hip.h: MELD_METRIC_L1 / MELD_METRIC_LINF)
METRICS = {"manhattan": 1, "cityblock": 1, "l1": 1, "chebyshev": 2}
MAX_KNN = 126  # the candidate lists hold 128 entries, as the euclidean search's


def metric_route(N, d, knn, decay, thresh, opts=None):
    """Which builder serves ``MELD(distance=<an L1 / L-inf metric>)``: "dense" (``dense.build_dense_knn_graph``, which refuses
    N > DENSE_MAX_N as it always has) or "metric_knn" (``build_metric_knn_graph``).  Raises NotImplementedError for the options
    neither builds: ``sample_idx``, ``bandwidth``, ``bandwidth_scale``, ``knn_max``, and the dense "exact" graph of thresh=0."""
    opts = opts or {}
    if any(opts.get(k) is not None for k in ("sample_idx", "bandwidth", "bandwidth_scale", "knn_max")) or (thresh == 0 and decay is not None):
        raise NotImplementedError("distance is implemented for the plain alpha-decay / unweighted kNN graph only with this metric")
    if N > DENSE_MAX_N and min(int(knn), N - 2) <= MAX_KNN and d <= 256 and thresh > 0:
        return "metric_knn"
    return "dense"


def build_metric_knn_graph(X, knn, decay, thresh, anisotropy, metric, kernel_symm="+", theta=None, reorder=True, ksel=None, profile=False,
                           ops=None):
    """Data [N, d <= 256] (CUDA fp64) -> DeviceGraph of the alpha-decay kernel under ``metric`` ([UPSTREAM graphtools
    ``kNNGraph(distance=metric)``]): bw_i = (knn+1)-th smallest distance of row i, self counted, max(bw, eps); K_ij = exp(-(d_ij / bw_i)^decay)
    wherever that is >= thresh; ``decay=None``: connectivity of the cells with d <= bw.  Then ``kernel_symm`` / ``theta``,
    anisotropy, zero diagonal and degrees, as ``graph.build_knn_graph`` assembles them.  The graph carries ``perm`` (the cells'
    locality order) as that builder's does."""
    if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float64 and X.dim() == 2):
        raise TypeError("build_metric_knn_graph expects a CUDA float64 tensor [N, d]")
    metric = str(metric).lower()
    if metric not in METRICS:
        raise ValueError("metric {!r} is not one of {}".format(metric, sorted(METRICS)))
    X = X.contiguous()
    N, d = int(X.shape[0]), int(X.shape[1])
    if d > 256:
        raise NotImplementedError("distance={!r} beyond the dense route is implemented for d <= 256 (got d = {})".format(metric, d))
    if thresh is None or not thresh > 0:
        raise NotImplementedError("distance={!r} beyond the dense route needs thresh > 0".format(metric))
    if min(int(knn), N - 2) > MAX_KNN:
        raise NotImplementedError("knn={} beyond the {} the candidate lists hold".format(knn, MAX_KNN))
    decay = float("inf") if decay is None else float(decay)
    knn, thresh, ksel = resolve_graph_params(N, knn, thresh, ksel)
    symm = symm_code(kernel_symm, theta)
    ops = ops if ops is not None else HipOps(X.device)
    lib, st, dev = ops.lib, stream(), X.device
    code = METRICS[metric]
    prune = opt("MELD_METRIC_PRUNE", "1") != "0"  # (development switch: the unpruned search for A-B comparisons)
    tm = _Timer(profile)

    perm = None
    if reorder:
        from .reorder import locality_permutation

        tm.start()
        perm = locality_permutation(X)
        if perm is not None:
            X = ops.gather_rows(X, perm)
        tm.stop("reorder")

    tm.start()
    T = int(lib.meld_metric_tile_rows())
    n_tiles = (N + T - 1) // T
    with _EventSpan("metric_knn_topk", N=N, d=d, metric=metric):
        box_lo = torch.empty(n_tiles * d, dtype=torch.float64, device=dev)
        box_hi = torch.empty(n_tiles * d, dtype=torch.float64, device=dev)
        check(lib.meld_metric_tile_boxes(ptr(X), N, d, ptr(box_lo), ptr(box_hi), st), "meld_metric_tile_boxes")
        tm.stop("tile_boxes")
        heap_d = torch.empty(ksel * n_tiles * T, dtype=torch.float64, device=dev)
        heap_i = torch.empty(ksel * n_tiles * T, dtype=torch.int32, device=dev)
        cand_idx = torch.empty(N * ksel, dtype=torch.int32, device=dev)
        cand_d = torch.empty(N * ksel, dtype=torch.float64, device=dev)
        cand_cnt = torch.empty(N, dtype=torch.int32, device=dev)
        tiles_done = torch.zeros(1, dtype=torch.int64, device=dev)
        check(lib.meld_metric_topk(ptr(X), N, d, code, ksel, ptr(box_lo), ptr(box_hi), int(prune), ptr(heap_d), ptr(heap_i), ptr(cand_idx),
                                   ptr(cand_d), ptr(cand_cnt), ptr(tiles_done), st), "meld_metric_topk")
        del heap_d, heap_i, box_lo, box_hi
    tm.stop("knn_topk")

    r = SimpleNamespace(cands=SimpleNamespace(idx=cand_idx, cnt=cand_cnt, cap=ksel))
    r.bw = torch.empty(N, dtype=torch.float64, device=dev)
    r.cand_val = torch.empty(N * ksel, dtype=torch.float64, device=dev)
    r.keep_cnt = torch.empty(N, dtype=torch.int32, device=dev)
    r.flag_rows = torch.empty(N, dtype=torch.int32, device=dev)
    n_flag = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib.meld_metric_refine(ptr(cand_idx), ptr(cand_d), ptr(cand_cnt), N, ksel, knn, decay, thresh, ptr(r.bw), ptr(r.cand_val),
                                 ptr(r.keep_cnt), ptr(r.flag_rows), ptr(n_flag), st), "meld_metric_refine")
    del cand_d
    r.keep_off = scan_i32(r.keep_cnt)
    n_flag_h, m_main, done_h = torch.stack([n_flag[0].to(torch.int64), r.keep_off[N], tiles_done[0]]).tolist()  # (one read-back)
    r.n_flag, r.m_main = int(n_flag_h), int(m_main)
    tm.stop("refine")

    s = _radius_sweep(lib, st, X, N, d, code, r, decay, thresh)
    tm.stop("radius_exact")

    a = SimpleNamespace(X=X, N=N, NR=N, q_begin=0, q_count=N, cross=False, tm=tm)
    keys, vals, assembled = ops._emit(a, r, s, ksel, True, symm)
    if r.m_main + s.fb_total == 0:
        raise ValueError("the kernel has no off-diagonal entries; cannot build a graph")
    tm.start()
    ksum = None
    if assembled is not None:  # (the kept candidates went straight into the row buckets)
        rowptr, col, val = assembled[:3]
        ksum = assembled[3] if len(assembled) > 3 else None
    else:
        rowptr, col, val = ops.assemble_rows(keys, vals, 0, N, N, symm=symm)
    del keys, vals
    tm.stop("symmetrize")
    if ksum is None:
        ksum = ops.row_sums(rowptr, val, N, 1.0)
    dw = ops.anisotropy_degrees(rowptr, col, val, N, ksum, 0, anisotropy)
    tm.stop("anisotropy_degree")

    nnz = int(col.shape[0])
    pairs = n_tiles * n_tiles
    info = dict(N=N, d=d, knn=knn, ksel=int(ksel), metric=metric, route="metric_knn", prune=bool(prune), n_flagged_rows=r.n_flag,
                tiles_done=int(done_h), tile_skip_fraction=1.0 - int(done_h) / pairs, nnz_directed=r.m_main + s.fb_total, nnz=nnz,
                mean_degree=nnz / N, stage_seconds=dict(tm.t), assemble=getattr(ops, "last_assemble", None))
    G = DeviceGraph(rowptr, col, val, dw, ksum=ksum, anisotropy=anisotropy, info=info)
    G.bandwidth = r.bw
    G.perm = perm
    G.ops = ops
    return G


def _radius_sweep(lib, st, X, N, d, code, r, decay, thresh):
    """Count and fill pass of the exact sweep over the flagged rows (meld_metric_radius), in the formats ``HipOps._emit`` takes."""
    dev = X.device
    s = SimpleNamespace(fb_total=0, fb_off=None, fb_col=None, fb_val=None, fb_cnt=None)
    n_flag = r.n_flag
    if n_flag == 0:
        return s
    r.flag_rows = flag_rows = torch.sort(r.flag_rows[:n_flag]).values.contiguous()  # deterministic order
    fb_cnt = torch.zeros(n_flag, dtype=torch.int32, device=dev)
    check(lib.meld_metric_radius(ptr(X), N, d, code, ptr(flag_rows), n_flag, ptr(r.bw), decay, thresh, 0, ptr(fb_cnt), None, None, None, None, st),
          "meld_metric_radius(count)")
    fb_off = scan_i32(fb_cnt)
    fb_total, most = (int(v) for v in torch.stack([fb_off[n_flag], fb_cnt.max().to(torch.int64)]).tolist())
    if most + 1 > N / 2:
        # a kernel radius that holds most of the data (many copies of one cell, a radius wider than the data): the graph is dense,
        # and the dense route is the tool for it
        raise NotImplementedError("degenerate neighbourhoods: the kernel radius of a row holds {} of the {} cells; such a graph is "
                                  "dense (the dense route serves N <= 16384)".format(most + 1, N))
    need = 12 * fb_total + 32 * (r.m_main + fb_total)
    if need > torch.cuda.get_device_properties(dev).total_memory:
        raise MemoryError(
            "the kernel radius covers {:.3g} neighbours per cell on average: the graph would hold {:.3g} entries ({:.0f} GB to "
            "assemble) -- raise decay or thresh".format((r.m_main + fb_total) / max(N, 1), float(r.m_main + fb_total), need / 1e9))
    fb_col = torch.empty(max(fb_total, 1), dtype=torch.int32, device=dev)
    fb_val = torch.empty(max(fb_total, 1), dtype=torch.float64, device=dev)
    cursor = torch.zeros(n_flag, dtype=torch.int32, device=dev)
    check(lib.meld_metric_radius(ptr(X), N, d, code, ptr(flag_rows), n_flag, ptr(r.bw), decay, thresh, 1, None, ptr(fb_off), ptr(cursor),
                                 ptr(fb_col), ptr(fb_val), st), "meld_metric_radius(fill)")
    s.fb_total, s.fb_off, s.fb_col, s.fb_val, s.fb_cnt = fb_total, fb_off, fb_col, fb_val, fb_cnt
    return s


# ---- new cells against a fitted L1 / L-inf graph (meld_amd/extend.py) ----------------------------------

def reference_cache(G, st):
    """The fitted cells as the search between two point sets reads them, built at the first extension call and kept on the
    state: ``X`` in the locality order (the graph's ``perm`` where it has one, else ``locality_permutation``, else the cells as
    they are -- then no copy at all), ``perm`` (position -> the caller's cell index, or None), the tile boxes."""
    c = getattr(st, "_refs", None)
    if c is not None:
        return c
    from .reorder import locality_permutation

    ops = G.ops if getattr(G, "ops", None) is not None else HipOps(st.X.device)
    X = st.X.contiguous()
    N, d = int(X.shape[0]), int(X.shape[1])
    perm = getattr(G, "perm", None)
    if perm is None and (G.info or {}).get("route") != "metric_knn":
        perm = locality_permutation(X)
    Xp = ops.gather_rows(X, perm) if perm is not None else X
    lib, dev = ops.lib, X.device
    T = int(lib.meld_metric_tile_rows())
    n_tiles = (N + T - 1) // T
    box_lo = torch.empty(n_tiles * d, dtype=torch.float64, device=dev)
    box_hi = torch.empty(n_tiles * d, dtype=torch.float64, device=dev)
    check(lib.meld_metric_tile_boxes(ptr(Xp), N, d, ptr(box_lo), ptr(box_hi), stream()), "meld_metric_tile_boxes")
    st._refs = SimpleNamespace(X=Xp, perm=perm, box_lo=box_lo, box_hi=box_hi, n_tiles=n_tiles, tile=T, ops=ops)
    return st._refs


def _cross_chunk_rows(M, N, d, ksel, slices, dev):
    """New cells per search call, from free memory as ``extend._chunk_rows`` sizes them: the sorted copy of the chunk, the
    slices' heaps and lists, the merged lists with their kernel values and the COO stream stay within a quarter of it."""
    free = int(torch.cuda.mem_get_info(dev)[0])
    per_q = 32 * d + 12 * int(ksel) * (2 * int(slices) + 4) + 256
    chunk = max(4096, min(1 << 18, (free // 4) // per_q))
    return int(min(M, (chunk // 64) * 64))


def cross_kernel_rows(G, st, Q, knn_c, decay, thresh, bandwidth=None, scale=1.0, n_slices=0):
    """Kernel rows of the new cells ``Q`` [M, d] (device fp64, the space the graph was built in) against the fitted cells of an
    L1 / L-inf graph, as ``extend.extend_rows`` returns them: (rowptr, col, val, rowsum), columns in the caller's order.

    bw_i = max(scale * (distance to the knn_c-th nearest fitted cell), eps), or max(scale * bandwidth, eps) for a number (then
    every row takes the sweep and nothing is searched); K_ij = exp(-(D_ij / bw_i)^decay) kept where >= thresh; ``decay`` = inf:
    the connectivity of the knn_c nearest fitted cells in (distance, column) order."""
    import math

    from .extend import extend_rows

    if int(Q.shape[1]) > 256:
        raise NotImplementedError("new cells on an L1 / L-inf graph are implemented for d <= 256 (got d = {})".format(int(Q.shape[1])))
    ksel = default_ksel(knn_c)
    if knn_c > ksel:
        raise NotImplementedError("knn={} beyond the {} entries the candidate lists hold".format(knn_c, ksel))
    refs = reference_cache(G, st)
    ops, lib, launch, dev = refs.ops, refs.ops.lib, stream(), Q.device
    Xp, N, d, M = refs.X, int(refs.X.shape[0]), int(refs.X.shape[1]), int(Q.shape[0])
    code = int(st.metric)
    prune = opt("MELD_METRIC_PRUNE", "1") != "0"
    fixed = bandwidth is not None and not math.isinf(decay)
    stats = dict(tiles_done=0, tile_pairs=0, n_flagged_rows=0, n_slices=[], prune=bool(prune))
    parts = []
    chunk = M if fixed else _cross_chunk_rows(M, N, d, ksel, lib.meld_metric_cross_slices(M, N, int(n_slices)), dev)
    for q0 in range(0, M, chunk):
        Qc = Q[q0:q0 + chunk].contiguous()
        m = int(Qc.shape[0])
        r = SimpleNamespace(m_main=0)
        if fixed:
            order = None
            r.bw = torch.full((m,), max(float(bandwidth) * scale, float(torch.finfo(torch.float64).eps)), dtype=torch.float64, device=dev)
            r.flag_rows, r.n_flag = torch.arange(m, dtype=torch.int32, device=dev), m
            keys = torch.empty(0, dtype=torch.int64, device=dev)
            vals = torch.empty(0, dtype=torch.float64, device=dev)
        else:
            # the reference tile nearest to every new cell; the cells sorted by it, so that a wave's 64 cells start from the same
            # few tiles and share a small box
            Qt = Qc.t().contiguous()  # [d][m]: lane = query, the reads of one coordinate coalesce
            seed_key = torch.full((m,), -1, dtype=torch.int64, device=dev)
            check(lib.meld_metric_cross_seed(ptr(Qt), m, ptr(refs.box_lo), ptr(refs.box_hi), N, d, code, ptr(seed_key), launch),
                  "meld_metric_cross_seed")
            seed, order = torch.sort(seed_key & 0xFFFFFFFF, stable=True)
            seed = seed.to(torch.int32)
            Qc = ops.gather_rows(Qc, order)
            Qt = Qc.t().contiguous()
            ns = int(lib.meld_metric_cross_slices(m, N, int(n_slices)))
            q_slots = ((m + refs.tile - 1) // refs.tile) * refs.tile
            heap_d = torch.empty(ns * ksel * q_slots, dtype=torch.float64, device=dev)
            heap_i = torch.empty(ns * ksel * q_slots, dtype=torch.int32, device=dev)
            part_idx = part_d = part_cnt = None
            if ns > 1:
                part_idx = torch.empty(ns * m * ksel, dtype=torch.int32, device=dev)
                part_d = torch.empty(ns * m * ksel, dtype=torch.float64, device=dev)
                part_cnt = torch.zeros(ns * m, dtype=torch.int32, device=dev)
            cand_idx = torch.empty(m * ksel, dtype=torch.int32, device=dev)
            cand_d = torch.empty(m * ksel, dtype=torch.float64, device=dev)
            cand_cnt = torch.empty(m, dtype=torch.int32, device=dev)
            tiles_done = torch.zeros(1, dtype=torch.int64, device=dev)
            with _EventSpan("metric_cross_topk", M=m, N=N, d=d, slices=ns):
                check(lib.meld_metric_cross_topk(ptr(Qt), m, ptr(Xp), N, d, code, ksel, ptr(refs.box_lo), ptr(refs.box_hi), ptr(seed), int(prune),
                                                 ns, ptr(heap_d), ptr(heap_i), ptr(part_idx), ptr(part_d), ptr(part_cnt), ptr(cand_idx),
                                                 ptr(cand_d), ptr(cand_cnt), ptr(tiles_done), launch), "meld_metric_cross_topk")
            del heap_d, heap_i, part_idx, part_d, part_cnt, Qt
            r.bw = torch.empty(m, dtype=torch.float64, device=dev)
            cand_val = torch.empty(m * ksel, dtype=torch.float64, device=dev)
            keep_cnt = torch.empty(m, dtype=torch.int32, device=dev)
            r.flag_rows = torch.empty(m, dtype=torch.int32, device=dev)
            n_flag = torch.zeros(1, dtype=torch.int32, device=dev)
            check(lib.meld_metric_cross_refine(ptr(cand_idx), ptr(cand_d), ptr(cand_cnt), m, ksel, knn_c - 1, decay, thresh, float(scale),
                                               ptr(r.bw), ptr(cand_val), ptr(keep_cnt), ptr(r.flag_rows), ptr(n_flag), launch),
                  "meld_metric_cross_refine")
            del cand_d
            n_flag_h, done_h = torch.stack([n_flag[0].to(torch.int64), tiles_done[0]]).tolist()  # (one read-back)
            r.n_flag = int(n_flag_h)
            # the kept candidates as (row << 32) | column: rows back in the caller's order, columns too
            kept = torch.nonzero(cand_val.view(m, ksel) > 0.0)
            vals = cand_val.view(m, ksel)[kept[:, 0], kept[:, 1]]
            keys = (order[kept[:, 0]] << 32) | cand_idx.view(m, ksel)[kept[:, 0], kept[:, 1]].to(torch.int64)
            r.m_main = int(keys.shape[0])
            stats["tiles_done"] += int(done_h)
            stats["tile_pairs"] += ((m + refs.tile - 1) // refs.tile) * refs.n_tiles
            stats["n_slices"].append(ns)
            del cand_idx, cand_val, kept
        s = _cross_radius_sweep(lib, launch, Qc, Xp, N, d, code, r, decay, thresh)
        stats["n_flagged_rows"] += r.n_flag
        if s.fb_total:
            rows = torch.repeat_interleave(r.flag_rows.to(torch.int64), s.fb_cnt.to(torch.int64), output_size=s.fb_total)
            if order is not None:
                rows = order[rows]
            keys = torch.cat([keys, (rows << 32) | s.fb_col[:s.fb_total].to(torch.int64)])
            vals = torch.cat([vals, s.fb_val[:s.fb_total]])
        if refs.perm is not None:  # the columns in the caller's order before the rows are sorted
            keys = (keys & ~0xFFFFFFFF) | refs.perm[keys & 0xFFFFFFFF]
        parts.append(extend_rows(keys.contiguous(), (0.5 * vals).contiguous(), 0, m, N))
    G.last_extend = stats
    return parts


def _cross_radius_sweep(lib, st, Q, X, N, d, code, r, decay, thresh):
    """``_radius_sweep`` for new cells (meld_metric_cross_radius).  A far-away new cell legitimately sees most fitted cells: no
    row is refused for that; the total size is."""
    dev = X.device
    s = SimpleNamespace(fb_total=0, fb_off=None, fb_col=None, fb_val=None, fb_cnt=None)
    n_flag, m = r.n_flag, int(Q.shape[0])
    if n_flag == 0:
        return s
    r.flag_rows = flag_rows = torch.sort(r.flag_rows[:n_flag]).values.contiguous()  # deterministic order
    fb_cnt = torch.zeros(n_flag, dtype=torch.int32, device=dev)
    check(lib.meld_metric_cross_radius(ptr(Q), m, ptr(X), N, d, code, ptr(flag_rows), n_flag, ptr(r.bw), decay, thresh, 0, ptr(fb_cnt), None, None,
                                       None, None, st), "meld_metric_cross_radius(count)")
    fb_off = scan_i32(fb_cnt)
    fb_total = int(fb_off[n_flag])
    need = 12 * fb_total + 48 * (r.m_main + fb_total)
    if need > torch.cuda.get_device_properties(dev).total_memory:
        raise MemoryError(
            "the kernel radius covers {:.3g} fitted cells per new cell on average: the kernel would hold {:.3g} entries ({:.0f} GB to "
            "assemble) -- raise decay or thresh".format((r.m_main + fb_total) / max(m, 1), float(r.m_main + fb_total), need / 1e9))
    fb_col = torch.empty(max(fb_total, 1), dtype=torch.int32, device=dev)
    fb_val = torch.empty(max(fb_total, 1), dtype=torch.float64, device=dev)
    cursor = torch.zeros(n_flag, dtype=torch.int32, device=dev)
    check(lib.meld_metric_cross_radius(ptr(Q), m, ptr(X), N, d, code, ptr(flag_rows), n_flag, ptr(r.bw), decay, thresh, 1, None, ptr(fb_off),
                                       ptr(cursor), ptr(fb_col), ptr(fb_val), st), "meld_metric_cross_radius(fill)")
    s.fb_total, s.fb_off, s.fb_col, s.fb_val, s.fb_cnt = fb_total, fb_off, fb_col, fb_val, fb_cnt
    return s
