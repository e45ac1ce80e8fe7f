"""Geodesic distances on a fitted graph: shortest paths from many sources at once, on the device.

[UPSTREAM graphtools 1.5.x ``BaseGraph.shortest_path(method="auto", distance=None)``, unpinned: it cannot be imported next to this
code] hands ``-log K``, the data distances or hop counts to scipy's ``graph_shortest_path``; without this module the route is
``graph.W`` exported to the host and ``scipy.sparse.csgraph.dijkstra``, serial per source.  Here the distances stay on the device:
``csrc/geodesic.hip`` (``meld_minplus_step``) is one synchronous Bellman-Ford round, ``y = min(x, min_e (x[col[e]] + len[e]))``, on a
row-major fp64 block of up to 128 sources in one stream of the CSR arrays (lanes = sources; wider source sets panel by panel through
the leading dimensions, ``diffuse.panels``), and the host repeats rounds until one lowers nothing, reading one device word per round.

Why the result is scipy's bit for bit: ``f_e(x) = fl(x + len_e)`` with ``len_e >= 0`` is monotone and inflationary, so Dijkstra is
exact for "the minimum over paths of the left-to-right floating-point sum"; the synchronous iteration descends from above through
values that are all such path sums and reaches the same least fixed point.  Round ``r`` has every shortest path of at most ``r``
edges right, so the number of rounds is the largest edge count of a shortest path plus the idle round that ends the loop -- above
the BFS radius of the graph, and at most ``N``.

Cost: every round streams the whole matrix for all columns of the panel, whatever has converged; a single source pays ``rounds x
(launch + read-back)`` and is not what this is for (``DESIGN.md`` 4.14 has the measurements against scipy).

``check_distance``, ``default_distance``, ``check_sources`` and ``data_refusal`` are pure helpers (no device).
"""
from __future__ import annotations

import numpy as np

from ._graph_steps import csr_operands, is_sharded, require_unsharded, rounds_until_unchanged
from .diffuse import panels

__all__ = ["DISTANCES", "check_distance", "default_distance", "check_sources", "data_refusal", "edge_lengths_device",
           "shortest_path_device", "shortest_path", "geodesic"]

DISTANCES = ("affinity", "data", "constant")
MAX_DATA_DIMS = 256  # columns of the cells ``meld_edge_lengths_l2`` takes


def check_distance(name):
    """``"affinity"`` (``-log`` of the weights), ``"data"`` (euclidean distances of the cells) or ``"constant"`` (hop counts)."""
    if not isinstance(name, str) or name not in DISTANCES:
        raise ValueError("distance {!r} not recognized. Choose from {}".format(name, list(DISTANCES)))
    return name


def default_distance(G):
    """graphtools' rule for ``distance=None``: ``"constant"`` for an unweighted graph (built with ``decay=None``), else
    ``"affinity"``."""
    st = getattr(G, "_extend_state", None)
    return "constant" if st is not None and np.isinf(st.decay) else "affinity"  # (the builder's decay: inf for decay=None)


def check_sources(sources, N):
    """``sources`` -- integers or a boolean mask of length ``N`` -- as an int64 array, in the order given.  Duplicates are allowed,
    and so is an empty input (an ``[N, 0]`` result).  ValueError for indices out of range (negative ones included), a mask of
    the wrong length, more than one dimension and anything that is neither integer nor boolean."""
    N = int(N)
    if hasattr(sources, "detach") and hasattr(sources, "cpu"):  # (a torch tensor, host or device)
        sources = sources.detach().cpu().numpy()
    s = np.asarray(sources)
    if s.ndim == 0:
        s = s.reshape(1)
    if s.ndim != 1:
        raise ValueError("sources must be one-dimensional, got shape {}".format(s.shape))
    if s.dtype == np.bool_:
        if s.shape[0] != N:
            raise ValueError("a boolean mask of sources must have one entry per cell ({}), got {}".format(N, s.shape[0]))
        return np.flatnonzero(s).astype(np.int64)
    if s.size == 0:
        return np.zeros(0, dtype=np.int64)
    if s.dtype.kind not in "iu":
        raise ValueError("sources must be integers or a boolean mask, got dtype {}".format(s.dtype))
    idx = s.astype(np.int64)
    bad = (idx < 0) | (idx >= N)
    if bad.any():
        raise ValueError("source index {} is out of range for {} cells".format(int(idx[bad][0]), N))
    return idx


def data_refusal(G):
    """Why ``distance="data"`` cannot run on this graph (a string), or None: the lengths are the euclidean distances of the rows
    the graph was searched on, so the graph must keep them and they must be the data."""
    info = getattr(G, "info", None) or {}
    if is_sharded(G):
        return "a row-sharded graph has no data distances (every rank holds a slice of the kernel only)"
    st = getattr(G, "_extend_state", None)
    if st is not None and getattr(st, "metric", None) is not None:
        return ("distance={!r} builds an L1 / L-inf graph: the data distances offered are euclidean; use distance='affinity' or "
                "'constant'".format(info.get("metric") or "manhattan / chebyshev"))
    if st is None:
        if info.get("adopted_from") is not None:
            return "a graph adopted from {} keeps no cells: data distances need them; use distance='affinity' or 'constant'".format(info["adopted_from"])
        if info.get("precomputed") is not None:
            return ("a graph of a precomputed {} matrix keeps no cells: data distances need them; use distance='affinity' or "
                    "'constant'".format(info["precomputed"]))
        return ("this graph was not built from cells by MELD.fit (fit(G), a weight matrix, or a graph that does not keep its cells): "
                "data distances need them; use distance='affinity' or 'constant'")
    if st.row_fn is not None:
        return ("distance={!r} builds its graph on transformed rows: their euclidean distances are not the data's; use "
                "distance='affinity' or 'constant'".format(info.get("metric") or "cosine / correlation"))
    if int(st.X.shape[1]) > MAX_DATA_DIMS:
        return "data distances are offered for cells of up to {} columns, the graph was searched on {}".format(MAX_DATA_DIMS, int(st.X.shape[1]))
    return None


# -- device side ---------------------------------------------------------------------------------------------------------------
def edge_lengths_device(G, distance=None):
    """The length of every stored entry: an fp64 device tensor aligned with ``G.col`` (device order), built once per
    ``(graph, distance)`` and kept on the graph.  ``"constant"``: ones.  ``"affinity"``: ``-log(val)``, which needs
    ``0 < val <= 1`` -- graphs built here always satisfy it, because the kernel's row sums include the unit diagonal and the
    anisotropy normalisation divides by them.  ``"data"``: ``meld_edge_lengths_l2`` on the rows the graph was searched on, brought
    to the device order; the lengths of ``(i, j)`` and ``(j, i)`` are bit-equal.  Every result is validated once: ValueError,
    counting the offenders, unless all lengths are finite and ``>= 0`` (an adopted graph with weights above 1 under
    ``"affinity"``); NotImplementedError, naming the case, where ``"data"`` has no cells to measure (``data_refusal``)."""
    import torch

    from ._device_ops import stream
    from ._lib import check, get_lib, ptr

    distance = default_distance(G) if distance is None else check_distance(distance)
    require_unsharded(G, "shortest paths are")
    kept = getattr(G, "_edge_lengths", None)
    if kept is None:
        kept = G._edge_lengths = {}
    if distance in kept:
        return kept[distance]
    if distance == "constant":
        L = torch.ones(G.nnz, dtype=torch.float64, device=G.val.device)
    elif distance == "affinity":
        L = -torch.log(G.val.to(torch.float64)) + 0.0  # (+ 0.0: a weight of exactly 1 gives +0, not -0)
    else:
        why = data_refusal(G)
        if why is not None:
            raise NotImplementedError(why)
        X = G._extend_state.X.to(torch.float64)
        X = (X.index_select(0, G.perm) if G.perm is not None else X).contiguous()
        L = torch.empty(G.nnz, dtype=torch.float64, device=G.val.device)
        if G.nnz:
            check(get_lib().meld_edge_lengths_l2(ptr(G.rowptr), ptr(G.col), G.N, ptr(X), int(X.shape[1]), int(X.shape[1]), ptr(L),
                                                 stream()), "meld_edge_lengths_l2")
    bad = int((~(torch.isfinite(L) & (L >= 0))).sum())
    if bad:
        raise ValueError("{} of the {} edge lengths under distance={!r} are not finite and >= 0{}".format(
            bad, G.nnz, distance, " (-log of a weight needs 0 < weight <= 1)" if distance == "affinity" else ""))
    kept[distance] = L
    return L


def shortest_path_device(G, sources, distance=None, min_only=False, device_order=False, max_rounds=None):
    """Shortest-path distances along the graph as an fp64 device tensor ``[N, p]``, column ``j`` the distances from
    ``sources[j]`` (``+inf`` where there is no path); with ``min_only`` ``[N]``, the distance to the nearest source (scipy's flag
    of that name).  Equal to ``scipy.sparse.csgraph.dijkstra(G.edge_lengths(distance), indices=sources)`` bit for bit where all
    lengths are positive.  Rows and sources are in the caller's order unless ``device_order``.  ``G.geodesic_info`` is
    ``dict(rounds=[per panel of 128 sources], distance, p)``; RuntimeError when a panel has not reached its fixed point after
    ``max_rounds`` rounds (default ``N``, which always suffices).  A single source is slower than scipy on the host where the
    graph has a long diameter: every round is a launch and a read-back."""
    import torch

    from . import filter as _filter
    from ._device_ops import stream
    from ._lib import check, get_lib, ptr

    require_unsharded(G, "shortest paths are")
    N, dev = G.N, G.val.device
    idx = check_sources(sources, N)
    distance = default_distance(G) if distance is None else check_distance(distance)
    max_rounds = N if max_rounds is None else int(max_rounds)
    if max_rounds < 1:
        raise ValueError("max_rounds must be at least 1, got {}".format(max_rounds))
    L = edge_lengths_device(G, distance)
    p = 1 if min_only else int(idx.shape[0])
    D = torch.full((N, p), float("inf"), dtype=torch.float64, device=dev)
    info = dict(rounds=[], distance=distance, p=int(idx.shape[0]))
    if p and idx.size:
        rows = torch.from_numpy(idx).to(dev)
        if not device_order:
            rows = _filter.device_rows_of(G, rows)
        D[rows, 0 if min_only else torch.arange(p, device=dev)] = 0.0
    if p and N:
        lib = get_lib()
        st = stream()
        rowptr, col, L = csr_operands(G, L)
        # the rounds of a panel take turns between its columns of D and of `other`, a block of the same shape (the same columns of
        # both: the ranges the entry compares never meet); the round that lowers nothing leaves both equal, so D holds the result
        # whichever it wrote
        other = torch.empty_like(D)
        changed = torch.zeros(1, dtype=torch.int32, device=dev)
        esz = D.element_size()
        for c0, w in panels(p):  # all rounds of one panel before the next
            bufs = (D.data_ptr() + c0 * esz, other.data_ptr() + c0 * esz)

            def one_round(r):
                check(lib.meld_minplus_step(ptr(rowptr), ptr(col), ptr(L), N, bufs[r & 1], p, bufs[(r + 1) & 1], p, w, ptr(changed), st),
                      "meld_minplus_step")

            def no_fixed_point(r):
                return "shortest paths: no fixed point after {} rounds (max_rounds={}) for sources {} .. {}".format(r, max_rounds, c0, c0 + w - 1)

            info["rounds"].append(rounds_until_unchanged(one_round, changed, max_rounds, no_fixed_point))
    G.geodesic_info = info
    if G.perm is not None and not device_order:
        D = _filter._to_caller_order(D, G) if p else D
    return D[:, 0] if min_only else D


def shortest_path(G, sources=None, distance=None, min_only=False, method="auto"):
    """``shortest_path_device`` as a host ndarray (``DeviceGraph.shortest_path``)."""
    if sources is None:
        if G.N > G.FOURIER_MAX_N:
            raise ValueError("all-pairs shortest paths are offered up to {} cells, the graph has {}: pass the cells to start from as "
                             "`sources`".format(G.FOURIER_MAX_N, G.N))
        sources = np.arange(G.N, dtype=np.int64)
    return shortest_path_device(G, sources, distance=distance, min_only=min_only).cpu().numpy()


def geodesic(G, sources, distance=None):
    """``(values, idx)`` for ``MELD.geodesic``: the fp64 device tensor ``[N, len(idx)]`` in the caller's order and the sources as
    int64 positions."""
    idx = check_sources(sources, G.N)
    return shortest_path_device(G, idx, distance=distance), idx
