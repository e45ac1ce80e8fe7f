"""Louvain communities of a device-resident graph: the usual "Louvain clusters" of the cells without exporting ``W``.

The reference clusters with scanpy's louvain and bisects the resolution for a wanted number of clusters
(``comparison/comparison.py``, ``find_n_clusters``); here the partition is made on the device, by a synchronous and deterministic
variant of the local-move rule (``csrc/louvain.hip`` states it; ``tests/louvain_reference.py`` restates it in numpy):

* a LEVEL runs rounds of ``meld_louvain_move`` from singletons.  Before a round the vertices are grouped by label (one radix sort)
  and ``meld_louvain_totals`` leaves the communities' degree sums and sizes; the round leaves the new labels, the modularity terms of
  the labels it READ and the number of movers, and the host reads those three numbers.  Labels whose modularity lies more than
  ``tol`` above that of the last accepted ones are accepted and the round's moves are tried next; labels that are not are dropped
  and the accepted round's moves are tried again with half the movers (at the h-th try in a row those whose vertex number is a
  multiple of 2^h: simultaneous moves that undo each other are thinned out).  The level ends when an accepted round moved nothing,
  after ``RETRY_HALVINGS`` tries in a row, or after ``max_rounds``; the labelling with the larger value is kept;
* the communities are numbered by their smallest member and the graph is contracted to ``C' A C`` by 64-bit keys
  ``(community of the row, community of the column)``, the radix sort and a reduce-by-key: linear in the entries;
* the next level runs on the contracted graph, until a level merges nothing.

Everything works in the CALLER's cell order: a graph that carries a locality permutation is renumbered first (the same sort), so
that ids, ties and the order of every sum -- and with them the result, bit for bit -- do not depend on ``G.perm``.  Only ``rowptr`` /
``col`` / ``val`` are read: subgraphs and adopted graphs work; a stored diagonal entry counts as it stands.  Single-GPU graphs only.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ._device_ops import coo_merge, csr_from_keys, scan_i32, sort_pairs, stream
from ._graph_steps import require_unsharded
from ._lib import check, get_lib, ptr

__all__ = ["LouvainRecord", "louvain_device", "louvain", "modularity", "DEFAULT_TOL", "DEFAULT_MAX_ROUNDS", "DEFAULT_MAX_LEVELS"]

DEFAULT_TOL = 1e-7
DEFAULT_MAX_ROUNDS = 1000
DEFAULT_MAX_LEVELS = 64
RETRY_HALVINGS = 3  # tries with half, a quarter, an eighth of a round's movers before a level gives up
# the resolutions the bisection for ``n_clusters`` starts from and the width at which it gives up: find_n_clusters of the reference
R_START, R_STOP, R_TOL = 0.01, 10.0, 0.001


def q_value(s_in, s_tot2, two_m, gamma):
    """``(sum_c in_c - gamma sum_c tot_c^2 / 2m) / 2m``, in this order of operations."""
    two_m, gamma = float(two_m), float(gamma)
    if two_m == 0.0:
        return 0.0
    t = gamma * float(s_tot2)
    t = t / two_m
    return (float(s_in) - t) / two_m


class LouvainRecord:
    """What ``DeviceGraph.louvain`` returns.  ``labels`` (host int32 ``[N]``, caller's order, communities numbered by their smallest
    cell), ``labels_device``, ``n_communities``, ``sizes`` (host int64), ``modularity``, ``resolution``, ``levels`` (per level
    ``dict(vertices, communities, rounds, Q)``; the last one merged nothing unless ``max_levels`` cut the run) and
    ``level_labels(l)``, the partition of the cells after level ``l``: the dendrogram, each level refining the next."""

    def __init__(self, labels_device, sizes, modularity, resolution, levels, level_labels_device):
        self.labels_device = labels_device
        self.sizes = sizes
        self.n_communities = int(sizes.shape[0])
        self.modularity = float(modularity)
        self.resolution = float(resolution)
        self.levels = levels
        self._level_labels = level_labels_device
        self._labels = None

    @property
    def labels(self):
        if self._labels is None:
            self._labels = self.labels_device.cpu().numpy()
        return self._labels

    def level_labels(self, level):
        return self._level_labels[level].cpu().numpy()

    def __repr__(self):
        return "{}(n_communities={}, modularity={:.6f}, resolution={:g}, levels={})".format(
            type(self).__name__, self.n_communities, self.modularity, self.resolution, len(self.levels))


def _totals(lib, st, label, k, ar):
    """``(tot, size, minm)`` of the labelling ``label`` of ``n`` vertices with degrees ``k``: the vertices grouped by label (one
    sort), then ``meld_louvain_totals``.  ``st`` is the CURRENT stream's handle (the sort goes to the current stream), here and below."""
    n, dev = int(label.shape[0]), label.device
    keys, vals = sort_pairs((label.to(torch.int64) << 32) | ar, k, n)
    tot = torch.empty(n, dtype=torch.float64, device=dev)
    size = torch.empty(n, dtype=torch.int32, device=dev)
    minm = torch.empty(n, dtype=torch.int32, device=dev)
    check(lib.meld_louvain_totals(ptr(keys), ptr(vals), n, n, ptr(tot), ptr(size), ptr(minm), st), "meld_louvain_totals")
    return tot, size, minm


def _contract(lib, st, rowptr, col, val, n, label, n_new, merge=True):
    """The CSR of ``C' A C`` for the one-hot ``C`` of ``label`` (values in ``[0, n_new)``), rows sorted; ``merge=False`` where the
    labels are a renumbering (no two entries meet)."""
    dev = rowptr.device
    nnz = int(col.shape[0])
    keys = torch.empty(nnz, dtype=torch.int64, device=dev)
    check(lib.meld_louvain_contract_keys(ptr(rowptr), ptr(col), n, ptr(label), ptr(keys), st), "meld_louvain_contract_keys")
    keys, vals = sort_pairs(keys, val, n_new)
    if merge:
        keys, vals, nnz = coo_merge(keys, vals)
        vals = vals[:nnz].clone()
    out_rowptr, out_col = csr_from_keys(keys, nnz, 0, n_new)
    return out_rowptr, out_col, vals


def _degrees(lib, st, rowptr, val, n):
    k = torch.empty(n, dtype=torch.float64, device=rowptr.device)
    check(lib.meld_csr_row_sums(ptr(rowptr), ptr(val), n, 0.0, ptr(k), st), "meld_csr_row_sums")
    return k


def _run_level(lib, st, rowptr, col, val, k, two_m, gamma, tol, max_rounds, start=None):
    """The rounds of one level from singletons, or from the labels ``start`` (int32 ids in ``[0, n)``; the Leiden run starts a
    level from the partition of the level before): ``(labels kept, Q, rounds)``."""
    n, dev = int(k.shape[0]), k.device
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    lanes = int(lib.meld_louvain_lanes(n, int(col.shape[0])))
    blocks = int(lib.meld_louvain_move_blocks(n, lanes))
    c = ar.to(torch.int32) if start is None else start
    own = torch.empty(n, dtype=torch.float64, device=dev)
    part_sum = torch.empty(blocks, dtype=torch.float64, device=dev)
    part_moved = torch.empty(blocks, dtype=torch.int32, device=dev)
    stats = torch.empty(3, dtype=torch.float64, device=dev)
    base, halvings, rounds = None, 0, 0
    while True:
        tot, size, _ = _totals(lib, st, c, k, ar)
        new = torch.empty_like(c)
        moved = torch.empty(n, dtype=torch.int32, device=dev)
        check(lib.meld_louvain_move(ptr(rowptr), ptr(col), ptr(val), n, ptr(c), ptr(k), ptr(tot), ptr(size), two_m, gamma, rounds, lanes,
                                    ptr(new), ptr(own), ptr(moved), ptr(part_sum), ptr(part_moved), ptr(stats), st), "meld_louvain_move")
        stats[2] = (tot * tot).sum()
        s_in, movers, s_tot2 = stats.tolist()  # (the one read-back of the round)
        q = q_value(s_in, s_tot2, two_m, gamma)
        rounds += 1
        if base is None or q - base[1] > tol:  # accepted: the round's moves are tried next
            base, halvings = (c, q, new, moved), 0
            if movers == 0 or rounds >= max_rounds:
                return c, q, rounds
            c = new
            continue
        # dropped: the accepted round's moves once more, with half the movers
        kept = (c, q) if q > base[1] else (base[0], base[1])
        halvings += 1
        mask = (base[3] != 0) & (ar % (1 << halvings) == 0)
        if halvings > RETRY_HALVINGS or rounds >= max_rounds or not bool(mask.any()):
            return kept[0], kept[1], rounds
        c = torch.where(mask, base[2], base[0])


def _renumber(lib, st, c, k):
    """Communities numbered by their smallest member: ``(labels int32, L, sizes int64 [L])``."""
    n, dev = int(c.shape[0]), c.device
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    _, size, minm = _totals(lib, st, c, k, ar)
    flags = torch.empty(n, dtype=torch.int32, device=dev)
    check(lib.meld_louvain_heads(ptr(c), ptr(minm), n, ptr(flags), st), "meld_louvain_heads")
    rank = scan_i32(flags)
    L = int(rank[n].item())
    out = torch.empty(n, dtype=torch.int32, device=dev)
    sizes = torch.empty(L, dtype=torch.int64, device=dev)
    check(lib.meld_louvain_renumber(ptr(c), ptr(minm), ptr(rank), ptr(size), n, ptr(out), ptr(sizes), st), "meld_louvain_renumber")
    return out, L, sizes


def _check_resolution(resolution):
    if isinstance(resolution, bool) or not isinstance(resolution, (int, float, np.integer, np.floating)) or not math.isfinite(resolution) \
            or resolution <= 0:
        raise ValueError("resolution must be a finite positive number, got {!r}".format(resolution))
    return float(resolution)


def _positive_int(name, value, default):
    if value is None:
        return default
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 1:
        raise ValueError("{} must be a positive integer, got {!r}".format(name, value))
    return int(value)


def _caller_order_csr(G, lib, st):
    """The graph's CSR with rows and columns in the caller's cell order (the arrays themselves where there is no permutation)."""
    if G.nnz == 0 or G.perm is None:
        return G.rowptr, G.col, G.val
    return _contract(lib, st, G.rowptr, G.col, G.val, G.N, G.perm.to(torch.int32), G.N, merge=False)


def _first_level(G, lib, st):
    """The start of a run: ``(rowptr, col, val, k, two_m)`` of ``G`` in the caller's cell order.  Where ``two_m`` is 0 the run has no
    levels; a graph without entries yields that and no arrays."""
    if not G.nnz:
        return None, None, None, None, 0.0
    rowptr, col, val = _caller_order_csr(G, lib, st)
    k = _degrees(lib, st, rowptr, val, G.N)
    return rowptr, col, val, k, float(k.sum().item())


def _next_level(lib, st, rowptr, col, val, n, label, n_new):
    """The step to the next level: ``(rowptr, col, val, k)`` of the graph contracted by ``label`` (values in ``[0, n_new)``)."""
    rowptr, col, val = _contract(lib, st, rowptr, col, val, n, label, n_new)
    return rowptr, col, val, _degrees(lib, st, rowptr, val, n_new)


def _run(G, gamma, tol, max_rounds, max_levels):
    lib, st = get_lib(), stream()
    N, dev = G.N, G.rowptr.device
    cell = torch.arange(N, dtype=torch.int32, device=dev)
    sizes = torch.ones(N, dtype=torch.int64, device=dev)
    levels, level_labels, q = [], [], 0.0
    rowptr, col, val, k, two_m = _first_level(G, lib, st)
    n = N
    while two_m > 0.0 and len(levels) < max_levels:  # (two_m == 0: no levels)
        c, q, rounds = _run_level(lib, st, rowptr, col, val, k, two_m, gamma, tol, max_rounds)
        c, L, _ = _renumber(lib, st, c, k)
        if L == n and levels:
            q = levels[-1]["Q"]  # (nothing merged: the partition, and so its Q, is the level before's; summed anew it could differ in the last bit)
        levels.append(dict(vertices=n, communities=L, rounds=rounds, Q=q))
        cell = c[cell.to(torch.int64)]
        level_labels.append(cell)
        if L == n:
            break
        # (cells per community: the sizes of the level's vertices, added by community -- integers)
        sizes = torch.zeros(L, dtype=torch.int64, device=dev).index_add_(0, c.to(torch.int64), sizes)
        rowptr, col, val, k = _next_level(lib, st, rowptr, col, val, n, c, L)
        n = L
    return LouvainRecord(cell, sizes.cpu().numpy(), q, gamma, levels, level_labels)


def _for_n_clusters(run, gamma, n_clusters):
    """``run(gamma)``, or for a wanted number of communities the record of the resolution that gives it: the bisection of
    find_n_clusters (reference comparison/comparison.py), iteratively.  ``run(g)`` returns a record with ``n_communities``."""
    if n_clusters is None:
        return run(gamma)
    lo, hi = R_START, R_STOP
    rec = run(lo)
    n_lo = rec.n_communities
    if n_lo == n_clusters:
        return rec
    if n_lo > n_clusters:
        raise ValueError("r_start is too large. Got: {}".format(lo))
    rec = run(hi)
    n_hi = rec.n_communities
    if n_hi == n_clusters:
        return rec
    if n_hi < n_clusters:
        raise ValueError("r_stop is too small. Got: {}".format(hi))
    while hi - lo >= R_TOL:
        mid = lo + (hi - lo) / 2
        rec = run(mid)
        if rec.n_communities == n_clusters:
            return rec
        if rec.n_communities < n_clusters:
            lo, n_lo = mid, rec.n_communities
        else:
            hi, n_hi = mid, rec.n_communities
    raise ValueError("no resolution between {} and {} gives {} communities: the nearest counts found are {} (resolution {:g}) and {} "
                     "(resolution {:g})".format(R_START, R_STOP, n_clusters, n_lo, lo, n_hi, hi))


def _community_run(G, slot, what, run_graph, resolution, n_clusters, tol, max_rounds, max_levels, recompute):
    """What ``louvain_device`` and ``leiden_device`` share: the arguments checked before anything touches the device (``what`` words the
    refusal of a row shard), the records of ``run_graph(G, gamma, tol, max_rounds, max_levels)`` kept in ``G.<slot>``, the bisection."""
    gamma = _check_resolution(resolution)
    n_clusters = _positive_int("n_clusters", n_clusters, None)
    max_rounds = _positive_int("max_rounds", max_rounds, DEFAULT_MAX_ROUNDS)
    max_levels = _positive_int("max_levels", max_levels, DEFAULT_MAX_LEVELS)
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not tol >= 0:
        raise ValueError("tol must be a number >= 0, got {!r}".format(tol))
    require_unsharded(G, what)
    tol = float(tol)
    kept = G.__dict__.setdefault(slot, {})

    def run(g):
        key = (g, tol, max_rounds, max_levels)
        if recompute or key not in kept:
            kept[key] = run_graph(G, g, tol, max_rounds, max_levels)
        return kept[key]

    return _for_n_clusters(run, gamma, n_clusters)


def louvain_device(G, resolution=1.0, n_clusters=None, tol=DEFAULT_TOL, max_rounds=None, max_levels=None, recompute=False):
    """The Louvain record of ``G`` (see ``DeviceGraph.louvain``); nothing but three numbers per round and the counts of a level
    goes through the host.  Kept on the graph per set of arguments."""
    return _community_run(G, "_louvain", "Louvain communities are", _run, resolution, n_clusters, tol, max_rounds, max_levels, recompute)


def louvain(G, **kwargs):
    return louvain_device(G, **kwargs)


def _check_labels(labels, N):
    """``labels`` (host or device, any integer dtype) as they came, checked: one entry per cell, no negative value."""
    on_device = isinstance(labels, torch.Tensor)
    if not on_device:
        labels = np.asarray(labels)
    if labels.ndim != 1 or int(labels.shape[0]) != N:
        raise ValueError("labels need one entry per cell ({}), got shape {}".format(N, tuple(labels.shape)))
    is_int = (not labels.dtype.is_floating_point and not labels.dtype.is_complex and labels.dtype != torch.bool) if on_device \
        else np.issubdtype(labels.dtype, np.integer)
    if not is_int:
        raise TypeError("labels must be integers, got dtype {}".format(labels.dtype))
    if int(labels.min()) < 0:
        raise ValueError("labels must not be negative, got {}".format(int(labels.min())))
    return labels


def modularity(G, labels, resolution=1.0):
    """``Q(labels; resolution)`` on ``G`` (see ``DeviceGraph.modularity``)."""
    require_unsharded(G, "the modularity of a labelling is")
    gamma = _check_resolution(resolution)
    labels = _check_labels(labels, G.N)
    if G.nnz == 0:
        return 0.0
    lib, st, dev, N = get_lib(), stream(), G.rowptr.device, G.N
    labels = labels.to(dev) if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(labels)).to(dev)
    c = torch.unique(labels, return_inverse=True)[1].to(torch.int32)  # (values in [0, L): they become addresses)
    if G.perm is not None:
        c = c[G.perm]
    c = c.contiguous()
    own = torch.empty(N, dtype=torch.float64, device=dev)
    k = torch.empty(N, dtype=torch.float64, device=dev)
    check(lib.meld_modularity_terms(ptr(G.rowptr), ptr(G.col), ptr(G.val), N, ptr(c), ptr(own), ptr(k), st), "meld_modularity_terms")
    tot, _, _ = _totals(lib, st, c, k, torch.arange(N, dtype=torch.int64, device=dev))
    s_in, s_tot2, two_m = torch.stack([own.sum(), (tot * tot).sum(), k.sum()]).tolist()
    return q_value(s_in, s_tot2, two_m, gamma)
