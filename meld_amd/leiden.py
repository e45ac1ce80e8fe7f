"""Leiden communities of a device-resident graph: the Louvain run of ``louvain.py`` with a REFINEMENT of every level's move
partition before the contraction, so that every community returned induces a connected subgraph.

The reference clusters with scanpy's leiden and bisects the resolution for a wanted number of clusters
(``comparison/comparison.py``, ``find_n_clusters(adata, k, "leiden")``); here the partition is made on the device by a synchronous
and deterministic rule (``csrc/leiden.hip`` states the refinement, ``tests/leiden_reference.py`` restates the run in numpy,
``DESIGN.md`` section 4.19):

* the MOVE phase of a level is Louvain's (``louvain._run_level``, ``meld_louvain_move``), from singletons on level 0 and from the
  move partition ``P`` of the level before afterwards (a vertex of the contracted graph starts with the smallest vertex of its
  ``P``-community as its label);
* the REFINEMENT starts from singletons and merges inside the communities of ``P`` only.  Before a round the vertices are grouped
  by sub-community (one radix sort, ``meld_louvain_totals``); ``meld_leiden_propose`` lets every vertex that is still alone and well
  connected to its community name the sub-community it gains most from, ``meld_leiden_commit`` lets it join unless its target is
  a single vertex that asked to leave itself, and leaves the number of movers: the one read-back of the round.  Nobody leaves a
  sub-community of two or more and a joiner has an entry to what it joins, so every sub-community is connected;
* the graph is contracted by the REFINED partition (``louvain._contract``); the run ends when a move phase leaves every vertex
  alone (the communities are then the sub-communities of the level before) or when a refinement merges nothing (the result is
  then the level's vertices, each alone).  Either way a returned community is one refined sub-community: connected in the cells'
  graph.  A run cut by ``max_levels`` returns the last move partition, as Louvain does, and has no such guarantee.

Upstream's randomised choice among the candidates and its test of the sub-community's own connection are not offered.  The
caller's cell order, the bits and the surface (subgraphs, adopted graphs, single-GPU graphs only) are those of ``louvain.py``.
"""
from __future__ import annotations

import torch

from ._device_ops import stream
from ._lib import check, get_lib, ptr
from .louvain import DEFAULT_TOL, LouvainRecord, _community_run, _first_level, _next_level, _renumber, _run_level, _totals, q_value

__all__ = ["LeidenRecord", "leiden_device"]


class LeidenRecord(LouvainRecord):
    """What ``DeviceGraph.leiden`` returns: the attributes of a ``LouvainRecord``, with ``levels`` holding per level
    ``dict(vertices, communities, subcommunities, rounds, refine_rounds, Q)`` (``communities`` and ``Q`` of the move partition,
    ``subcommunities`` of its refinement, which the next level's vertices are) and ``level_labels(l)`` the cells' refined
    sub-communities after level ``l`` (for the last level the labels returned): each level refines the next."""


def _refine(lib, st, rowptr, col, val, k, P, two_m, gamma, max_rounds):
    """The refinement of the partition ``P`` (int32 labels in ``[0, n)``) from singletons: ``(sub, rounds)``."""
    n, dev = int(k.shape[0]), k.device
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    lanes = int(lib.meld_louvain_lanes(n, int(col.shape[0])))
    tot_comm, _, _ = _totals(lib, st, P, k, ar)
    sub = ar.to(torch.int32)
    prop = torch.empty(n, dtype=torch.int32, device=dev)
    part_moved = torch.empty(int(lib.meld_leiden_commit_blocks(n)), dtype=torch.int32, device=dev)
    movers = torch.empty(1, dtype=torch.int64, device=dev)
    rounds = 0
    while rounds < max_rounds:
        tot, size, _ = _totals(lib, st, sub, k, ar)
        new = torch.empty_like(sub)
        check(lib.meld_leiden_propose(ptr(rowptr), ptr(col), ptr(val), n, ptr(P), ptr(sub), ptr(k), ptr(tot), ptr(size), ptr(tot_comm),
                                      two_m, gamma, rounds, lanes, ptr(prop), st), "meld_leiden_propose")
        check(lib.meld_leiden_commit(ptr(sub), ptr(prop), ptr(size), n, ptr(new), ptr(part_moved), ptr(movers), st), "meld_leiden_commit")
        rounds += 1
        sub = new
        if int(movers.item()) == 0:  # (the one read-back of the round)
            break
    return sub, rounds


def _next_start(P, S_lab, S):
    """The start labels of the contracted graph's vertices: the smallest of them in the ``P``-community they lie in."""
    dev = P.device
    sub_p = torch.empty(S, dtype=torch.int64, device=dev)
    sub_p[S_lab.to(torch.int64)] = P.to(torch.int64)  # (the members of a sub-community agree)
    ids = torch.arange(S, dtype=torch.int64, device=dev)
    first = torch.full((S,), S, dtype=torch.int64, device=dev).scatter_reduce_(0, sub_p, ids, "amin")
    return first[sub_p].to(torch.int32)


def _singleton_q(lib, st, rowptr, col, val, n, two_m, gamma):
    """Q of the partition that leaves every vertex of the level alone (the diagonal holds the inner weights)."""
    dev = rowptr.device
    own = torch.empty(n, dtype=torch.float64, device=dev)
    k = torch.empty(n, dtype=torch.float64, device=dev)
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    check(lib.meld_modularity_terms(ptr(rowptr), ptr(col), ptr(val), n, ptr(ids), ptr(own), ptr(k), st), "meld_modularity_terms")
    s_in, s_tot2 = torch.stack([own.sum(), (k * k).sum()]).tolist()
    return q_value(s_in, s_tot2, two_m, gamma)


def _run(G, gamma, tol, max_rounds, max_levels):
    lib, st = get_lib(), stream()
    N, dev = G.N, G.rowptr.device
    cell = torch.arange(N, dtype=torch.int32, device=dev)
    levels, level_labels, q, start = [], [], 0.0, None
    rowptr, col, val, k, two_m = _first_level(G, lib, st)
    n = N
    while two_m > 0.0 and len(levels) < max_levels:  # (two_m == 0: no levels)
        c, q, rounds = _run_level(lib, st, rowptr, col, val, k, two_m, gamma, tol, max_rounds, start)
        P, L, _ = _renumber(lib, st, c, k)
        if L == n:  # every community is one vertex: the partition is the one the level before moved to
            if levels:
                q = levels[-1]["Q"]
            levels.append(dict(vertices=n, communities=L, subcommunities=n, rounds=rounds, refine_rounds=0, Q=q))
            level_labels.append(cell)
            break
        sub, refine_rounds = _refine(lib, st, rowptr, col, val, k, P, two_m, gamma, max_rounds)
        S_lab, S, _ = _renumber(lib, st, sub, k)
        levels.append(dict(vertices=n, communities=L, subcommunities=S, rounds=rounds, refine_rounds=refine_rounds, Q=q))
        if S == n:  # the refinement merged nothing: the level's vertices, each alone
            q = _singleton_q(lib, st, rowptr, col, val, n, two_m, gamma)
            level_labels.append(cell)
            break
        if len(levels) == max_levels:  # cut: the move partition, as Louvain returns it
            cell = P[cell.to(torch.int64)]
            level_labels.append(cell)
            break
        cell = S_lab[cell.to(torch.int64)]
        level_labels.append(cell)
        start = _next_start(P, S_lab, S)
        rowptr, col, val, k = _next_level(lib, st, rowptr, col, val, n, S_lab, S)
        n = S
    sizes = torch.bincount(cell.to(torch.int64))  # (labels are numbered by smallest cell: every number below the largest occurs)
    return LeidenRecord(cell, sizes.cpu().numpy(), q, gamma, levels, level_labels)


def leiden_device(G, resolution=1.0, n_clusters=None, tol=DEFAULT_TOL, max_rounds=None, max_levels=None, recompute=False):
    """The Leiden record of ``G`` (see ``DeviceGraph.leiden``); nothing but the numbers a round reads back and the counts of a
    level goes through the host.  Kept on the graph per set of arguments."""
    return _community_run(G, "_leiden", "Leiden communities are", _run, resolution, n_clusters, tol, max_rounds, max_levels, recompute)
