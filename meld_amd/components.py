"""Connectivity of a device-resident graph: component labels and induced subgraphs without a round trip through the host.

pygsp's surface (``is_connected``, ``extract_components``, ``subgraph``) on ``DeviceGraph``; the labels are exactly
``scipy.sparse.csgraph.connected_components(G.W, directed=False)``.  The kernels are ``csrc/components.hip``: hook-and-compress
rounds on an int32 parent array (the host reads one device word per round and stops at the first round that wrote nothing),
then labels numbered by the smallest caller-order index of each component; an induced subgraph is a count pass, a scan and a fill
pass over the parent's CSR.  Single-GPU graphs only.
"""
from __future__ import annotations

import numpy as np
import torch

from ._device_ops import scan_i32, stream
from ._graph_steps import require_unsharded, rounds_until_unchanged
from ._lib import check, get_lib, ptr

__all__ = ["default_max_rounds", "selection_index", "connected_components_device", "subgraph"]


def default_max_rounds(N):
    """Rounds after which the labelling gives up: ``4 ceil(log2 N) + 64``.  Every round but the last lowers a label, so the loop
    ends by itself; the cap only bounds what a defect could cost (the hardest numberings tried take 13 rounds at 4,096 vertices)."""
    N = int(N)
    if N < 1:
        raise ValueError("a graph has at least one vertex, got N={}".format(N))
    return 4 * (N - 1).bit_length() + 64  # ((N - 1).bit_length() == ceil(log2 N) for N >= 1)


def selection_index(ind, N):
    """The cells a selection names, as an int64 vector in the order given: ``ind`` is an integer array (host or device) or a
    boolean mask with one entry per cell.  ValueError for an empty selection, duplicates, indices outside ``[0, N)`` and a mask of
    another length; TypeError for anything that is neither integer nor boolean.  A device tensor is checked on its device and
    returned as one; everything else comes back as a numpy array."""
    on_device = isinstance(ind, torch.Tensor) and ind.device.type != "cpu"
    if isinstance(ind, torch.Tensor) and not on_device:
        ind = ind.numpy()
    if not on_device:
        ind = np.asarray(ind)
    xp = torch if on_device else np
    if ind.ndim != 1:
        raise ValueError("the selection must be one-dimensional, got shape {}".format(tuple(ind.shape)))
    if int(ind.shape[0]) == 0:
        raise ValueError("the selection is empty")
    is_bool = ind.dtype == (torch.bool if on_device else np.bool_)
    is_int = (not ind.dtype.is_floating_point and not ind.dtype.is_complex and not is_bool) if on_device else np.issubdtype(ind.dtype, np.integer)
    if is_bool:
        if int(ind.shape[0]) != N:
            raise ValueError("a boolean mask needs one entry per cell ({}), got {}".format(N, int(ind.shape[0])))
        ind = xp.nonzero(ind)
        ind = ind[:, 0] if on_device else ind[0]
    elif not is_int:
        raise TypeError("the selection must be an integer array or a boolean mask, got dtype {}".format(ind.dtype))
    k = int(ind.shape[0])
    if k == 0:
        raise ValueError("the selection is empty")
    ind = ind.to(torch.int64) if on_device else ind.astype(np.int64)
    lo, hi = int(ind.min()), int(ind.max())
    if lo < 0 or hi >= N:
        raise ValueError("the selection holds indices outside [0, {}): {} .. {}".format(N, lo, hi))
    seen = xp.bincount(ind, minlength=N)
    if int(seen.max()) > 1:
        raise ValueError("the selection names {} cells more than once".format(int((seen > 1).sum())))
    return ind


def connected_components_device(G, recompute=False, max_rounds=None):
    """``(n_components, labels)`` of ``G``: ``labels`` an int32 device tensor ``[N]`` in the caller's cell order, components
    numbered by their smallest cell.  Kept on the graph (with the sizes, and ``G.components_info``); RuntimeError when
    ``max_rounds`` rounds (default ``default_max_rounds(N)``) do not reach the fixed point."""
    require_unsharded(G, "connected components are")
    kept = getattr(G, "_components", None)
    if kept is not None and not recompute:
        return kept["n"], kept["labels"]
    N, dev = G.N, G.rowptr.device
    max_rounds = default_max_rounds(N) if max_rounds is None else int(max_rounds)
    if max_rounds < 1:
        raise ValueError("max_rounds must be at least 1, got {}".format(max_rounds))
    lib, st = get_lib(), stream()
    parent = torch.arange(N, dtype=torch.int32, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    def one_round(_):
        check(lib.meld_cc_round(ptr(G.rowptr), ptr(G.col), N, ptr(parent), ptr(changed), st), "meld_cc_round")

    def no_fixed_point(r):
        return "connected components: no fixed point after {} rounds of hook-and-compress (max_rounds={})".format(r, max_rounds)

    rounds = rounds_until_unchanged(one_round, changed, max_rounds, no_fixed_point)
    min_orig = torch.empty(N, dtype=torch.int32, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    flags = torch.empty(N, dtype=torch.int32, device=dev)
    check(lib.meld_cc_minima(ptr(parent), ptr(G.perm), N, ptr(min_orig), ptr(count), ptr(flags), st), "meld_cc_minima")
    rank = scan_i32(flags)
    n = int(rank[N].item())
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    sizes = torch.empty(n, dtype=torch.int64, device=dev)
    check(lib.meld_cc_labels(ptr(parent), ptr(G.perm), ptr(min_orig), ptr(count), ptr(rank), N, ptr(labels), ptr(sizes), st), "meld_cc_labels")
    sizes = sizes.cpu().numpy()
    G._components = dict(n=n, labels=labels, sizes=sizes)
    G.components_info = dict(rounds=rounds, n_components=n, largest=int(sizes.max()))
    return n, labels


def subgraph(G, ind):
    """The graph induced by the cells ``ind`` (see ``DeviceGraph.subgraph``)."""
    from .graph import DeviceGraph

    require_unsharded(G, "a subgraph is")
    N, dev = G.N, G.rowptr.device
    ind = selection_index(ind, N)
    orig_idx = ind.cpu().numpy() if isinstance(ind, torch.Tensor) else ind
    idx = ind if isinstance(ind, torch.Tensor) else torch.from_numpy(ind).to(dev)
    k = int(idx.shape[0])
    # position of every cell in the selection (-1: dropped), then in the parent's device order
    pos = torch.full((N,), -1, dtype=torch.int64, device=dev)
    pos[idx] = torch.arange(k, dtype=torch.int64, device=dev)
    if G.perm is not None:
        pos = pos[G.perm]
    keep = pos >= 0
    rows = torch.nonzero(keep)[:, 0]  # the kept rows, ascending: the result's device order
    new_index = torch.full((N,), -1, dtype=torch.int32, device=dev)
    new_index[rows] = torch.arange(k, dtype=torch.int32, device=dev)
    sub_perm = pos[rows]  # device row t of the result is cell sub_perm[t] of the result

    lib, st = get_lib(), stream()
    counts = torch.empty(k, dtype=torch.int32, device=dev)
    check(lib.meld_subgraph_count(ptr(G.rowptr), ptr(G.col), ptr(new_index), N, ptr(counts), st), "meld_subgraph_count")
    rowptr = scan_i32(counts)
    nnz = int(rowptr[k].item())
    col = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(nnz, dtype=torch.float64, device=dev)
    dw = torch.zeros(k, dtype=torch.float64, device=dev)
    if nnz:
        check(lib.meld_subgraph_fill(ptr(G.rowptr), ptr(G.col), ptr(G.val), ptr(new_index), N, ptr(rowptr), ptr(col), ptr(val), st), "meld_subgraph_fill")
        check(lib.meld_csr_row_sums(ptr(rowptr), ptr(val), k, 0.0, ptr(dw), st), "meld_csr_row_sums")

    info = dict(orig_idx=orig_idx)
    if "knn" in G.info:
        info["knn"] = G.info["knn"]
    sub = DeviceGraph(rowptr, col, val, dw, ksum=None, anisotropy=G.anisotropy, info=info)
    # the parent's kernel restricted to the kept cells: its diagonal is carried, not recomputed from row sums that have changed
    sub._kdiag = G.kernel_diagonal()[rows].contiguous()
    bw = getattr(G, "bandwidth", None)
    if bw is not None:
        sub.bandwidth = bw[rows].contiguous() if isinstance(bw, torch.Tensor) and bw.dim() == 1 and int(bw.shape[0]) == N else bw
        if getattr(G, "bandwidth_to_metric", None) is not None:
            sub.bandwidth_to_metric = G.bandwidth_to_metric
    if not bool((sub_perm == torch.arange(k, dtype=torch.int64, device=dev)).all()):
        sub.perm = sub_perm
    return sub
