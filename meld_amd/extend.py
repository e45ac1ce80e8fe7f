"""Out-of-sample extension of a fitted graph: kernel, transitions and interpolation for cells that were not in ``fit``.

The graph object the reference hands out (``meld_op.graph``, a graphtools ``kNNGraph``) answers new cells with
[UPSTREAM graphtools 1.5.x ``kNNGraph.build_kernel_to_data(Y)``, ``BaseGraph.extend_to_data(Y)``,
``BaseGraph.interpolate(transform, transitions=None, Y=None)``]; ``DeviceGraph`` carries the same three names
(``meld_amd/graph.py``), implemented here:

* the kernel rows of the new cells come from the search between two point sets the MNN graph already uses
  (``HipOps.directed_kernel_coo(n_refs=N)``: MFMA candidate search, exact refinement, certification / exact sweep), the new
  cells stacked behind the fitted ones chunk by chunk; the bandwidth of a new cell is the distance to its knn-th nearest FITTED
  cell (it is not among them), as ``oracle.kernel_to_data`` restates upstream.  Data wider than the search kernels keep the
  library route (``mnn.cross_kernel``), a fixed numeric ``bandwidth`` takes a library route of its own (``_fixed_bandwidth_kernel``);
  the L1 / L-inf graphs take the exact search of ``csrc/metric_knn.hip`` (``metric_knn.cross_kernel_rows``);
* ``csrc/extend.hip`` turns the query-major half of the COO stream into the rectangular CSR ``[M, N]`` with its row sums
  (``meld_extend_rows``) and applies the row-normalised rows to a signal on the fitted cells without writing the transitions
  (``meld_extend_apply``).

[UPSTREAM, unpinned] readings of graphtools (it cannot be imported next to this code): ``extend_to_data`` is the plain
``sklearn.preprocessing.normalize(kernel, "l1", axis=1)`` of ``build_kernel_to_data`` -- no anisotropy, no symmetrisation enter
it --; the wording of the shape errors is ``Data._check_extension_shape``'s.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

from ._device_ops import stream
from ._lib import check, get_lib, ptr

__all__ = ["ExtensionState", "attach_extension_state", "kernel_to_data_device", "apply_transitions"]

_EPS = float(np.finfo(float).eps)


class ExtensionState(SimpleNamespace):
    """What a graph keeps for new cells: ``X`` the fp64 device matrix ``[N, d]`` the search saw, in the caller's cell order (a
    reference, not a copy); ``n_features_in``; ``project`` (raw device rows -> the d columns: PCA ``(Y - mean) V`` or, for sparse
    input, the truncated SVD's ``Y V``; None without a reduction); ``row_fn`` (the metric front end, row-wise; None for
    euclidean); the kernel's parameters as the builder received them (``decay`` in the units of the euclidean search, inf for
    ``decay=None``); ``bandwidth`` (None or the argument of ``fit``), ``bandwidth_scale``, ``knn_max``; ``ksel`` (the length of the
    candidate rows the graph was built with, or None for the default of the knn in use)."""


def attach_extension_state(G, X, n_features_in, project, row_fn, knn, decay, thresh, bandwidth=None, bandwidth_scale=None, knn_max=None,
                           ksel=None, metric=None, model=None):
    G._extend_state = ExtensionState(X=X, n_features_in=int(n_features_in), project=project, row_fn=row_fn, knn=int(knn),
                                     decay=float(decay), thresh=float(thresh), bandwidth=bandwidth,
                                     bandwidth_scale=1.0 if bandwidth_scale is None else float(bandwidth_scale), knn_max=knn_max, ksel=ksel,
                                     metric=metric, model=model)
    return G


def refusal(G):
    """Why this graph cannot be extended (a string), or None."""
    from .metric_knn import METRICS

    info = getattr(G, "info", None) or {}
    if G.n_rows != G.N or getattr(G, "comm", None) is not None:
        return "a row-sharded graph cannot be extended to new cells (every rank holds a slice of the kernel only)"
    if info.get("adopted_from") is not None:
        return "a graph adopted from {} keeps neither its cells nor its kernel's parameters: it cannot be extended to new cells".format(info["adopted_from"])
    if info.get("graph") == "mnn":
        return "an MNN graph (sample_idx) cannot be extended to new cells: a new cell belongs to no sample"
    l1 = getattr(getattr(G, "_extend_state", None), "metric", None) is not None  # (an L1 / L-inf graph that kept its cells)
    if not l1 and (info.get("route") == "metric_knn" or info.get("metric") in METRICS):
        return "the L1 / L-inf graphs (distance={!r}) cannot be extended to new cells: the search between two point sets is euclidean".format(info.get("metric"))
    if not l1 and info.get("dense"):
        return ("a dense graph (thresh=0, a precomputed matrix, or a kernel evaluated densely) cannot be extended to new cells: "
                "only the sparse euclidean kNN graph keeps a comparable kernel")
    if getattr(G, "_extend_state", None) is None:
        return "this graph was not built from cells by MELD.fit (from_scipy / a weight matrix): it has no cells to extend from"
    st = G._extend_state
    if st.knn_max is not None:
        return "a graph built with knn_max cannot be extended to new cells (graphtools' capped re-search is not implemented between two point sets)"
    if callable(st.bandwidth):
        return "a callable bandwidth cannot be extended to new cells"
    if st.bandwidth is not None and np.ndim(st.bandwidth) != 0:
        return "a per-cell bandwidth says nothing about new cells: only one fixed number can be extended"
    return None


def state_of(G):
    why = refusal(G)
    if why is not None:
        raise NotImplementedError(why)
    return G._extend_state


def check_extension_shape(shape, n_features_in, d):
    """[UPSTREAM, unpinned graphtools ``Data._check_extension_shape``]: "raw" (``n_features_in`` columns: to be projected) or
    "reduced" (``d`` columns), else the ValueError upstream words."""
    if len(shape) != 2:
        raise ValueError("Expected a 2D matrix. Y has shape {}".format(tuple(shape)))
    if shape[1] == d and n_features_in != d:
        return "reduced"
    if shape[1] == n_features_in:
        return "raw"
    if n_features_in != d:
        raise ValueError("Y must be of shape either (n, {}) or (n, {})".format(n_features_in, d))
    raise ValueError("Y must be of shape (n, {})".format(n_features_in))


def _to_device(Y, dev):
    """numpy array / torch tensor / DataFrame -> fp64 device tensor (any shape)."""
    if isinstance(Y, torch.Tensor):
        return Y.to(device=dev, dtype=torch.float64)
    Y = np.asarray(getattr(Y, "values", Y))
    if Y.dtype == object:
        Y = Y.astype(np.float64)
    return torch.from_numpy(np.ascontiguousarray(Y, dtype=np.float64)).to(dev)


def _project_sparse(st, Y, dev):
    """Sparse new cells -> the d columns, on the device and without a dense copy of ``Y`` where the graph reduced its data:
    ``Y V`` (sparse fit: the truncated SVD, uncentred) or ``Y V - mean V`` (dense fit: PCA) through ``DeviceCSR.matmul``; without
    a reduction the rows are densified (they are as wide as the search's own operands)."""
    from .sparse import DeviceCSR

    A = DeviceCSR.from_input(Y, device=dev)
    d = int(st.X.shape[1])
    kind = check_extension_shape(A.shape, st.n_features_in, d)
    if kind == "reduced":  # (scores are dense by nature: a sparse matrix of that width is a mistake)
        raise ValueError("Y must be of shape either (n, {}) or (n, {})".format(st.n_features_in, d) + ": sparse input has to carry the {} "
                         "columns of the data".format(st.n_features_in))
    model = getattr(st, "model", None)
    if model is None:
        if st.project is not None:
            raise NotImplementedError("this graph keeps its projection as a function only: sparse new cells need the model")
        return A.to_dense()
    Q = A.matmul(model["V"])
    if model["kind"] == "pca":
        Q -= model["mean"].reshape(1, -1).to(torch.float64) @ model["V"]
    return Q


def prepare_queries(st, Y):
    """New cells -> the space the search ran in: shape check, the stored projection, the metric's row front end.  ``Y``: an
    array, a tensor, a DataFrame, or whatever ``sparse.is_sparse_input`` accepts."""
    from .sparse import is_sparse_input

    dev = st.X.device
    d = int(st.X.shape[1])
    if is_sparse_input(Y):
        Q = _project_sparse(st, Y, dev)  # (checks shape, structure and finiteness on the way)
    else:
        shape = tuple(getattr(Y, "shape", np.shape(Y)))
        kind = check_extension_shape(shape, st.n_features_in, d)
        Q = _to_device(Y, dev)
        if Q.shape[0] == 0:
            raise ValueError("Y holds no cells")
        if not bool(torch.isfinite(Q.sum(dim=0)).all()) and not bool(torch.isfinite(Q).all()):
            raise ValueError("Input data contains NaN or infinity")
        if kind == "raw" and st.project is not None:
            Q = st.project(Q)
    if st.row_fn is not None:
        Q = st.row_fn(Q)
    return Q.contiguous()


def _fixed_bandwidth_kernel(Xq, Yr, bw, decay, thresh, q_chunk=4096, r_chunk=32768):
    """Library route for graphtools' fixed ``bandwidth``: (row, col, K) of every pair with exp(-(dist / bw)^decay) >= thresh --
    a GEMM-form screen (fp64 rocBLAS) with a rounding allowance, then the exact distances by direct differences.  The radius is
    known in advance, so there is no neighbour search to run.  It screens every pair of a new and a fitted cell (2 d flops and
    8 bytes of the screen matrix each): the cost of ``mnn.cross_kernel``, not that of the search."""
    from .mnn import _exact_dist

    dev = Xq.device
    nq, nr = int(Xq.shape[0]), int(Yr.shape[0])
    mean = Yr.mean(dim=0)
    Xq = (Xq - mean).contiguous()
    Yr = (Yr - mean).contiguous()
    n2r = (Yr * Yr).sum(dim=1)
    rad2 = (bw * float((-math.log(thresh)) ** (1.0 / decay))) ** 2
    rows, cols, vals = [], [], []
    for q0 in range(0, nq, q_chunk):
        Q = Xq[q0:q0 + q_chunk]
        n2q = (Q * Q).sum(dim=1)
        slack = 1e-9 * rad2 + 1e-12 * (n2q + n2r.max())
        for r0 in range(0, nr, r_chunk):
            r1 = min(nr, r0 + r_chunk)
            D = n2q[:, None] + n2r[None, r0:r1] - 2.0 * (Q @ Yr[r0:r1].T)
            hit = torch.nonzero(D <= (rad2 + slack)[:, None])
            if hit.shape[0] == 0:
                continue
            qi, ri = hit[:, 0] + q0, hit[:, 1] + r0
            v = torch.exp(-torch.pow(_exact_dist(Xq, Yr, qi, ri) / bw, decay))
            v = torch.where(torch.isnan(v), torch.ones_like(v), v)
            keep = v >= thresh
            rows.append(qi[keep])
            cols.append(ri[keep])
            vals.append(v[keep])
    if not rows:
        z = torch.empty(0, dtype=torch.int64, device=dev)
        return z, z.clone(), torch.empty(0, dtype=torch.float64, device=dev)
    return torch.cat(rows), torch.cat(cols), torch.cat(vals)


def extend_rows(keys, half_vals, row_begin, n_rows, n_cols):
    """``meld_extend_rows``: (keys (row << 32) | col, values K / 2) -> (rowptr, col, val = K, rowsum) of the rectangular CSR."""
    lib, dev = get_lib(), keys.device
    n = int(keys.shape[0])
    rowptr = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
    col = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    val = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
    rowsum = torch.empty(n_rows, dtype=torch.float64, device=dev)
    tb = int(lib.meld_extend_rows_temp_bytes(n, n_rows))
    tmp = torch.empty(tb, dtype=torch.uint8, device=dev)
    check(lib.meld_extend_rows(ptr(keys), ptr(half_vals), n, int(row_begin), int(n_rows), int(n_cols), ptr(rowptr), ptr(col), ptr(val), ptr(rowsum),
                               ptr(tmp), tb, stream()), "meld_extend_rows")
    return rowptr, col[:n], val[:n], rowsum


def apply_transitions(csr, F, colmap=None):
    """``meld_extend_apply``: diag(1 / rowsum) K F on the device.  ``csr``: (rowptr, col, val, rowsum); ``F``: fp64 device
    ``[N, p]``; ``colmap``: int64 ``[N]``, the row of F that holds cell j (F in the graph's device order), or None."""
    rowptr, col, val, rowsum = csr
    F = F.contiguous()
    M, p = int(rowsum.shape[0]), int(F.shape[1])
    out = torch.zeros(M, p, dtype=torch.float64, device=F.device)
    if int(col.shape[0]) == 0 or p == 0:
        return out
    check(get_lib().meld_extend_apply(ptr(rowptr), ptr(col), ptr(val), ptr(rowsum), M, ptr(F), int(F.shape[0]), p, ptr(colmap), ptr(out), stream()),
          "meld_extend_apply")
    return out


def _chunk_rows(M, N, d, ksel, dev):
    """New cells per search call: the stacked [fitted; new] matrix, the operands, candidate rows and COO stream of a chunk
    stay within a quarter of the free memory (the fitted cells' share is there whatever the chunk)."""
    free = int(torch.cuda.mem_get_info(dev)[0])
    fixed = 16 * N * d  # the stacked copy of the fitted cells + their search operands
    per_q = 16 * d + 96 * int(ksel) + 256
    room = max(free // 4 - fixed, 0)
    chunk = max(4096, min(1 << 18, room // per_q))
    return int(min(M, (chunk // 128) * 128))


def _stack_scaled(ops, Xr, Qc):
    """The stacked matrix [fitted; new] of one search call, multiplied by a power of two so that its largest centred coordinate
    lies in (1/2, 1), and its column statistics.

    No longer needed for correctness: ``meld_knn16_prepare_cross`` now hands the search the queries' norms in input units, as it
    does the references' (tests/test_gpu_cross_search.py), and certification does not depend on the unit of length.  It was
    introduced when a query's norm reached the error allowance in the search's scaled units (data / absmax), which for cells
    with coordinates above 1 made the allowance too small and let a new cell far from the centre be certified with neighbours
    missing.  Kept because it is harmless and keeps the extension's results as they were: the kernel only sees distances as the
    ratio dist / bandwidth and a power of two scales every coordinate exactly, so the values are those of the unscaled cells,
    bit for bit."""
    N, m, d = int(Xr.shape[0]), int(Qc.shape[0]), int(Xr.shape[1])
    Xcat = torch.empty(N + m, d, dtype=torch.float64, device=Xr.device)
    Xcat[:N] = Xr
    Xcat[N:] = Qc
    sums, cmin, cmax = ops.col_stats(Xcat)
    mean = sums / (N + m)
    absmax = float(torch.maximum(cmax - mean, mean - cmin).max())
    t = 1.0
    if absmax > 0.0 and math.isfinite(absmax):
        t = 2.0 ** (-math.ceil(math.log2(absmax * 1.001)))  # (1.001: the search takes its absmax in fp32)
    if t != 1.0:
        Xcat.mul_(t)
        sums, cmin, cmax = sums * t, cmin * t, cmax * t
    return Xcat, (sums, cmin, cmax)


def _concat_rows(parts):
    """Row blocks (rowptr, col, val, rowsum) of consecutive new cells -> one CSR."""
    if len(parts) == 1:
        return parts[0]
    offs, rowptrs = 0, []
    for i, p in enumerate(parts):
        rowptrs.append((p[0] if i == len(parts) - 1 else p[0][:-1]) + offs)
        offs += int(p[1].shape[0])
    return torch.cat(rowptrs), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]), torch.cat([p[3] for p in parts])


def kernel_to_data_device(G, Y, knn=None, bandwidth=None, bandwidth_scale=None, n_slices=0):
    """The kernel from the new cells ``Y`` to the fitted cells as device tensors ``(rowptr int64 [M + 1], col int32, val fp64,
    rowsum fp64 [M])``: rectangular CSR ``[M, N]``, columns in the caller's cell order, sorted inside a row.  Nothing goes
    through the host.  ``n_slices`` (L1 / L-inf graphs): slices of the fitted cells the search of few new cells is split into,
    0 = chosen from their number and the device; the result does not depend on it."""
    from .graph import HipOps, default_ksel
    from .mnn import cross_kernel

    st = state_of(G)
    if callable(bandwidth):
        raise NotImplementedError("a callable bandwidth cannot be extended to new cells")
    knn = st.knn if knn is None else int(knn)
    if knn < 1:
        raise ValueError("knn must be at least 1, got {}".format(knn))
    bw = st.bandwidth if bandwidth is None else bandwidth
    if bw is not None and np.ndim(bw) != 0:
        raise NotImplementedError("a per-cell bandwidth says nothing about new cells: only one fixed number can be extended")
    scale = st.bandwidth_scale if bandwidth_scale is None else float(bandwidth_scale)
    if not (scale > 0 and math.isfinite(scale)):
        raise ValueError("bandwidth_scale must be positive and finite, got {!r}".format(bandwidth_scale))
    decay, thresh = st.decay, float(max(st.thresh, _EPS))
    if math.isinf(decay):
        bw, scale = None, 1.0  # [UPSTREAM build_kernel_to_data]: the connectivity of the knn nearest cells, returned before bandwidths are looked at
    Q = prepare_queries(st, Y)
    Xr = st.X
    N, d, M = int(Xr.shape[0]), int(Xr.shape[1]), int(Q.shape[0])
    knn_c = int(min(knn, N))  # graphtools clips knn to the number of fitted cells
    if getattr(st, "metric", None) is not None:
        from .metric_knn import cross_kernel_rows

        return _concat_rows(cross_kernel_rows(G, st, Q, knn_c, decay, thresh, bandwidth=bw, scale=scale, n_slices=n_slices))
    ops = G.ops if getattr(G, "ops", None) is not None else HipOps(Xr.device)
    ks = default_ksel(knn_c) if st.ksel is None else max(int(st.ksel), default_ksel(knn_c))
    hot = bw is None and ops.search == "f16x3" and ops.lib.meld_knn16_kblocks(d) >= 0 and knn_c >= 2 and N >= 3 and ks >= knn_c + 1
    if not hot and bw is None and scale != 1.0:
        raise NotImplementedError("bandwidth_scale on the library route (data wider than the search kernels, or knn < 2) is not implemented")
    chunk = _chunk_rows(M, N, d, ks, Xr.device) if hot else M
    parts = []
    for q0 in range(0, M, chunk):
        Qc = Q[q0:q0 + chunk]
        m = int(Qc.shape[0])
        if hot:
            Xcat, stats = _stack_scaled(ops, Xr, Qc)
            keys, vals, _, _ = ops.directed_kernel_coo(Xcat, N, m, knn_c - 1, decay, thresh, ks, n_refs=N, bw_scale=scale, col_stats=stats)
            half = keys.shape[0] // 2  # (the query-major half; the stream carries K / 2)
            parts.append(extend_rows(keys[:half].contiguous(), vals[:half].contiguous(), N, m, N))
            del Xcat, keys, vals
            continue
        if bw is not None:
            r, c, v = _fixed_bandwidth_kernel(Qc, Xr, max(float(bw) * scale, _EPS), decay, thresh)
        else:
            r, c, v = cross_kernel(Qc, Xr, knn_c, decay, thresh)
        parts.append(extend_rows(((r << 32) | c).contiguous(), (0.5 * v).contiguous(), 0, m, N))
    return _concat_rows(parts)


def to_scipy(csr, N, normalise=False):
    """Host export of ``kernel_to_data_device``'s result (``normalise``: every row divided by its sum -- the transitions)."""
    from scipy import sparse

    rowptr, col, val, rowsum = (t.cpu().numpy() for t in csr)
    if normalise:
        s = np.repeat(np.where(rowsum > 0, rowsum, 1.0), np.diff(rowptr))
        val = val / s
    return sparse.csr_matrix((val, col, rowptr), shape=(rowptr.shape[0] - 1, N))


def interpolate(G, transform, transitions=None, Y=None):
    """[UPSTREAM graphtools ``BaseGraph.interpolate``]: ``transitions @ transform``; with ``Y`` the transitions of the new
    cells are applied on the device and never written (``meld_extend_apply``)."""
    if transitions is None and Y is None:
        raise ValueError("Either transitions or Y must be provided.")
    if transitions is not None:
        return np.asarray(transitions @ np.asarray(getattr(transform, "values", transform), dtype=np.float64))
    st = state_of(G)
    F = _to_device(transform, st.X.device)
    one_d = F.dim() == 1
    if one_d:
        F = F[:, None]
    if F.dim() != 2 or int(F.shape[0]) != G.N:
        raise ValueError("transform must have one row per fitted cell ({}), got shape {}".format(G.N, tuple(F.shape)))
    out = apply_transitions(kernel_to_data_device(G, Y), F).cpu().numpy()
    return out[:, 0] if one_d else out
