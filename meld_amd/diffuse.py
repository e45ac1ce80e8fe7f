"""Diffusion of cell signals over a fitted graph: the random walk of the kernel matrix, applied ``t`` times on the device.

The reference's tutorial notebooks smooth gene expression with [UPSTREAM magic-impute, unpinned: it cannot be imported next to this
code] ``magic.MAGIC().fit_transform(data, genes=...)``, whose approximate solver is ``diff_op^t`` applied to the PCA scores and
mapped back to the requested genes.  The operator is graphtools' ``diff_op = normalize(K, "l1", axis=1)`` -- what
``DeviceGraph.diff_op`` exports to the host -- and here it is never formed: ``csrc/diffuse.hip`` (``meld_diffuse_step``) applies
``D^-1 (W + diag(kd))`` to a row-major fp64 signal of up to 128 columns in one stream of the CSR arrays, wider signals panel by
panel through the leading dimensions.

``check_t``, ``panels`` and ``column_index`` are pure helpers (no device).  ``diffuse_device`` is ``DeviceGraph.diffuse_device``,
``impute`` is ``MELD.impute``.
"""
from __future__ import annotations

import numbers

import numpy as np

from ._graph_steps import csr_operands, is_sharded, require_unsharded

__all__ = ["check_t", "panels", "column_index", "diffuse_device", "impute"]

MAX_COLS = 128  # columns of one launch (``meld_diffuse_max_cols()``; tests/test_diffuse_host.py holds the two together)


def check_t(t):
    """The number of diffusion steps: an integer >= 0 (numpy integers included), returned as ``int``."""
    if isinstance(t, str) and t == "auto":
        raise NotImplementedError("t='auto' (MAGIC's Procrustes stopping rule) is not implemented: pass the number of steps t as an integer")
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, (numbers.Integral, np.integer)):
        raise ValueError("t must be an integer >= 0, got t={!r}".format(t))
    if int(t) < 0:
        raise ValueError("t must be an integer >= 0, got t={!r}".format(t))
    return int(t)


def panels(p):
    """``[(first_column, width), ...]`` with ``width <= 128``, contiguous, covering ``p`` columns: a function of ``p`` alone."""
    p = int(p)
    if p < 0:
        raise ValueError("the number of columns must not be negative, got {}".format(p))
    return [(c0, min(MAX_COLS, p - c0)) for c0 in range(0, p, MAX_COLS)]


def column_index(genes, n_features, names=None):
    """``genes`` -- integers, a boolean mask of length ``n_features``, or names looked up in ``names`` -- as an int64 index into
    the ``n_features`` columns.  ValueError for an index out of range (negative ones included), a mask of the wrong length,
    an unknown name, and names where the graph kept none."""
    n_features = int(n_features)
    if isinstance(genes, (str, bytes)) or np.ndim(genes) == 0:
        genes = [genes]
    g = np.asarray(list(genes) if not isinstance(genes, np.ndarray) else genes)
    if g.ndim != 1:
        raise ValueError("genes must be one-dimensional, got shape {}".format(g.shape))
    if g.dtype == np.bool_:
        if g.shape[0] != n_features:
            raise ValueError("a boolean mask of genes must have one entry per column ({}), got {}".format(n_features, g.shape[0]))
        return np.flatnonzero(g).astype(np.int64)
    if g.size == 0:
        return np.zeros(0, dtype=np.int64)
    if g.dtype.kind in "iu":
        idx = g.astype(np.int64)
        bad = (idx < 0) | (idx >= n_features)
        if bad.any():
            raise ValueError("gene index {} is out of range for {} columns".format(int(idx[bad][0]), n_features))
        return idx
    if g.dtype.kind in "USO":
        if names is None:
            raise ValueError("genes were given by name, but fit received no column names (pass a DataFrame to fit, or integer indices)")
        where = {}
        for i, name in enumerate(names):
            where.setdefault(name, i)
        missing = [x for x in g.tolist() if x not in where]
        if missing:
            raise ValueError("unknown gene name {!r} ({} of the {} requested are not columns of the data)".format(missing[0], len(missing), g.size))
        return np.asarray([where[x] for x in g.tolist()], dtype=np.int64)
    raise ValueError("genes must be integers, a boolean mask or names, got dtype {}".format(g.dtype))


# -- device side ---------------------------------------------------------------------------------------------------------------
def walk_vectors(G):
    """``(kd, s)``: the kernel's diagonal and the row sums ``s = dw + kd`` of ``K`` in the device order, contiguous fp64 device
    tensors, built once and kept on the graph.  ValueError, naming their number, where cells have no positive row sum."""
    kept = getattr(G, "_walk_vectors", None)
    if kept is None:
        import torch

        kd = G.kernel_diagonal().to(torch.float64)[: G.N].contiguous()
        s = (G.dw_dev[: G.N] + kd).contiguous()
        bad = int((~(s > 0)).sum())
        if bad:
            raise ValueError("{} cells have no positive kernel row sum (isolated, with a zero kernel diagonal): the random walk is "
                             "not defined there".format(bad))
        kept = G._walk_vectors = (kd, s)
    return kept


def _signal_device(F, G):
    """``F`` (device tensor, host array, DataFrame) as an fp64 tensor [N, p] on the graph's device, and whether it was 1-D;
    the shape errors are ``filter._checked_signal``'s."""
    import torch

    dev = G.val.device
    if isinstance(F, torch.Tensor):
        X = F.to(device=dev, dtype=torch.float64)
    else:
        X = torch.from_numpy(np.ascontiguousarray(np.asarray(getattr(F, "values", F), dtype=np.float64))).to(dev)
    if X.dim() == 0 or int(X.shape[0]) != G.N:
        raise ValueError("First dimension should be the number of nodes G.N = {}, got {}.".format(G.N, tuple(X.shape)))
    flat = X.dim() == 1
    if flat:
        X = X[:, None]
    if X.dim() != 2:
        raise ValueError("At most 2 dimensions are supported.")
    return X, flat


def diffuse_device(G, F, t=1, device_order=False):
    """``P^t F`` as an fp64 device tensor ([N, p], or [N] for 1-D input), ``P = D^-1 (W + diag(kd))`` the graph's ``diff_op``.
    Rows in the caller's order unless ``device_order`` (then neither input nor output is permuted).  ``t = 0``: a copy."""
    import torch

    from . import filter as _filter
    from ._device_ops import stream
    from ._lib import check, get_lib, ptr

    t = check_t(t)
    require_unsharded(G, "the diffusion operator is")
    X, flat = _signal_device(F, G)
    permuted = G.perm is not None and not device_order
    X = X.index_select(0, G.perm) if (permuted and t > 0) else X.contiguous()
    ours = not (isinstance(F, torch.Tensor) and X.data_ptr() == F.data_ptr())  # (else X is the caller's storage: never written)
    N, p = int(X.shape[0]), int(X.shape[1])
    if t == 0 or p == 0:
        out = X if ours else X.clone()
        return out[:, 0] if flat else out
    kd, s = walk_vectors(G)
    # two buffers take turns: the first step reads X and writes `first`; X itself is the second buffer where it is a copy of ours
    first = torch.empty_like(X)
    second = (X if ours else torch.empty_like(X)) if t >= 2 else None
    bufs = (first, second)
    lib = get_lib()
    st = stream()
    rowptr, col, val = csr_operands(G, G.val)
    esz = X.element_size()
    for c0, w in panels(p):  # all t steps of one panel before the next
        src = X
        for step in range(t):
            dst = bufs[step & 1]
            check(lib.meld_diffuse_step(ptr(rowptr), ptr(col), ptr(val), ptr(kd), ptr(s), N, src.data_ptr() + c0 * esz, p,
                                        dst.data_ptr() + c0 * esz, p, w, st), "meld_diffuse_step")
            src = dst
    out = bufs[(t - 1) & 1]
    if permuted:
        out = _filter._to_caller_order(out, G)
    return out[:, 0] if flat else out


def diffuse(G, F, t=1):
    """``diffuse_device`` as a host ndarray; a DataFrame (or Series) comes back as one, index and columns kept."""
    import pandas as pd

    out = diffuse_device(G, F, t=t).cpu().numpy()
    if isinstance(F, pd.DataFrame):
        return pd.DataFrame(out, index=F.index, columns=F.columns)
    if isinstance(F, pd.Series):
        return pd.Series(out, index=F.index, name=F.name)
    return out


def impute_refusal(G):
    """Why ``MELD.impute`` cannot run on this graph (a string), or None."""
    info = getattr(G, "info", None) or {}
    if is_sharded(G):
        return "a row-sharded graph cannot impute (every rank holds a slice of the kernel only)"
    st = getattr(G, "_extend_state", None)
    if st is None:
        if info.get("adopted_from") is not None:
            return ("a graph adopted from {} keeps no data to impute: diffuse a signal of your own with "
                    "graph.diffuse(signal, t)".format(info["adopted_from"]))
        return ("this graph was not built from cells by MELD.fit (fit(G), a precomputed matrix, or a graph that does not keep its "
                "cells): it holds no data to impute; diffuse a signal of your own with graph.diffuse(signal, t)")
    if st.row_fn is not None:
        return ("distance={!r} builds its graph on transformed rows: the stored rows are not the data, impute cannot map them back; "
                "diffuse the data yourself with graph.diffuse(signal, t)".format(info.get("metric") or "cosine / correlation"))
    return None


def impute(G, genes=None, t=3):
    """``(values, idx)``: the columns ``idx`` (int64, host) of the data ``fit`` saw after ``t`` steps of diffusion of the matrix
    the graph was searched on, mapped back through the stored model; ``values`` an fp64 device tensor ``[N, len(idx)]`` in the
    caller's cell order."""
    import torch

    t = check_t(t)
    why = impute_refusal(G)
    if why is not None:
        raise NotImplementedError(why)
    st = G._extend_state
    n_features = int(st.n_features_in)
    idx = np.arange(n_features, dtype=np.int64) if genes is None else column_index(genes, n_features, getattr(st, "columns", None))
    Xt = diffuse_device(G, st.X, t=t)
    model = getattr(st, "model", None)
    sel = torch.from_numpy(idx).to(Xt.device)
    if model is None:
        if st.project is not None:
            raise NotImplementedError("this graph keeps its projection as a function only: impute needs the model")
        return Xt.index_select(1, sel), idx
    V = model["V"].to(torch.float64).index_select(0, sel)  # [len(idx), d]
    out = Xt @ V.T  # (one library GEMM)
    if model["kind"] == "pca":
        out += model["mean"].to(torch.float64).reshape(-1).index_select(0, sel)[None, :]
    return out, idx
