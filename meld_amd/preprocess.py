"""Preprocessing of the counts on the device CSR: filter cells and genes, normalise by library size, transform.

Every notebook of the reference does these steps with scprep before it calls ``meld.MELD()``
(``scprep.filter.filter_library_size``, ``filter_rare_genes``, ``filter_gene_set_expression``,
``scprep.normalize.library_size_normalize``, ``scprep.transform.sqrt``; notebooks/MELD_thresholding.Tcell.ipynb and
notebooks/Wagner2018_Chordin_Cas9_Mutagenesis.ipynb).  Here the raw counts go up once as a ``DeviceCSR`` and csrc/preprocess.hip does
the rest: one pass for the per-cell statistics, one for the per-gene capture counts, one rewrite of the matrix.  Nothing is
densified and nothing but per-cell and per-gene vectors comes back to the host.

* measures: ``library_size``, ``gene_capture_count``, ``gene_set_expression`` (host arrays; ``*_device`` return the tensors);
* filters: ``filter_library_size``, ``filter_gene_set_expression``, ``filter_rare_genes``, ``filter_empty_cells``,
  ``filter_empty_genes`` -> ``(DeviceCSR, kept_indices)``; the indices stand in for scprep's ``*extra_data``: ``labels[kept]``;
* ``library_size_normalize``, ``sqrt``, ``log``, ``arcsinh``;
* per-gene moments and selection: ``gene_mean``, ``gene_variance``, ``gene_variability``, ``highly_variable_genes`` (one launch on the
  gene-major copy ``DeviceCSR.T``; ``gene_moments_device`` returns the tensors, ``variability_from_moments`` is the host rule);
* ``run``: the notebooks' sequence fused -- three statistics passes over the input and ONE rewrite; the transformed matrix for the
  SVD and the normalised one for ``rank_sum_test`` share their structure.  Bit for bit the result of the single functions called
  one after another.

Input everywhere: a ``DeviceCSR``, anything ``DeviceCSR.from_input`` takes, or a dense matrix (numpy, DataFrame, tensor: compressed on
the device).  The labels of a DataFrame or an AnnData-like object travel with the matrix (``DeviceCSR.cell_index`` / ``gene_names``).

The argument checks of this module run before anything touches the device (tests/test_preprocess_host.py).
"""
from __future__ import annotations

import numbers
from types import SimpleNamespace

import numpy as np

__all__ = ["TRANSFORMS", "library_size", "library_size_device", "gene_capture_count", "gene_capture_count_device",
           "gene_set_expression", "gene_set_expression_device", "filter_library_size", "filter_gene_set_expression",
           "filter_rare_genes", "filter_empty_cells", "filter_empty_genes", "library_size_normalize", "sqrt", "log", "arcsinh",
           "select", "run", "gene_moments_device", "gene_mean", "gene_variance", "variability_from_moments", "gene_variability",
           "highly_variable_genes"]

# the transform codes of include/meld_hip.h (MELD_PREP_*)
TRANSFORMS = {None: 0, "identity": 0, "sqrt": 1, "log": 2, "log2": 3, "log10": 4, "arcsinh": 5}
_LOG_BASES = {2: "log2", "e": "log", 10: "log10"}


# ---- argument checks (no device) --------------------------------------------------------------------------------------------------------
def _cutoff_rule(name, cutoff, percentile, keep_cells):
    """scprep's rules: exactly one of ``cutoff`` / ``percentile``; a pair means "between".  Returns (kind, value(s), keep_cells)."""
    if (cutoff is None) == (percentile is None):
        raise ValueError("{}: expected exactly one of `cutoff` and `percentile`, got cutoff={!r}, percentile={!r}".format(name, cutoff, percentile))
    value = cutoff if cutoff is not None else percentile
    if isinstance(value, numbers.Number):
        pair = False
        value = float(value)
    else:
        value = [float(v) for v in value]
        if len(value) != 2:
            raise ValueError("{}: expected a number or a pair (lower, upper), got {!r}".format(name, value))
        pair = True
    if pair:
        keep_cells = "between"
    if keep_cells not in ("above", "below", "between"):
        raise ValueError("{}: expected `keep_cells` in ['above', 'below', 'between'], got {!r}".format(name, keep_cells))
    if keep_cells == "between" and not pair:
        raise ValueError("{}: keep_cells='between' needs a pair (lower, upper)".format(name))
    if percentile is not None and not all(0.0 <= v <= 100.0 for v in (value if pair else [value])):
        raise ValueError("{}: percentile {!r} outside [0, 100]".format(name, percentile))
    return ("cutoff" if cutoff is not None else "percentile"), value, keep_cells


def _keep_mask(values, kind, value, keep_cells):
    """The strict comparisons of scprep on host values; returns (mask, the cutoff(s) used)."""
    cut = np.percentile(values, value) if kind == "percentile" else (np.asarray(value, dtype=np.float64) if keep_cells == "between" else value)
    if keep_cells == "above":
        return values > cut, float(cut)
    if keep_cells == "below":
        return values < cut, float(cut)
    return (values > cut[0]) & (values < cut[1]), (float(cut[0]), float(cut[1]))


def _transform_code(transform):
    if transform not in TRANSFORMS:
        raise ValueError("unknown transform {!r}: expected one of {}".format(transform, sorted(k for k in TRANSFORMS if k)))
    return TRANSFORMS[transform]


def _check_pseudocount(pseudocount, base):
    if pseudocount != 1:
        raise ValueError("log: a sparse matrix takes pseudocount=1 only (log(0 + {}) would not stay zero); got {!r}".format(pseudocount, pseudocount))
    if base not in _LOG_BASES:
        raise ValueError("log: expected base in [2, 'e', 10], got {!r}".format(base))
    return _LOG_BASES[base]


def _check_rescale(rescale):
    if rescale is None or rescale in ("median", "mean"):
        return rescale
    if isinstance(rescale, numbers.Number) and not isinstance(rescale, bool):
        return float(rescale)
    raise ValueError("library_size_normalize: expected rescale in ['median', 'mean'], a number or None, got {!r}".format(rescale))


# ---- the device side --------------------------------------------------------------------------------------------------------------------
def _labels_of(X):
    """(cell_index, gene_names) of a DataFrame or an AnnData-like input, else (None, None)."""
    try:
        import pandas as pd
    except ImportError:  # pragma: no cover
        pd = None
    if pd is not None and isinstance(X, pd.DataFrame):
        return np.asarray(X.index), np.asarray(X.columns)
    if hasattr(X, "obs_names") and hasattr(X, "var_names"):
        return np.asarray(X.obs_names), np.asarray(X.var_names)
    return None, None


def as_device_csr(X, device="cuda"):
    """The input as a ``DeviceCSR`` (itself where it is one), its labels attached."""
    import torch

    from . import sparse as _sp

    if isinstance(X, _sp.DeviceCSR):
        return X
    cells, genes = _labels_of(X)
    if _sp.is_sparse_input(X):
        A = _sp.DeviceCSR.from_input(X, device=device)
    else:
        # dense: uploaded and compressed on the device (as meld_amd/diffexp.py compresses dense input)
        inner = _sp._unwrap(X)
        if isinstance(inner, torch.Tensor):
            D = inner if inner.is_cuda else inner.to(device)
        else:
            arr = np.asarray(getattr(inner, "values", inner))
            if arr.dtype not in (np.float32, np.float64):
                arr = arr.astype(np.float64)
            D = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
        if D.dim() != 2 or D.shape[0] < 1 or D.shape[1] < 1:
            raise ValueError("Expected a non-empty 2D data matrix, got shape {}".format(tuple(D.shape)))
        if D.dtype not in (torch.float32, torch.float64):
            D = D.to(torch.float64)
        if not bool(torch.isfinite(D).all()):
            raise ValueError("Input data contains NaN or infinity")
        S = D.contiguous().to_sparse_csr()
        A = _sp.DeviceCSR(S.crow_indices().to(torch.int64), S.col_indices().to(torch.int32).contiguous(), S.values().contiguous(),
                          (int(D.shape[0]), int(D.shape[1])))
        A._validate()
    A.cell_index, A.gene_names = cells, genes
    return A


def _arrays(A):
    """The operand of the entry points; a matrix without entries has no addresses for col and val: any will do, nothing reads them."""
    import torch

    from ._lib import ptr

    col, val = A.col, A.val
    if A.nnz == 0:
        col = torch.zeros(1, dtype=torch.int32, device=A.device)
        val = torch.zeros(1, dtype=torch.float64, device=A.device)
    return (ptr(A.rowptr), ptr(col), ptr(val), 1 if val.dtype == torch.float32 else 0, A.shape[0], A.shape[1]), (col, val)


def row_stats_device(A, col_mask=None, cutoff=0.0):
    """``(sum, abs_sum, count)`` of every row (fp64, fp64, int32 device tensors [N]) from one launch of ``meld_prep_row_stats``;
    ``col_mask``: a uint8 / bool device tensor [G], the statistics then cover its columns only."""
    import torch

    from ._device_ops import stream
    from ._lib import check, get_lib, ptr

    N, G = A.shape
    dev = A.device
    s = torch.empty(N, dtype=torch.float64, device=dev)
    a = torch.empty(N, dtype=torch.float64, device=dev)
    c = torch.empty(N, dtype=torch.int32, device=dev)
    if col_mask is not None:
        col_mask = col_mask.to(device=dev, dtype=torch.uint8).contiguous()
        if int(col_mask.shape[0]) != G:
            raise ValueError("row_stats: a column mask of {} entries for {} columns".format(int(col_mask.shape[0]), G))
    mat, hold = _arrays(A)
    check(get_lib().meld_prep_row_stats(*mat, ptr(col_mask), float(cutoff), ptr(s), ptr(a), ptr(c), stream()), "meld_prep_row_stats")
    del hold
    return s, a, c


def col_counts_device(A, row_keep=None, cutoff=0.0):
    """int32 device tensor [G]: per column the entries above ``cutoff`` in the rows ``row_keep`` keeps (uint8 / bool [N]; None: all)."""
    import torch

    from ._device_ops import stream
    from ._lib import check, get_lib, ptr

    N, G = A.shape
    count = torch.zeros(G, dtype=torch.int32, device=A.device)
    if row_keep is not None:
        row_keep = row_keep.to(device=A.device, dtype=torch.uint8).contiguous()
        if int(row_keep.shape[0]) != N:
            raise ValueError("col_counts: a row mask of {} entries for {} rows".format(int(row_keep.shape[0]), N))
    mat, hold = _arrays(A)
    check(get_lib().meld_prep_col_counts(*mat, ptr(row_keep), float(cutoff), ptr(count), stream()), "meld_prep_col_counts")
    del hold
    return count


def select(A, rows=None, cols=None, scale=None, rescale=1.0, transform=None, cofactor=5.0, keep_normalized=False):
    """The one rewrite (``meld_prep_select_count``, the scan, ``meld_prep_select_fill``): rows ``rows`` and columns ``cols`` of ``A``
    (ascending host int arrays; None: all), the values ``f((v / scale[i]) * rescale)`` (``scale``: fp64 device tensor per kept row or
    None: ``f(v)``).  Returns the ``DeviceCSR`` (fp64 values), or ``(transformed, normalized)`` sharing ``rowptr`` and ``col`` with
    ``keep_normalized``."""
    import torch

    from . import sparse as _sp
    from ._device_ops import scan_i32, stream
    from ._lib import check, get_lib, ptr

    code = _transform_code(transform)
    lib, st, dev = get_lib(), stream(), A.device
    N, G = A.shape
    if rows is None:
        rows_d = torch.arange(N, dtype=torch.int32, device=dev)
        rows_h = None
    else:
        rows_h = np.asarray(rows, dtype=np.int64)
        rows_d = torch.from_numpy(rows_h.astype(np.int32)).to(dev)
    n_keep = int(rows_d.shape[0])
    col_map, n_cols_out, cols_h = None, G, None
    if cols is not None:
        cols_h = np.asarray(cols, dtype=np.int64)
        n_cols_out = int(cols_h.shape[0])
        col_map = torch.full((G,), -1, dtype=torch.int32, device=dev)
        col_map[torch.from_numpy(cols_h).to(dev)] = torch.arange(n_cols_out, dtype=torch.int32, device=dev)
    if n_keep < 1 or n_cols_out < 1:
        raise ValueError("select: nothing to keep ({} rows, {} columns)".format(n_keep, n_cols_out))
    if scale is not None:
        scale = scale.to(device=dev, dtype=torch.float64).contiguous()
        if int(scale.shape[0]) != n_keep:
            raise ValueError("select: {} scales for {} kept rows".format(int(scale.shape[0]), n_keep))
    mat, hold = _arrays(A)
    counts = torch.empty(n_keep, dtype=torch.int32, device=dev)
    check(lib.meld_prep_select_count(mat[0], mat[1], N, G, ptr(rows_d), n_keep, ptr(col_map), ptr(counts), st), "meld_prep_select_count")
    rowptr = scan_i32(counts)
    nnz = int(rowptr[-1])
    out_col = torch.empty(nnz, dtype=torch.int32, device=dev)
    out_val = torch.empty(nnz, dtype=torch.float64, device=dev)
    out_norm = torch.empty(nnz, dtype=torch.float64, device=dev) if keep_normalized else None
    if nnz:
        check(lib.meld_prep_select_fill(*mat, ptr(rows_d), n_keep, ptr(col_map), ptr(scale), float(rescale), code, float(cofactor),
                                        ptr(rowptr), ptr(out_col), ptr(out_val), ptr(out_norm), st), "meld_prep_select_fill")
    del hold, counts
    cells = A.cell_index if rows_h is None or A.cell_index is None else np.asarray(A.cell_index)[rows_h]
    genes = A.gene_names if cols_h is None or A.gene_names is None else np.asarray(A.gene_names)[cols_h]
    out = _sp.DeviceCSR(rowptr, out_col, out_val, (n_keep, n_cols_out))
    out.cell_index, out.gene_names = cells, genes
    if not keep_normalized:
        return out
    norm = _sp.DeviceCSR(rowptr, out_col, out_norm, (n_keep, n_cols_out))
    norm.cell_index, norm.gene_names = cells, genes
    return out, norm


def _gene_mask(A, genes):
    """``genes`` (boolean mask, integer indices, or names where the matrix carries column names) as a host bool mask [G]."""
    G = A.shape[1]
    g = np.asarray(getattr(genes, "values", genes))
    if g.ndim != 1:
        raise ValueError("genes: expected a 1D mask, index list or list of names, got shape {}".format(g.shape))
    if g.dtype == np.bool_:
        if g.shape[0] != G:
            raise ValueError("genes: a mask of {} entries for {} genes".format(g.shape[0], G))
        return g.copy()
    if g.dtype.kind not in "iu":
        if A.gene_names is None:
            raise ValueError("genes: names were given but the matrix carries no gene names")
        import pandas as pd

        idx = pd.Index(A.gene_names).get_indexer(g)
        if (idx < 0).any():
            raise ValueError("genes: {!r} not among the gene names".format(list(g[idx < 0][:5])))
        g = idx
    if g.size and (g.min() < -G or g.max() >= G):
        raise ValueError("genes: index outside [0, {})".format(G))
    mask = np.zeros(G, dtype=bool)
    mask[g] = True
    return mask


# ---- measures -------------------------------------------------------------------------------------------------------------------------------
def library_size_device(X):
    return row_stats_device(as_device_csr(X))[0]


def library_size(X):
    """The sum of every cell's values (``scprep.measure.library_size``): fp64 [N] on the host."""
    return library_size_device(X).cpu().numpy()


def gene_capture_count_device(X, cutoff=0):
    return col_counts_device(as_device_csr(X), None, cutoff).long()


def gene_capture_count(X, cutoff=0):
    """The number of cells in which each gene exceeds ``cutoff`` (``scprep.measure.gene_capture_count``): int64 [G] on the host."""
    return gene_capture_count_device(X, cutoff).cpu().numpy()


def gene_set_expression_device(X, genes):
    import torch

    A = as_device_csr(X)
    mask = torch.from_numpy(_gene_mask(A, genes).astype(np.uint8)).to(A.device)
    return row_stats_device(A, mask)[0]


def gene_set_expression(X, genes):
    """The sum of every cell's values over ``genes`` (``scprep.measure.gene_set_expression`` with its default ``library_size_normalize
    =False``): fp64 [N] on the host."""
    return gene_set_expression_device(X, genes).cpu().numpy()


# ---- filters --------------------------------------------------------------------------------------------------------------------------------
def _kept(name, mask, what):
    kept = np.flatnonzero(mask).astype(np.int64)
    if kept.shape[0] == 0:
        raise ValueError("{}: the filter leaves no {}".format(name, what))
    return kept


def filter_library_size(X, cutoff=None, percentile=None, keep_cells="above"):
    """``scprep.filter.filter_library_size``: keep the cells whose library size is above (``>``) / below (``<``) the cutoff, or
    strictly between a pair; ``percentile``: ``np.percentile`` of the library sizes instead.  Returns ``(DeviceCSR, kept)``."""
    rule = _cutoff_rule("filter_library_size", cutoff, percentile, keep_cells)
    A = as_device_csr(X)
    mask, _ = _keep_mask(library_size(A), *rule)
    kept = _kept("filter_library_size", mask, "cell")
    return select(A, rows=kept), kept


def filter_gene_set_expression(X, genes, cutoff=None, percentile=None, keep_cells="below"):
    """``scprep.filter.filter_gene_set_expression``: the same rules on the summed expression of ``genes`` (the notebooks drop cells
    rich in mitochondrial genes with it)."""
    rule = _cutoff_rule("filter_gene_set_expression", cutoff, percentile, keep_cells)
    A = as_device_csr(X)
    mask, _ = _keep_mask(gene_set_expression(A, genes), *rule)
    kept = _kept("filter_gene_set_expression", mask, "cell")
    return select(A, rows=kept), kept


def filter_rare_genes(X, cutoff=0, min_cells=5):
    """``scprep.filter.filter_rare_genes``: keep the genes that exceed ``cutoff`` in at least ``min_cells`` cells."""
    A = as_device_csr(X)
    kept = _kept("filter_rare_genes", gene_capture_count(A, cutoff) >= min_cells, "gene")
    return select(A, cols=kept), kept


def filter_empty_cells(X):
    """``scprep.filter.filter_empty_cells``: keep the cells of positive library size."""
    A = as_device_csr(X)
    kept = _kept("filter_empty_cells", library_size(A) > 0, "cell")
    return select(A, rows=kept), kept


def filter_empty_genes(X):
    """Keep the genes with a positive value in at least one cell (``scprep.filter.filter_empty_genes`` on non-negative data, where a
    positive column sum is the same thing; per-gene sums are not computed here)."""
    A = as_device_csr(X)
    kept = _kept("filter_empty_genes", gene_capture_count(A, 0) >= 1, "gene")
    return select(A, cols=kept), kept


# ---- normalisation and transforms -----------------------------------------------------------------------------------------------------------
def _rescale_value(rescale, libsize):
    if rescale == "median":
        return float(np.median(libsize))
    if rescale == "mean":
        return float(np.mean(libsize))
    return 1.0 if rescale is None else float(rescale)


def library_size_normalize(X, rescale=10000, return_library_size=False):
    """``scprep.normalize.library_size_normalize``: every cell divided by the sum of its magnitudes (sklearn's l1 ``normalize``: a
    cell without any keeps its values) and multiplied by ``rescale`` -- a number, ``"median"`` or ``"mean"`` (of the library sizes,
    taken with numpy on the host) or None for 1.  The library size returned on request is the plain sum of the cell."""
    rescale = _check_rescale(rescale)
    A = as_device_csr(X)
    s, a, _ = row_stats_device(A)
    libsize = s.cpu().numpy()
    out = select(A, scale=a, rescale=_rescale_value(rescale, libsize))
    return (out, libsize) if return_library_size else out


def sqrt(X):
    """``scprep.transform.sqrt``; ValueError on negative values."""
    A = as_device_csr(X)
    if A.nnz and bool((A.val < 0).any()):
        raise ValueError("sqrt: cannot take the square root of negative values")
    return select(A, transform="sqrt")


def log(X, pseudocount=1, base=10):
    """``scprep.transform.log``: log(x + 1) in base 2, "e" or 10.  ValueError for ``pseudocount != 1``, as scprep raises for a sparse
    matrix: the zeros would not stay zero."""
    name = _check_pseudocount(pseudocount, base)
    A = as_device_csr(X)
    if A.nnz and bool((A.val <= -1).any()):
        raise ValueError("log: values of -1 or below have no logarithm after the pseudocount")
    return select(A, transform=name)


def arcsinh(X, cofactor=5):
    """``scprep.transform.arcsinh``: asinh(x / cofactor)."""
    if not cofactor > 0:
        raise ValueError("arcsinh: expected cofactor > 0, got {!r}".format(cofactor))
    return select(as_device_csr(X), transform="arcsinh", cofactor=cofactor)


# ---- per-gene moments and highly variable genes ---------------------------------------------------------------------------------------------
def _check_ddof(name, ddof):
    if isinstance(ddof, bool) or ddof not in (0, 1):
        raise ValueError("{}: expected ddof in [0, 1], got {!r}".format(name, ddof))
    return int(ddof)


def _check_kernel(name, kernel_size, smooth):
    """``kernel_size``: an odd integer >= 1 (genes) or a fraction in (0, 1] of the genes; ``smooth``: an integer >= 0."""
    if isinstance(kernel_size, bool) or not isinstance(kernel_size, numbers.Real):
        raise ValueError("{}: expected `kernel_size` an odd integer or a fraction of the genes, got {!r}".format(name, kernel_size))
    if isinstance(kernel_size, numbers.Integral):
        if kernel_size < 1 or kernel_size % 2 == 0:
            raise ValueError("{}: an integer `kernel_size` must be odd and at least 1, got {!r}".format(name, kernel_size))
    elif not 0.0 < kernel_size <= 1.0:
        raise ValueError("{}: a fractional `kernel_size` must lie in (0, 1], got {!r}".format(name, kernel_size))
    if isinstance(smooth, bool) or not isinstance(smooth, numbers.Integral) or smooth < 0:
        raise ValueError("{}: expected `smooth` an integer >= 0, got {!r}".format(name, smooth))


def _check_n_top(name, n_top_genes, G=None):
    if isinstance(n_top_genes, bool) or not isinstance(n_top_genes, numbers.Integral) or n_top_genes < 1 or (G is not None and n_top_genes > G):
        raise ValueError("{}: expected `n_top_genes` an integer in [1, {}], got {!r}".format(name, "G" if G is None else G, n_top_genes))
    return int(n_top_genes)


def _hvg_rule(name, cutoff, percentile, n_top_genes, G=None):
    """Exactly one of the three rules: ("cutoff" | "percentile", value, "above") as ``_cutoff_rule`` returns it, or ("n_top_genes", n)."""
    given = [k for k, v in (("cutoff", cutoff), ("percentile", percentile), ("n_top_genes", n_top_genes)) if v is not None]
    if len(given) != 1:
        raise ValueError("{}: expected exactly one of `cutoff`, `percentile` and `n_top_genes`, got {}".format(name, given or "none"))
    if n_top_genes is not None:
        return ("n_top_genes", _check_n_top(name, n_top_genes, G))
    if not isinstance(cutoff if cutoff is not None else percentile, numbers.Number):
        raise ValueError("{}: expected a number for `{}`".format(name, given[0]))
    return _cutoff_rule(name, cutoff, percentile, "above")


def _hvg_keep(name, variability, rule):
    """The rule on host variabilities: (bool mask, the cutoff used -- for ``n_top_genes`` the smallest variability kept)."""
    if rule[0] == "n_top_genes":
        n = _check_n_top(name, rule[1], variability.shape[0])
        top = np.argsort(-variability, kind="stable")[:n]  # ties go to the lower gene index
        mask = np.zeros(variability.shape[0], dtype=bool)
        mask[top] = True
        return mask, float(variability[top[-1]])
    return _keep_mask(variability, *rule)


def _input_genes(X):
    """The number of genes where the input states it without the device (else None)."""
    shape = getattr(X, "shape", None)
    return int(shape[1]) if shape is not None and len(shape) == 2 else None


def _moments(T, n_kept, row_keep=None, row_scale=None, rescale=1.0, code=0, cofactor=5.0, gene_mask=None, ddof=1):
    """One launch of ``meld_prep_gene_moments`` on the gene-major ``DeviceCSR`` ``T`` [G, N]."""
    import torch

    from ._device_ops import stream
    from ._lib import check, get_lib, ptr

    G, N = T.shape
    dev = T.device
    if n_kept < 1 or n_kept - ddof < 1:
        raise ValueError("gene_moments: {} kept cells leave nothing to average with ddof={}".format(n_kept, ddof))

    def vector(x, dtype, n, what):
        if x is None:
            return None
        x = (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(device=dev, dtype=dtype).contiguous()
        if x.dim() != 1 or int(x.shape[0]) != n:
            raise ValueError("gene_moments: `{}` of shape {} for {} {}".format(what, tuple(x.shape), n, "cells" if n == N else "genes"))
        return x

    row_keep = vector(row_keep, torch.uint8, N, "row_keep")
    row_scale = vector(row_scale, torch.float64, N, "row_scale")
    gene_mask = vector(gene_mask, torch.uint8, G, "gene_mask")
    count = torch.empty(G, dtype=torch.int32, device=dev)
    mean = torch.empty(G, dtype=torch.float64, device=dev)
    var = torch.empty(G, dtype=torch.float64, device=dev)
    mat, hold = _arrays(T)
    check(get_lib().meld_prep_gene_moments(*mat, ptr(row_keep), ptr(row_scale), float(rescale), code, float(cofactor), ptr(gene_mask),
                                           int(n_kept), ddof, ptr(count), ptr(mean), ptr(var), stream()), "meld_prep_gene_moments")
    del hold
    return count, mean, var


def _is_host_csc(X):
    from . import sparse as _sp

    if isinstance(X, _sp.DeviceCSR):
        return False
    inner = _sp._unwrap(X)
    return bool(_sp._scipy_sparse().issparse(inner) and inner.format == "csc")


def _gene_major(X):
    """The gene-major copy of the input: ``as_device_csr(X).T`` (cached on a ``DeviceCSR``); the arrays of a host
    ``scipy.sparse.csc_matrix`` ARE that copy and go up as they are (the route of meld_amd/diffexp.py)."""
    if _is_host_csc(X):
        from .diffexp import _gene_major as upload_csc

        return upload_csc(X)
    return as_device_csr(X).T


def gene_moments_device(X, row_keep=None, row_scale=None, rescale=1.0, transform=None, cofactor=5.0, gene_mask=None, ddof=1):
    """``(count, mean, var)`` of every gene over the kept cells: int32, fp64, fp64 device tensors [G], one launch of
    ``meld_prep_gene_moments`` on the gene-major copy of ``X`` (``DeviceCSR.T``, transposed on first use and cached).

    ``row_keep``: bool / uint8 [N] (None: every cell).  ``row_scale``: fp64 [N], with ``rescale``, ``transform`` and ``cofactor``
    the value map of ``select``: the moments are those of ``f((v / row_scale[i]) * rescale)`` without that matrix being written.
    ``gene_mask``: bool / uint8 [G], a gene outside it gets ``count = -1`` and zeros.  ``ddof``: 0 or 1.  ``count`` is the number of
    stored entries in kept cells; the variance is a two-pass one, the implicit zeros included."""
    import torch

    code = _transform_code(transform)
    ddof = _check_ddof("gene_moments", ddof)
    if code == TRANSFORMS["arcsinh"] and not cofactor > 0:
        raise ValueError("gene_moments: expected cofactor > 0, got {!r}".format(cofactor))
    if isinstance(rescale, bool) or not isinstance(rescale, numbers.Real):
        raise ValueError("gene_moments: expected a number for `rescale`, got {!r}".format(rescale))
    T = _gene_major(X)
    if row_keep is None:
        n_kept = T.shape[1]
    elif isinstance(row_keep, torch.Tensor):
        n_kept = int((row_keep != 0).sum())
    else:
        n_kept = int(np.count_nonzero(np.asarray(row_keep)))
    return _moments(T, n_kept, row_keep, row_scale, rescale, code, cofactor, gene_mask, ddof)


def gene_mean(X):
    """The mean of every gene over all cells: fp64 [G] on the host."""
    return gene_moments_device(X, ddof=0)[1].cpu().numpy()


def gene_variance(X, ddof=1):
    """The variance of every gene over all cells (two passes, implicit zeros included): fp64 [G] on the host."""
    ddof = _check_ddof("gene_variance", ddof)
    return gene_moments_device(X, ddof=ddof)[2].cpu().numpy()


def variability_from_moments(mean, var, kernel_size=0.005, smooth=5):
    """The variability of genes from their means and variances: the variance minus the variance EXPECTED of a gene of that mean.

    Restates ``scprep.measure.gene_variability`` from its documentation (a rolling median of the mean-variance curve, smoothed);
    where scprep differs in a detail, THIS is the definition (tests/hvg_reference.py restates it):

    * ``order``: the stable argsort of ``mean`` (ties: the lower gene index first);
    * ``k``: ``kernel_size`` itself where it is an integer >= 1 (odd, else ValueError), else ``2 * (int(kernel_size * G) // 2) + 1``;
    * expected variance: ``scipy.signal.medfilt(var[order], k)`` (zeros beyond the ends), then ``smooth`` passes of a three-point
      mean ``((left + centre) + right) / 3`` with the end values replicated;
    * variability: ``var - expected``, scattered back to gene order.

    A host function on two fp64 arrays [G]; returns fp64 [G]."""
    from scipy.signal import medfilt

    _check_kernel("gene_variability", kernel_size, smooth)
    mean = np.asarray(mean, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    if mean.ndim != 1 or mean.shape != var.shape or mean.shape[0] < 1:
        raise ValueError("gene_variability: expected two vectors of one length, got shapes {} and {}".format(mean.shape, var.shape))
    G = mean.shape[0]
    k = int(kernel_size) if isinstance(kernel_size, numbers.Integral) else 2 * (int(kernel_size * G) // 2) + 1
    order = np.argsort(mean, kind="stable")
    expected = medfilt(var[order], k)
    for _ in range(smooth):
        padded = np.concatenate([expected[:1], expected, expected[-1:]])
        expected = ((padded[:-2] + padded[1:-1]) + padded[2:]) / 3.0
    out = np.empty(G, dtype=np.float64)
    out[order] = var[order] - expected
    return out


def gene_variability(X, kernel_size=0.005, smooth=5, return_means=False):
    """``scprep.measure.gene_variability`` as ``variability_from_moments`` defines it, from the device moments (``ddof=1``): fp64
    [G] on the host, or ``(variability, means)``."""
    _check_kernel("gene_variability", kernel_size, smooth)
    _, mean, var = gene_moments_device(X)
    mean = mean.cpu().numpy()
    v = variability_from_moments(mean, var.cpu().numpy(), kernel_size, smooth)
    return (v, mean) if return_means else v


def highly_variable_genes(X, kernel_size=0.05, smooth=5, cutoff=None, percentile=80, n_top_genes=None):
    """``scprep.select.highly_variable_genes``: keep the genes whose variability is above (``>``) ``cutoff``, above the
    ``percentile`` of the variabilities, or the ``n_top_genes`` most variable ones (ties: the lower gene index).  Exactly one rule:
    ``percentile=80`` is the default only while the other two are None.  Returns ``(DeviceCSR, kept)``.  The first call on a matrix
    transposes it (cached as ``DeviceCSR.T``)."""
    name = "highly_variable_genes"
    _check_kernel(name, kernel_size, smooth)
    if (cutoff is not None or n_top_genes is not None) and percentile == 80:
        percentile = None
    rule = _hvg_rule(name, cutoff, percentile, n_top_genes, _input_genes(X))
    src = X if _is_host_csc(X) else as_device_csr(X)  # (one upload; a CSC input's own arrays serve the moments)
    _, mean, var = gene_moments_device(src)
    v = variability_from_moments(mean.cpu().numpy(), var.cpu().numpy(), kernel_size, smooth)
    mask, _ = _hvg_keep(name, v, rule)
    kept = _kept(name, mask, "gene")
    return select(as_device_csr(src), cols=kept), kept


# ---- the fused route ------------------------------------------------------------------------------------------------------------------------
def run(X, min_library_size=None, max_library_size=None, library_size_percentile=None, min_cells=5, gene_cutoff=0, rescale=10000,
        transform="sqrt", keep_normalized=True, cofactor=5, hvg_percentile=None, hvg_cutoff=None, n_top_genes=None, hvg_kernel_size=0.05,
        hvg_smooth=5):
    """The notebooks' sequence in one go: cells by library size, genes by capture count over the KEPT cells, library sizes over the
    KEPT genes, then one rewrite that selects, normalises and transforms.

    ``min_library_size`` / ``max_library_size``: strict bounds (``filter_library_size(cutoff=...)``, above / below / between);
    ``library_size_percentile``: a number (keep above) or a pair (between) instead; none of them: every cell stays.  ``min_cells`` /
    ``gene_cutoff``: ``filter_rare_genes`` (``min_cells=None``: every gene stays).  ``rescale``: as ``library_size_normalize`` (None: no
    normalisation at all).  ``transform``: None, "sqrt", "log" (natural), "log2", "log10" or "arcsinh" (``cofactor``).

    ``hvg_percentile`` / ``hvg_cutoff`` / ``n_top_genes`` (at most one; none: nothing below happens, no transposition, no further
    launch): ``highly_variable_genes`` with ``hvg_kernel_size`` / ``hvg_smooth`` on the normalised and transformed values of the
    kept cells, over the genes that passed ``min_cells`` -- one moments launch on the input's gene-major copy (``DeviceCSR.T``,
    transposed on first use) between the library sizes and the rewrite, which then writes the selected genes only.  The cells are
    still normalised by their library size over the genes of ``min_cells`` (normalise, then select), and ``library_size`` stays
    over those; ``genes`` are the selected ones; ``info["hvg"]`` holds ``mean``, ``variance``, ``variability`` (host, over
    ``info["hvg"]["genes"]``, the genes of ``min_cells``), the ``rule`` and the ``cutoff`` used.

    Returns a record: ``data`` (``DeviceCSR``, transformed), ``normalized`` (shares ``rowptr`` and ``col`` with ``data``; None unless
    ``keep_normalized``), ``cells`` / ``genes`` (host int64 indices into the input), ``library_size`` (kept cells over kept genes,
    host), ``cell_index`` / ``gene_names`` (kept labels, or None) and ``info``.  ValueError naming the filter that would leave no
    cell or no gene."""
    import torch

    code = _transform_code(transform)
    rescale = _check_rescale(rescale)
    cutoffs = [c for c in (min_library_size, max_library_size) if c is not None]
    if cutoffs and library_size_percentile is not None:
        raise ValueError("run: expected library-size bounds or `library_size_percentile`, not both")
    rule = None
    if library_size_percentile is not None:
        rule = _cutoff_rule("run", None, library_size_percentile, "above")
    elif len(cutoffs) == 2:
        rule = _cutoff_rule("run", (min_library_size, max_library_size), None, "between")
    elif cutoffs:
        rule = _cutoff_rule("run", cutoffs[0], None, "above" if min_library_size is not None else "below")
    if transform == "arcsinh" and not cofactor > 0:
        raise ValueError("run: expected cofactor > 0, got {!r}".format(cofactor))
    hvg = None
    if hvg_percentile is not None or hvg_cutoff is not None or n_top_genes is not None:
        _check_kernel("run (highly_variable_genes)", hvg_kernel_size, hvg_smooth)
        hvg = _hvg_rule("run (highly_variable_genes)", hvg_cutoff, hvg_percentile, n_top_genes, _input_genes(X))

    A = as_device_csr(X)
    N, G = A.shape
    dev = A.device
    info = dict(shape_before=(N, G), nnz_before=A.nnz, library_size_cutoff=None, min_cells=min_cells, gene_cutoff=gene_cutoff)
    # 1. cells by library size
    cells = np.arange(N, dtype=np.int64)
    row_keep = None
    if rule is not None:
        mask, info["library_size_cutoff"] = _keep_mask(row_stats_device(A)[0].cpu().numpy(), *rule)
        cells = _kept("run (filter_library_size)", mask, "cell")
        row_keep = torch.from_numpy(mask.astype(np.uint8)).to(dev)
    # 2. genes by capture count over the kept cells
    genes = np.arange(G, dtype=np.int64)
    col_mask = None
    if min_cells is not None:
        gmask = col_counts_device(A, row_keep, gene_cutoff).cpu().numpy() >= min_cells
        genes = _kept("run (filter_rare_genes)", gmask, "gene")
        col_mask = torch.from_numpy(gmask.astype(np.uint8)).to(dev)
    # 3. library sizes over the kept genes (the sums of the rows the rewrite is about to leave, bit for bit)
    scale, value = None, 1.0
    s, a, _ = row_stats_device(A, col_mask)
    idx = torch.from_numpy(cells).to(dev)
    libsize = s[idx].cpu().numpy()
    if rescale is not None:
        scale = a[idx].contiguous()
        value = _rescale_value(rescale, libsize)
    info["rescale"] = value if rescale is not None else None
    # 3 1/2. highly variable genes among the genes of step 2: the moments of the values the rewrite WOULD leave, from the input's
    # gene-major copy (normalise, then select: the scales above stay those over the genes of step 2)
    if hvg is not None:
        name = "run (highly_variable_genes)"
        _, mean, var = _moments(A.T, len(cells), row_keep, None if rescale is None else a, value, code, cofactor, col_mask, 1)
        passed = torch.from_numpy(genes).to(dev)
        mean, var = mean[passed].cpu().numpy(), var[passed].cpu().numpy()
        variability = variability_from_moments(mean, var, hvg_kernel_size, hvg_smooth)
        mask, cut = _hvg_keep(name, variability, hvg)
        info["hvg"] = dict(mean=mean, variance=var, variability=variability, rule=hvg[0], cutoff=cut, genes=genes)
        genes = genes[_kept(name, mask, "gene")]
    # 4. one count + scan + fill
    out = select(A, rows=None if rule is None else cells, cols=None if min_cells is None and hvg is None else genes, scale=scale,
                 rescale=value, transform=transform, cofactor=cofactor, keep_normalized=keep_normalized)
    data, normalized = out if keep_normalized else (out, None)
    info.update(shape_after=data.shape, nnz_after=data.nnz, transform=transform, transform_code=code)
    return SimpleNamespace(data=data, normalized=normalized, cells=cells, genes=genes, library_size=libsize, cell_index=data.cell_index,
                           gene_names=data.gene_names, info=info)
