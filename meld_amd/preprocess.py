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
           "select", "run"]

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


# ---- the fused route ------------------------------------------------------------------------------------------------------------------------
def run(X, min_library_size=None, max_library_size=None, library_size_percentile=None, min_cells=5, gene_cutoff=0, rescale=10000,
        transform="sqrt", keep_normalized=True, cofactor=5):
    """The notebooks' sequence in one go: cells by library size, genes by capture count over the KEPT cells, library sizes over the
    KEPT genes, then one rewrite that selects, normalises and transforms.

    ``min_library_size`` / ``max_library_size``: strict bounds (``filter_library_size(cutoff=...)``, above / below / between);
    ``library_size_percentile``: a number (keep above) or a pair (between) instead; none of them: every cell stays.  ``min_cells`` /
    ``gene_cutoff``: ``filter_rare_genes`` (``min_cells=None``: every gene stays).  ``rescale``: as ``library_size_normalize`` (None: no
    normalisation at all).  ``transform``: None, "sqrt", "log" (natural), "log2", "log10" or "arcsinh" (``cofactor``).

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
    # 4. one count + scan + fill
    out = select(A, rows=None if rule is None else cells, cols=None if min_cells is None else genes, scale=scale, rescale=value,
                 transform=transform, cofactor=cofactor, keep_normalized=keep_normalized)
    data, normalized = out if keep_normalized else (out, None)
    info.update(shape_after=data.shape, nnz_after=data.nnz, transform=transform, transform_code=code)
    return SimpleNamespace(data=data, normalized=normalized, cells=cells, genes=genes, library_size=libsize, cell_index=data.cell_index,
                           gene_names=data.gene_names, info=info)
