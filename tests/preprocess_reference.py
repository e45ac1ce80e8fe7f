"""Host restatement of meld_amd/preprocess.py in numpy / scipy, written from the semantics of scprep (which cannot be imported next to
this code) and checked against scipy and sklearn by tests/test_preprocess_reference.py.

One function per public function of the module, on a canonical ``scipy.sparse.csr_matrix``.  Filters return ``(matrix, kept)``.
The value map is ``(v / s) * r`` with ``np.sqrt`` / ``np.log`` / ``np.log2`` / ``np.log10`` / ``np.arcsinh``, operation by operation
as csrc/preprocess.hip states it."""
from types import SimpleNamespace

import numpy as np
from scipy import sparse


def standard_matrix(N=300, G=500, seed=0):
    """Poisson counts of genes with log-normal rates in cells with log-normal depths: density 7.4 %, row lengths 10 to 104."""
    rng = np.random.default_rng(seed)
    rates = np.exp(rng.normal(-3.5, 1.5, size=G))
    depths = np.exp(rng.normal(0.0, 0.5, size=N))
    X = sparse.csr_matrix(rng.poisson(depths[:, None] * rates[None, :]).astype(np.float64))
    X.sort_indices()
    return X


def _row_of_entry(X):
    return np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))


# ---- measures -------------------------------------------------------------------------------------------------------------------------------
def library_size(X):
    return np.bincount(_row_of_entry(X), weights=X.data.astype(np.float64), minlength=X.shape[0])


def abs_library_size(X):
    return np.bincount(_row_of_entry(X), weights=np.abs(X.data.astype(np.float64)), minlength=X.shape[0])


def gene_capture_count(X, cutoff=0, rows=None):
    sel = X.data > cutoff
    if rows is not None:
        sel &= np.asarray(rows, dtype=bool)[_row_of_entry(X)]
    return np.bincount(X.indices[sel], minlength=X.shape[1]).astype(np.int64)


def gene_mask(X, genes):
    g = np.asarray(genes)
    if g.dtype == np.bool_:
        return g
    mask = np.zeros(X.shape[1], dtype=bool)
    mask[g] = True
    return mask


def gene_set_expression(X, genes):
    sel = gene_mask(X, genes)[X.indices]
    return np.bincount(_row_of_entry(X)[sel], weights=X.data[sel].astype(np.float64), minlength=X.shape[0])


def row_stats_long(X, col_mask=None, cutoff=0.0):
    """(sum, abs_sum) in long double, count, and the number of counted entries per row: what the tolerance of the device sums is
    stated against."""
    sel = np.ones(X.nnz, dtype=bool) if col_mask is None else np.asarray(col_mask, dtype=bool)[X.indices]
    r = _row_of_entry(X)[sel]
    v = X.data[sel].astype(np.longdouble)
    s = np.zeros(X.shape[0], dtype=np.longdouble)
    a = np.zeros(X.shape[0], dtype=np.longdouble)
    np.add.at(s, r, v)
    np.add.at(a, r, np.abs(v))
    count = np.bincount(r[X.data[sel] > cutoff], minlength=X.shape[0]).astype(np.int32)
    return s, a, count, np.bincount(r, minlength=X.shape[0])


# ---- filters --------------------------------------------------------------------------------------------------------------------------------
def keep_mask(values, cutoff=None, percentile=None, keep_cells="above"):
    if (cutoff is None) == (percentile is None):
        raise ValueError("exactly one of cutoff and percentile")
    cut = cutoff if cutoff is not None else np.percentile(values, percentile)
    if np.ndim(cut) == 1:
        keep_cells = "between"
    if keep_cells == "above":
        return values > cut
    if keep_cells == "below":
        return values < cut
    if keep_cells == "between":
        return (values > cut[0]) & (values < cut[1])
    raise ValueError(keep_cells)


def select(X, rows=None, cols=None):
    """Rows and columns by explicit loops over the entries (checked against scipy's slicing by the tests)."""
    rows = np.arange(X.shape[0]) if rows is None else np.asarray(rows)
    new_col = np.arange(X.shape[1]) if cols is None else np.full(X.shape[1], -1, dtype=np.int64)
    if cols is not None:
        new_col[np.asarray(cols)] = np.arange(len(cols))
    indptr, indices, data = [0], [], []
    for i in rows:
        for e in range(X.indptr[i], X.indptr[i + 1]):
            c = new_col[X.indices[e]]
            if c >= 0:
                indices.append(c)
                data.append(X.data[e])
        indptr.append(len(indices))
    n_cols = X.shape[1] if cols is None else len(cols)
    return sparse.csr_matrix((np.asarray(data, dtype=np.float64), np.asarray(indices, dtype=np.int32), np.asarray(indptr, dtype=np.int64)),
                             shape=(len(rows), n_cols))


def filter_library_size(X, cutoff=None, percentile=None, keep_cells="above"):
    kept = np.flatnonzero(keep_mask(library_size(X), cutoff, percentile, keep_cells))
    return select(X, rows=kept), kept


def filter_gene_set_expression(X, genes, cutoff=None, percentile=None, keep_cells="below"):
    kept = np.flatnonzero(keep_mask(gene_set_expression(X, genes), cutoff, percentile, keep_cells))
    return select(X, rows=kept), kept


def filter_rare_genes(X, cutoff=0, min_cells=5):
    kept = np.flatnonzero(gene_capture_count(X, cutoff) >= min_cells)
    return select(X, cols=kept), kept


def filter_empty_cells(X):
    kept = np.flatnonzero(library_size(X) > 0)
    return select(X, rows=kept), kept


def filter_empty_genes(X):
    kept = np.flatnonzero(gene_capture_count(X, 0) >= 1)
    return select(X, cols=kept), kept


# ---- normalisation and transforms -----------------------------------------------------------------------------------------------------------
def rescale_value(rescale, libsize):
    if rescale == "median":
        return float(np.median(libsize))
    if rescale == "mean":
        return float(np.mean(libsize))
    return 1.0 if rescale is None else float(rescale)


def library_size_normalize(X, rescale=10000, return_library_size=False):
    libsize = library_size(X)
    s = abs_library_size(X)
    s = np.where(s == 0, 1.0, s)  # sklearn: a row without magnitude is left alone
    r = rescale_value(rescale, libsize)
    out = X.astype(np.float64)
    out.data = (out.data / s[_row_of_entry(X)]) * r
    return (out, libsize) if return_library_size else out


def _mapped(X, f):
    out = X.astype(np.float64)
    out.data = f(out.data)
    return out


def sqrt(X):
    if (X.data < 0).any():
        raise ValueError("negative values")
    return _mapped(X, np.sqrt)


def log(X, pseudocount=1, base=10):
    if pseudocount != 1:
        raise ValueError("pseudocount")
    f = {2: np.log2, "e": np.log, 10: np.log10}[base]
    return _mapped(X, lambda v: f(v + 1.0))


def arcsinh(X, cofactor=5):
    return _mapped(X, lambda v: np.arcsinh(v / float(cofactor)))


TRANSFORMS = {None: lambda X: X.astype(np.float64), "sqrt": sqrt, "log": lambda X: log(X, base="e"), "log2": lambda X: log(X, base=2),
              "log10": lambda X: log(X, base=10), "arcsinh": arcsinh}


def run(X, min_library_size=None, max_library_size=None, library_size_percentile=None, min_cells=5, gene_cutoff=0, rescale=10000,
        transform="sqrt"):
    cells = np.arange(X.shape[0])
    Y = X
    if library_size_percentile is not None:
        Y, cells = filter_library_size(X, percentile=library_size_percentile)
    elif min_library_size is not None and max_library_size is not None:
        Y, cells = filter_library_size(X, cutoff=(min_library_size, max_library_size))
    elif min_library_size is not None:
        Y, cells = filter_library_size(X, cutoff=min_library_size, keep_cells="above")
    elif max_library_size is not None:
        Y, cells = filter_library_size(X, cutoff=max_library_size, keep_cells="below")
    genes = np.arange(X.shape[1])
    if min_cells is not None:
        Y, genes = filter_rare_genes(Y, cutoff=gene_cutoff, min_cells=min_cells)
    libsize = library_size(Y)
    normalized = library_size_normalize(Y, rescale) if rescale is not None else Y.astype(np.float64)
    return SimpleNamespace(data=TRANSFORMS[transform](normalized), normalized=normalized, cells=cells.astype(np.int64),
                           genes=genes.astype(np.int64), library_size=libsize)
