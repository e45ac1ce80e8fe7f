"""Host restatement of the per-gene moments and the highly-variable-gene rule of meld_amd/preprocess.py, in numpy / scipy (no import of
meld_amd), checked against numpy and scipy by tests/test_hvg_reference.py.

``moments_long`` evaluates the value map in fp64, operation by operation as csrc/preprocess.hip states it, and every sum in
``np.longdouble``; ``moment_bounds`` are the tolerances the device moments are held to, derived from it (not measured):

    eta      = (cnt + 1) eps abs_sum / n_kept                       the mean: a sum of cnt terms in ANY order is off by at most
                                                                    (cnt - 1) u sum|x| (u = eps / 2), the values themselves by
                                                                    at most 2 u each (a transform of 1 ulp on either side), the
                                                                    division by u
    var_tol  = ((cnt + 8) eps ss + n_kept eta^2) / (n_kept - ddof)  sum (x - a)^2 = sum (x - m)^2 + n (a - m)^2 for the mean a the
                                                                    device used in place of m; the rest as above

with eps = 2^-52, cnt the counted entries of the gene, abs_sum = sum |x| and ss = sum (x - mean)^2 over all kept cells."""
from types import SimpleNamespace

import numpy as np
from scipy import sparse
from scipy.signal import medfilt

from tests import preprocess_reference as ref

EPS = 2.0 ** -52

_MAPS = {None: lambda w, c: w, "identity": lambda w, c: w, "sqrt": lambda w, c: np.sqrt(w), "log": lambda w, c: np.log(w + 1.0),
         "log2": lambda w, c: np.log2(w + 1.0), "log10": lambda w, c: np.log10(w + 1.0), "arcsinh": lambda w, c: np.arcsinh(w / c)}


def value_map(v, s=None, rescale=1.0, transform=None, cofactor=5.0):
    """x = f(w), w = (v / s) * rescale where a scale is given (a scale of 0 keeps v, rescale still multiplies), else v: fp64"""
    v = np.asarray(v, dtype=np.float64)
    w = v
    if s is not None:
        s = np.asarray(s, dtype=np.float64)
        w = np.where(s == 0.0, v, v / np.where(s == 0.0, 1.0, s)) * float(rescale)
    with np.errstate(invalid="ignore"):
        return _MAPS[transform](w, float(cofactor))


def moments_long(X, row_keep=None, row_scale=None, rescale=1.0, transform=None, cofactor=5.0, gene_mask=None, ddof=1):
    """Per gene of a scipy.sparse matrix [N, G]: ``count`` (stored entries of kept cells, -1 for a masked gene), ``mean``, ``var``,
    ``abs_sum`` and ``ss`` in long double, and ``n_kept``."""
    C = sparse.csc_matrix(X)
    N, G = C.shape
    keep = np.ones(N, dtype=bool) if row_keep is None else np.asarray(row_keep).astype(bool)
    n_kept = int(keep.sum())
    count = np.zeros(G, dtype=np.int64)
    mean = np.zeros(G, dtype=np.longdouble)
    var = np.zeros(G, dtype=np.longdouble)
    abs_sum = np.zeros(G, dtype=np.longdouble)
    ss = np.zeros(G, dtype=np.longdouble)
    for g in range(G):
        if gene_mask is not None and not gene_mask[g]:
            count[g] = -1
            continue
        cells = C.indices[C.indptr[g]:C.indptr[g + 1]]
        v = C.data[C.indptr[g]:C.indptr[g + 1]]
        sel = keep[cells]
        cells, v = cells[sel], v[sel]
        x = value_map(v, None if row_scale is None else np.asarray(row_scale)[cells], rescale, transform, cofactor).astype(np.longdouble)
        count[g] = x.shape[0]
        abs_sum[g] = np.abs(x).sum()
        mean[g] = x.sum() / np.longdouble(n_kept)
        ss[g] = ((x - mean[g]) ** 2).sum() + np.longdouble(n_kept - count[g]) * mean[g] ** 2
        var[g] = ss[g] / np.longdouble(n_kept - ddof)
    return SimpleNamespace(count=count, mean=mean, var=var, abs_sum=abs_sum, ss=ss, n_kept=n_kept, ddof=ddof)


def moment_bounds(m):
    """(eta, var_tol) per gene for the reference moments ``m`` (the module docstring); zeros for masked genes"""
    cnt = np.maximum(m.count, 0).astype(np.longdouble)
    eta = (cnt + 1) * EPS * m.abs_sum / m.n_kept
    var_tol = ((cnt + 8) * EPS * m.ss + m.n_kept * eta ** 2) / (m.n_kept - m.ddof)
    return eta, var_tol


def kernel_length(kernel_size, G):
    if isinstance(kernel_size, (int, np.integer)):
        if kernel_size < 1 or kernel_size % 2 == 0:
            raise ValueError("kernel_size")
        return int(kernel_size)
    return 2 * (int(kernel_size * G) // 2) + 1


def smooth_once(y):
    """three-point mean, the end values replicated"""
    out = np.empty_like(y)
    for i in range(y.shape[0]):
        left = y[i - 1] if i > 0 else y[0]
        right = y[i + 1] if i + 1 < y.shape[0] else y[-1]
        out[i] = ((left + y[i]) + right) / 3.0
    return out


def variability(mean, var, kernel_size=0.005, smooth=5):
    mean = np.asarray(mean, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    G = mean.shape[0]
    order = np.asarray(sorted(range(G), key=lambda g: (mean[g], g)), dtype=np.int64)  # ties: the lower gene index first
    expected = medfilt(var[order], kernel_length(kernel_size, G))
    for _ in range(smooth):
        expected = smooth_once(expected)
    out = np.empty(G, dtype=np.float64)
    out[order] = var[order] - expected
    return out


def select_genes(variability, cutoff=None, percentile=None, n_top_genes=None):
    """kept gene indices (ascending) under exactly one of the three rules, and the cutoff used"""
    if sum(r is not None for r in (cutoff, percentile, n_top_genes)) != 1:
        raise ValueError("exactly one rule")
    G = variability.shape[0]
    if n_top_genes is not None:
        if not 1 <= n_top_genes <= G:
            raise ValueError("n_top_genes")
        ranked = sorted(range(G), key=lambda g: (-variability[g], g))[:n_top_genes]  # ties: the lower gene index
        return np.sort(np.asarray(ranked, dtype=np.int64)), float(variability[ranked[-1]])
    cut = cutoff if cutoff is not None else np.percentile(variability, percentile)
    return np.flatnonzero(variability > cut).astype(np.int64), float(cut)


def highly_variable_genes(X, kernel_size=0.05, smooth=5, cutoff=None, percentile=None, n_top_genes=None):
    m = moments_long(X)
    v = variability(m.mean.astype(np.float64), m.var.astype(np.float64), kernel_size, smooth)
    kept, cut = select_genes(v, cutoff, percentile, n_top_genes)
    return ref.select(sparse.csr_matrix(X), cols=kept), kept, SimpleNamespace(moments=m, variability=v, cutoff=cut)


def run_with_hvg(X, hvg_percentile=None, hvg_cutoff=None, n_top_genes=None, hvg_kernel_size=0.05, hvg_smooth=5, **kwargs):
    """The step-by-step sequence of tests/preprocess_reference.py, then the selection on the matrix it leaves."""
    out = ref.run(X, **kwargs)
    m = moments_long(out.data)
    v = variability(m.mean.astype(np.float64), m.var.astype(np.float64), hvg_kernel_size, hvg_smooth)
    kept, cut = select_genes(v, hvg_cutoff, hvg_percentile, n_top_genes)
    return SimpleNamespace(data=ref.select(out.data, cols=kept), normalized=ref.select(out.normalized, cols=kept), cells=out.cells,
                           genes=out.genes[kept], genes_before=out.genes, kept=kept, library_size=out.library_size, full=out, moments=m,
                           variability=v, cutoff=cut)
