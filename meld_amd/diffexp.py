"""Rank-sum differential expression on the device: which genes differ between groups of cells.

The reference ends its analyses with a Wilcoxon rank-sum (Mann-Whitney U) test per gene
(``de.test.two_sample(data, grouping=classes, test='rank')`` in notebooks/MELD_thresholding.Tcell.ipynb).  Here the expression
matrix stays on the device as the CSC copy of the data (``DeviceCSR.T``: one row per gene), csrc/ranksum.hip sorts every gene's
selected non-zero entries ONCE and ranks them for all classes at the same time (the implicit zeros are one tie group whose ranks are
known without touching them), and only G x k integers come back to the host, where the p- and q-values are a few vector operations.

* ``encode_classes`` / ``pvalues`` / ``bh_qvalues``: plain numpy, no GPU (the host tier tests them against scipy);
* ``rank_sums_device``: the raw device tensors (``rank2``, ``tie``, ``nnz``, ``sum``) and the class sizes;
* ``rank_sum_test``: the frames (also ``meld_amd.rank_sum_test`` and ``MELD.rank_sum_test``).

The statistic is scipy's ``mannwhitneyu(x, y, use_continuity=True, alternative="two-sided", method="asymptotic")``: ``statistic``
equal exactly, the p-value to rounding.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

__all__ = ["MAX_CLASSES", "MAX_SELECTED", "encode_classes", "pvalues", "bh_qvalues", "rank_sums_device", "rank_sum_test"]

MAX_CLASSES = 64  # MELD_RANKSUM_MAX_CLASSES of include/meld_hip.h (rank_sums_device asks the library)
MAX_SELECTED = 2097151  # MELD_RANKSUM_MAX_SELECTED: the cube of a tie group's size is taken in int64
LONG_BATCH_ENTRIES = 1 << 27  # stored entries the long route gathers and sorts at a time (32 bytes each + the sort's scratch)


# ---- host helpers (numpy only) ------------------------------------------------------------------------------------------------------
def encode_classes(groups, group=None, reference=None, n_cells=None, max_classes=MAX_CLASSES):
    """Class codes of the cells for one run of the kernels.  ``groups``: length-N labels (array or Series, any sortable or hashable
    dtype; NaN / None: the cell is ignored).  Returns ``(codes, classes)``: ``codes`` int32 [N] in {-1, 0 .. k-1} and ``classes`` the
    list of what each code stands for.

    * ``group`` and ``reference`` given: code 0 = ``group``, 1 = ``reference``, every other cell -1;
    * ``group`` alone: code 0 = ``group``, 1 = every other labelled cell (``classes[1]`` is None);
    * neither: the distinct labels, sorted where they can be sorted (else in order of appearance), one code each.

    ValueError for labels of the wrong length, a label that does not occur, an empty group or reference, ``reference`` without
    ``group``, and more than ``max_classes`` distinct labels."""
    import pandas as pd

    raw = np.asarray(getattr(groups, "values", groups))
    if raw.ndim == 2 and 1 in raw.shape:
        raw = raw.reshape(-1)
    if raw.ndim != 1:
        raise ValueError("rank_sum_test: groups must be one label per cell, got shape {}".format(raw.shape))
    if n_cells is not None and raw.shape[0] != int(n_cells):
        raise ValueError("rank_sum_test: length mismatch: {} group labels for {} cells".format(raw.shape[0], int(n_cells)))
    try:
        fcodes, uniques = pd.factorize(raw, sort=True)
    except TypeError:  # labels that cannot be ordered among themselves
        fcodes, uniques = pd.factorize(raw, sort=False)
    uniques = list(uniques)

    def index_of(label, what):
        for i, u in enumerate(uniques):
            if u == label:
                return i
        raise ValueError("rank_sum_test: {} label {!r} is absent from groups".format(what, label))

    if group is None:
        if reference is not None:
            raise ValueError("rank_sum_test: a reference needs a group to compare with it")
        if len(uniques) > int(max_classes):
            raise ValueError("rank_sum_test: {} classes, the kernel takes at most {}".format(len(uniques), int(max_classes)))
        if len(uniques) == 0:
            raise ValueError("rank_sum_test: empty group: no cell carries a label")
        return fcodes.astype(np.int32), uniques
    gi = index_of(group, "group")
    codes = np.full(raw.shape[0], -1, dtype=np.int32)
    if reference is None:
        codes[fcodes >= 0] = 1
        codes[fcodes == gi] = 0
        classes = [uniques[gi], None]
    else:
        ri = index_of(reference, "reference")
        if ri == gi:
            raise ValueError("rank_sum_test: empty reference: group and reference are the same label {!r}".format(group))
        codes[fcodes == ri] = 1
        codes[fcodes == gi] = 0
        classes = [uniques[gi], uniques[ri]]
    if not (codes == 0).any():  # (a label that occurs has cells: kept for callers that pass codes of their own)
        raise ValueError("rank_sum_test: empty group {!r}".format(group))
    if not (codes == 1).any():
        raise ValueError("rank_sum_test: empty reference: no labelled cell outside group {!r}".format(group))
    return codes, classes


def pvalues(rank2, tie, n1, n2):
    """``(statistic, pval)`` of the two-sided asymptotic Mann-Whitney test with continuity correction, from the integers of the
    device: ``rank2`` twice the rank sum of the group (n1 cells) among the n = n1 + n2 selected cells, ``tie`` the sum of t^3 - t over
    the tie groups.  ``statistic`` is U1 (scipy's); p = 1.0 where every value is tied (the standard deviation is 0)."""
    from scipy.special import ndtr

    rank2 = np.asarray(rank2, dtype=np.int64)
    tie = np.asarray(tie, dtype=np.int64).astype(np.float64)
    n1, n2 = int(n1), int(n2)
    if n1 < 1 or n2 < 1:
        raise ValueError("rank_sum_test: empty group or reference (n1={}, n2={})".format(n1, n2))
    n = n1 + n2
    u1 = (rank2 - n1 * (n1 + 1)).astype(np.float64) / 2.0  # (an integer below 2^53 halved: exact)
    prod = float(n1) * float(n2)
    u = np.maximum(u1, prod - u1)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sqrt(prod / 12.0 * ((n + 1) - tie / (n * (n - 1.0))))
        z = (u - prod / 2.0 - 0.5) / s
        p = np.minimum(1.0, 2.0 * ndtr(-z))
    p = np.where(s == 0, 1.0, p)
    return u1, p


def bh_qvalues(p):
    """Benjamini-Hochberg adjusted p-values (``scipy.stats.false_discovery_control(p, method="bh")``)."""
    p = np.asarray(p, dtype=np.float64)
    g = p.shape[0]
    if g == 0:
        return p.copy()
    order = np.argsort(p, kind="stable")
    q = p[order] * (g / np.arange(1, g + 1))
    q = np.minimum.accumulate(q[::-1])[::-1]
    out = np.empty(g, dtype=np.float64)
    out[order] = np.clip(q, 0.0, 1.0)
    return out


# ---- the device run ---------------------------------------------------------------------------------------------------------------------
def _gene_major(data, device="cuda"):
    """The CSR of X^T (one row per gene) as a ``DeviceCSR`` [G, N], for X a ``DeviceCSR``, a sparse input or a dense matrix."""
    import torch

    from . import sparse as _sp

    if isinstance(data, _sp.DeviceCSR):
        return data.T  # (cached on the matrix the caller holds)
    inner = _sp._unwrap(data)
    scipy_sparse = _sp._scipy_sparse()
    if scipy_sparse.issparse(inner) and inner.format == "csc":
        # the CSC arrays ARE the CSR of the transpose: uploaded as they are, no device transpose
        A = inner
        if A.ndim != 2 or A.shape[0] < 1 or A.shape[1] < 1:
            raise ValueError("Expected a non-empty 2D data matrix, got shape {}".format(A.shape))
        if max(A.shape) > np.iinfo(np.int32).max:
            raise ValueError("sparse input: shape {} does not fit the kernels' int32 indices".format(A.shape))
        if not A.has_canonical_format:
            A = A.copy()
            A.sum_duplicates()
        values = np.asarray(A.data)
        if values.dtype not in (np.float32, np.float64):
            values = values.astype(np.float64)
        M = _sp.DeviceCSR(torch.from_numpy(np.asarray(A.indptr)).to(device).to(torch.int64),
                          torch.from_numpy(np.asarray(A.indices)).to(device).to(torch.int32).contiguous(),
                          torch.from_numpy(values).to(device).contiguous(), (A.shape[1], A.shape[0]))
        M._validate()
        return M
    if _sp.is_sparse_input(data):
        return _sp.DeviceCSR.from_input(data, device=device).T
    # dense: uploaded, transposed and compressed on the device
    if isinstance(inner, torch.Tensor):
        X = inner if inner.is_cuda else inner.to(device)
    else:
        arr = np.asarray(getattr(inner, "values", inner))
        if arr.dtype not in (np.float32, np.float64):
            arr = arr.astype(np.float64)
        X = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
    if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("Expected a non-empty 2D data matrix, got shape {}".format(tuple(X.shape)))
    if X.dtype not in (torch.float32, torch.float64):
        X = X.to(torch.float64)
    if not bool(torch.isfinite(X).all()):
        raise ValueError("Input data contains NaN or infinity")
    S = X.t().contiguous().to_sparse_csr()
    M = _sp.DeviceCSR(S.crow_indices().to(torch.int64), S.col_indices().to(torch.int32).contiguous(), S.values().contiguous(),
                      (int(X.shape[1]), int(X.shape[0])))
    M._validate()
    return M


def _n_cells(data):
    from . import sparse as _sp

    if isinstance(data, _sp.DeviceCSR):
        return data.shape[0]
    return int(_sp._unwrap(data).shape[0])


def _long_batches(lens, limit):
    """Consecutive runs of the long genes whose stored entries sum to at most ``limit`` (a single gene may exceed it)."""
    out, lo, acc = [], 0, 0
    for i, n in enumerate(lens):
        if i > lo and acc + n > limit:
            out.append((lo, i))
            lo, acc = i, 0
        acc += int(n)
    if lo < len(lens):
        out.append((lo, len(lens)))
    return out


def rank_sums_device(data, codes, k, force_long=False, timings=None):
    """The rank-sum integers of every gene for ``k`` classes of cells, on the device.

    ``data``: a ``DeviceCSR`` (its cached ``.T`` is used), anything ``DeviceCSR.from_input`` takes, a host ``scipy.sparse.csc_matrix``
    (uploaded as it is: it is the CSR of the transpose), or dense (numpy, DataFrame, device tensor; compressed on the device).
    ``codes``: int [N] in {-1, 0 .. k-1}, -1 = the cell takes no part.  ``force_long``: send every gene through the long route
    (gather, radix sort, scan from global memory) instead of choosing by stored length; the integers are the same either way.
    ``timings``: an optional dict that receives the stages' seconds (the stream is synchronised between them).

    Returns a namespace of device tensors ``rank2`` [G, k] int64 (twice the rank sums), ``tie`` [G] int64 (sum of t^3 - t),
    ``nnz`` [G, k] int32, ``sum`` [G, k] fp64, ``n_c`` [k] int64 (the class sizes) and the int ``m`` (selected cells).

    ``tie`` is exact in int64 up to ``MAX_SELECTED`` = 2,097,151 selected cells; more are refused with a ValueError (nothing wider is
    accumulated).  ValueError also for codes of the wrong length and for k outside [1, ``meld_ranksum_max_classes()``]."""
    import time

    import torch

    from ._device_ops import stream
    from ._lib import check, get_lib, ptr

    lib = get_lib()
    k = int(k)
    kmax = int(lib.meld_ranksum_max_classes())
    if not 1 <= k <= kmax:
        raise ValueError("rank_sums_device: {} classes, the kernel takes 1 to {}".format(k, kmax))
    host_codes = None if isinstance(codes, torch.Tensor) else np.asarray(codes)
    n_codes = int(codes.shape[0]) if host_codes is None else int(host_codes.shape[0])
    if n_codes != _n_cells(data):
        raise ValueError("rank_sums_device: length mismatch: {} codes for {} cells".format(n_codes, _n_cells(data)))
    selected = int(((codes >= 0) & (codes < k)).sum()) if host_codes is None else int(((host_codes >= 0) & (host_codes < k)).sum())
    limit = int(lib.meld_ranksum_max_selected())
    if selected > limit:  # (before the matrix is uploaded or transposed)
        raise ValueError("rank_sums_device: {} selected cells, the tie term is exact in int64 up to {} (select fewer cells)".format(selected, limit))

    def lap(name, t0):
        if timings is not None:
            torch.cuda.synchronize()
            timings[name] = timings.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    t0 = time.perf_counter()
    AT = _gene_major(data)
    t0 = lap("transpose", t0)
    G, N = AT.shape
    dev = AT.device
    code = (codes.to(dev) if host_codes is None else torch.from_numpy(host_codes.astype(np.int32, copy=False)).to(dev)).to(torch.int32).contiguous()
    valid = (code >= 0) & (code < k)
    n_c = torch.bincount(code[valid].to(torch.int64), minlength=k).to(torch.int64)
    m = int(n_c.sum())
    st = stream()
    rank2 = torch.empty(G, k, dtype=torch.int64, device=dev)
    tie = torch.empty(G, dtype=torch.int64, device=dev)
    nnz = torch.empty(G, k, dtype=torch.int32, device=dev)
    sums = torch.empty(G, k, dtype=torch.float64, device=dev)
    lens = AT.rowptr[1:] - AT.rowptr[:-1]
    cap = int(lib.meld_ranksum_lds_max())
    is_long = torch.ones_like(lens, dtype=torch.bool) if force_long else lens > cap
    short = torch.nonzero(~is_long).flatten().to(torch.int32)
    long_ = torch.nonzero(is_long).flatten().to(torch.int32)
    t0 = lap("plan", t0)
    # (a matrix without entries has no addresses for col and val: the entries want any, nothing reads them)
    col, val = (AT.col, AT.val) if AT.nnz else (torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float64, device=dev))
    mat = (ptr(AT.rowptr), ptr(col), ptr(val), 1 if val.dtype == torch.float32 else 0, G)
    check(lib.meld_ranksum_sums(*mat, ptr(code), N, k, ptr(sums), st), "meld_ranksum_sums")
    t0 = lap("sums", t0)
    if int(short.shape[0]):
        check(lib.meld_ranksum_short(*mat, ptr(short), int(short.shape[0]), ptr(code), N, k, ptr(n_c), m, ptr(rank2), ptr(tie), ptr(nnz),
                                     st), "meld_ranksum_short")
    t0 = lap("short", t0)
    if int(long_.shape[0]):
        long_lens = lens[long_.to(torch.int64)]
        for lo, hi in _long_batches(long_lens.cpu().numpy(), LONG_BATCH_ENTRIES):
            genes = long_[lo:hi].contiguous()
            nl = hi - lo
            off = torch.zeros(nl + 1, dtype=torch.int64, device=dev)
            torch.cumsum(long_lens[lo:hi], 0, out=off[1:])
            total = int(off[-1])
            buf = torch.empty(4, max(total, 1), dtype=torch.int64, device=dev)  # image, payload and their sorted copies
            if total:
                check(lib.meld_ranksum_gather(*mat, ptr(genes), ptr(off), nl, total, ptr(code), N, k, ptr(buf[0]), ptr(buf[1]), st),
                      "meld_ranksum_gather")
                tb = int(lib.meld_sort_temp_bytes(total))
                tmp = torch.empty(tb, dtype=torch.uint8, device=dev)
                # by value, then (stable) by slot: every gene's segment ends up at off[slot], ascending, dead entries last
                check(lib.meld_sort_pairs_u64_u64(ptr(buf[0]), ptr(buf[2]), ptr(buf[1]), ptr(buf[3]), total, 0, 64, ptr(tmp), tb, st),
                      "meld_sort_pairs_u64_u64")
                end_bit = 32 + max(1, int(nl - 1).bit_length())
                check(lib.meld_sort_pairs_u64_u64(ptr(buf[3]), ptr(buf[1]), ptr(buf[2]), ptr(buf[0]), total, 32, end_bit, ptr(tmp), tb, st),
                      "meld_sort_pairs_u64_u64")
                del tmp
            check(lib.meld_ranksum_scan(ptr(buf[0]), ptr(buf[1]), ptr(genes), ptr(off), nl, G, k, ptr(n_c), m, ptr(rank2), ptr(tie),
                                        ptr(nnz), st), "meld_ranksum_scan")
            del buf
    lap("long", t0)
    return SimpleNamespace(rank2=rank2, tie=tie, nnz=nnz, sum=sums, n_c=n_c, m=m)


def _gene_index(data, gene_names, n_genes):
    import pandas as pd

    if gene_names is not None:
        names = pd.Index(gene_names)
        if len(names) != n_genes:
            raise ValueError("rank_sum_test: length mismatch: {} gene names for {} genes".format(len(names), n_genes))
        return names
    if isinstance(data, pd.DataFrame):
        return data.columns
    return pd.RangeIndex(n_genes)


def _frame(index, rank2, tie, nnz_g, nnz_r, sum_g, sum_r, n1, n2):
    import pandas as pd

    stat, p = pvalues(rank2, tie, n1, n2)
    mean_g, mean_r = sum_g / n1, sum_r / n2
    with np.errstate(divide="ignore", invalid="ignore"):
        lfc = np.log2(mean_g / mean_r)
    return pd.DataFrame({"statistic": stat, "pval": p, "qval": bh_qvalues(p), "mean_group": mean_g, "mean_reference": mean_r,
                         "log2fc": lfc, "nnz_group": nnz_g.astype(np.int64), "nnz_reference": nnz_r.astype(np.int64)}, index=index)


def rank_sum_test(data, groups, group=None, reference=None, gene_names=None):
    """Wilcoxon rank-sum (Mann-Whitney U) test of every gene between groups of cells, on the device.

    ``data``: cells x genes, as for ``rank_sums_device``.  ``groups``: one label per cell (NaN / None: the cell is ignored).

    * ``group`` and ``reference``: those two labels' cells;
    * ``group`` alone: its cells against every other labelled cell;
    * neither: a dict ``{label: frame}`` of each label against the rest, all from one device run.

    A frame is indexed by gene (a DataFrame's columns, else ``gene_names``, else integers) with the columns ``statistic`` (U of the
    group, scipy's), ``pval`` (two-sided, asymptotic, continuity-corrected; 1.0 for a gene whose values are all tied), ``qval``
    (Benjamini-Hochberg over the genes), ``mean_group``, ``mean_reference`` (zeros included), ``log2fc`` = log2 of their ratio as
    numpy evaluates it, ``nnz_group`` and ``nnz_reference``.

    ValueError, before anything is launched, for a label absent from ``groups``, an empty group or reference, more classes than the
    kernel takes, a length mismatch, and more than 2,097,151 selected cells."""
    codes, classes = encode_classes(groups, group, reference, n_cells=_n_cells(data))
    k = len(classes)
    if k < 2:
        raise ValueError("rank_sum_test: empty reference: every labelled cell carries the label {!r}".format(classes[0]))
    res = rank_sums_device(data, codes, k)
    index = _gene_index(data, gene_names, int(res.rank2.shape[0]))
    rank2, tie, nnz, sums, n_c = (t.cpu().numpy() for t in (res.rank2, res.tie, res.nnz, res.sum, res.n_c))
    if group is not None:
        return _frame(index, rank2[:, 0], tie, nnz[:, 0], nnz[:, 1], sums[:, 0], sums[:, 1], int(n_c[0]), int(n_c[1]))
    out = {}
    nnz_all = nnz.astype(np.int64).sum(axis=1)
    for c, label in enumerate(classes):
        rest = np.delete(sums, c, axis=1).sum(axis=1)  # (the other classes' sums added up, not a difference of totals)
        out[label] = _frame(index, rank2[:, c], tie, nnz[:, c], nnz_all - nnz[:, c], sums[:, c], rest, int(n_c[c]), res.m - int(n_c[c]))
    return out
