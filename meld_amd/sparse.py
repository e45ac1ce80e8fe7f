"""Sparse cell-by-gene input: the matrix goes to the device as CSR and graphtools' truncated SVD runs there.

For sparse data graphtools' ``Data._reduce_data`` [UPSTREAM graphtools/base.py] fits
``sklearn.decomposition.TruncatedSVD(n_pca, random_state=...)`` -- an SVD of the data as given, NOT centred -- where dense
data gets a centred PCA.  This module is that front end without a dense copy of the matrix anywhere:

* ``to_host_csr``: scipy.sparse (any format), pandas frames of sparse columns and AnnData-like objects with a sparse ``.X``
  become one canonical scipy CSR matrix on the host (no densification);
* ``DeviceCSR``: the CSR arrays on the device (values in the dtype they came in: fp32 is widened inside the kernels), the
  work plan of the products, the transpose built lazily (``meld_csr_transpose_keys`` + the radix sort and CSR assembly of
  the affinity build: rows ascending inside each column, so products with it are deterministic);
* ``truncated_svd_project``: the exact top-k right singular subspace through the Gram matrix X^T X for G <= pca.EXACT_MAX
  genes, the randomized range finder of ``pca.py`` otherwise; every product against X is ``meld_csr_spmm_f64``
  (csrc/csr_dense.hip);
* ``reduce_data``: the one reduction step of the graph build, sparse (this SVD) or dense (``pca.pca_project``).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import pca as _pca
from ._device_ops import csr_from_keys, sort_pairs, stream
from ._lib import check, get_lib, ptr

__all__ = ["is_sparse_input", "to_host_csr", "DeviceCSR", "truncated_svd_project", "reduce_data"]


def _scipy_sparse():
    from scipy import sparse

    return sparse


def _is_torch_csr(X):
    return isinstance(X, torch.Tensor) and X.layout == torch.sparse_csr


def _unwrap(X):
    if hasattr(X, "X") and not isinstance(X, (np.ndarray, torch.Tensor)):  # AnnData-like
        X = X.X
    return X


def _pandas_sparse(X):
    """A DataFrame whose columns are all sparse (pandas only offers ``.sparse`` on those)."""
    try:
        import pandas as pd
    except ImportError:  # pragma: no cover
        return False
    if not isinstance(X, pd.DataFrame):
        return False
    try:
        return hasattr(X.sparse, "to_coo")
    except AttributeError:
        return False


def is_sparse_input(X):
    """True for the inputs this front end takes: scipy.sparse, all-sparse DataFrames, AnnData-like objects with a sparse
    ``.X``, device tensors of layout ``torch.sparse_csr`` and a ``DeviceCSR`` (a matrix that is on the device already, the
    output of ``meld_amd.preprocess`` for one)."""
    if _is_torch_csr(X) or isinstance(X, DeviceCSR):
        return True
    X = _unwrap(X)
    return _is_torch_csr(X) or _scipy_sparse().issparse(X) or _pandas_sparse(X)


def to_host_csr(X):
    """The canonical scipy CSR matrix of a host sparse input (COO, LIL, DOK, CSC, ... -> CSR as graphtools does; duplicates
    summed and indices sorted only where the matrix is not canonical already).  Never densifies."""
    sparse = _scipy_sparse()
    X = _unwrap(X)
    if _pandas_sparse(X):
        X = X.sparse.to_coo()
    if not sparse.issparse(X):
        raise TypeError("expected a sparse matrix, got {}".format(type(X).__name__))
    if X.ndim != 2:
        raise ValueError("Expected a 2D data matrix, got shape {}".format(X.shape))
    A = X if X.format == "csr" else X.tocsr()
    if not A.has_canonical_format:
        A = A.copy()
        A.sum_duplicates()
    return A


class DeviceCSR:
    """A CSR matrix on the device: rowptr [n_rows + 1] int64, col [nnz] int32, val [nnz] fp32 or fp64, ``shape``."""

    def __init__(self, rowptr, col, val, shape):
        self.rowptr, self.col, self.val = rowptr, col, val
        self.shape = (int(shape[0]), int(shape[1]))
        self.nnz = int(col.shape[0])
        self._plan = None
        self._T = None
        # the labels of the rows and columns where the input carried them (meld_amd/preprocess.py keeps them through its filters)
        self.cell_index = None
        self.gene_names = None

    @property
    def device(self):
        return self.rowptr.device

    @classmethod
    def from_input(cls, X, device="cuda"):
        """Upload a host sparse input (or adopt a device ``torch.sparse_csr`` tensor, no PCIe), check its indices and values.
        A ``DeviceCSR`` is returned as it is."""
        if isinstance(X, cls):
            return X
        X = _unwrap(X)
        if _is_torch_csr(X):
            if X.dim() != 2:
                raise ValueError("Expected a 2D data matrix, got shape {}".format(tuple(X.shape)))
            dev = X.device if X.is_cuda else torch.device(device)
            rowptr = X.crow_indices().to(device=dev, dtype=torch.int64)
            col = X.col_indices().to(dev)
            if int(X.shape[1]) > np.iinfo(np.int32).max:
                raise ValueError("sparse input: {} columns do not fit the kernels' int32 column indices".format(int(X.shape[1])))
            col = col.to(torch.int32)  # (narrowed on the device)
            val = X.values().to(dev)
            shape = tuple(X.shape)
        else:
            A = to_host_csr(X)
            if A.shape[1] > np.iinfo(np.int32).max:
                raise ValueError("sparse input: {} columns do not fit the kernels' int32 column indices".format(A.shape[1]))
            rowptr = torch.from_numpy(np.asarray(A.indptr)).to(device).to(torch.int64)
            col = torch.from_numpy(np.asarray(A.indices)).to(device)
            if col.dtype != torch.int32:
                col = col.to(torch.int32)
            data = np.asarray(A.data)
            val = torch.from_numpy(data if data.dtype in (np.float32, np.float64) else data.astype(np.float64)).to(device)
            shape = A.shape
        if val.dtype not in (torch.float32, torch.float64):
            val = val.to(torch.float64)
        if shape[0] < 1 or shape[1] < 1:
            raise ValueError("Expected a non-empty 2D data matrix, got shape {}".format(tuple(shape)))
        if shape[0] > np.iinfo(np.int32).max:
            raise ValueError("sparse input: {} rows do not fit the kernels' int32 row indices".format(shape[0]))
        M = cls(rowptr, col.contiguous(), val.contiguous(), shape)
        M._validate()
        return M

    def _validate(self):
        """Structure and values, on the device, before any kernel reads through the indices."""
        if int(self.rowptr.shape[0]) != self.shape[0] + 1:
            raise ValueError("sparse input: indptr has {} entries for {} rows".format(int(self.rowptr.shape[0]), self.shape[0]))
        if self.nnz:
            bad = torch.stack([self.rowptr[0] != 0, self.rowptr[-1] != self.nnz, (self.rowptr[1:] < self.rowptr[:-1]).any(),
                               self.col.min() < 0, self.col.max() >= self.shape[1]])
            if bool(bad.any()):
                raise ValueError("sparse input: inconsistent CSR structure (indptr / column indices out of range)")
            if not bool(torch.isfinite(self.val).all()):
                raise ValueError("Input data contains NaN or infinity")
        elif int(self.rowptr[-1]) != 0:
            raise ValueError("sparse input: inconsistent CSR structure (indptr / column indices out of range)")

    @property
    def val_f32(self):
        return 1 if self.val.dtype == torch.float32 else 0

    # ---- the work plan of meld_csr_spmm_f64: units of at most MELD_CSR_SEG entries ------------------------------------
    def plan(self):
        if self._plan is None:
            seg = get_lib().meld_csr_seg_length()
            lens = self.rowptr[1:] - self.rowptr[:-1]
            nseg = torch.clamp((lens + seg - 1) // seg, min=1)
            ends = torch.cumsum(nseg, 0)
            n_units = int(ends[-1])
            unit_off = ends - nseg
            unit_row = torch.repeat_interleave(torch.arange(self.shape[0], dtype=torch.int32, device=self.device), nseg,
                                               output_size=n_units)
            split = nseg > 1
            split_rows = torch.nonzero(split).flatten().to(torch.int32)
            slots = torch.where(split, nseg, torch.zeros_like(nseg))
            part_off = torch.cumsum(slots, 0) - slots
            n_slots = int(slots.sum())
            self._plan = dict(unit_row=unit_row, unit_off=unit_off.contiguous(), n_units=n_units, part_off=part_off.contiguous(),
                              split_rows=split_rows, n_slots=n_slots)
        return self._plan

    def matmul(self, B, out=None):
        """X @ B for a dense fp64 device matrix B [G, r] (row-major, any leading dimension >= r)."""
        if B.dim() != 2 or int(B.shape[0]) != self.shape[1]:
            raise ValueError("matmul: operand of shape {} against a {} matrix".format(tuple(B.shape), self.shape))
        if B.dtype != torch.float64 or B.stride(1) != 1:
            B = B.to(torch.float64).contiguous()
        r = int(B.shape[1])
        Y = torch.empty(self.shape[0], r, dtype=torch.float64, device=self.device) if out is None else out
        p = self.plan()
        partial = torch.empty(max(p["n_slots"], 1) * r, dtype=torch.float64, device=self.device) if p["n_slots"] else None
        check(get_lib().meld_csr_spmm_f64(ptr(self.rowptr), ptr(self.col), ptr(self.val), self.val_f32, self.shape[0],
                                          ptr(p["unit_row"]), ptr(p["unit_off"]), p["n_units"], ptr(p["part_off"]),
                                          ptr(p["split_rows"]), int(p["split_rows"].shape[0]), ptr(partial), ptr(B),
                                          int(B.stride(0)), r, ptr(Y), int(Y.stride(0)), stream()), "meld_csr_spmm_f64")
        return Y

    # ---- the transpose (CSC of X as the CSR of X^T) --------------------------------------------------------------------
    def transpose_bytes(self):
        """Device bytes the transposition needs at its peak (keys and values, sorted copies, sort scratch)."""
        return 32 * self.nnz + int(get_lib().meld_sort_temp_bytes(max(self.nnz, 1)))

    @property
    def T(self):
        if self._T is None:
            self._T = self._transpose()
        return self._T

    def _transpose(self):
        lib, st, dev = get_lib(), stream(), self.device
        N, G = self.shape
        nnz = self.nnz
        if nnz == 0:
            return DeviceCSR(torch.zeros(G + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                             torch.empty(0, dtype=torch.float64, device=dev), (G, N))
        need = self.transpose_bytes()
        free, _ = torch.cuda.mem_get_info(dev)
        if need > free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev):
            raise MemoryError("sparse input: transposing {} entries needs {:.1f} GB of device memory, {:.1f} GB are free".format(
                nnz, need / 1e9, free / 1e9))
        keys = torch.empty(nnz, dtype=torch.int64, device=dev)
        vals = torch.empty(nnz, dtype=torch.float64, device=dev)
        check(lib.meld_csr_transpose_keys(ptr(self.rowptr), ptr(self.col), ptr(self.val), self.val_f32, N, ptr(keys), ptr(vals), st),
              "meld_csr_transpose_keys")
        keys, vals = sort_pairs(keys, vals, G)  # (the unsorted keys and values are released here, the sort's scratch before)
        rowptr, col = csr_from_keys(keys, nnz, 0, G)
        return DeviceCSR(rowptr, col, vals, (G, N))

    # ---- densification -------------------------------------------------------------------------------------------------
    def rows_to_dense(self, lo, hi, out=None):
        """Rows [lo, hi) as a dense fp64 block [hi - lo, G]."""
        G = self.shape[1]
        if out is None:
            out = torch.empty(hi - lo, G, dtype=torch.float64, device=self.device)
        check(get_lib().meld_csr_rows_to_dense_f64(ptr(self.rowptr), ptr(self.col), ptr(self.val), self.val_f32, int(lo), int(hi - lo),
                                                   G, ptr(out), int(out.stride(0)), stream()), "meld_csr_rows_to_dense_f64")
        return out

    def to_dense(self):
        return self.rows_to_dense(0, self.shape[0])

    def to_scipy(self):
        """The matrix on the host: a ``scipy.sparse.csr_matrix`` of the same structure (stored zeros included) and value dtype."""
        indptr = self.rowptr.cpu().numpy()
        indices = self.col.cpu().numpy()
        if self.nnz > np.iinfo(np.int32).max:
            indices = indices.astype(np.int64)
        else:
            indptr = indptr.astype(np.int32)
        return _scipy_sparse().csr_matrix((self.val.cpu().numpy(), indices, indptr), shape=self.shape)


def truncated_svd_project(A, k, seed=42, return_model=False):
    """Scores X V [N, k] (fp64, on A's device) of the top-k right singular vectors V [G, k] of the UNCENTRED matrix (graphtools'
    TruncatedSVD for sparse input).  ``A``: a ``DeviceCSR`` or any sparse input ``DeviceCSR.from_input`` takes.  Optionally
    returns (scores, V)."""
    if not isinstance(A, DeviceCSR):
        A = DeviceCSR.from_input(A)
    N, G = A.shape
    k = int(k)
    if not 1 <= k <= min(N, G):
        raise ValueError("n_components={} must lie in [1, min(N, G)={}]".format(k, min(N, G)))
    dev = A.device
    if G <= _pca.EXACT_MAX:
        # Gram matrix X^T X from dense row blocks of at most ~1 GiB, then the exact eigenvectors
        C = torch.zeros(G, G, dtype=torch.float64, device=dev)
        for lo, hi in _pca._row_chunks(N, G):
            D = A.rows_to_dense(lo, hi)
            C.addmm_(D.T, D)
            del D
        _, evec = torch.linalg.eigh(C)  # ascending
        V = _pca._flip_signs(evec[:, -k:].flip(1).contiguous())
    else:
        # randomized range finder of pca.py (k + 10 columns, 4 power iterations with QR), products on the CSR matrix
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        r = min(k + 10, min(N, G))
        Q = torch.randn(G, r, dtype=torch.float64, device=dev, generator=gen)
        AT = A.T
        Y = A.matmul(Q)
        for _ in range(4):
            Y, _ = torch.linalg.qr(Y)
            Z, _ = torch.linalg.qr(AT.matmul(Y))
            Y = A.matmul(Z)
        Qy, _ = torch.linalg.qr(Y)
        B = AT.matmul(Qy).T  # [r, G] = Qy^T X
        _, _, Vt = torch.linalg.svd(B, full_matrices=False)
        V = _pca._flip_signs(Vt[:k].T.contiguous())
    Y = A.matmul(V)
    if return_model:
        return Y, V
    return Y


def reduce_data(data, kind, n_components, random_state=None, log=None):
    """The reduction the graph is built on ([UPSTREAM graphtools ``Data._reduce_data``], chosen by ``graph_plan.plan_reduction``):
    ``kind="svd"``: the uncentred truncated SVD of a ``DeviceCSR``; ``"pca"``: the exact top-``n_components`` subspace of a dense
    device matrix (meld_amd/pca.py); ``None``: the data as they are, a ``DeviceCSR`` densified on the device.  Returns
    ``scores``, ``project`` (raw device rows of new cells -> their scores, None without a reduction), ``model`` (its tensors)
    and ``n_features_in``."""
    seed = 42 if random_state is None else int(random_state)
    project = model = None
    n_features_in = int(data.shape[1])
    if kind == "svd":
        if log is not None:
            log("Calculating truncated SVD ({} components)...".format(n_components))
        data, V = truncated_svd_project(data, n_components, seed=seed, return_model=True)
        project = lambda Q, V=V: Q @ V  # noqa: E731  (graphtools' TruncatedSVD: uncentred)
        model = dict(kind="svd", V=V)
    elif kind == "pca":
        if log is not None:
            log("Calculating PCA ({} components)...".format(n_components))
        data, mean, V = _pca.pca_project(data, n_components, seed=seed, return_model=True)
        project = lambda Q, mean=mean, V=V: (Q - mean) @ V  # noqa: E731
        model = dict(kind="pca", mean=mean, V=V)
    elif isinstance(data, DeviceCSR):
        data = data.to_dense()
    return SimpleNamespace(scores=data, project=project, model=model, n_features_in=n_features_in)
