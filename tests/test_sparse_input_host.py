"""Sparse input, CPU tier: the host normalisation of every accepted type (never densified), refit detection, the work plan
of the CSR products and the register budget of csrc/csr_dense.hip.  No GPU needed."""
import os

import numpy as np
import pandas as pd
import pytest
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoDenseCSR(sparse.csr_matrix):
    """A CSR matrix that refuses to be densified."""

    def toarray(self, *a, **k):
        raise AssertionError("densified on the host")

    def todense(self, *a, **k):
        raise AssertionError("densified on the host")


class _NoDenseCSC(sparse.csc_matrix):
    def toarray(self, *a, **k):
        raise AssertionError("densified on the host")

    def todense(self, *a, **k):
        raise AssertionError("densified on the host")


class _AnnDataStub:
    def __init__(self, X):
        self.X = X


def _fixture():
    rng = np.random.default_rng(0)
    X = sparse.random(60, 45, density=0.1, format="csr", random_state=rng)
    X[3, :] = 0
    X.eliminate_zeros()
    return X


def _equal(A, X):
    return (A.format == "csr" and A.has_canonical_format and A.shape == X.shape and np.array_equal(A.indptr, X.indptr)
            and np.array_equal(A.indices, X.indices) and np.array_equal(A.data, X.data))


def test_every_accepted_host_type_normalises_to_canonical_csr():
    from meld_amd.sparse import is_sparse_input, to_host_csr

    X = _fixture()
    forms = {
        "csr": X, "csc": X.tocsc(), "coo": X.tocoo(), "lil": X.tolil(), "dok": X.todok(), "bsr": X.tobsr(),
        "csr_array": sparse.csr_array(X), "coo_array": sparse.coo_array(X), "pandas": pd.DataFrame.sparse.from_spmatrix(X),
        "anndata": _AnnDataStub(X), "anndata_csc": _AnnDataStub(X.tocsc()),
        "no_dense_csr": _NoDenseCSR(X), "no_dense_csc": _NoDenseCSC(X.tocsc()), "anndata_no_dense": _AnnDataStub(_NoDenseCSR(X)),
    }
    for name, data in forms.items():
        assert is_sparse_input(data), name
        assert _equal(to_host_csr(data), X), name


def test_duplicates_and_unsorted_indices_are_made_canonical():
    from meld_amd.sparse import to_host_csr

    X = _fixture()
    coo = X.tocoo()
    dup = sparse.coo_matrix((np.concatenate([coo.data * 0.5, coo.data * 0.5])[::-1],
                             (np.concatenate([coo.row, coo.row])[::-1], np.concatenate([coo.col, coo.col])[::-1])), shape=X.shape)
    A = to_host_csr(dup)
    assert A.shape == X.shape and abs(A - X).max() < 1e-15 and A.has_canonical_format
    # an unsorted CSR is sorted on a copy: the caller's matrix is left as it is
    U = sparse.csr_matrix((X.data.copy(), X.indices.copy(), X.indptr.copy()), shape=X.shape)
    r = int(np.argmax(np.diff(U.indptr)))
    lo, hi = U.indptr[r], U.indptr[r + 1]
    U.indices[lo:hi] = U.indices[lo:hi][::-1].copy()
    U.data[lo:hi] = U.data[lo:hi][::-1].copy()
    U.has_sorted_indices = False
    before = U.indices.copy()
    assert _equal(to_host_csr(U), X)
    assert np.array_equal(U.indices, before)


def test_dense_inputs_are_not_taken_for_sparse():
    from meld_amd.sparse import is_sparse_input

    X = _fixture().toarray()
    for data in (X, pd.DataFrame(X), _AnnDataStub(X), X.tolist()):
        assert not is_sparse_input(data)


def test_non_2d_sparse_input_is_rejected():
    import meld_amd

    with pytest.raises(ValueError, match="2D"):
        meld_amd.MELD(n_pca=5).fit(sparse.coo_array(np.arange(1.0, 6.0)))


def test_refit_detection_compares_structure_and_values():
    from meld_amd.estimator import _same_csr

    X = _fixture()
    assert _same_csr(X, X.copy())
    Y = X.copy()
    Y.data[0] += 1.0
    assert not _same_csr(X, Y)
    assert not _same_csr(X, X[:, :44].tocsr())
    assert not _same_csr(X.toarray(), X)
    Z = X.copy().tolil()
    Z[3, 0] = 1.0
    assert not _same_csr(X, Z.tocsr())


def test_product_work_plan():
    """The units of meld_csr_spmm_f64: one per MELD_CSR_SEG entries of a row (one for an empty row), consecutive per row;
    partial slots only for rows of more than one segment."""
    import torch

    from meld_amd._lib import get_lib
    from meld_amd.sparse import DeviceCSR

    seg = get_lib().meld_csr_seg_length()
    lens = np.array([0, 1, seg, seg + 1, 3 * seg, 0, 2 * seg + 5])
    rowptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    nnz = int(lens.sum())
    A = DeviceCSR(rowptr, torch.zeros(nnz, dtype=torch.int32), torch.zeros(nnz, dtype=torch.float64), (len(lens), 10))
    p = A.plan()
    nseg = [1, 1, 1, 2, 3, 1, 3]
    assert p["n_units"] == sum(nseg)
    assert p["unit_row"].tolist() == [i for i, s in enumerate(nseg) for _ in range(s)]
    assert p["unit_off"].tolist() == list(np.cumsum([0] + nseg[:-1]))
    assert p["split_rows"].tolist() == [3, 4, 6]
    assert p["n_slots"] == 8
    assert [int(p["part_off"][i]) for i in (3, 4, 6)] == [0, 2, 5]


def test_csr_kernels_do_not_spill():
    from tests.test_kernel_resources import _resource_usage

    rows = _resource_usage(os.path.join(ROOT, "meld_amd", "csrc", "csr_dense.hip"))
    assert sum("csr_spmm_kernel" in k for k in rows) == 4, sorted(rows)
    assert any("csr_spmm_merge_kernel" in k for k in rows) and any("csr_transpose_keys_kernel" in k for k in rows)
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]:"] == 0, (name, r)
        if "csr_spmm_kernel" in name:
            assert r["Occupancy [waves/SIMD]:"] == 8, (name, r)
