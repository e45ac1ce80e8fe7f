"""Sparse new cells (meld_amd/extend.py ``prepare_queries``): after a fit on sparse input the new cells are projected with the
truncated SVD's ``Y V`` on the device CSR matrix, after a dense fit with PCA with ``Y V - mean V``, without a reduction they are
densified at their own width -- in no case is a dense copy of ``Y`` at full gene width formed on the host or the device."""
import numpy as np
import pandas as pd
import pytest
import torch
from scipy import sparse

pytestmark = pytest.mark.gpu


def _random_counts(N, G, density, seed):
    rng = np.random.default_rng(seed)
    return sparse.random(N, G, density=density, format="csr", random_state=rng, data_rvs=lambda n: rng.poisson(3.0, n) + 1.0)


def _labels(N, seed=0):
    return np.where(np.random.default_rng(seed).random(N) < 0.5, "expt", "ctrl")


def _torch_csr(Y):
    return torch.sparse_csr_tensor(torch.from_numpy(Y.indptr.astype(np.int64)), torch.from_numpy(Y.indices.astype(np.int64)),
                                   torch.from_numpy(Y.data), size=Y.shape).cuda()


@pytest.fixture(scope="module")
def sparse_fit():
    import meld_amd

    A = _random_counts(3000 + 200, 500, 0.05, 1)
    X, Y = A[:3000], A[3000:]
    op = meld_amd.MELD(n_pca=20, knn=7, verbose=0)
    op.fit_transform(X, _labels(3000))
    return op, Y, op.transform_new(Y.toarray())


@pytest.mark.parametrize("form", ["scipy_csr", "scipy_csc", "torch_sparse_csr", "sparse_dataframe"])
def test_sparse_new_cells_after_a_sparse_fit(sparse_fit, form):
    op, Y, want = sparse_fit
    assert op.graph._extend_state.model["kind"] == "svd" and op.graph.n_features_in == 500
    Ys = {"scipy_csr": Y, "scipy_csc": Y.tocsc(), "torch_sparse_csr": _torch_csr(Y), "sparse_dataframe": pd.DataFrame.sparse.from_spmatrix(Y)}[form]
    out = op.transform_new(Ys)
    assert out.shape == want.shape and list(out.columns) == list(want.columns)
    np.testing.assert_allclose(out.values, want.values, rtol=1e-9, atol=0)
    # the kernel itself: same pattern as that of the dense copy
    a, b = op.graph.build_kernel_to_data(Ys), op.graph.build_kernel_to_data(Y.toarray())
    assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
    np.testing.assert_allclose(a.data, b.data, rtol=1e-9, atol=0)


def test_sparse_cells_of_the_reduced_width_are_refused(sparse_fit):
    op, Y, _ = sparse_fit
    with pytest.raises(ValueError, match=r"Y must be of shape either \(n, 500\) or \(n, 20\)"):
        op.transform_new(Y[:, :20])
    with pytest.raises(ValueError, match=r"Y must be of shape either \(n, 500\) or \(n, 20\)"):
        op.transform_new(Y[:, :21])


@pytest.mark.parametrize("distance", ["euclidean", "manhattan"])
def test_sparse_new_cells_after_a_dense_fit_with_pca(distance):
    import meld_amd

    A = _random_counts(2000 + 150, 300, 0.05, 2)
    X, Y = A[:2000].toarray(), A[2000:]
    op = meld_amd.MELD(n_pca=15, knn=7, distance=distance, verbose=0)
    op.fit_transform(X, _labels(2000))
    assert op.graph._extend_state.model["kind"] == "pca"
    np.testing.assert_allclose(op.transform_new(Y).values, op.transform_new(Y.toarray()).values, rtol=1e-9, atol=0)


@pytest.mark.parametrize("fit_sparse", [False, True])
def test_sparse_new_cells_without_a_reduction(fit_sparse):
    import meld_amd

    A = _random_counts(1500 + 100, 40, 0.3, 3)
    X, Y = A[:1500], A[1500:]
    op = meld_amd.MELD(n_pca=None, knn=7, verbose=0)
    op.fit_transform(X if fit_sparse else X.toarray(), _labels(1500))
    assert op.graph._extend_state.model is None
    np.testing.assert_allclose(op.transform_new(Y).values, op.transform_new(Y.toarray()).values, rtol=1e-9, atol=0)


def test_peak_memory_stays_below_half_a_dense_copy_of_the_new_cells():
    import meld_amd

    M, F = 2000, 30000
    A = _random_counts(2500 + M, F, 0.01, 4)
    X, Y = A[:2500], A[2500:]
    op = meld_amd.MELD(n_pca=20, knn=5, verbose=0)
    op.fit_transform(X, _labels(2500))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = op.transform_new(Y)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("sparse new cells M={} F={} nnz={}: peak device memory {:.1f} MB ({:.4f} of a dense copy)".format(M, F, Y.nnz, peak / 1e6, peak / (M * F * 8)))
    assert peak < M * F * 8 / 2
    assert out.shape == (M, 2) and np.isfinite(out.values).all()
