"""Sparse cell-by-gene input on the device (meld_amd/sparse.py, csrc/csr_dense.hip): the CSR products against scipy, the
transpose, the densification, graphtools' uncentred truncated SVD, and MELD.fit on sparse matrices end to end."""
import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu


def _sparse_mod():
    from meld_amd import sparse as msp

    return msp


def _oracle():
    from oracle import meld_oracle

    return meld_oracle


def _skewed_csr(N, G, density, seed, full_row=None, empty_rows=(), full_col=None, empty_cols=()):
    rng = np.random.default_rng(seed)
    X = sparse.random(N, G, density=density, format="lil", random_state=rng, data_rvs=lambda n: rng.normal(size=n) * 3)
    if full_row is not None:
        X[full_row, :] = rng.normal(size=(1, G)) + 5.0
    for r in empty_rows:
        X[r, :] = 0
    if full_col is not None:
        X[:, full_col] = (rng.normal(size=(N, 1)) + 5.0)
    for c in empty_cols:
        X[:, c] = 0
    X = X.tocsr()
    X.eliminate_zeros()
    X.sort_indices()
    return X


def _counts(N, G, programs=6, seed=0, scale=30.0):
    """Nonnegative counts from a few latent programs (usages x sparse nonnegative loadings, Poisson)."""
    rng = np.random.default_rng(seed)
    use = rng.dirichlet(np.full(programs, 0.3), size=N) * rng.uniform(0.5, 1.5, size=(N, 1))
    load = rng.gamma(0.6, 1.0, size=(programs, G)) * (rng.random((programs, G)) < 0.15)
    X = rng.poisson(scale * use @ load).astype(np.float64)
    return sparse.csr_matrix(X)


def _check_product(Y, X, B):
    ref = X @ B
    bound = abs(X) @ np.abs(B)
    err = np.abs(Y - ref).max()
    assert err <= 1e-13 * max(bound.max(), 1e-300), (err, bound.max())


@pytest.mark.parametrize("r", [1, 7, 64, 110, 128, 200])
@pytest.mark.parametrize("vdtype", [np.float32, np.float64])
@pytest.mark.parametrize("itype", [np.int32, np.int64])
def test_forward_product_matches_scipy(r, vdtype, itype):
    import torch

    msp = _sparse_mod()
    # G = 1237 (a multiple of nothing), one row with all G entries (more than one segment), empty rows
    X = _skewed_csr(300, 1237, 0.05, seed=r, full_row=7, empty_rows=(0, 5, 299))
    X.data = X.data.astype(vdtype)
    X.indptr = X.indptr.astype(itype)
    X.indices = X.indices.astype(itype)
    assert X.getnnz(axis=1)[7] == 1237 > _sparse_mod().get_lib().meld_csr_seg_length()
    A = msp.DeviceCSR.from_input(X)
    assert A.val.dtype == (torch.float32 if vdtype == np.float32 else torch.float64)
    rng = np.random.default_rng(r + 1)
    Bh = rng.normal(size=(1237, r))
    B = torch.from_numpy(Bh).cuda()
    Y1 = A.matmul(B).cpu().numpy()
    Y2 = A.matmul(B).cpu().numpy()
    assert np.array_equal(Y1, Y2)  # deterministic from call to call
    _check_product(Y1, X.astype(np.float64), Bh)
    assert np.all(Y1[[0, 5, 299]] == 0)
    # an operand with a leading dimension larger than r (odd: the element-wise load path)
    wide = torch.zeros(1237, r + 3, dtype=torch.float64, device="cuda")
    wide[:, :r] = B
    assert np.array_equal(A.matmul(wide[:, :r]).cpu().numpy(), Y1)
    if vdtype == np.float32:
        # fp32 values and their fp64 widening give the same bits
        Xw = X.astype(np.float64)
        assert np.array_equal(msp.DeviceCSR.from_input(Xw).matmul(B).cpu().numpy(), Y1)


@pytest.mark.parametrize("r", [7, 110])
def test_transposed_product_matches_scipy(r):
    import torch

    msp = _sparse_mod()
    # N = 3000 > the segment length: the column present in every row is split across waves in the transpose
    X = _skewed_csr(3000, 411, 0.03, seed=11, full_col=17, empty_cols=(0, 3, 410))
    A = msp.DeviceCSR.from_input(X)
    AT = A.T
    assert AT.shape == (411, 3000)
    rp = AT.rowptr.cpu().numpy()
    cols = AT.col.cpu().numpy()
    assert np.array_equal(rp, X.tocsc().indptr)
    for g in (17, 100):  # rows ascending inside each column
        assert np.array_equal(cols[rp[g]:rp[g + 1]], X.tocsc().indices[X.tocsc().indptr[g]:X.tocsc().indptr[g + 1]])
    Yh = np.random.default_rng(r).normal(size=(3000, r))
    Yd = torch.from_numpy(Yh).cuda()
    Z1 = AT.matmul(Yd).cpu().numpy()
    Z2 = AT.matmul(Yd).cpu().numpy()
    assert np.array_equal(Z1, Z2)
    _check_product(Z1, X.T.tocsr(), Yh)
    assert np.all(Z1[[0, 3, 410]] == 0)
    # a second transposition of the same matrix is the same
    assert np.array_equal(msp.DeviceCSR.from_input(X).T.matmul(Yd).cpu().numpy(), Z1)


@pytest.mark.parametrize("vdtype", [np.float32, np.float64])
def test_densify_is_exact(vdtype):
    msp = _sparse_mod()
    X = _skewed_csr(500, 333, 0.04, seed=2, full_row=3, empty_rows=(1,))
    X.data = X.data.astype(vdtype)
    A = msp.DeviceCSR.from_input(X)
    assert np.array_equal(A.to_dense().cpu().numpy(), X.toarray().astype(np.float64))
    assert np.array_equal(A.rows_to_dense(100, 250).cpu().numpy(), X[100:250].toarray().astype(np.float64))


def _exact_uncentred_scores(X, k):
    D = X.toarray()
    _, s, Vt = np.linalg.svd(D, full_matrices=False)
    return D @ Vt[:k].T, s


@pytest.mark.parametrize("branch", ["exact", "randomized"])
def test_truncated_svd_matches_the_exact_uncentred_svd(branch):
    from scipy.spatial.distance import pdist

    from meld_amd import pca as mpca

    msp = _sparse_mod()
    X = _counts(2000, 500, programs=6, seed=4)
    k = 6
    Yr, s = _exact_uncentred_scores(X, k)
    assert s[k - 1] > 3 * s[k]  # the gap at k
    old = mpca.EXACT_MAX
    try:
        if branch == "randomized":
            mpca.EXACT_MAX = 400
        Y, V = msp.truncated_svd_project(X, k, seed=0, return_model=True)
    finally:
        mpca.EXACT_MAX = old
    Y = Y.cpu().numpy()
    assert Y.shape == (2000, k) and V.shape == (500, k)
    sub = np.random.default_rng(0).choice(2000, size=400, replace=False)
    tol = 1e-9 if branch == "exact" else 1e-6
    assert np.abs(pdist(Y[sub]) - pdist(Yr[sub])).max() <= tol * pdist(Yr[sub]).max()


def test_fit_on_sparse_input_builds_graphtools_graph():
    """n_pca < min(shape): the graph of the UNCENTRED truncated-SVD scores (graphtools on scipy.sparse input), not that of
    the centred PCA scores the dense path computes."""
    import meld_amd

    mo = _oracle()
    X = _counts(2500, 700, programs=6, seed=7)
    k = 6
    rng = np.random.default_rng(1)
    labels = np.where(rng.random(2500) > 0.5, "treat", "ctrl")
    scores, _ = _exact_uncentred_scores(X, k)
    G_ref = mo.build_graph(scores, knn=7)
    op = meld_amd.MELD(n_pca=k, knn=7, chebyshev_order=30)
    op.fit(X)
    W = op.graph.W
    assert (W != 0).multiply(G_ref.W != 0).nnz == W.nnz == G_ref.W.nnz
    assert abs(W - G_ref.W).max() <= 1e-8
    assert op.data_nu is not None and tuple(op.data_nu.shape) == (2500, k)
    lmax = mo.estimate_lmax(G_ref.L, G_ref.dw)
    op.graph.lmax = lmax
    dens = op.transform(labels)
    ref = mo.meld_filter(mo.sample_indicators(labels)[1], G_ref, beta=60, chebyshev_order=30, lmax=lmax)
    assert np.abs(dens.values - ref).max() <= 1e-5 * np.abs(ref).max()
    # the centred PCA graph of the same data is a different graph: the test tells the two apart
    G_pca = mo.build_graph(X.toarray(), knn=7, n_pca=k)
    assert (G_pca.W != 0).multiply(G_ref.W != 0).nnz < G_ref.W.nnz
    assert abs(G_pca.W - G_ref.W).max() > 1e-4


class _AnnDataStub:
    def __init__(self, X):
        self.X = X


def _same_graph(W1, W2):
    W1, W2 = W1.tocsr(), W2.tocsr()
    W1.sort_indices()
    W2.sort_indices()
    return (W1.shape == W2.shape and np.array_equal(W1.indptr, W2.indptr) and np.array_equal(W1.indices, W2.indices)
            and np.array_equal(W1.data, W2.data))


@pytest.mark.parametrize("n_pca", [6, 40])
def test_input_forms_give_the_same_graph(n_pca):
    import pandas as pd
    import torch

    import meld_amd
    from meld_amd import pca as mpca

    X = _counts(1500, 450, programs=6, seed=5)
    forms = {
        "csr": X, "csc": X.tocsc(), "coo": X.tocoo(), "lil": X.tolil(),
        "csr_array": sparse.csr_array(X), "csr_f32": X.astype(np.float32),
        "pandas": pd.DataFrame.sparse.from_spmatrix(X), "anndata": _AnnDataStub(X),
        "torch": torch.sparse_csr_tensor(torch.from_numpy(X.indptr.astype(np.int64)), torch.from_numpy(X.indices.astype(np.int64)),
                                         torch.from_numpy(X.data), size=X.shape).cuda(),
    }
    old = mpca.EXACT_MAX
    try:
        if n_pca == 40:
            mpca.EXACT_MAX = 400  # the randomized branch
        Ws = {}
        for name, data in forms.items():
            op = meld_amd.MELD(n_pca=n_pca, knn=7)
            op.fit(data)
            Ws[name] = op.graph.W
    finally:
        mpca.EXACT_MAX = old
    for name, W in Ws.items():
        assert _same_graph(W, Ws["csr"]), name


def test_no_reduction_keeps_the_dense_result():
    """n_pca=None (and n_pca >= min(shape)): densified on the device, the same graph as the dense input gives today."""
    import meld_amd

    X = _counts(1500, 40, programs=5, seed=9)
    X32 = X.astype(np.float32)
    for data, dense in ((X, X.toarray()), (X32, X32.toarray())):
        for n_pca in (None, 40, 100):
            W_sp = meld_amd.MELD(n_pca=n_pca, knn=7).fit(data).graph.W
            W_de = meld_amd.MELD(n_pca=n_pca, knn=7).fit(dense).graph.W
            assert _same_graph(W_sp, W_de), n_pca


def test_fit_memory_stays_below_a_dense_copy():
    import torch

    import meld_amd

    N, G = 50_000, 16_000
    rng = np.random.default_rng(0)
    X = sparse.random(N, G, density=0.005, format="csr", random_state=rng, data_rvs=lambda n: rng.poisson(3.0, n) + 1.0)
    op = meld_amd.MELD(knn=5)  # n_pca = 100 < min(shape), G > pca.EXACT_MAX: the randomized branch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    op.fit(X)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("sparse fit N={} G={} nnz={}: peak device memory {:.1f} MB ({:.3f} of a dense copy)".format(
        N, G, X.nnz, peak / 1e6, peak / (N * G * 8)))
    assert peak < N * G * 8 / 4
    assert op.graph.W.shape == (N, N)


def test_refit_detection_and_errors():
    import torch

    import meld_amd

    X = _counts(1200, 300, programs=5, seed=3)
    op = meld_amd.MELD(n_pca=5, knn=7)
    op.fit(X)
    g = op.graph
    op.fit(X.copy())  # equal matrix: no rebuild
    assert op.graph is g
    X2 = X.copy()
    X2.data[0] += 1.0
    op.fit(X2)  # one value changed: rebuilt
    assert op.graph is not g
    # device tensors: identity
    T = torch.sparse_csr_tensor(torch.from_numpy(X.indptr.astype(np.int64)), torch.from_numpy(X.indices.astype(np.int64)),
                                torch.from_numpy(X.data), size=X.shape).cuda()
    op.fit(T)
    g = op.graph
    op.fit(T)
    assert op.graph is g
    bad = X.copy()
    bad.data[3] = np.nan
    with pytest.raises(ValueError, match="Input data contains NaN or infinity"):
        meld_amd.MELD(n_pca=5).fit(bad)
    bad.data[3] = np.inf
    with pytest.raises(ValueError, match="Input data contains NaN or infinity"):
        meld_amd.MELD(n_pca=None).fit(bad)
    with pytest.raises(ValueError, match="2D"):
        meld_amd.MELD(n_pca=5).fit(sparse.coo_array(np.arange(5.0)))
