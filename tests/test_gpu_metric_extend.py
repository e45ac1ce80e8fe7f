"""New cells on the L1 / L-infinity graphs (meld_amd/metric_knn.py ``cross_kernel_rows``, csrc/metric_knn.hip) on the GPU.

Expected values are a brute force written here: ``scipy.spatial.distance.cdist(Y, X, metric)`` and the semantics of DESIGN.md
section 4.10 -- bw_i = max(s * (knn_c-th smallest D_i.), eps), K_ij = exp(-(D_ij / bw_i)^decay) kept where >= max(thresh, eps),
a new cell has no self entry, ``decay=None`` is the connectivity of the knn_c nearest fitted cells in (distance, column) order.
Tolerances are those of the L1 / L-inf graph itself: identical pattern, values rtol = 1e-9.  Every comparison first asserts
that no brute-force value lies within 1e-6 (relative) of the threshold, so that the pattern is well defined."""
import numpy as np
import pandas as pd
import pytest
import torch
from scipy import sparse
from scipy.spatial.distance import cdist

pytestmark = pytest.mark.gpu

METRICS = ["manhattan", "chebyshev"]
SCIPY_NAME = {"manhattan": "cityblock", "chebyshev": "chebyshev"}
EPS = float(np.finfo(float).eps)


def _cells(N, M, d, seed):
    from oracle import meld_oracle as mo

    A, labels = mo.synthetic_cells(N + M, n_dims=d, seed=seed)
    return A[:N], A[N:], labels[:N]


def brute_kernel(X, Y, metric, knn, decay=40, thresh=1e-4, scale=1.0, bandwidth=None):
    """The kernel from Y to X, dense semantics; asserts the margin around the threshold."""
    D = cdist(Y, X, SCIPY_NAME[metric])
    M, N = D.shape
    knn_c = min(int(knn), N)
    if decay is None:
        K = np.zeros((M, N))
        first = np.argsort(D, axis=1, kind="stable")[:, :knn_c]  # (stable: ties by column)
        K[np.arange(M)[:, None], first] = 1.0
        return sparse.csr_matrix(K)
    thr = max(float(thresh), EPS)
    if bandwidth is None:
        bw = np.maximum(scale * np.partition(D, knn_c - 1, axis=1)[:, knn_c - 1], EPS)
    else:
        bw = np.full(M, max(scale * float(bandwidth), EPS))
    # beyond 1.5 kernel radii a value is exp(-(1.5^decay) * log(1 / thr)): zero for every purpose here, and nowhere near thr
    rf = (-np.log(thr)) ** (1.0 / decay)
    near = D <= 1.5 * rf * bw[:, None]
    r, c = np.nonzero(near)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.exp(-np.power(D[r, c] / bw[r], decay))
    v[np.isnan(v)] = 1.0
    gap = np.abs(v - thr).min() / thr
    print("closest brute-force value to thresh (relative): {:.3g}".format(gap))
    assert gap > 1e-6, gap
    keep = v >= thr
    return sparse.csr_matrix((v[keep], (r[keep], c[keep])), shape=(M, N))


def assert_same_kernel(got, ref, rtol=1e-9):
    got, ref = sparse.csr_matrix(got), sparse.csr_matrix(ref)
    got.sort_indices()
    ref.sort_indices()
    assert got.shape == ref.shape
    assert np.array_equal(got.indptr, ref.indptr), np.nonzero(np.diff(got.indptr) != np.diff(ref.indptr))[0][:10]
    assert np.array_equal(got.indices, ref.indices)
    np.testing.assert_allclose(got.data, ref.data, rtol=rtol, atol=0)


def assert_same_bits(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _fit(X, metric, knn, **kw):
    import meld_amd

    kw.setdefault("n_pca", None)  # (the default reduces data wider than 100 columns: the brute force here is on the cells as given)
    return meld_amd.MELD(knn=knn, distance=metric, verbose=0, **kw).fit(X)


_FITS = {}


def fit20k(metric):
    """The 20,000-cell fit (route ``metric_knn``) with its densities, shared by the tests of a metric."""
    if metric not in _FITS:
        import meld_amd

        X, Y, labels = _cells(20000, 3000, 10, 5)
        op = meld_amd.MELD(knn=7, distance=metric, verbose=0)
        op.fit_transform(X, labels)
        assert op.graph.info["route"] == "metric_knn"
        _FITS[metric] = (op, X, Y, brute_kernel(X, Y, metric, 7))
    return _FITS[metric]


def _far(Y):
    Y = Y.copy()
    Y[:3] += 200.0  # three new cells far from everything: every fitted cell lies within their kernel radius
    return Y


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("N,M,d,seed,knn,edit", [
    (200, 63, 3, 4, 5, None),       # a partial tile and a partial wave
    (1000, 130, 17, 3, 5, None),    # d no multiple of 16, M = 2 * 64 + 2
    (600, 70, 50, 7, 7, _far),      # three rows take the sweep and see every fitted cell
    (300, 5, 256, 11, 5, None),     # the widest rows the kernels take, fewer new cells than lanes
    (8500, 64, 5, 2, 5, None),      # a dense fit large enough for a locality order of the cached fitted cells
])
def test_against_brute_force_dense_route(metric, N, M, d, seed, knn, edit):
    X, Y, _ = _cells(N, M, d, seed)
    if edit is not None:
        Y = edit(Y)
    op = _fit(X, metric, knn)
    assert op.graph.info.get("dense")
    ref = brute_kernel(X, Y, metric, knn)
    got = op.graph.build_kernel_to_data(Y)
    assert_same_kernel(got, ref)
    if edit is not None:
        assert (np.diff(got.indptr)[:3] == N).all() and op.graph.last_extend["n_flagged_rows"] >= 3


@pytest.mark.parametrize("metric", METRICS)
def test_against_brute_force_metric_knn_route(metric):
    op, X, Y, ref = fit20k(metric)
    assert_same_kernel(op.graph.build_kernel_to_data(Y), ref)


@pytest.mark.parametrize("metric", METRICS)
def test_same_bits_whatever_the_route_through_the_search(metric, monkeypatch):
    op, X, Y, _ = fit20k(metric)
    G = op.graph
    base = G.kernel_to_data_device(Y)
    pruned = dict(G.last_extend)
    assert pruned["prune"]
    # slices of the fitted cells: one, four, chosen
    for ns in (1, 4):
        assert_same_bits(G.kernel_to_data_device(Y, n_slices=ns), base)
        assert G.last_extend["n_slices"] == [ns]
    # new cells in several chunks (sized from free memory in production: here 1024 at a time)
    from meld_amd import metric_knn as mk

    with monkeypatch.context() as mp:
        mp.setattr(mk, "_cross_chunk_rows", lambda M, *rest: min(M, 1024))
        assert_same_bits(G.kernel_to_data_device(Y), base)
        assert len(G.last_extend["n_slices"]) == 3
    # a few new cells: the automatic choice splits the fitted cells
    few = G.kernel_to_data_device(Y[:100])
    assert max(G.last_extend["n_slices"]) > 1
    assert_same_bits(G.kernel_to_data_device(Y[:100], n_slices=1), few)
    # new cells in another order: the same rows, permuted
    p = np.random.default_rng(0).permutation(Y.shape[0])
    a, b = G.build_kernel_to_data(Y[p]), sparse.csr_matrix(G.build_kernel_to_data(Y))[p]
    assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data)
    # every tile visited: the same bits, more tile pairs
    G.kernel_to_data_device(Y, n_slices=1)
    pruned = dict(G.last_extend)
    monkeypatch.setenv("MELD_METRIC_PRUNE", "0")
    assert_same_bits(G.kernel_to_data_device(Y, n_slices=1), base)
    unpruned = dict(G.last_extend)
    assert not unpruned["prune"] and unpruned["tiles_done"] == unpruned["tile_pairs"]
    assert pruned["tiles_done"] < unpruned["tiles_done"], (pruned, unpruned)
    print("tile pairs visited: {} of {}".format(pruned["tiles_done"], unpruned["tiles_done"]))


@pytest.mark.parametrize("metric", METRICS)
def test_copies_of_a_fitted_cell(metric):
    """45 copies of one fitted cell, more than the 32 entries of a candidate list: new cells equal to it have an eps bandwidth,
    new cells near it a list that ends inside the kernel radius -- both take the sweep."""
    X, Y, _ = _cells(900, 40, 8, 9)
    X[100:145] = X[17]
    Y[:5] = X[17]
    Y[5:10] = X[17] + 1e-3 * np.arange(1, 6)[:, None]
    op = _fit(X, metric, 5)
    ref = brute_kernel(X, Y, metric, 5)
    got = op.graph.build_kernel_to_data(Y)
    assert_same_kernel(got, ref)
    assert op.graph.last_extend["n_flagged_rows"] >= 10
    for r in range(5):
        row = got[r].toarray().ravel()
        assert row[17] == 1.0 and (row[100:145] == 1.0).all() and row.sum() == 46.0


@pytest.mark.parametrize("metric", METRICS)
def test_options(metric):
    X, Y, _ = _cells(1500, 200, 12, 13)
    op = _fit(X, metric, 6)
    G = op.graph
    assert_same_kernel(G.build_kernel_to_data(Y, knn=11), brute_kernel(X, Y, metric, 11))
    for s in (0.5, 2.0):
        assert_same_kernel(G.build_kernel_to_data(Y, bandwidth_scale=s), brute_kernel(X, Y, metric, 6, scale=s))
    b = float(np.median(cdist(Y, X, SCIPY_NAME[metric]).min(axis=1))) * 1.5
    assert_same_kernel(G.build_kernel_to_data(Y, bandwidth=b), brute_kernel(X, Y, metric, 6, bandwidth=b))
    assert_same_kernel(G.build_kernel_to_data(Y, bandwidth=b, bandwidth_scale=0.5), brute_kernel(X, Y, metric, 6, bandwidth=b, scale=0.5))
    # the unweighted graph: the knn nearest fitted cells, no bandwidth looked at (continuous data: no ties)
    opn = _fit(X, metric, 6, decay=None)
    ref = brute_kernel(X, Y, metric, 6, decay=None)
    assert (np.diff(ref.indptr) == 6).all()
    assert_same_kernel(opn.graph.build_kernel_to_data(Y), ref)
    assert_same_kernel(opn.graph.build_kernel_to_data(Y, bandwidth=b, bandwidth_scale=3.0), ref)
    assert_same_kernel(opn.graph.build_kernel_to_data(Y, knn=9), brute_kernel(X, Y, metric, 9, decay=None))


def _check_transitions(op, Y, ref):
    from sklearn.preprocessing import normalize

    T = op.graph.extend_to_data(Y)
    np.testing.assert_allclose(np.asarray(T.sum(axis=1)).ravel(), 1.0, rtol=1e-12)
    assert_same_kernel(T, normalize(ref, "l1", axis=1))
    want = normalize(ref, "l1", axis=1) @ op.sample_densities.values
    out = op.transform_new(Y)
    assert list(out.columns) == list(op.sample_densities.columns) and out.shape == want.shape
    np.testing.assert_allclose(out.values, want, rtol=1e-9, atol=0)
    F = torch.from_numpy(np.ascontiguousarray(op.sample_densities.values)).cuda()
    np.testing.assert_allclose(op.graph.interpolate_device(F, Y).cpu().numpy(), want, rtol=1e-9, atol=0)
    np.testing.assert_allclose(op.graph.interpolate(op.sample_densities.values, Y=Y), want, rtol=1e-9, atol=0)


@pytest.mark.parametrize("metric", METRICS)
def test_transitions_and_interpolation(metric):
    import meld_amd

    X, Y, labels = _cells(600, 70, 50, 7)
    op = meld_amd.MELD(knn=7, distance=metric, verbose=0)
    op.fit_transform(X, labels)
    assert op.graph.info.get("dense")
    _check_transitions(op, Y, brute_kernel(X, Y, metric, 7))
    op, X, Y, ref = fit20k(metric)
    _check_transitions(op, Y, ref)


@pytest.mark.parametrize("metric", METRICS)
def test_pca_model_raw_and_reduced_cells(metric):
    import meld_amd
    from sklearn.preprocessing import normalize

    X, Y, labels = _cells(800, 90, 40, 21)
    op = meld_amd.MELD(knn=5, distance=metric, n_pca=10, verbose=0)
    op.fit_transform(X, labels)
    st = op.graph._extend_state
    assert op.graph.n_features_in == 40 and tuple(st.X.shape) == (800, 10)
    mean, V = st.model["mean"].cpu().numpy().reshape(1, -1), st.model["V"].cpu().numpy()
    Xr, Yr = st.X.cpu().numpy(), (Y - mean) @ V
    ref = brute_kernel(Xr, Yr, metric, 5)
    assert_same_kernel(op.graph.build_kernel_to_data(Y), ref)
    assert_same_kernel(op.graph.build_kernel_to_data(Yr), ref)
    want = normalize(ref, "l1", axis=1) @ op.sample_densities.values
    np.testing.assert_allclose(op.transform_new(Y).values, want, rtol=1e-9, atol=0)
    np.testing.assert_allclose(op.transform_new(pd.DataFrame(Yr)).values, want, rtol=1e-9, atol=0)
    with pytest.raises(ValueError, match=r"Y must be of shape either \(n, 40\) or \(n, 10\)"):
        op.graph.build_kernel_to_data(Y[:, :11])
