"""The L1 / L-infinity kNN graph beyond the dense route (meld_amd/metric_knn.py, csrc/metric_knn.hip) on the GPU: against the
oracle (which hands the metric to sklearn), against the dense route, pruned against unpruned, and at full size against a
library brute force."""
import os

import numpy as np
import pytest
import torch
from scipy import sparse

pytestmark = pytest.mark.gpu


def _oracle():
    from oracle import meld_oracle as mo

    return mo


def _csr_equal_pattern_close(A, B, rtol):
    A = sparse.csr_matrix(A)
    B = sparse.csr_matrix(B)
    A.sort_indices()
    B.sort_indices()
    assert A.shape == B.shape
    assert A.nnz == B.nnz, (A.nnz, B.nnz)
    assert np.array_equal(A.indptr, B.indptr)
    assert np.array_equal(A.indices, B.indices)
    np.testing.assert_allclose(A.data, B.data, rtol=rtol, atol=0)


@pytest.fixture(scope="module")
def cells20k():
    mo = _oracle()
    return mo.synthetic_cells(20000, n_dims=10, seed=5)


@pytest.mark.parametrize("metric", ["manhattan", "chebyshev"])
def test_beyond_the_dense_route_matches_the_oracle(metric, cells20k):
    import meld_amd

    mo = _oracle()
    X, labels = cells20k
    G = mo.build_graph(X, knn=7, algorithm="brute", distance=metric)
    lmax = mo.estimate_lmax(G.L, G.dw)
    op = meld_amd.MELD(knn=7, distance=metric, chebyshev_order=30, lmax=lmax, verbose=0).fit(X)
    assert op.graph.info["route"] == "metric_knn" and op.graph.info["metric"] == metric
    _csr_equal_pattern_close(op.graph.W, G.W, rtol=1e-9)
    np.testing.assert_allclose(op.graph.dw, G.dw, rtol=1e-9)
    np.testing.assert_allclose(op.graph.bandwidth_host, G.info["bandwidth"], rtol=1e-12, atol=0)
    out = op.transform(labels)
    samples, ind = mo.sample_indicators(labels)
    ref = mo.meld_filter(ind, G, beta=60, chebyshev_order=30, lmax=lmax)
    assert list(out.columns) == list(samples)
    assert np.abs(out.values - ref).max() <= 1e-5 * np.abs(ref).max()


@pytest.mark.parametrize("metric,kw", [
    ("cityblock", dict(decay=None)),
    ("chebyshev", dict(decay=None)),
    ("l1", dict(kernel_symm="*")),
    ("manhattan", dict(kernel_symm="mnn", theta=0.5)),
    ("chebyshev", dict(kernel_symm="mnn", theta=0.5)),
    ("manhattan", dict(anisotropy=0.5)),
])
def test_graph_options_match_the_oracle(metric, kw, cells20k):
    import meld_amd

    mo = _oracle()
    X, _ = cells20k
    G = mo.build_graph(X, knn=7, algorithm="brute", distance="manhattan" if metric in ("cityblock", "l1") else metric, **kw)
    op = meld_amd.MELD(knn=7, distance=metric, verbose=0, **kw).fit(X)
    assert op.graph.info["route"] == "metric_knn"
    _csr_equal_pattern_close(op.graph.W, G.W, rtol=1e-9)
    np.testing.assert_allclose(op.graph.dw, G.dw, rtol=1e-9)


@pytest.mark.parametrize("metric", ["manhattan", "chebyshev"])
def test_copies_of_a_cell_match_the_oracle(metric, cells20k):
    """45 and 70 copies of two cells: bandwidth eps on those rows (more copies than knn + 1), their rows through the exact sweep."""
    import meld_amd

    mo = _oracle()
    X = cells20k[0].copy()
    X[100:145] = X[99]
    X[5000:5070] = X[4999]
    G = mo.build_graph(X, knn=7, algorithm="brute", distance=metric)
    op = meld_amd.MELD(knn=7, distance=metric, verbose=0).fit(X)
    assert op.graph.info["n_flagged_rows"] >= 45 + 70
    _csr_equal_pattern_close(op.graph.W, G.W, rtol=1e-9)
    np.testing.assert_allclose(op.graph.dw, G.dw, rtol=1e-9)
    np.testing.assert_allclose(op.graph.bandwidth_host, G.info["bandwidth"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("metric", ["manhattan", "chebyshev"])
def test_equals_the_dense_route(metric):
    from meld_amd.dense import build_dense_knn_graph
    from meld_amd.metric_knn import build_metric_knn_graph

    mo = _oracle()
    X, _ = mo.synthetic_cells(8000, n_dims=12, seed=8)
    Xd = torch.from_numpy(X).cuda()
    A = build_metric_knn_graph(Xd, 9, 40, 1e-4, 1, metric)
    B = build_dense_knn_graph(Xd, 9, 40, 1e-4, anisotropy=1, metric=metric)
    _csr_equal_pattern_close(A.W, B.W, rtol=1e-12)
    np.testing.assert_allclose(A.bandwidth_host, B.bandwidth_host, rtol=1e-12, atol=0)


def _graph_bits(G):
    W = sparse.csr_matrix(G.W)
    W.sort_indices()
    return W.indptr.copy(), W.indices.copy(), W.data.copy(), np.asarray(G.bandwidth_host).copy()


@pytest.mark.parametrize("metric", ["manhattan", "chebyshev"])
def test_pruned_build_is_bit_identical_to_unpruned(metric, monkeypatch):
    from meld_amd.metric_knn import build_metric_knn_graph

    mo = _oracle()
    X, _ = mo.synthetic_cells(50000, n_dims=20, seed=11)
    Xd = torch.from_numpy(X).cuda()
    a = build_metric_knn_graph(Xd, 7, 40, 1e-4, 1, metric)
    b = build_metric_knn_graph(Xd, 7, 40, 1e-4, 1, metric)
    monkeypatch.setenv("MELD_DEV", "1")
    monkeypatch.setenv("MELD_METRIC_PRUNE", "0")
    c = build_metric_knn_graph(Xd, 7, 40, 1e-4, 1, metric)
    assert a.info["prune"] and not c.info["prune"] and c.info["tile_skip_fraction"] == 0.0
    ba, bb, bc = _graph_bits(a), _graph_bits(b), _graph_bits(c)
    for x, y, z in zip(ba, bb, bc):
        assert np.array_equal(x, y) and np.array_equal(x, z)


def test_clustered_data_skips_tiles():
    from meld_amd.metric_knn import build_metric_knn_graph

    mo = _oracle()
    X, _ = mo.synthetic_cells(200000, n_dims=20, seed=12)
    G = build_metric_knn_graph(torch.from_numpy(X).cuda(), 7, 40, 1e-4, 1, "manhattan")
    assert G.info["tile_skip_fraction"] > 0.0, G.info


def test_full_size_neighbours_match_a_brute_force():
    """1M x 50, manhattan: bandwidths and neighbour sets (the cells inside the kernel radius) of 2,000 random rows against a chunked
    library brute force over all cells."""
    import meld_amd

    mo = _oracle()
    N, knn = 10**6, 7
    X, _ = mo.synthetic_cells(N, n_dims=50, seed=0)
    op = meld_amd.MELD(knn=knn, distance="manhattan", n_pca=None, verbose=0).fit(X)
    G = op.graph
    assert G.info["route"] == "metric_knn"
    bw = np.asarray(G.bandwidth_host)
    Xd = torch.from_numpy(X).cuda()
    rows = np.sort(np.random.default_rng(0).choice(N, 2000, replace=False))
    # the directed kernel row i holds the cells j != i with exp(-(d_ij / bw_i)^40) >= 1e-4; the symmetrised W holds the union of
    # both directions: check the bandwidths, and that every cell of the directed row is a neighbour in W
    W = sparse.csr_matrix(G.W)
    rf = (-np.log(1e-4)) ** (1 / 40)
    for lo in range(0, rows.shape[0], 8):  # (8 x 1M pairs a launch: the library kernel is wrong beyond 2^32 threads in one)
        r = rows[lo : lo + 8]
        D = torch.cdist(Xd[torch.from_numpy(r).cuda()], Xd, p=1.0)
        kth = torch.kthvalue(D, knn + 1, dim=1).values.cpu().numpy()
        np.testing.assert_allclose(bw[r], np.maximum(kth, np.finfo(float).eps), rtol=1e-12, atol=0)
        Dh = D.cpu().numpy()
        for t, i in enumerate(r):
            inside = set(np.nonzero(Dh[t] < bw[i] * rf * (1 - 1e-9))[0].tolist()) - {int(i)}
            got = set(W.indices[W.indptr[i] : W.indptr[i + 1]].tolist())
            assert inside <= got, (i, len(inside - got))
            far = Dh[t][list(got)] > bw[i] * rf * (1 + 1e-9)
            # (an entry beyond row i's radius comes from the other direction: row j's radius holds i)
            for j in np.asarray(list(got))[far]:
                assert Dh[t][j] <= bw[j] * rf * (1 + 1e-9), (i, j)


@pytest.mark.parametrize("metric", ["manhattan", "chebyshev"])
def test_degenerate_neighbourhoods_are_refused(metric):
    import meld_amd

    with pytest.raises(NotImplementedError, match="degenerate"):
        meld_amd.MELD(distance=metric, verbose=0).fit(np.zeros((20000, 3)))
