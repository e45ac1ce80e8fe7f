"""Connected components and induced subgraphs on the device (meld_amd/components.py, csrc/components.hip) against scipy on the
host: labels and weights compare exactly, with no tolerance."""
import math

import numpy as np
import pytest
import torch
from scipy import sparse
from scipy.sparse.csgraph import connected_components

pytestmark = pytest.mark.gpu


def _sym(a, b, n, w=None):
    w = np.ones(len(a)) if w is None else w
    W = sparse.coo_matrix((w, (a, b)), shape=(n, n))
    return (W + W.T).tocsr()


def _path(order, n=None):
    order = np.asarray(order)
    return _sym(order[:-1], order[1:], len(order) if n is None else n)


def _adv(m):
    """the recursively interleaved numbering: adv(m) = [2x for x in adv(m/2)] + reversed([2x + 1 ...])"""
    if m == 1:
        return [0]
    h = _adv(m // 2)
    return [2 * x for x in h] + [2 * x + 1 for x in reversed(h)]


def _zigzag(n):
    z = np.empty(n, dtype=np.int64)
    z[0::2] = np.arange((n + 1) // 2)
    z[1::2] = n - 1 - np.arange(n // 2)
    return z


def _grid(g, rng):
    idx = rng.permutation(g * g).reshape(g, g)
    a = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    b = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    return _sym(a, b, g * g)


def _mixture(rng):
    """5,000 vertices: three random-numbered paths (2,000 / 1,500 / 500), 250 disjoint pairs, 500 isolated vertices"""
    n = 5000
    ids = rng.permutation(n)
    a, b, at = [], [], 0
    for length in (2000, 1500, 500):
        p = ids[at:at + length]
        a.append(p[:-1])
        b.append(p[1:])
        at += length
    pairs = ids[at:at + 500].reshape(250, 2)
    a.append(pairs[:, 0])
    b.append(pairs[:, 1])
    return _sym(np.concatenate(a), np.concatenate(b), n)


def _shapes():
    rng = np.random.default_rng(7)
    return {
        "path_random": lambda: _path(rng.permutation(4097)),
        "path_in_order": lambda: _path(np.arange(4097)),
        "path_zigzag": lambda: _path(_zigzag(4097)),
        "path_interleaved": lambda: _path(_adv(4096)),
        "grid_random": lambda: _grid(64, rng),
        "star_centre_last": lambda: _sym(np.full(2999, 2999), np.arange(2999), 3000),
        "mixture_753": lambda: _mixture(rng),
        "one_vertex": lambda: sparse.csr_matrix((1, 1)),
        "two_vertices_no_edge": lambda: sparse.csr_matrix((2, 2)),
    }


@pytest.mark.parametrize("name", list(_shapes()))
def test_adversarial_shapes_equal_scipy(name):
    from meld_amd.components import default_max_rounds
    from meld_amd.graph import DeviceGraph

    W = _shapes()[name]()
    n_ref, lab_ref = connected_components(W, directed=False)
    if name == "mixture_753":
        assert n_ref == 753
    G = DeviceGraph.from_scipy(W)
    n, lab = G.connected_components()
    print(name, "rounds", G.components_info["rounds"], "components", n)
    assert n == n_ref and lab.dtype == np.int32
    assert np.array_equal(lab, lab_ref)
    assert G.component_sizes.dtype == np.int64 and np.array_equal(G.component_sizes, np.bincount(lab_ref))
    assert G.is_connected() == (n_ref == 1)
    assert G.components_info["rounds"] <= default_max_rounds(W.shape[0])
    assert G.components_info == dict(rounds=G.components_info["rounds"], n_components=n_ref, largest=int(np.bincount(lab_ref).max()))
    n_dev, lab_dev = G.connected_components_device()
    assert n_dev == n_ref and lab_dev.is_cuda and lab_dev.dtype == torch.int32 and tuple(lab_dev.shape) == (W.shape[0],)


@pytest.fixture(scope="module")
def blobs():
    """MELD(knn=5).fit on 9,000 x 10 cells, three unit-variance Gaussian blobs centred at 0, 30 and 60 in every coordinate, rows
    shuffled: above the 8,192 cells from which the builder permutes the cells for locality."""
    import meld_amd as meld

    rng = np.random.default_rng(3)
    X = rng.normal(size=(9000, 10)) + np.repeat([0.0, 30.0, 60.0], 3000)[:, None]
    X = X[rng.permutation(9000)]
    op = meld.MELD(knn=5, verbose=False).fit(X)
    G = op.graph
    W = G.W
    return dict(G=G, W=W, ref=connected_components(W, directed=False))


def test_fitted_graph_with_a_locality_permutation(blobs):
    G, (n_ref, lab_ref) = blobs["G"], blobs["ref"]
    assert G.perm is not None
    assert n_ref == 3
    n, lab = G.connected_components()
    assert n == 3 and np.array_equal(lab, lab_ref)
    assert np.array_equal(G.component_sizes, np.bincount(lab_ref)) and not G.is_connected()
    e, _ = G.fourier_basis(8)
    assert int((e <= 1e-6 * 2 * G.dw.max()).sum()) == 3


@pytest.fixture(scope="module")
def random_parent():
    from meld_amd.graph import DeviceGraph

    A = sparse.random(3000, 3000, density=0.004, random_state=np.random.RandomState(5), format="csr")
    A = sparse.triu(A, k=1)
    W = (A + A.T).tocsr()
    W.sort_indices()
    return dict(G=DeviceGraph.from_scipy(W), W=W)


@pytest.mark.parametrize("parent", ["random", "fitted"])
@pytest.mark.parametrize("selection", ["sorted", "shuffled", "mask"])
def test_subgraph_equals_scipy_slicing(parent, selection, random_parent, blobs):
    P = random_parent if parent == "random" else blobs
    G, W = P["G"], P["W"]
    N = W.shape[0]
    rng = np.random.default_rng(13)
    ind = np.sort(rng.choice(N, N // 2, replace=False))
    if selection == "shuffled":
        ind = rng.permutation(ind)
    arg = ind
    if selection == "mask":
        arg = np.zeros(N, dtype=bool)
        arg[ind] = True
    sub = G.subgraph(arg)
    ref = W[ind][:, ind].tocsr()
    ref.sort_indices()
    got = sub.W
    assert sub.N == len(ind) and got.shape == ref.shape
    assert np.array_equal(got.indptr, ref.indptr) and np.array_equal(got.indices, ref.indices)
    assert np.array_equal(got.data.view(np.int64), ref.data.view(np.int64))  # bit for bit
    # rows hold fewer than 1,000 positive terms: any summation order agrees within 2 (n - 1) 2^-53 < 2.3e-13
    assert np.diff(ref.indptr).max() < 1000
    np.testing.assert_allclose(sub.dw, np.ravel(ref.sum(1)), rtol=1e-12, atol=0)
    assert np.array_equal(sub.K.diagonal(), G.K.diagonal()[ind])
    assert sub.info["orig_idx"].dtype == np.int64 and np.array_equal(sub.info["orig_idx"], ind)
    assert sub.knn == G.knn
    if selection == "shuffled" or G.perm is not None:
        assert sub.perm is not None
    # the same selection from the device
    dev = G.subgraph(torch.from_numpy(arg).cuda())
    assert np.array_equal(dev.rowptr.cpu().numpy(), sub.rowptr.cpu().numpy()) and np.array_equal(dev.col.cpu().numpy(), sub.col.cpu().numpy())
    assert np.array_equal(dev.info["orig_idx"], ind)


def test_extract_components_and_largest_component(blobs):
    G, (n_ref, lab_ref) = blobs["G"], blobs["ref"]
    parts = G.extract_components()
    assert len(parts) == 3
    for c, sub in enumerate(parts):
        assert sub.info["component"] == c
        assert np.array_equal(sub.info["orig_idx"], np.flatnonzero(lab_ref == c))
        assert sub.is_connected()
    assert np.array_equal(np.sort(np.concatenate([s.info["orig_idx"] for s in parts])), np.arange(G.N))
    big = G.largest_component()
    assert big.N == G.component_sizes.max()
    assert big.info["component"] == int(np.argmax(G.component_sizes))


def test_largest_component_through_the_estimator(blobs):
    """MELD.fit on the largest component, a common injected lmax, against the same estimator on the scipy-sliced weights: 1e-11,
    the bar tests/test_gpu_fullsize.py sets for this recurrence on a device-built against a scipy-built CSR."""
    import meld_amd as meld
    from meld_amd.graph import DeviceGraph

    G, W = blobs["G"], blobs["W"]
    big = G.largest_component()
    idx = big.info["orig_idx"]
    labels = np.random.default_rng(2).integers(0, 2, size=G.N)
    other = DeviceGraph.from_scipy(W[idx][:, idx])
    lmax = 2.0 * float(big.dw.max())
    big.lmax = lmax
    other.lmax = lmax
    got = meld.MELD(verbose=False).fit(big).transform(labels[idx])
    want = meld.MELD(verbose=False).fit(other).transform(labels[idx])
    assert got.shape == (len(idx), 2) and np.isfinite(got.values).all()
    np.testing.assert_allclose(got.values, want.values, rtol=1e-11, atol=0)


def test_argument_errors(random_parent):
    """All host-side raises after normal launches."""
    from meld_amd.graph import DeviceGraph

    G = random_parent["G"]
    N = G.N
    for bad in (np.array([1, 2, 2]), torch.tensor([5, 7, 5]).cuda()):
        with pytest.raises(ValueError, match="more than once"):
            G.subgraph(bad)
    for bad in (np.array([0, N]), np.array([-1, 3]), torch.tensor([0, N]).cuda()):
        with pytest.raises(ValueError, match="outside"):
            G.subgraph(bad)
    for bad in (np.array([], dtype=np.int64), np.zeros(N, dtype=bool), torch.zeros(N, dtype=torch.bool).cuda()):
        with pytest.raises(ValueError, match="empty"):
            G.subgraph(bad)
    with pytest.raises(ValueError, match="one entry per cell"):
        G.subgraph(np.ones(N - 1, dtype=bool))
    for bad in (np.array([1.0, 2.0]), torch.tensor([1.0, 2.0]).cuda()):
        with pytest.raises(TypeError, match="integer array or a boolean mask"):
            G.subgraph(bad)
    P = DeviceGraph.from_scipy(_path(np.random.default_rng(7).permutation(4097)))
    with pytest.raises(RuntimeError, match=r"after 1 rounds"):
        P.connected_components_device(max_rounds=1)
    assert getattr(P, "_components", None) is None
    assert P.connected_components_device()[0] == 1 and P.components_info["rounds"] <= 4 * math.ceil(math.log2(4097)) + 64
