"""Louvain without a device: the host restatement (tests/louvain_reference.py) against networkx -- its modularity against
``networkx.community.modularity``, its partitions against ``louvain_communities`` on five families of kNN graphs --, the argument
contract of the C entries (every refusal comes before any launch), the argument checks of ``meld_amd.louvain`` that raise before
anything touches the device, and what hipcc reports for the kernels of csrc/louvain.hip (no private memory)."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import sparse
from scipy.spatial import cKDTree

from tests import louvain_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Q of the restatement may fall short of networkx's worst seed by this much (DESIGN.md section 4.17 holds the table behind it:
# twice the largest deficit over the five families below)
QUALITY_MARGIN = 0.0084


def knn_graph(X, knn=7):
    """Symmetrised Gaussian-weighted kNN graph: exp(-(d / d_knn)^2) to the knn nearest points, (K + K') / 2, no diagonal."""
    d, idx = cKDTree(X).query(X, k=knn + 1)
    bw = d[:, -1:]
    n = X.shape[0]
    K = sparse.csr_matrix((np.exp(-(d[:, 1:] / bw) ** 2).ravel(), (np.repeat(np.arange(n), knn), idx[:, 1:].ravel())), shape=(n, n))
    W = ((K + K.T) * 0.5).tocsr()
    W.setdiag(0)
    W.eliminate_zeros()
    W.sort_indices()
    return W


def blobs(n, d, centres, sigma, spread, seed):
    rng = np.random.default_rng(seed)
    mu = rng.normal(0.0, spread, (centres, d))
    return mu[rng.integers(0, centres, n)] + rng.normal(0.0, sigma, (n, d))


def swiss_roll(n, seed):
    rng = np.random.default_rng(seed)
    t = 1.5 * np.pi * (1 + 2 * rng.uniform(size=n))
    return np.c_[t * np.cos(t), 21 * rng.uniform(size=n), t * np.sin(t)]


FAMILIES = {
    "blobs_1500x10_6": lambda: blobs(1500, 10, 6, 1.0, 10.0, 1),
    "blobs_3000x20_12": lambda: blobs(3000, 20, 12, 1.0, 10.0, 2),
    "overlap_3000x10_8": lambda: blobs(3000, 10, 8, 1.2, 1.0, 3),
    "swiss_roll_3000": lambda: swiss_roll(3000, 4),
    "uniform_4000x5": lambda: np.random.default_rng(5).uniform(size=(4000, 5)),
}


def networkx_q(W, gamma, seeds=range(5)):
    import networkx as nx

    G = nx.from_scipy_sparse_array(W)
    return [nx.community.modularity(G, nx.community.louvain_communities(G, weight="weight", resolution=gamma, seed=s),
                                    weight="weight", resolution=gamma) for s in seeds]


def test_modularity_equals_networkx():
    import networkx as nx

    rng = np.random.default_rng(0)
    W = knn_graph(blobs(300, 5, 4, 1.0, 3.0, 0))
    G = nx.from_scipy_sparse_array(W)
    for gamma, L in ((1.0, 1), (1.0, 7), (0.3, 30), (2.0, 300)):
        labels = rng.integers(0, L, 300) * 3 + 5  # (any integers)
        parts = [set(np.nonzero(labels == v)[0]) for v in np.unique(labels)]
        want = nx.community.modularity(G, parts, weight="weight", resolution=gamma)
        assert abs(ref.modularity(W, labels, gamma) - want) <= 1e-12


def test_contraction_keeps_q_and_two_m():
    W = knn_graph(blobs(400, 5, 4, 1.0, 3.0, 1))
    rng = np.random.default_rng(1)
    c, L = ref.renumber(rng.integers(0, 40, 400))
    assert c[0] == 0 and np.all(np.diff(np.r_[-1, [np.nonzero(c == v)[0][0] for v in range(L)]]) > 0)  # (numbered by smallest member)
    B = ref.contract(W, c, L)
    assert abs(B - B.T).max() < 1e-15 and abs(B.sum() - W.sum()) < 1e-9
    assert abs(ref.modularity(B, np.arange(L), 0.5) - ref.modularity(W, c, 0.5)) < 1e-12


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("gamma", [1.0, 0.3])
def test_quality_against_networkx(family, gamma):
    W = knn_graph(FAMILIES[family]())
    got = ref.louvain(W, gamma)
    assert abs(got["modularity"] - ref.modularity(W, got["labels"], gamma)) < 1e-12
    qs = [lv["Q"] for lv in got["levels"]]
    assert all(b >= a for a, b in zip(qs, qs[1:]))
    theirs = networkx_q(W, gamma)
    print("louvain quality {} gamma={}: Q={:.6f} networkx min={:.6f} max={:.6f} deficit={:+.6f} levels={} rounds={}".format(
        family, gamma, got["modularity"], min(theirs), max(theirs), min(theirs) - got["modularity"], len(got["levels"]),
        [lv["rounds"] for lv in got["levels"]]))
    assert got["modularity"] >= min(theirs) - QUALITY_MARGIN


def test_edge_cases_of_the_restatement():
    empty = ref.louvain(sparse.csr_matrix((5, 5)))
    assert empty["labels"].tolist() == [0, 1, 2, 3, 4] and empty["modularity"] == 0.0 and empty["levels"] == []
    # two triangles joined by an edge, an isolated vertex in between
    e = [(0, 1), (1, 2), (0, 2), (4, 5), (5, 6), (4, 6), (2, 4)]
    W = sparse.coo_matrix((np.ones(7), tuple(zip(*e))), shape=(7, 7))
    W = (W + W.T).tocsr()
    got = ref.louvain(W)
    assert got["labels"].tolist() == [0, 0, 0, 1, 2, 2, 2]
    for fine, coarse in zip(got["level_labels"], got["level_labels"][1:]):
        assert len(set(zip(fine, coarse))) == len(set(fine))  # (nested)


def test_argument_contract_of_the_library():
    """Every bad call returns -1 with the entry's name in the message.  The addresses are host memory: nothing may touch them, and
    nothing does -- the checks come before any launch."""
    from meld_amd import _lib

    lib = _lib.get_lib()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    b = a + 256

    def refused(name, status):
        assert status == -1, name
        assert lib.meld_last_error().decode().startswith(name + ":"), lib.meld_last_error()

    assert lib.meld_louvain_lanes(100, 6400) == 16 and lib.meld_louvain_lanes(100, 6401) == 64
    assert lib.meld_louvain_move_blocks(33, 16) == 3 and lib.meld_louvain_move_blocks(33, 64) == 9 and lib.meld_louvain_move_blocks(33, 32) == 0
    move = lib.meld_louvain_move
    good = [a, a, a, 4, a, a, a, a, 8.0, 1.0, 0, 16, b, a, a, a, a, a, None]
    for i in (0, 4, 5, 6, 7, 12, 13, 14, 15, 16, 17):  # (the required pointers)
        refused("meld_louvain_move", move(*[None if j == i else v for j, v in enumerate(good)]))
    for i, v in ((3, 0), (3, 2 ** 31), (8, -1.0), (8, float("inf")), (9, 0.0), (9, float("nan")), (10, -1), (11, 32), (12, a)):
        refused("meld_louvain_move", move(*[v if j == i else w for j, w in enumerate(good)]))
    totals = lib.meld_louvain_totals
    for i in (0, 1, 4, 5, 6):
        refused("meld_louvain_totals", totals(*[None if j == i else v for j, v in enumerate([a, a, 4, 4, a, a, a, None])]))
    refused("meld_louvain_totals", totals(a, a, 0, 4, a, a, a, None))
    refused("meld_louvain_totals", totals(a, a, 4, 0, a, a, a, None))
    for i in (0, 1, 3):
        refused("meld_louvain_heads", lib.meld_louvain_heads(*[None if j == i else v for j, v in enumerate([a, a, 4, a, None])]))
    refused("meld_louvain_heads", lib.meld_louvain_heads(a, a, 0, a, None))
    for i in (0, 1, 2, 3, 5, 6):
        refused("meld_louvain_renumber", lib.meld_louvain_renumber(*[None if j == i else v for j, v in enumerate([a, a, a, a, 4, a, a, None])]))
    refused("meld_louvain_renumber", lib.meld_louvain_renumber(a, a, a, a, -1, a, a, None))
    for i in (0, 1, 3, 4):
        refused("meld_louvain_contract_keys", lib.meld_louvain_contract_keys(*[None if j == i else v for j, v in enumerate([a, a, 4, a, a, None])]))
    refused("meld_louvain_contract_keys", lib.meld_louvain_contract_keys(a, a, 0, a, a, None))
    for i in (0, 4, 5, 6):
        refused("meld_modularity_terms", lib.meld_modularity_terms(*[None if j == i else v for j, v in enumerate([a, a, a, 4, a, a, a, None])]))
    refused("meld_modularity_terms", lib.meld_modularity_terms(a, a, a, 2 ** 31, a, a, a, None))


def test_louvain_refuses_before_touching_the_device():
    """A stub with the attributes the checks read: none of these calls gets as far as a tensor."""
    from meld_amd.louvain import louvain_device, modularity

    def stub(**kw):
        return SimpleNamespace(**dict(dict(N=100, n_rows=100, comm=None), **kw))

    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", None):
        with pytest.raises(ValueError, match="resolution"):
            louvain_device(stub(), resolution=bad)
    with pytest.raises(ValueError, match="only defined for an unsharded graph"):
        louvain_device(stub(n_rows=50))
    with pytest.raises(ValueError, match="only defined for an unsharded graph"):
        modularity(stub(n_rows=50), np.zeros(100, dtype=np.int64))
    for name in ("max_rounds", "max_levels", "n_clusters"):
        with pytest.raises(ValueError, match=name):
            louvain_device(stub(), **{name: 0})
    with pytest.raises(ValueError, match="tol"):
        louvain_device(stub(), tol=-1.0)
    with pytest.raises(ValueError, match="one entry per cell"):
        modularity(stub(), np.zeros(99, dtype=np.int64))
    with pytest.raises(ValueError, match="negative"):
        modularity(stub(), np.r_[np.zeros(99, dtype=np.int64), -1])
    with pytest.raises(TypeError, match="integers"):
        modularity(stub(), np.zeros(100))
    with pytest.raises(ValueError, match="resolution"):
        modularity(stub(), np.zeros(100, dtype=np.int64), resolution=0)


def test_estimator_needs_a_fit():
    import meld_amd

    with pytest.raises(ValueError, match="must be `fit`"):
        meld_amd.MELD().louvain()


def test_louvain_kernels_do_not_spill():
    """The kernels as hipcc compiles them with the build's flags: no private memory, full occupancy (they wait on memory)."""
    from tests.test_kernel_resources import _resource_usage

    rows = _resource_usage(os.path.join(ROOT, "meld_amd", "csrc", "louvain.hip"))
    kernels = {k: v for k, v in rows.items() if ("louvain_" in k or "modularity_" in k) and "_kernel" in k}
    assert len(kernels) == 8, sorted(rows)  # (the move kernel at 16 and at 64 lanes per row)
    for name, r in kernels.items():
        assert r["ScratchSize [bytes/lane]:"] == 0, (name, r)
        if "louvain_move" in name:  # (reported: 64 VGPRs at 16 and at 64 lanes per row, 8 waves per SIMD; past 64 registers, one wave fewer)
            assert r["VGPRs:"] <= 80 and r["Occupancy [waves/SIMD]:"] >= 6, (name, r)
        else:
            assert r["VGPRs:"] <= 64 and r["Occupancy [waves/SIMD]:"] == 8, (name, r)
