"""Leiden without a device: the host restatement (tests/leiden_reference.py) -- its invariants on the Louvain test graphs and on five
families of kNN graphs, the communities Louvain leaves disconnected and Leiden does not, its modularity against networkx --, the
argument contract of the C entries of csrc/leiden.hip (every refusal comes before any launch), the argument checks of
``meld_amd.leiden`` that raise before anything touches the device, and what hipcc reports for the kernels (no private memory)."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
from scipy.sparse.csgraph import connected_components

from tests import leiden_reference as ref
from tests import louvain_reference as lref
from tests.test_gpu_louvain import _MAKERS, _graph
from tests.test_louvain_host import FAMILIES, QUALITY_MARGIN, knn_graph, networkx_q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_RUNS = {}


def _family_graph(family):
    if ("W", family) not in _RUNS:
        _RUNS["W", family] = knn_graph(FAMILIES[family]())
    return _RUNS["W", family]


def _weights(name):
    return _family_graph(name) if name in FAMILIES else _graph(name)


def _run(name, gamma):
    """The restatement's run on a graph of the two collections, made once (``refine`` asserts its invariants as it goes)."""
    if (name, gamma) not in _RUNS:
        _RUNS[name, gamma] = ref.leiden(_weights(name), gamma)
    return _RUNS[name, gamma]


def _nested(fine, coarse):
    return np.unique(np.c_[fine, coarse], axis=0).shape[0] == np.unique(fine).shape[0]


def assert_every_community_is_connected(W, labels):
    W = lref.csr(W)
    for c in np.unique(labels):
        idx = np.nonzero(labels == c)[0]
        assert connected_components(W[idx][:, idx], directed=False)[0] == 1, (c, idx[:10])


CASES = [(name, gamma) for name in sorted(_MAKERS) for gamma in (1.0, 0.5, 2.0)] + [(f, gamma) for f in sorted(FAMILIES) for gamma in (1.0, 0.3)]


@pytest.mark.parametrize("name,gamma", CASES)
def test_invariants_of_the_restatement(name, gamma):
    W = _weights(name)
    got = _run(name, gamma)
    for P, sub in got["level_parts"]:
        assert _nested(sub, P)  # every sub-community lies in one community of the move partition
    labels = got["labels"]
    assert labels.shape[0] == W.shape[0]
    assert_every_community_is_connected(W, labels)
    assert np.all(np.diff(np.unique(labels, return_index=True)[1]) > 0) and labels.max() + 1 == np.unique(labels).shape[0]  # by smallest cell
    assert np.array_equal(got["level_labels"][-1], labels) if got["levels"] else got["level_labels"] == []
    for fine, coarse in zip(got["level_labels"], got["level_labels"][1:]):
        assert _nested(fine, coarse)
    assert abs(got["modularity"] - lref.modularity(W, labels, gamma)) < 1e-12
    for lv in got["levels"]:
        assert lv["vertices"] >= lv["subcommunities"] >= lv["communities"] >= 1
    assert [lv["vertices"] for lv in got["levels"][1:]] == [lv["subcommunities"] for lv in got["levels"][:-1]]


def test_priority_is_a_bijection_per_round():
    ids = np.arange(1 << 16)
    for rnd in (0, 1, 7):
        p = ref.pri(ids, rnd)
        assert p.max() < 2 ** 32 and np.unique(p).shape[0] == ids.shape[0]
    assert int(ref.pri(np.array([5]), 2)[0]) != int(ref.pri(np.array([5]), 3)[0])


@pytest.mark.parametrize("name,gamma,louvain_leaves", [("regular_4097", 2.0, 5), ("hub_4500", 2.0, 8), ("overlap_3000x10_8", 1.0, 1)])
def test_louvain_leaves_disconnected_communities_and_leiden_none(name, gamma, louvain_leaves):
    W = _weights(name)
    theirs = lref.louvain(W, gamma)["labels"]
    assert ref.disconnected_communities(W, theirs) == louvain_leaves >= 1
    assert ref.disconnected_communities(W, _run(name, gamma)["labels"]) == 0


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("gamma", [1.0, 0.3])
def test_quality_against_networkx(family, gamma):
    W = _family_graph(family)
    got = _run(family, gamma)
    louvain_q = lref.louvain(W, gamma)["modularity"]
    theirs = networkx_q(W, gamma)
    print("leiden quality {} gamma={}: Q={:.6f} louvain restatement={:.6f} ({:+.6f}) networkx min={:.6f} max={:.6f} communities={} "
          "rounds={} refine rounds={}".format(family, gamma, got["modularity"], louvain_q, got["modularity"] - louvain_q, min(theirs),
                                              max(theirs), len(set(got["labels"])), [lv["rounds"] for lv in got["levels"]],
                                              [lv["refine_rounds"] for lv in got["levels"]]))
    assert got["modularity"] >= min(theirs) - QUALITY_MARGIN


def test_edge_cases_of_the_restatement():
    from scipy import sparse

    empty = ref.leiden(sparse.csr_matrix((5, 5)))
    assert empty["labels"].tolist() == [0, 1, 2, 3, 4] and empty["modularity"] == 0.0 and empty["levels"] == []
    e = [(0, 1), (1, 2), (0, 2), (4, 5), (5, 6), (4, 6), (2, 4)]  # two triangles joined by an edge, an isolated vertex in between
    W = sparse.coo_matrix((np.ones(7), tuple(zip(*e))), shape=(7, 7))
    W = (W + W.T).tocsr()
    got = ref.leiden(W)
    assert got["labels"].tolist() == [0, 0, 0, 1, 2, 2, 2]
    # a run cut after one level returns that level's move partition, as Louvain does
    big = _graph("regular_4097")
    cut = ref.leiden(big, 1.0, max_levels=1)
    P, L = lref.renumber(ref.run_level(lref.csr(big), 1.0, float(big.sum()))[0])
    assert len(cut["levels"]) == 1 and np.array_equal(cut["labels"], P) and cut["levels"][0]["communities"] == L


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

    assert lib.meld_leiden_commit_blocks(0) == 0 and lib.meld_leiden_commit_blocks(256) == 1 and lib.meld_leiden_commit_blocks(257) == 2
    propose = lib.meld_leiden_propose
    #       rowptr col val n  comm sub k  tot size tot_comm two_m gamma round lanes prop stream
    good = [a, a, a, 4, a, a + 64, a, a, a + 128, a, 8.0, 1.0, 0, 16, b, None]
    for i in (0, 4, 5, 6, 7, 8, 9, 14):  # (the required pointers)
        refused("meld_leiden_propose", propose(*[None if j == i else v for j, v in enumerate(good)]))
    for i, v in ((3, 0), (3, 2 ** 31), (10, -1.0), (10, float("inf")), (11, 0.0), (11, float("nan")), (11, float("inf")), (12, -1), (13, 32),
                 (14, a), (14, a + 64), (14, a + 128)):
        refused("meld_leiden_propose", propose(*[v if j == i else w for j, w in enumerate(good)]))
    commit = lib.meld_leiden_commit
    #       sub prop size n new_sub part_moved movers stream
    good = [a, a + 64, a + 128, 4, b, a, a, None]
    for i in (0, 1, 2, 4, 5, 6):
        refused("meld_leiden_commit", commit(*[None if j == i else v for j, v in enumerate(good)]))
    for i, v in ((3, 0), (3, 2 ** 31), (4, a), (4, a + 64), (4, a + 128)):
        refused("meld_leiden_commit", commit(*[v if j == i else w for j, w in enumerate(good)]))
    assert not any(buf)  # (nothing was written)


def test_leiden_refuses_before_touching_the_device():
    """A stub with the attributes the checks read: none of these calls gets as far as a tensor."""
    from meld_amd.leiden import leiden_device

    def stub(**kw):
        return SimpleNamespace(**dict(dict(N=100, n_rows=100, comm=None), **kw))

    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", None):
        with pytest.raises(ValueError, match="resolution"):
            leiden_device(stub(), resolution=bad)
    with pytest.raises(ValueError, match="only defined for an unsharded graph"):
        leiden_device(stub(n_rows=50))
    for name in ("max_rounds", "max_levels", "n_clusters"):
        with pytest.raises(ValueError, match=name):
            leiden_device(stub(), **{name: 0})
    with pytest.raises(ValueError, match="tol"):
        leiden_device(stub(), tol=-1.0)


def test_estimator_needs_a_fit():
    import meld_amd

    with pytest.raises(ValueError, match="must be `fit`"):
        meld_amd.MELD().leiden()
    assert "LeidenRecord" in meld_amd.__all__


def test_leiden_kernels_do_not_spill():
    """The kernels as hipcc compiles them with the build's flags: no private memory."""
    from tests.test_kernel_resources import _resource_usage

    rows = _resource_usage(os.path.join(ROOT, "meld_amd", "csrc", "leiden.hip"))
    kernels = {k: v for k, v in rows.items() if "leiden_" in k and "_kernel" in k}
    assert len(kernels) == 4, sorted(rows)  # (the propose kernel at 16 and at 64 lanes per row, commit, count)
    for name, r in kernels.items():
        assert r["ScratchSize [bytes/lane]:"] == 0, (name, r)
        if "leiden_propose" in name:
            # reported: 68 VGPRs at 16 lanes per row, 70 at 64, 7 waves per SIMD both (four entries per lane with their sums: the
            # row pass of label_rows.hpp in its LOCAL form; up to 72 registers keep the seventh wave)
            assert r["VGPRs:"] <= 72 and r["Occupancy [waves/SIMD]:"] >= 7, (name, r)
        else:  # reported: 8 (commit) and 10 (count) VGPRs, 8 waves per SIMD
            assert r["VGPRs:"] <= 16 and r["Occupancy [waves/SIMD]:"] == 8, (name, r)
