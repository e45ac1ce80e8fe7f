"""Leiden communities on the device (meld_amd/leiden.py, csrc/leiden.hip) against the host restatement (tests/leiden_reference.py),
on the graphs of tests/test_gpu_louvain.py: rows shorter than a lane group, longer than a wave, longer than many LDS tiles, rows
without entries, a stored diagonal, one vertex.  Weights are small integers and the resolutions dyadic, so every sum and every score
is exact whatever the order: proposals, labels, counts and modularities must be EQUAL.  Real weights (kNN kernels built by
``MELD.fit``) are held to the definitions to 1e-12, to networkx's quality within the margin of DESIGN.md section 4.17, and to the
point of the rule: every community induces a connected subgraph."""
import numpy as np
import pytest
import torch
from scipy import sparse

from tests import leiden_reference as ref
from tests import louvain_reference as lref
from tests.test_gpu_louvain import GAMMAS, ROUND_GRAPHS, _MAKERS, _dev, _fit, _graph, _six_groups
from tests.test_leiden_host import assert_every_community_is_connected
from tests.test_louvain_host import QUALITY_MARGIN, blobs, networkx_q

pytestmark = pytest.mark.gpu

_PARTS = {}


def _move_partition(name, gamma):
    """The restatement's move partition of level 0 (numbered by smallest member), made once."""
    if (name, gamma) not in _PARTS:
        W = _graph(name)
        two_m = float(lref.degrees(W).sum())
        c = ref.run_level(W, gamma, two_m)[0] if two_m > 0 else np.arange(W.shape[0])
        _PARTS[name, gamma] = lref.renumber(c)[0]
    return _PARTS[name, gamma]


def _device_round(W, P, sub, gamma, rnd, lanes):
    """One refinement round on the device: ``(new sub, proposals, movers)`` as numpy / int."""
    from meld_amd import louvain as lv
    from meld_amd._lib import check, get_lib, ptr

    n = W.shape[0]
    k = lref.degrees(W)
    two_m = float(k.sum())
    lib, st = get_lib(), torch.cuda.current_stream().cuda_stream
    rowptr, col, val = _dev(W)
    ar = torch.arange(n, dtype=torch.int64, device="cuda")
    kd = torch.from_numpy(k).cuda()
    Pd, subd = torch.from_numpy(P.astype(np.int32)).cuda(), torch.from_numpy(sub.astype(np.int32)).cuda()
    tot_comm, _, _ = lv._totals(lib, st, Pd, kd, ar)
    tot, size, _ = lv._totals(lib, st, subd, kd, ar)
    prop = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    new = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    part = torch.empty(lib.meld_leiden_commit_blocks(n), dtype=torch.int32, device="cuda")
    movers = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    check(lib.meld_leiden_propose(ptr(rowptr), ptr(col), ptr(val), n, ptr(Pd), ptr(subd), ptr(kd), ptr(tot), ptr(size), ptr(tot_comm), two_m,
                                  gamma, rnd, lanes, ptr(prop), st), "meld_leiden_propose")
    check(lib.meld_leiden_commit(ptr(subd), ptr(prop), ptr(size), n, ptr(new), ptr(part), ptr(movers), st), "meld_leiden_commit")
    return new.cpu().numpy(), prop.cpu().numpy(), int(movers.item())


@pytest.mark.parametrize("rnd", [0, 2])
@pytest.mark.parametrize("name", ROUND_GRAPHS)
def test_one_refinement_round_equals_the_restatement(name, rnd):
    """Round 0 from singletons, round 2 from the restatement's state after two rounds."""
    W = _graph(name)
    n = W.shape[0]
    k = lref.degrees(W)
    two_m = float(k.sum())
    for gamma in GAMMAS:
        P = _move_partition(name, gamma)
        sub = np.arange(n, dtype=np.int64)
        for r in range(rnd):
            sub = ref.refine_round(W, P, sub, k, two_m, gamma, r)[0]
        w_new, w_prop, w_movers = ref.refine_round(W, P, sub, k, two_m, gamma, rnd)
        if rnd == 0 and name.startswith(("hub", "regular", "isolated", "one_label", "level1")):
            assert w_movers > 0  # (the case exercises moves)
        if rnd == 2 and n > 1:
            assert (np.bincount(sub, minlength=n)[sub] > 1).any()  # (rows that leave before any gather)
        for lanes in (16, 64):
            new, prop, movers = _device_round(W, P, sub, gamma, rnd, lanes)
            what = (name, rnd, gamma, lanes)
            assert np.array_equal(prop, w_prop), what
            assert np.array_equal(new, w_new), what
            assert movers == w_movers, what


def test_a_row_whose_neighbours_lie_in_other_communities_stays():
    """Vertex 7 of the random graph is made a community of its own (a label no other vertex carries): every entry of its row
    lies outside, it proposes nothing and nobody may join it."""
    W = _graph("regular_4097")
    n = W.shape[0]
    k = lref.degrees(W)
    P = _move_partition("regular_4097", 1.0).copy()
    v = 7
    assert W.indptr[v + 1] > W.indptr[v]
    P[v] = P.max() + 1
    sub = np.arange(n, dtype=np.int64)
    w_new, w_prop, w_movers = ref.refine_round(W, P, sub, k, float(k.sum()), 1.0, 0)
    assert w_prop[v] == -1 and w_new[v] == v and not (w_prop == v).any() and w_movers > 0
    for lanes in (16, 64):
        new, prop, movers = _device_round(W, P, sub, 1.0, 0, lanes)
        assert np.array_equal(prop, w_prop) and np.array_equal(new, w_new) and movers == w_movers, lanes


def _hub_outside_its_community():
    """``(W, P, k)``: hub_300 with everyone in one community, except the hub's neighbours beyond its first three, each alone."""
    W = _graph("hub_300")
    hub = 4096
    nbrs = W.indices[W.indptr[hub] : W.indptr[hub + 1]]
    P = np.zeros(W.shape[0], dtype=np.int64)
    P[nbrs[3:]] = 1 + np.arange(nbrs.shape[0] - 3)
    return W, lref.renumber(P)[0], lref.degrees(W)


def test_a_long_row_that_is_not_well_connected_leaves_after_its_first_chunk():
    """The hub's row of 300 entries takes five chunks at 16 lanes per row and two at 64; three of its entries lie in its community,
    which is far too little for its degree: the row meets all its entries with the first chunk, proposes nothing and scores
    nothing, while the rest of the graph moves."""
    W, P, k = _hub_outside_its_community()
    n, hub, gamma = W.shape[0], 4096, 1.0
    two_m = float(k.sum())
    lo, hi = W.indptr[hub], W.indptr[hub + 1]
    cols, vals = W.indices[lo:hi], W.data[lo:hi]
    inside = (P[cols] == P[hub]) & (cols != hub)
    in_c = float(vals[inside].sum())
    tot_c = float(k[P == P[hub]].sum())
    assert hi - lo > 256  # (more than one chunk at 64 lanes per row, more than four at 16)
    assert in_c > 0 and in_c * two_m < gamma * k[hub] * (tot_c - k[hub])
    sub = np.arange(n, dtype=np.int64)
    w_new, w_prop, w_movers = ref.refine_round(W, P, sub, k, two_m, gamma, 0)
    assert w_prop[hub] == -1 and w_movers > 0
    for lanes in (16, 64):
        new, prop, movers = _device_round(W, P, sub, gamma, 0, lanes)
        assert np.array_equal(prop, w_prop) and np.array_equal(new, w_new) and movers == w_movers, lanes


def _assert_record_equals(rec, want, what):
    assert rec.labels.dtype == np.int32 and np.array_equal(rec.labels, want["labels"]), what
    assert rec.levels == want["levels"], (what, rec.levels, want["levels"])
    assert rec.modularity == want["modularity"], what
    assert rec.n_communities == len(set(want["labels"])) and np.array_equal(rec.sizes, np.bincount(want["labels"])), what
    assert np.array_equal(rec.labels_device.cpu().numpy(), rec.labels)
    assert len(want["level_labels"]) == len(rec.levels)
    for l, lab in enumerate(want["level_labels"]):
        assert np.array_equal(rec.level_labels(l), lab), (what, l)
    for l in range(len(rec.levels) - 1):  # nested: a community of level l lies in one community of level l + 1
        fine, coarse = rec.level_labels(l), rec.level_labels(l + 1)
        assert np.unique(np.c_[fine, coarse], axis=0).shape[0] == np.unique(fine).shape[0], (what, l)
    firsts = np.unique(rec.labels, return_index=True)[1]  # numbered by smallest cell
    assert np.all(np.diff(firsts) > 0)


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("name", sorted(_MAKERS))
def test_whole_run_equals_the_restatement(name, gamma):
    from meld_amd.graph import DeviceGraph
    from meld_amd.leiden import LeidenRecord

    W = _graph(name)
    G = DeviceGraph.from_scipy(W)
    want = ref.leiden(W, gamma)
    rec = G.leiden(resolution=gamma)
    assert isinstance(rec, LeidenRecord) and rec.resolution == gamma
    print(name, gamma, "levels", [(lv["vertices"], lv["communities"], lv["subcommunities"], lv["rounds"], lv["refine_rounds"]) for lv in rec.levels],
          "Q", rec.modularity)
    _assert_record_equals(rec, want, (name, gamma))
    assert G.modularity(rec.labels, gamma) == pytest.approx(rec.modularity, abs=1e-12)
    assert_every_community_is_connected(W, rec.labels)
    if name == "ring_of_cliques":
        assert rec.n_communities <= 32 and all(len(set(rec.labels[q * 6:(q + 1) * 6])) == 1 for q in range(32))  # (no clique is split)


@pytest.mark.parametrize("name,gamma,louvain_leaves", [("regular_4097", 2.0, 5), ("hub_4500", 2.0, 8)])
def test_louvain_leaves_disconnected_communities_and_leiden_none(name, gamma, louvain_leaves):
    from meld_amd.graph import DeviceGraph

    W = _graph(name)
    G = DeviceGraph.from_scipy(W)
    assert ref.disconnected_communities(W, G.louvain(resolution=gamma).labels) == louvain_leaves >= 1
    assert ref.disconnected_communities(W, G.leiden(resolution=gamma).labels) == 0


def test_a_run_cut_by_max_levels_returns_the_move_partition():
    from meld_amd.graph import DeviceGraph

    W = _graph("hub_70")
    _assert_record_equals(DeviceGraph.from_scipy(W).leiden(max_levels=2), ref.leiden(W, 1.0, max_levels=2), "cut")


@pytest.mark.parametrize("name", ["hub_300", "isolated_and_pairs", "level1_diagonal"])
def test_the_device_order_does_not_matter(name):
    """The same graph stored in another order, with the permutation that says so: the same record, bit for bit."""
    from meld_amd.graph import DeviceGraph

    W = _graph(name)
    p = np.random.default_rng(3).permutation(W.shape[0])
    G = DeviceGraph.from_scipy(W[p][:, p])
    G.perm = torch.from_numpy(p).cuda()
    assert abs(G.W - W).max() == 0
    _assert_record_equals(G.leiden(), ref.leiden(W, 1.0), name)


FAMILIES = {
    "blobs_3000x10": lambda: blobs(3000, 10, 6, 1.0, 10.0, 1),
    "uniform_4000x5": lambda: np.random.default_rng(5).uniform(size=(4000, 5)),
    "overlap_3000x10_8": lambda: blobs(3000, 10, 8, 1.2, 1.0, 3),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_real_weights(family):
    G = _fit(FAMILIES[family]()).graph
    W = G.W
    rec = G.leiden()
    assert abs(rec.modularity - G.modularity(rec.labels)) <= 1e-12
    assert abs(rec.modularity - lref.modularity(W, rec.labels)) <= 1e-12
    theirs = networkx_q(W, 1.0)
    print(family, "Q", rec.modularity, "louvain", G.louvain().modularity, "networkx", min(theirs), max(theirs), "levels",
          [(lv["vertices"], lv["communities"], lv["subcommunities"], lv["rounds"], lv["refine_rounds"]) for lv in rec.levels])
    assert rec.modularity >= min(theirs) - QUALITY_MARGIN
    assert_every_community_is_connected(W, rec.labels)
    again = G.leiden(recompute=True)
    assert again is not rec and np.array_equal(again.labels, rec.labels) and again.modularity == rec.modularity and again.levels == rec.levels
    assert all(np.array_equal(again.level_labels(l), rec.level_labels(l)) for l in range(len(rec.levels)))
    assert G.leiden() is again  # (kept on the graph)


def test_locality_reordering_does_not_change_the_communities():
    """A graph large enough to be built in locality order, and the same cells built as given: the same communities."""
    import meld_amd

    X = torch.from_numpy(blobs(9000, 5, 8, 1.0, 3.0, 7)).cuda()
    A = meld_amd.build_knn_graph(X, knn=7, reorder=True)
    B = meld_amd.build_knn_graph(X, knn=7, reorder=False)
    assert A.perm is not None and B.perm is None
    ra, rb = A.leiden(), B.leiden()
    assert np.array_equal(ra.labels, rb.labels) and abs(ra.modularity - rb.modularity) <= 1e-12
    assert [(lv["vertices"], lv["communities"], lv["subcommunities"]) for lv in ra.levels] == [(lv["vertices"], lv["communities"], lv["subcommunities"]) for lv in rb.levels]


def test_n_clusters():
    from meld_amd.graph import DeviceGraph

    G = DeviceGraph.from_scipy(_six_groups(np.random.default_rng(0)))
    assert G.leiden(resolution=0.01).n_communities == 1  # (the bisection has work to do)
    rec = G.leiden(n_clusters=6)
    assert rec.n_communities == 6 and np.array_equal(rec.labels, np.repeat(np.arange(6), 40))
    assert 0.01 <= rec.resolution <= 10 and rec.sizes.tolist() == [40] * 6
    apart = DeviceGraph.from_scipy(_six_groups(np.random.default_rng(0), joined=False))
    with pytest.raises(ValueError, match="r_start is too large. Got: 0.01"):
        apart.leiden(n_clusters=3)
    with pytest.raises(ValueError, match="r_stop is too small. Got: 10"):
        apart.leiden(n_clusters=241)


def test_estimator_returns_a_series_on_the_cells_index():
    import pandas as pd

    X = pd.DataFrame(blobs(600, 5, 6, 1.0, 10.0, 2), index=["cell{}".format(i) for i in range(600)])
    op = _fit(X)
    s = op.leiden(resolution=0.5)
    assert isinstance(s, pd.Series) and s.name == "leiden" and list(s.index) == list(X.index)
    assert np.array_equal(s.to_numpy(), op.graph.leiden(resolution=0.5).labels)


def test_subgraph_row_shard_and_no_entries():
    from meld_amd.graph import DeviceGraph

    W = _graph("hub_300")
    G = DeviceGraph.from_scipy(W)
    ind = np.random.default_rng(5).permutation(W.shape[0])[:3000]  # (not ascending: the subgraph carries a permutation)
    sub = G.subgraph(ind)
    assert sub.perm is not None
    Ws = sub.W
    assert abs(Ws - W[ind][:, ind]).max() == 0
    _assert_record_equals(sub.leiden(resolution=0.5), ref.leiden(Ws, 0.5), "subgraph")
    shard = DeviceGraph(G.rowptr[:101].clone(), G.col, G.val, G.dw_dev[:100].clone(), n_total=G.N)
    with pytest.raises(ValueError, match="only defined for an unsharded graph"):
        shard.leiden()
    empty = DeviceGraph.from_scipy(sparse.csr_matrix((5, 5)))
    rec = empty.leiden()
    assert rec.labels.tolist() == [0, 1, 2, 3, 4] and rec.modularity == 0.0 and rec.n_communities == 5 and rec.sizes.tolist() == [1] * 5
    assert rec.levels == []
    with pytest.raises(ValueError, match="resolution"):
        G.leiden(resolution=0.0)
