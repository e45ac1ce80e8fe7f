"""Louvain communities on the device (meld_amd/louvain.py, csrc/louvain.hip) against the host restatement
(tests/louvain_reference.py).  The shapes are those at which the kernels can go wrong, not workload sizes: rows shorter than a lane
group, longer than a wave, longer than many LDS tiles, rows without entries, a stored diagonal, one vertex.  Weights are small
integers and the resolutions dyadic, so every sum and every score is exact whatever the order: labels, weights, counts and
modularities must be EQUAL.  Real weights (kNN kernels built by ``MELD.fit``) are held to the definitions to 1e-12 and to networkx's
quality within the margin measured for the rule in DESIGN.md section 4.17."""
import numpy as np
import pytest
import torch
from scipy import sparse
from scipy.sparse.csgraph import connected_components

from tests import louvain_reference as ref
from tests.test_louvain_host import QUALITY_MARGIN, blobs, networkx_q

pytestmark = pytest.mark.gpu

GAMMAS = (1.0, 0.5, 2.0)


def _sym(a, b, w, n):
    W = sparse.coo_matrix((w, (a, b)), shape=(n, n)).tocsr()
    W = sparse.triu(W + W.T, k=1)  # (one weight per pair)
    return ref.csr(W + W.T)


def _regular(n, rng, fan=3):
    a = np.repeat(np.arange(n), fan)
    b = rng.integers(0, n, a.shape[0])
    keep = a != b
    return _sym(a[keep], b[keep], rng.integers(1, 8, keep.sum()).astype(np.float64), n)


def _with_hub(W, hub, entries, rng):
    n = W.shape[0]
    others = rng.permutation(np.r_[0:hub, hub + 1:n])[:entries]
    H = _sym(np.full(entries, hub), others, rng.integers(1, 8, entries).astype(np.float64), n)
    W = W.tolil()
    W[hub, :] = 0
    W[:, hub] = 0
    out = ref.csr(W.tocsr() + H)
    out.eliminate_zeros()
    assert out.indptr[hub + 1] - out.indptr[hub] == entries
    return out


def _mixture(rng):
    """4,097 vertices in random numbering: 500 without entries, 250 disjoint pairs, the rest a random graph."""
    n = 4097
    ids = rng.permutation(n)
    core = ids[1000:]
    R = _regular(core.shape[0], rng).tocoo()
    pairs = ids[500:1000].reshape(250, 2)
    a = np.r_[core[R.row], pairs[:, 0], pairs[:, 1]]
    b = np.r_[core[R.col], pairs[:, 1], pairs[:, 0]]
    pw = rng.integers(1, 8, 250).astype(np.float64)
    W = ref.csr(sparse.coo_matrix((np.r_[R.data, pw, pw], (a, b)), shape=(n, n)))
    assert (np.diff(W.indptr) == 0).sum() >= 500 and abs(W - W.T).max() == 0
    return W


def _ring_of_cliques(cliques=32, size=6):
    n = cliques * size
    a, b = [], []
    for q in range(cliques):
        for i in range(size):
            for j in range(i + 1, size):
                a.append(q * size + i)
                b.append(q * size + j)
        a.append(q * size + size - 1)
        b.append(((q + 1) % cliques) * size)
    return _sym(np.array(a), np.array(b), np.ones(len(a)), n)


def _level1(rng):
    """A contracted graph: 128 vertices, rows of about 120 entries, the communities' inner weights on the diagonal."""
    W = _regular(4097, rng)
    c, L = ref.renumber(rng.integers(0, 128, 4097))
    B = ref.contract(W, c, L)
    assert B.diagonal().sum() > 0 and B.nnz > 64 * L  # (the 64-lane kernel is the one a run chooses)
    return B


_GRAPHS = {}


def _graph(name):
    """The graphs of this file, made once (fixed seeds) and never changed."""
    if name not in _GRAPHS:
        rng = np.random.default_rng(sorted(_MAKERS).index(name))
        _GRAPHS[name] = _MAKERS[name](rng)
    return _GRAPHS[name]


_MAKERS = {
    "regular_4097": lambda rng: _regular(4097, rng),
    "hub_70": lambda rng: _with_hub(_regular(4097, rng), 17, 70, rng),
    "hub_300": lambda rng: _with_hub(_regular(4097, rng), 4096, 300, rng),
    "hub_4500": lambda rng: _with_hub(_regular(5003, rng), 2500, 4500, rng),  # (4,500 entries need more than 4,097 vertices)
    "isolated_and_pairs": _mixture,
    "one_label_row": lambda rng: _with_hub(_regular(4097, rng), 5, 100, rng),
    "level1_diagonal": _level1,
    "one_vertex": lambda rng: sparse.csr_matrix((1, 1)),
    "one_vertex_diagonal": lambda rng: sparse.csr_matrix(np.array([[3.0]])),
    "ring_of_cliques": lambda rng: _ring_of_cliques(),
}
ROUND_GRAPHS = [g for g in sorted(_MAKERS) if g != "ring_of_cliques"]


def _start(W, name, start):
    n = W.shape[0]
    if start == "identity":
        return np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(11)
    c = rng.integers(0, max(n // 8, 1), n)
    if name == "one_label_row":  # every entry of row 5 carries label 9 (and row 5 another one)
        c[W.indices[W.indptr[5]:W.indptr[6]]] = 9
        c[5] = 3
    return c


def _dev(W):
    return (torch.from_numpy(W.indptr.astype(np.int64)).cuda(), torch.from_numpy(W.indices.astype(np.int32)).cuda(),
            torch.from_numpy(W.data.astype(np.float64)).cuda())


@pytest.mark.parametrize("start", ["identity", "random"])
@pytest.mark.parametrize("name", ROUND_GRAPHS)
def test_one_round_equals_the_restatement(name, start):
    from meld_amd import louvain as lv
    from meld_amd._lib import check, get_lib, ptr

    W = _graph(name)
    n = W.shape[0]
    c = _start(W, name, start)
    k = ref.degrees(W)
    two_m = float(k.sum())
    lib, st = get_lib(), torch.cuda.current_stream().cuda_stream
    rowptr, col, val = _dev(W)
    kd, cd = torch.from_numpy(k).cuda(), torch.from_numpy(c.astype(np.int32)).cuda()
    tot, size, minm = lv._totals(lib, st, cd, kd, torch.arange(n, dtype=torch.int64, device="cuda"))
    present, first = np.unique(c, return_index=True)
    assert np.array_equal(tot.cpu().numpy(), np.bincount(c, weights=k, minlength=n))
    assert np.array_equal(size.cpu().numpy(), np.bincount(c, minlength=n))
    want_min = np.full(n, -1)
    want_min[present] = first
    assert np.array_equal(minm.cpu().numpy(), want_min)
    s_tot2 = float((tot * tot).sum().item())
    if name == "one_label_row" and start == "random":
        assert set(c[W.indices[W.indptr[5]:W.indptr[6]]]) == {9}
    for lanes in (16, 64):
        blocks = lib.meld_louvain_move_blocks(n, lanes)
        for gamma, rnd in zip(GAMMAS, (0, 1, 2)):
            new, own, moved = (torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((n,), -7.0, dtype=torch.float64, device="cuda"),
                               torch.full((n,), -7, dtype=torch.int32, device="cuda"))
            part_sum = torch.empty(blocks, dtype=torch.float64, device="cuda")
            part_moved = torch.empty(blocks, dtype=torch.int32, device="cuda")
            stats = torch.empty(2, dtype=torch.float64, device="cuda")
            check(lib.meld_louvain_move(ptr(rowptr), ptr(col), ptr(val), n, ptr(cd), ptr(kd), ptr(tot), ptr(size), two_m, gamma, rnd, lanes,
                                        ptr(new), ptr(own), ptr(moved), ptr(part_sum), ptr(part_moved), ptr(stats), st), "meld_louvain_move")
            w_new, w_own, w_moved = ref.move_round(W, c, k, two_m, gamma, rnd)
            what = (name, start, lanes, gamma, rnd)
            assert np.array_equal(new.cpu().numpy(), w_new), what
            assert np.array_equal(own.cpu().numpy(), w_own), what
            assert np.array_equal(moved.cpu().numpy(), w_moved.astype(np.int32)), what
            s_in, movers = stats.tolist()
            assert movers == w_moved.sum() and s_in == w_own.sum(), what
            tot_ref = np.bincount(c, weights=k, minlength=n)
            assert lv.q_value(s_in, s_tot2, two_m, gamma) == ref.q_value(w_own.sum(), (tot_ref * tot_ref).sum(), two_m, gamma), what
            if n > 1 and start == "identity":
                assert w_moved.sum() > 0 or not W.nnz, what  # (the case exercises moves)


def _assert_record_equals(rec, want, what):
    assert rec.labels.dtype == np.int32 and np.array_equal(rec.labels, want["labels"]), what
    assert rec.levels == want["levels"], (what, rec.levels, want["levels"])
    assert rec.modularity == want["modularity"], what
    assert rec.n_communities == len(set(want["labels"])) and np.array_equal(rec.sizes, np.bincount(want["labels"])), what
    assert np.array_equal(rec.labels_device.cpu().numpy(), rec.labels)
    for l, lab in enumerate(want["level_labels"]):
        assert np.array_equal(rec.level_labels(l), lab), (what, l)
    for l in range(len(rec.levels) - 1):  # nested: a community of level l lies in one community of level l + 1
        fine, coarse = rec.level_labels(l), rec.level_labels(l + 1)
        assert np.unique(np.c_[fine, coarse], axis=0).shape[0] == np.unique(fine).shape[0], (what, l)
    # numbered by smallest cell
    firsts = np.unique(rec.labels, return_index=True)[1]
    assert np.all(np.diff(firsts) > 0)


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("name", sorted(_MAKERS))
def test_whole_run_equals_the_restatement(name, gamma):
    from meld_amd.graph import DeviceGraph

    W = _graph(name)
    G = DeviceGraph.from_scipy(W)
    want = ref.louvain(W, gamma)
    rec = G.louvain(resolution=gamma)
    print(name, gamma, "levels", [(lv["vertices"], lv["communities"], lv["rounds"]) for lv in rec.levels], "Q", rec.modularity)
    _assert_record_equals(rec, want, (name, gamma))
    assert G.modularity(rec.labels, gamma) == pytest.approx(rec.modularity, abs=1e-12)
    if name == "ring_of_cliques":
        assert rec.n_communities <= 32 and all(len(set(rec.labels[q * 6:(q + 1) * 6])) == 1 for q in range(32))  # (no clique is split)


@pytest.mark.parametrize("name", ["hub_300", "isolated_and_pairs", "level1_diagonal"])
def test_the_device_order_does_not_matter(name):
    """The same graph stored in another order, with the permutation that says so: the same record, bit for bit."""
    from meld_amd.graph import DeviceGraph

    W = _graph(name)
    n = W.shape[0]
    p = np.random.default_rng(3).permutation(n)
    G = DeviceGraph.from_scipy(W[p][:, p])
    G.perm = torch.from_numpy(p).cuda()
    assert abs(G.W - W).max() == 0
    want = ref.louvain(W, 1.0)
    _assert_record_equals(G.louvain(), want, name)
    labels = np.random.default_rng(4).integers(0, 50, n) * 7
    assert G.modularity(labels, 0.5) == ref.modularity(W, labels, 0.5) == DeviceGraph.from_scipy(W).modularity(torch.from_numpy(labels).cuda(), 0.5)


def _fit(X, **kw):
    import meld_amd

    return meld_amd.MELD(knn=7, verbose=False, **kw).fit(X)


@pytest.mark.parametrize("family", ["blobs_3000x10", "uniform_4000x5"])
def test_real_weights(family):
    X = blobs(3000, 10, 6, 1.0, 10.0, 1) if family == "blobs_3000x10" else np.random.default_rng(5).uniform(size=(4000, 5))
    G = _fit(X).graph
    W = G.W
    rec = G.louvain()
    assert abs(rec.modularity - G.modularity(rec.labels)) <= 1e-12
    assert abs(rec.modularity - ref.modularity(W, rec.labels)) <= 1e-12
    qs = [lv["Q"] for lv in rec.levels]
    assert all(b >= a for a, b in zip(qs, qs[1:])), qs
    theirs = networkx_q(W, 1.0)
    print(family, "Q", rec.modularity, "networkx", min(theirs), max(theirs), "levels", [(lv["vertices"], lv["rounds"]) for lv in rec.levels])
    assert rec.modularity >= min(theirs) - QUALITY_MARGIN
    _, comp = connected_components(W, directed=False)
    assert np.unique(np.c_[rec.labels, comp], axis=0).shape[0] == rec.n_communities  # (no community spans two components)
    again = G.louvain(recompute=True)
    assert again is not rec and np.array_equal(again.labels, rec.labels) and again.modularity == rec.modularity and again.levels == rec.levels
    assert G.louvain() is again  # (kept on the graph)


def test_locality_reordering_does_not_change_the_communities():
    """A graph large enough to be built in locality order, and the same cells built as given: the same communities."""
    import meld_amd

    X = torch.from_numpy(blobs(9000, 5, 8, 1.0, 3.0, 7)).cuda()
    A = meld_amd.build_knn_graph(X, knn=7, reorder=True)
    B = meld_amd.build_knn_graph(X, knn=7, reorder=False)
    assert A.perm is not None and B.perm is None
    ra, rb = A.louvain(), B.louvain()
    assert np.array_equal(ra.labels, rb.labels) and abs(ra.modularity - rb.modularity) <= 1e-12
    assert [(lv["vertices"], lv["communities"], lv["rounds"]) for lv in ra.levels] == [(lv["vertices"], lv["communities"], lv["rounds"]) for lv in rb.levels]


def _six_groups(rng, joined=True):
    """Six dense groups of 40 vertices (weight 5), neighbours in a ring joined by six edges of weight 4: 2 % of the weight, so
    that one community is the best partition at resolution 0.01 (above 5/6 of the resolution) and the six groups at 1."""
    n, a, b, w = 240, [], [], []
    for q in range(6):
        for i in range(40):
            for j in range(i + 1, 40):
                if rng.uniform() < 0.3:
                    a.append(q * 40 + i), b.append(q * 40 + j), w.append(5.0)
        for t in range(6 if joined else 0):
            a.append(q * 40 + t), b.append(((q + 1) % 6) * 40 + 20 + t), w.append(4.0)
    return _sym(np.array(a), np.array(b), np.array(w), n)


def test_n_clusters():
    from meld_amd.graph import DeviceGraph

    G = DeviceGraph.from_scipy(_six_groups(np.random.default_rng(0)))
    assert G.louvain(resolution=0.01).n_communities == 1  # (the bisection has work to do)
    rec = G.louvain(n_clusters=6)
    assert rec.n_communities == 6 and np.array_equal(rec.labels, np.repeat(np.arange(6), 40))
    assert 0.01 <= rec.resolution <= 10 and rec.sizes.tolist() == [40] * 6
    apart = DeviceGraph.from_scipy(_six_groups(np.random.default_rng(0), joined=False))
    with pytest.raises(ValueError, match="r_start is too large. Got: 0.01"):
        apart.louvain(n_clusters=3)
    with pytest.raises(ValueError, match="r_stop is too small. Got: 10"):
        apart.louvain(n_clusters=241)


def test_estimator_returns_a_series_on_the_cells_index():
    import pandas as pd

    X = pd.DataFrame(blobs(600, 5, 6, 1.0, 10.0, 2), index=["cell{}".format(i) for i in range(600)])
    op = _fit(X)
    s = op.louvain(resolution=0.5)
    assert isinstance(s, pd.Series) and s.name == "louvain" and list(s.index) == list(X.index)
    assert np.array_equal(s.to_numpy(), op.graph.louvain(resolution=0.5).labels)


def test_subgraph_row_shard_and_no_entries():
    from meld_amd.graph import DeviceGraph

    W = _graph("hub_300")
    G = DeviceGraph.from_scipy(W)
    ind = np.random.default_rng(5).permutation(W.shape[0])[:3000]  # (not ascending: the subgraph carries a permutation)
    sub = G.subgraph(ind)
    assert sub.perm is not None
    Ws = sub.W
    assert abs(Ws - W[ind][:, ind]).max() == 0
    _assert_record_equals(sub.louvain(resolution=0.5), ref.louvain(Ws, 0.5), "subgraph")
    shard = DeviceGraph(G.rowptr[:101].clone(), G.col, G.val, G.dw_dev[:100].clone(), n_total=G.N)
    with pytest.raises(ValueError, match="only defined for an unsharded graph"):
        shard.louvain()
    with pytest.raises(ValueError, match="only defined for an unsharded graph"):
        shard.modularity(np.zeros(G.N, dtype=np.int64))
    empty = DeviceGraph.from_scipy(sparse.csr_matrix((5, 5)))
    rec = empty.louvain()
    assert rec.labels.tolist() == [0, 1, 2, 3, 4] and rec.modularity == 0.0 and rec.n_communities == 5 and rec.sizes.tolist() == [1] * 5
    assert rec.levels == [] and empty.modularity(np.arange(5)) == 0.0
    with pytest.raises(ValueError, match="resolution"):
        G.louvain(resolution=0.0)
    with pytest.raises(ValueError, match="one entry per cell"):
        G.modularity(np.zeros(3, dtype=np.int64))
    with pytest.raises(ValueError, match="negative"):
        G.modularity(np.full(G.N, -1))
