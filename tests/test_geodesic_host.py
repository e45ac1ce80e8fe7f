"""Geodesic distances, host side (no GPU): the pure helpers of meld_amd/geodesic.py, the argument checks of ``meld_minplus_step``
and ``meld_edge_lengths_l2`` (every case of the contract in include/meld_hip.h is refused before any launch), the round kernels'
register budget, the host
restatement of the rounds (tests/geodesic_reference.py) against scipy's dijkstra -- bit for bit where all lengths are positive --
and against a plain Dijkstra where some are zero, and the estimator's not-fitted error."""
import ctypes
import heapq
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import sparse
from scipy.sparse.csgraph import dijkstra

from tests.geodesic_reference import jacobi_host, zero_length_graph


# -- pure helpers ---------------------------------------------------------------------------------------------------------------
def test_check_distance():
    from meld_amd.geodesic import check_distance

    for name in ("affinity", "data", "constant"):
        assert check_distance(name) == name
    for bad in ("euclidean", "Affinity", None, 1, ""):
        with pytest.raises(ValueError, match=r"affinity.*data.*constant"):
            check_distance(bad)


def test_default_distance_is_graphtools_rule():
    from meld_amd.geodesic import default_distance

    unweighted = SimpleNamespace(_extend_state=SimpleNamespace(decay=float("inf")))  # (decay=None reaches the builder as inf)
    assert default_distance(unweighted) == "constant"
    assert default_distance(SimpleNamespace(_extend_state=SimpleNamespace(decay=40.0))) == "affinity"
    assert default_distance(SimpleNamespace(_extend_state=None)) == "affinity"
    assert default_distance(SimpleNamespace()) == "affinity"


def test_check_sources():
    from meld_amd.geodesic import check_sources

    out = check_sources([3, 0, 3], 5)  # duplicates are allowed, the order is kept
    assert out.dtype == np.int64 and out.tolist() == [3, 0, 3]
    assert check_sources(np.array([4], dtype=np.int32), 5).tolist() == [4]
    assert check_sources(range(3), 5).tolist() == [0, 1, 2]
    assert check_sources(np.uint8(2), 5).tolist() == [2]
    for empty in ([], np.zeros(0, dtype=np.int64), np.zeros(5, dtype=bool)):
        out = check_sources(empty, 5)
        assert out.dtype == np.int64 and out.shape == (0,)
    mask = np.array([True, False, True, False, False])
    out = check_sources(mask, 5)
    assert out.dtype == np.int64 and out.tolist() == [0, 2]
    for bad in ([-1], [5], [0, 7], np.array([2, -3])):
        with pytest.raises(ValueError, match="out of range"):
            check_sources(bad, 5)
    with pytest.raises(ValueError, match="mask"):
        check_sources(mask[:4], 5)
    with pytest.raises(ValueError, match="one-dimensional"):
        check_sources([[0, 1], [2, 3]], 5)
    with pytest.raises(ValueError, match="integers"):
        check_sources([0.5], 5)


def test_data_refusal_names_the_case():
    from meld_amd.geodesic import data_refusal

    X = np.zeros((10, 3))

    def graph(state, info=None, n_rows=10, comm=None):
        return SimpleNamespace(N=10, n_rows=n_rows, comm=comm, info=info or {}, _extend_state=state)

    def state(**kw):
        return SimpleNamespace(**dict(dict(X=X, row_fn=None, metric=None, decay=40.0), **kw))

    assert data_refusal(graph(state())) is None
    assert "not built from cells" in data_refusal(graph(None))
    assert "PyGSPGraph" in data_refusal(graph(None, dict(adopted_from="PyGSPGraph")))
    assert "precomputed distance" in data_refusal(graph(None, dict(precomputed="distance")))
    assert "cosine" in data_refusal(graph(state(row_fn=lambda Q: Q), dict(metric="cosine")))
    assert "cosine / correlation" in data_refusal(graph(state(row_fn=lambda Q: Q)))
    assert "L1 / L-inf" in data_refusal(graph(state(metric=1), dict(metric="manhattan")))
    assert "row-sharded" in data_refusal(graph(state(), n_rows=5))
    assert "row-sharded" in data_refusal(graph(state(), comm=object()))
    assert "256" in data_refusal(graph(state(X=np.zeros((10, 257)))))


# -- the C entries ----------------------------------------------------------------------------------------------------------------
def test_max_cols_is_the_panel_width():
    from meld_amd import _lib, diffuse

    assert _lib.get_lib().meld_minplus_max_cols() == 128 == diffuse.MAX_COLS


def test_round_entry_rejects_its_contract_before_any_launch():
    """Every pointer is a plausible host address: nothing may touch it.  Each case returns -1 and names the entry."""
    from meld_amd import _lib

    lib = _lib.get_lib()
    buf = (ctypes.c_double * 4096)()
    a = ctypes.addressof(buf)
    x, y = a, a + 8 * 2048  # 4 rows of ld 8: [x, x + 32), [y, y + 32) doubles apart
    good = dict(rowptr=a, col=a, len=a, n_rows=4, x=x, ldx=8, y=y, ldy=8, p=8, changed=a)
    order = ("rowptr", "col", "len", "n_rows", "x", "ldx", "y", "ldy", "p", "changed")
    cases = {name + " NULL": {name: None} for name in ("rowptr", "col", "len", "x", "y", "changed")}
    cases.update({
        "p = 0": dict(p=0),
        "p = 129": dict(p=129, ldx=256, ldy=256),
        "ldx < p": dict(ldx=7),
        "ldy < p": dict(ldy=7),
        "n_rows < 0": dict(n_rows=-1),
        "y == x": dict(y=x),
        "y inside x's range": dict(y=x + 8 * 16),
        "x inside y's range": dict(x=y + 8 * 31),
    })
    for what, change in cases.items():
        args = dict(good, **change)
        lib.meld_scale_f64(None, 1.0, None, 10, None)  # (leaves another entry's message behind)
        assert lib.meld_minplus_step(*[args[k] for k in order], None) == -1, what
        assert lib.meld_last_error().decode().startswith("meld_minplus_step:"), (what, lib.meld_last_error())


def test_edge_length_entry_rejects_its_contract_before_any_launch():
    from meld_amd import _lib

    lib = _lib.get_lib()
    buf = (ctypes.c_double * 4096)()
    a = ctypes.addressof(buf)
    good = dict(rowptr=a, col=a, n_rows=4, X=a, ldX=8, d=8, out=a)
    order = ("rowptr", "col", "n_rows", "X", "ldX", "d", "out")
    cases = {name + " NULL": {name: None} for name in ("rowptr", "col", "X", "out")}
    cases.update({
        "d = 0": dict(d=0),
        "d = 257": dict(d=257, ldX=512),
        "ldX < d": dict(ldX=7),
        "n_rows < 0": dict(n_rows=-1),
        "n_rows = 2^31": dict(n_rows=2 ** 31),
    })
    for what, change in cases.items():
        args = dict(good, **change)
        lib.meld_scale_f64(None, 1.0, None, 10, None)
        assert lib.meld_edge_lengths_l2(*[args[k] for k in order], None) == -1, what
        assert lib.meld_last_error().decode().startswith("meld_edge_lengths_l2:"), (what, lib.meld_last_error())
    # no rows: a successful no-op, whatever col and out are
    assert lib.meld_edge_lengths_l2(a, None, 0, a, 8, 8, None, None) == 0


def test_round_kernels_compile_without_private_memory():
    """Both instantiations at the diffusion kernel's chunk sizes: no private memory, 4 and 3 waves per SIMD.  The
    round shares its pass over the matrix (csrc/csr_wave_stream.hpp) with the diffusion step and the wide recurrence step: the
    same holds for all five kernels, the wide step (which also keeps a z row) at 3 waves per SIMD."""
    import os

    from meld_amd import build as mbuild
    from tests.test_metric_knn_host import ROOT, _resource_usage

    assert "geodesic.hip" in mbuild.SOURCES
    rows = _resource_usage(os.path.join(ROOT, "meld_amd", "csrc", "geodesic.hip"))
    step = sorted(k for k in rows if "minplus_step_kernel" in k)
    assert len(step) == 2 and any("edge_lengths_l2_kernel" in k for k in rows), sorted(rows)
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]:"] == 0, (name, r)
    one, two = (rows[k] for k in step)  # (mangled names: ...ILi1EE..., ...ILi2EE...)
    assert "ILi1E" in step[0] and "ILi2E" in step[1]
    assert one["Occupancy [waves/SIMD]:"] >= 4 and two["Occupancy [waves/SIMD]:"] >= 3, (one, two)

    for src, kernel, waves in (("diffuse.hip", "diffuse_step_kernel", (4, 3)), ("spmm.hip", "cheby_step_wide_kernel", (3,))):
        assert src in mbuild.SOURCES
        rows = _resource_usage(os.path.join(ROOT, "meld_amd", "csrc", src))
        names = sorted(k for k in rows if kernel in k)
        assert len(names) == len(waves), sorted(rows)
        for name, least in zip(names, waves):  # (sorted: ...ILi1EE... before ...ILi2EE...)
            print(name, rows[name])
            assert rows[name]["ScratchSize [bytes/lane]:"] == 0 and rows[name]["Occupancy [waves/SIMD]:"] >= least, (name, rows[name])


# -- the rounds on the host ---------------------------------------------------------------------------------------------------------
def _alpha_decay_lengths(n=400, k=4, decay=4.0, thresh=1e-4, seed=0):
    """``-log w`` of a symmetrised alpha-decay kNN kernel (bandwidth = the distance to the k-th neighbour), zero diagonal.  The
    decay is mild, so that no weight rounds to 1: every length is positive."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, 3))
    dist = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    bw = np.sort(dist, axis=1)[:, k]
    K = np.exp(-(dist / bw[:, None]) ** decay)
    K[K < thresh] = 0.0
    W = (K + K.T) / 2
    np.fill_diagonal(W, 0.0)
    W = sparse.csr_matrix(W)
    assert 0 < W.data.min() and W.data.max() < 1
    L = W.copy()
    L.data = -np.log(W.data)
    return L


def test_jacobi_rounds_are_dijkstra_bit_for_bit():
    L = _alpha_decay_lengths()
    assert (L.data > 0).all() and abs(L - L.T).nnz == 0
    src = [0, 17, 399]
    D, rounds = jacobi_host(L, src)
    ref = dijkstra(L, indices=src).T
    assert D.shape == (400, 3) and np.array_equal(D, ref)  # (the inf pattern included)
    hops = dijkstra(L, indices=src, unweighted=True)
    finite = hops[np.isfinite(hops)]
    print("rounds {}, hop radius {}".format(rounds, int(finite.max())))
    assert int(finite.max()) + 1 <= rounds <= 400  # (rounds follow the weighted paths' edge counts, not the BFS depth)
    near, _ = jacobi_host(L, src, min_only=True)
    assert near.shape == (400,) and np.array_equal(near, dijkstra(L, indices=src, min_only=True))
    assert np.array_equal(near, D.min(axis=1))


def _plain_dijkstra(indptr, indices, lengths, source):
    n = indptr.shape[0] - 1
    dist = [float("inf")] * n
    dist[source] = 0.0
    heap = [(0.0, source)]
    while heap:
        du, u = heapq.heappop(heap)
        if du > dist[u]:
            continue
        for e in range(indptr[u], indptr[u + 1]):
            v, t = indices[e], du + lengths[e]
            if t < dist[v]:
                dist[v] = t
                heapq.heappush(heap, (t, v))
    return np.array(dist)


def test_jacobi_rounds_with_zero_length_edges():
    L = zero_length_graph()
    src = [3, 500, 999]  # (999 is isolated)
    D, _ = jacobi_host(L, src)
    for j, s in enumerate(src):
        assert np.array_equal(D[:, j], _plain_dijkstra(L.indptr, L.indices, L.data, s)), s
    assert D[999, 2] == 0.0 and np.isinf(np.delete(D[:, 2], 999)).all()


def test_geodesic_before_fit():
    import meld_amd

    with pytest.raises(ValueError, match="fit"):
        meld_amd.MELD().geodesic([0])
