"""The landmark operator on the device (meld_amd/landmark.py, csrc/landmark.hip) against the host reference
tests/landmark_reference.py (tied to a dense statement of graphtools' definition by tests/test_landmark_host.py).

Tolerances, derived.  u = 2^-53; every term is non-negative, so relative errors add and never cancel: a value that passes through
k roundings is within ``(1 + u)^k - 1`` of the exact one, and two computations of k1 and k2 roundings are within ``(k1 + k2) u`` of
each other to first order -- written below as ``2 (m + 1) u`` with ``m + 1 >= max(k1, k2)``, the form of tests/test_gpu_diffuse.py.

* A merged entry that sums ``m`` kernel entries: ``m - 1`` additions on the device (storage order, the diagonal last) and in scipy
  (its own order): ``2 (m + 1) u`` relative.  ``rowsum``: the same with ``m`` the row's length, the diagonal included.  With dyadic
  weights every sum is exact in any order: bit-equal.
* A transition ``A[j, l] / r[j]`` (``m`` terms over a row of ``R`` terms): ``(m - 1) + (R - 1) + 1`` roundings on the device; scipy
  multiplies by the rounded reciprocal instead, one rounding more: ``2 (m + R + 1) u``.
* ``landmark_op[l, q] = (sum_j fl(fl(A[j, l] / r[j]) A[j, q])) / s[l]`` over the ``n_l`` cells of landmark ``l``'s support, ``R`` the
  longest row of ``K`` (a bound on the terms of any ``A[j, .]`` and ``r[j]``).  Device: ``A[j, l]``, ``r[j]`` and ``A[j, q]`` carry at
  most ``R - 1`` roundings each, the division one, the fma chain at most ``n_l`` (products are not rounded), ``s[l]`` at most
  ``(R - 1) + n_l + 6`` (its terms, then per-lane sums and a six-level butterfly), the last division one: ``4 R + 2 n_l + 4``.  Host
  (two scaled copies of ``A`` and a sparse product): ``2 (R - 1) + 2`` for ``pnm``, ``2 (R - 1) + n_l + 2`` for ``pmn``, one per product,
  at most ``n_l`` for the sum: ``4 R + 2 n_l + 1``.  So ``m = 4 R + 2 n_l + 3`` and the bound is ``2 (m + 1) u`` relative per entry;
  the rows (summed in extended precision by the test) are within the same bound of 1.
* Products with a signal ``T``: the dot-product bounds of tests/test_gpu_extend.py, ``rtol = 1e-12, atol = 1e-14``.

Shapes: the merge kernels take one wave per row, four rows per workgroup and 256 entries per trip through LDS (N in {1, 2, 63, 64,
65, 257, 1000, 4097}; the star's hub holds N - 1 entries: 17 trips at 4097); the Gram takes 64 cells of a landmark per batch in
groups of 8 cells of at most 8 entries (L = 1: one landmark with every cell; L = N - 1 on the star: a row of 4,096 distinct labels,
the one-cell-at-a-time path) and ``meld_landmark_max()`` landmarks at most."""
import numpy as np
import pytest
import torch
from scipy import sparse

from tests import landmark_reference as ref
from tests.test_gpu_diffuse import _MAKERS

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SIZES = (1, 2, 63, 64, 65, 257, 1000, 4097)
GRAPHS = [("path", n) for n in SIZES] + [("star", n) for n in SIZES] + [(k, n) for k in ("random", "dyadic") for n in (65, 1000, 4097)]
LABELS = ("L1", "L2", "L64", "L65", "Nm1", "gaps")
_GRAPHS, _CASES = {}, {}


def _labels(case, n, seed):
    """Labels in the caller's order, not compacted.  "Nm1": every cell its own label, except that cell n // 3 (the star's hub)
    takes its successor's -- N - 1 landmarks, a gap for the compaction, and the hub's neighbours all carry distinct labels."""
    rng = np.random.default_rng(seed)
    if case == "L1":
        return np.full(n, 3, dtype=np.int64)
    if case == "L2":
        return rng.integers(0, 2, n)
    if case in ("L64", "L65"):
        L = int(case[1:])
        lab = rng.integers(0, L, n)
        lab[: min(n, L)] = np.arange(L)[: min(n, L)]  # (every label present where the cells suffice)
        return lab[rng.permutation(n)]
    if case == "Nm1":
        lab = np.arange(n)
        lab[n // 3] = lab[(n // 3 + 1) % n]
        return lab
    if case == "gaps":
        return 3 * rng.integers(0, 20, n) + 5
    raise KeyError(case)


def _graph(kind, n):
    if (kind, n) not in _GRAPHS:
        from meld_amd.graph import DeviceGraph

        G = DeviceGraph.from_scipy(_MAKERS[kind](n))
        K = G.K
        K.sort_indices()
        _GRAPHS[(kind, n)] = (G, K)
    return _GRAPHS[(kind, n)]


def _host(K, compact, L):
    """The reference and the term counts the bounds need."""
    out = ref.landmark_algebra(K, compact, L)
    ones = sparse.csr_matrix((np.ones_like(K.data), K.indices, K.indptr), shape=K.shape)
    terms = ref.merged(ones, compact, L)  # (kernel entries behind every merged entry)
    assert np.array_equal(terms.indptr, out["A"].indptr) and np.array_equal(terms.indices, out["A"].indices)
    out.update(terms=terms.data, row_len=np.diff(K.indptr), support=np.diff(out["A"].T.tocsr().indptr))
    return out


def _device_csr(lm, G):
    """``transitions_device`` as scipy CSR with rows in the caller's order, raw values, and the raw row sums."""
    rowptr, col, val, rowsum = (t.cpu().numpy() for t in lm.transitions_device)
    A = sparse.csr_matrix((val, col, rowptr), shape=(G.N, lm.n_landmark))
    inv = G._inv_perm_host()
    return (A, rowsum) if inv is None else (A[inv].tocsr(), rowsum[inv])


def _case(kind, n, case):
    key = (kind, n, case)
    if key not in _CASES:
        from meld_amd.landmark import compact_labels

        G, K = _graph(kind, n)
        lab = _labels(case, n, 1000 * n + len(kind) + len(case))
        compact, values = compact_labels(lab)
        L = int(values.shape[0])
        lm = G.landmarks(clusters=lab)
        assert lm.n_landmark == L and np.array_equal(lm.clusters, compact) and lm.clusters.dtype == np.int32
        assert torch.equal(lm.clusters_device.cpu(), torch.from_numpy(compact))
        A, rowsum = _device_csr(lm, G)
        _CASES[key] = dict(G=G, K=K, lab=lab, L=L, lm=lm, A=A, rowsum=rowsum, host=_host(K, compact, L))
    return _CASES[key]


def _check_merged(A, rowsum, host, exact=False):
    want = host["A"]
    assert A.shape == want.shape
    assert np.array_equal(A.indptr, want.indptr), "rows of different length"
    assert np.array_equal(A.indices, want.indices), "different sparsity pattern (or labels not ascending)"
    for i in np.flatnonzero(np.diff(A.indptr) > 1)[:2000]:  # (sorted and unique, said once more without the reference)
        assert np.all(np.diff(A.indices[A.indptr[i]:A.indptr[i + 1]]) > 0)
    if exact:
        assert np.array_equal(A.data, want.data) and np.array_equal(rowsum, host["r"])
        return
    err = np.abs(A.data - want.data)
    tol = 2 * (host["terms"] + 1) * U * want.data
    rerr = np.abs(rowsum - host["r"])
    rtol = 2 * (host["row_len"] + 1) * U * host["r"]
    print("merged: worst entry {:.2e} of its bound, worst row sum {:.2e} of its bound".format(
        float((err / tol).max()) if err.size else 0.0, float((rerr / np.maximum(rtol, 1e-300)).max()) if rerr.size else 0.0))
    assert np.all(err <= tol) and np.all(rerr <= rtol)


def _check_op(lm, host):
    L = lm.n_landmark
    op = lm.landmark_op
    assert isinstance(op, np.ndarray) and op.shape == (L, L) and op.dtype == np.float64
    assert lm.landmark_op_device.dtype == torch.float64 and tuple(lm.landmark_op_device.shape) == (L, L)
    want = host["landmark_op"]
    R = int(host["row_len"].max())
    m = 4 * R + 2 * host["support"] + 3  # (per landmark row)
    bound = 2 * (m + 1) * U
    err = np.abs(op - want)
    tol = bound[:, None] * want
    sums = np.asarray(op.astype(np.longdouble).sum(1), dtype=np.float64)
    s_err = np.abs(np.asarray(lm.landmark_sums.cpu().numpy()) - host["s"])
    s_tol = 2 * (R + host["support"] + 7) * U * host["s"]
    print("landmark_op L={}: worst entry {:.2e} of its bound, worst row sum {:.2e} of its bound".format(
        L, float((err / np.maximum(tol, 1e-300)).max()), float((np.abs(sums - 1.0) / bound).max())))
    assert op.min() >= 0.0
    assert np.all(err <= tol)  # (where the reference is zero the device is zero: the same pattern of products)
    assert np.all(np.abs(sums - 1.0) <= bound)
    assert np.all(s_err <= s_tol)


# 1. merged rows against scipy ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LABELS)
@pytest.mark.parametrize("kind,n", GRAPHS)
def test_merged_rows(kind, n, case):
    c = _case(kind, n, case)
    if kind == "star" and n >= 63:
        hub = n // 3
        K, compact = c["K"], c["lm"].clusters
        nb = K.indices[K.indptr[hub]:K.indptr[hub + 1]]
        nb = nb[nb != hub]
        assert nb.size == n - 1  # (one row far above one trip through LDS)
        if case == "Nm1":
            assert c["L"] == n - 1 and np.unique(compact[nb]).size == nb.size  # the hub's neighbours all carry distinct labels
        if case == "L1":
            assert np.unique(compact[nb]).size == 1  # ... and here they all share one
    if kind == "random":
        assert int((np.diff(c["K"].indptr) == 1).sum()) >= 10  # (isolated vertices: the diagonal alone)
    _check_merged(c["A"], c["rowsum"], c["host"], exact=(kind == "dyadic"))


# 2. the operator against the host reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LABELS)
@pytest.mark.parametrize("kind,n", GRAPHS)
def test_landmark_op(kind, n, case):
    c = _case(kind, n, case)
    _check_op(c["lm"], c["host"])
    T = c["lm"].transitions
    assert sparse.issparse(T) and T.format == "csr" and T.shape == (n, c["L"])
    np.testing.assert_allclose(np.asarray(T.sum(1)).ravel(), 1.0, rtol=1e-14)


def test_as_many_landmarks_as_the_accumulator_holds():
    from meld_amd._lib import get_lib
    from meld_amd.graph import DeviceGraph
    from meld_amd.landmark import LANDMARK_MAX

    L = get_lib().meld_landmark_max()
    assert L == LANDMARK_MAX and L >= 4096
    n = 2 * L
    G = DeviceGraph.from_scipy(_MAKERS["random"](n))
    K = G.K
    K.sort_indices()
    rng = np.random.default_rng(5)
    lab = np.r_[np.arange(L), rng.integers(0, L, n - L)][rng.permutation(n)]
    lm = G.landmarks(clusters=lab)
    assert lm.n_landmark == L
    host = _host(K, lab.astype(np.int32), L)
    _check_merged(*_device_csr(lm, G), host)
    _check_op(lm, host)


# 3. determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,case", [("star", 4097, "Nm1"), ("star", 4097, "L2"), ("random", 4097, "L65"), ("random", 1000, "gaps"),
                                         ("path", 257, "L64")])
def test_two_builds_are_bit_equal(kind, n, case):
    c = _case(kind, n, case)
    a = c["lm"]
    assert c["G"].landmarks(clusters=c["lab"]) is a  # (kept per argument set)
    b = c["G"].landmarks(clusters=c["lab"], recompute=True)
    assert b is not a
    for x, y in zip(a.transitions_device, b.transitions_device):
        assert torch.equal(x, y)
    assert torch.equal(a.landmark_sums, b.landmark_sums) and torch.equal(a.landmark_op_device, b.landmark_op_device)


# 4. fitted graphs ----------------------------------------------------------------------------------------------------------------
def _mixture(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)) + np.repeat([0.0, 6.0, 12.0], n // 3)[:, None]
    return X[rng.permutation(n)]


def _check_transitions(T, K, compact, L, host):
    """``T`` against ``normalize(K @ onehot, "l1")``: the same pattern, entries within ``2 (m + R + 1) u``."""
    want = ref.l1_rows(host["A"])
    want.sort_indices()
    T = sparse.csr_matrix(T)
    T.sort_indices()
    assert T.shape == want.shape and np.array_equal(T.indptr, want.indptr) and np.array_equal(T.indices, want.indices)
    R = np.repeat(np.diff(K.indptr), np.diff(want.indptr))
    tol = 2 * (host["terms"] + R + 1) * U * want.data
    err = np.abs(T.data - want.data)
    print("transitions: worst entry {:.2e} of its bound".format(float((err / tol).max())))
    assert np.all(err <= tol)


def _fitted_check(G, L, seed):
    K = G.K
    K.sort_indices()
    lab = np.random.default_rng(seed).integers(0, L, G.N)
    lab[:L] = np.arange(L)
    lm = G.landmarks(clusters=lab)
    host = _host(K, lab.astype(np.int32), L)
    _check_merged(*_device_csr(lm, G), host)
    _check_transitions(lm.transitions, K, lab, L, host)
    _check_op(lm, host)
    return lm, host


@pytest.fixture(scope="module")
def fitted():
    import meld_amd

    return {a: meld_amd.MELD(knn=5, anisotropy=a, verbose=False).fit(_mixture(3000, 20, 1)) for a in (1, 0)}


@pytest.mark.parametrize("anisotropy", [1, 0])
def test_fitted_graph(fitted, anisotropy):
    G = fitted[anisotropy].graph
    kd = G.kernel_diagonal().cpu().numpy()
    if anisotropy:
        assert float(np.abs(kd - 1.0).max()) > 1e-3  # (what this case is about)
    _fitted_check(G, 40, 11 + anisotropy)


def test_fitted_graph_in_the_locality_order():
    """9,000 cells: above the 8,192 from which the builder permutes the cells; the labels stay in the caller's order."""
    import meld_amd

    op = meld_amd.MELD(knn=5, verbose=False).fit(_mixture(9000, 20, 2))
    G = op.graph
    assert G.perm is not None
    lm, host = _fitted_check(G, 300, 13)
    assert op.landmarks(clusters=lm.clusters) is lm  # (the estimator delegates; compact labels are their own compaction)
    T = np.random.default_rng(3).standard_normal((300, 5))
    got = lm.interpolate(T)
    np.testing.assert_allclose(got, lm.transitions @ T, rtol=1e-12, atol=1e-14)
    in_order = lm.interpolate_device(torch.from_numpy(T).cuda(), device_order=True)
    assert torch.equal(in_order, torch.from_numpy(got).cuda().index_select(0, G.perm))


# 5. new cells ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 65, 500])
def test_new_cells(fitted, M):
    G = fitted[1].graph
    L = 40
    lab = np.random.default_rng(21).integers(0, L, G.N)
    lab[:L] = np.arange(L)
    lm = G.landmarks(clusters=lab)
    Y = _mixture(501, 20, 30 + M)[:M]
    KY = G.build_kernel_to_data(Y)
    KY.sort_indices()
    host = dict(A=ref.merged(KY, lab, L))
    ones = sparse.csr_matrix((np.ones_like(KY.data), KY.indices, KY.indptr), shape=KY.shape)
    host["terms"] = ref.merged(ones, lab, L).data
    E = lm.extend_to_data(Y)
    assert sparse.issparse(E) and E.format == "csr" and E.shape == (M, L)
    _check_transitions(E, KY, lab, L, host)
    np.testing.assert_allclose(np.asarray(E.sum(1)).ravel(), 1.0, rtol=1e-14)
    rowptr, col, val, rowsum = lm.extend_to_data_device(Y)
    assert val.dtype == torch.float64 and col.dtype == torch.int32 and tuple(rowsum.shape) == (M,)
    want = ref.l1_rows(host["A"])
    for p in (70, 3, 1):
        T = np.random.default_rng(p).standard_normal((L, p))
        got = lm.interpolate(T, Y=Y)
        assert got.shape == (M, p)
        np.testing.assert_allclose(got, want @ T, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(lm.interpolate(T), lm.transitions @ T, rtol=1e-12, atol=1e-14)
    v = lm.interpolate(T[:, 0], Y=torch.from_numpy(Y))  # (a vector comes back as a vector: the same product as one column)
    assert v.shape == (M,) and np.array_equal(v, got[:, 0])
    with pytest.raises(ValueError, match="one row per landmark"):
        lm.interpolate(np.zeros((L + 1, 2)))


# 6. default clustering -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blobs():
    import meld_amd

    rng = np.random.default_rng(8)
    truth = np.repeat(np.arange(4), 200)
    X = rng.normal(size=(800, 10)) + 40.0 * np.eye(4, 10)[truth]
    order = rng.permutation(800)
    X, truth = X[order], truth[order]
    op = meld_amd.MELD(knn=5, n_landmark=50, verbose=False).fit(X)
    return op, truth


def test_default_clustering_recovers_separate_blobs(blobs):
    """Four components, four landmarks: the clustering has to find them.  (What it took: the range finder iterates to a residual,
    31 products here where a fixed 4 left the blobs mixed, and ``n_svd`` is clipped to ``n_landmark`` -- ``default_clusters``.)"""
    op, truth = blobs
    G = op.graph
    assert G.connected_components()[0] == 4
    lm = G.landmarks(4, random_state=0)
    print("default clustering:", lm.info)
    assert lm.n_landmark == 4
    pairs = set(zip(truth.tolist(), lm.clusters.tolist()))
    assert len(pairs) == 4, sorted(pairs)  # (a partition: every blob one landmark, every landmark one blob)
    assert lm.info["clustering"] == "default" and lm.info["n_svd"] <= 100 and lm.info["kmeans_iterations"] >= 1
    assert lm.info["entries"] == int(lm.transitions_device[1].shape[0])
    np.testing.assert_allclose(lm.landmark_op, np.eye(4), rtol=0, atol=1e-13)  # (no kernel entry joins two components)


@pytest.mark.parametrize("n_landmark", [4, 10, 50])
def test_default_clustering_labels(blobs, n_landmark):
    op, _ = blobs
    G = op.graph
    lm = G.landmarks(n_landmark, random_state=3)
    L = lm.n_landmark
    assert 1 <= L <= n_landmark and np.array_equal(np.unique(lm.clusters), np.arange(L))
    again = G.landmarks(n_landmark, random_state=3, recompute=True)
    assert again is not lm and np.array_equal(again.clusters, lm.clusters)
    assert tuple(lm.landmark_op.shape) == (L, L)
    np.testing.assert_allclose(lm.landmark_op.sum(1), 1.0, rtol=1e-12)


def test_recorded_n_landmark_is_the_default(blobs):
    op, _ = blobs
    assert op.graph.n_landmark == 50
    lm = op.landmarks()
    assert lm.n_landmark <= 50 and lm is op.graph.landmarks(50)


# 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(fitted):
    from types import SimpleNamespace

    from meld_amd.graph import DeviceGraph
    from meld_amd.landmark import LANDMARK_MAX

    G = fitted[1].graph
    with pytest.raises(ValueError, match="less than the number of cells"):
        G.landmarks(G.N)
    with pytest.raises(ValueError, match="neither n_landmark nor clusters"):
        G.landmarks()
    with pytest.raises(ValueError, match="one entry per cell"):
        G.landmarks(clusters=np.zeros(G.N - 1, dtype=np.int64))
    with pytest.raises(ValueError, match="negative"):
        G.landmarks(clusters=torch.full((G.N,), -1, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError, match="integers"):
        G.landmarks(clusters=np.zeros(G.N))
    big = DeviceGraph.from_scipy(_MAKERS["path"](LANDMARK_MAX + 2))
    with pytest.raises(ValueError, match="above the {} landmarks".format(LANDMARK_MAX)):
        big.landmarks(LANDMARK_MAX + 1)
    with pytest.raises(ValueError, match=str(LANDMARK_MAX)):
        big.landmarks(clusters=np.arange(LANDMARK_MAX + 2))
    adopted = DeviceGraph.from_foreign(SimpleNamespace(W=_MAKERS["random"](257)))
    lm = adopted.landmarks(clusters=np.arange(257) % 7)
    assert lm.n_landmark == 7
    with pytest.raises(NotImplementedError, match="adopted from SimpleNamespace"):
        lm.extend_to_data(np.zeros((3, 20)))
    with pytest.raises(NotImplementedError, match="adopted from SimpleNamespace"):
        lm.interpolate(np.zeros((7, 2)), Y=np.zeros((3, 20)))
    with pytest.raises(NotImplementedError, match="landmark operator"):
        G.landmark_op
