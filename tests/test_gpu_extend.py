"""Out-of-sample extension on the GPU against the oracle fixture tests/golden/g9_extend.npz (oracle.kernel_to_data, the
restatement of graphtools' kNNGraph.build_kernel_to_data for cells that are not among the references).  Tolerances are those of
tests/test_gpu_parity.py: kernel weights 1e-9 relative with an identical sparsity pattern (the fixture's generator guarantees the
pattern is well defined), densities 1e-5 relative to the column maximum."""
import os

import numpy as np
import pandas as pd
import pytest
import torch
from scipy import sparse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {"a": dict(knn=5, decay=40, thresh=1e-4), "b": dict(knn=5, decay=None, thresh=1e-4), "w": dict(knn=20, decay=2, thresh=1e-4)}
QUERIES = ("q150", "q63", "q1")


@pytest.fixture(scope="module")
def g9():
    return np.load(os.path.join(ROOT, "tests", "golden", "g9_extend.npz"))


def _kernel(z, tag, q, n=600):
    ip = z["K_{}_{}_indptr".format(tag, q)]
    return sparse.csr_matrix((z["K_{}_{}_data".format(tag, q)], z["K_{}_{}_indices".format(tag, q)].astype(np.int32), ip), shape=(len(ip) - 1, n))


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _csr_same(A, B, rtol):
    A, B = sparse.csr_matrix(A), sparse.csr_matrix(B)
    A.sort_indices()
    B.sort_indices()
    assert A.shape == B.shape
    assert np.array_equal(A.indptr, B.indptr), "rows of different length"
    assert np.array_equal(A.indices, B.indices), "different sparsity pattern"
    np.testing.assert_allclose(A.data, B.data, rtol=rtol, atol=0)


@pytest.fixture(scope="module")
def graphs(g9):
    """One fitted graph per parameter set on the fixture's 600 x 8 cells (shared, never modified)."""
    import meld_amd

    out = {}
    for tag, par in PARAMS.items():
        op = meld_amd.MELD(n_pca=None, **par)
        op.fit(g9["ref"].astype(np.float64))
        out[tag] = op.graph
    return out


@pytest.mark.parametrize("tag", ["a", "b", "w"])
def test_build_kernel_to_data_matches_the_fixture(g9, graphs, tag):
    G = graphs[tag]
    assert G.perm is None and G.n_features_in == 8
    for q in QUERIES:
        K = G.build_kernel_to_data(g9[q].astype(np.float64))
        assert sparse.issparse(K) and K.format == "csr" and K.shape == (g9[q].shape[0], 600)
        for r in range(K.shape[0]):  # (columns sorted inside a row, as exported)
            assert np.all(np.diff(K.indices[K.indptr[r]:K.indptr[r + 1]]) > 0)
        _csr_same(K, _kernel(g9, tag, q), rtol=1e-9)
    if tag == "w":
        assert np.diff(K.indptr).max() <= 128


@pytest.mark.parametrize("tag", ["a", "b", "w"])
def test_extend_to_data_rows_sum_to_one(g9, graphs, tag):
    G = graphs[tag]
    T = G.extend_to_data(g9["q150"].astype(np.float64))
    np.testing.assert_allclose(np.asarray(T.sum(1)).ravel(), 1.0, rtol=1e-14)
    K = _kernel(g9, tag, "q150")
    _csr_same(T, sparse.diags(1.0 / np.asarray(K.sum(1)).ravel()) @ K, rtol=1e-9)


@pytest.mark.parametrize("tag", ["a", "b", "w"])
@pytest.mark.parametrize("q", QUERIES)
def test_interpolate_matches_the_fixture(g9, graphs, tag, q):
    G = graphs[tag]
    F = g9["F"].astype(np.float64)
    Y = g9[q].astype(np.float64)
    T = G.extend_to_data(Y)
    for p in (1, 3, 7):
        got = G.interpolate(F[:, :p], Y=Y)
        want = g9["TF_{}_{}".format(tag, q)][:, :p]
        assert got.shape == want.shape
        for c in range(p):
            assert np.abs(got[:, c] - want[:, c]).max() / np.abs(want[:, c]).max() < 1e-5
        # the device product and the host product of the exported transitions are the same matrix product
        np.testing.assert_allclose(got, G.interpolate(F[:, :p], transitions=T), rtol=1e-12, atol=1e-14)
    # torch tensors and DataFrames go the same way; a vector comes back as a vector
    v = G.interpolate(torch.from_numpy(F[:, 0]), Y=torch.from_numpy(Y))
    assert v.shape == (Y.shape[0],)
    np.testing.assert_array_equal(v, G.interpolate(pd.DataFrame(F[:, :1]), Y=pd.DataFrame(Y))[:, 0])


def test_copy_of_a_fitted_cell_gets_weight_on_itself(g9, graphs):
    Y = g9["q150"].astype(np.float64)
    K = graphs["a"].build_kernel_to_data(Y)
    T = graphs["a"].extend_to_data(Y)
    for r, c in zip(g9["copy_rows"], g9["copies"]):
        assert K[r, c] == 1.0
        assert T[r, c] > 0 and T[r, c] == T[r].max()
    # bandwidth_scale widens the kernel, a fixed bandwidth replaces the neighbour distance (graphtools' keywords)
    K2 = graphs["a"].build_kernel_to_data(Y, bandwidth_scale=1.5)
    A, A2 = K.toarray(), K2.toarray()
    assert K2.nnz > K.nnz and (A2[A > 0] >= A[A > 0]).all()
    d = np.sqrt(((Y[:, None, :] - g9["ref"].astype(np.float64)[None, :, :]) ** 2).sum(-1))
    Kf = graphs["a"].build_kernel_to_data(Y, bandwidth=0.3)
    want = np.exp(-((d / 0.3) ** 40))
    want[want < 1e-4] = 0
    assert np.array_equal(Kf.toarray() > 0, want > 0)
    np.testing.assert_allclose(Kf.toarray(), want, rtol=1e-9, atol=0)


def test_pca_model_projects_raw_cells(g9):
    import meld_amd
    from tests.golden import make_golden_extend as gen

    Xp = gen.pca_cells()
    assert gen.sha(Xp) == str(g9["pca_raw_sha"])
    raw_ref, raw_q = Xp[:600], Xp[600:]
    op = meld_amd.MELD(n_pca=8, **PARAMS["a"])
    op.fit(raw_ref)
    G = op.graph
    assert G.n_features_in == 40
    want = sparse.csr_matrix((g9["K_pca_data"], g9["K_pca_indices"].astype(np.int32), g9["K_pca_indptr"]), shape=(63, 600))
    _csr_same(G.build_kernel_to_data(raw_q), want, rtol=1e-9)
    # reduced input: the oracle's own scores (sklearn's exact PCA), up to the sign of each component
    dev_q = G._extend_state.project(torch.from_numpy(raw_q).cuda()).cpu().numpy()
    sign = np.sign((dev_q * g9["pca_red_q"]).sum(0))
    np.testing.assert_allclose(dev_q, g9["pca_red_q"] * sign, rtol=0, atol=1e-9 * np.abs(dev_q).max())
    _csr_same(G.build_kernel_to_data(g9["pca_red_q"] * sign), want, rtol=1e-9)
    with pytest.raises(ValueError, match=r"Y must be of shape either \(n, 40\) or \(n, 8\)"):
        G.build_kernel_to_data(np.zeros((3, 9)))


def test_permuted_graph_answers_in_the_callers_order():
    """A graph large enough for the locality order (``perm`` set): kernel and interpolation in the caller's order equal those of the
    same cells built without the reordering; F handed over in device order (columns translated in the kernel) gives the same."""
    import meld_amd
    from meld_amd.extend import attach_extension_state
    from meld_amd.graph import build_knn_graph
    from oracle import meld_oracle as mo

    X, _ = mo.synthetic_cells(9000 + 130, n_dims=8, seed=5)
    ref, Y = X[:9000], X[9000:].copy()
    Y[3], Y[77] = ref[1234], ref[8999]
    op = meld_amd.MELD(n_pca=None, knn=5)
    op.fit(ref)
    G = op.graph
    assert G.perm is not None
    Xd = torch.from_numpy(ref).cuda()
    H = build_knn_graph(Xd, knn=5, decay=40, thresh=1e-4, reorder=False)
    attach_extension_state(H, Xd, 8, None, None, knn=5, decay=40, thresh=1e-4)
    assert H.perm is None
    K, KH = G.build_kernel_to_data(Y), H.build_kernel_to_data(Y)
    _csr_same(K, KH, rtol=1e-12)
    assert K[3, 1234] == 1.0 and K[77, 8999] == 1.0
    # ... and, independent of the extension's code, graphtools' kernel restated in NumPy on direct differences: bandwidth = the
    # distance to the knn-th fitted cell, exp(-(d / bw)^decay) >= thresh.  The pattern is well defined on these seeded cells
    # (asserted: no value within 1e-6 of thresh; the nearest is 6 % off), so it has to be identical.
    d = np.sqrt(((Y[:, None, :] - ref[None, :, :]) ** 2).sum(-1))
    bw = np.maximum(np.sort(d, axis=1)[:, 4], np.finfo(float).eps)
    want = np.exp(-((d / bw[:, None]) ** 40))
    assert not (np.abs(want / 1e-4 - 1.0) <= 1e-6).any()
    want[want < 1e-4] = 0
    _csr_same(K, sparse.csr_matrix(want), rtol=1e-9)
    F = np.random.default_rng(3).normal(size=(9000, 3))
    a = G.interpolate(F, Y=Y)
    np.testing.assert_allclose(a, H.interpolate(F, Y=Y), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(a, G.extend_to_data(Y) @ F, rtol=1e-12, atol=1e-14)
    Fd = torch.from_numpy(F).cuda()
    b = G.interpolate_device(Fd.index_select(0, G.perm), torch.from_numpy(Y).cuda(), device_order=True)
    assert b.is_cuda and tuple(b.shape) == (130, 3)
    np.testing.assert_array_equal(b.cpu().numpy(), a)


def test_transform_new_after_fit_transform(g9):
    import meld_amd

    ref, Y = g9["ref"].astype(np.float64), g9["q150"].astype(np.float64)
    op = meld_amd.MELD(lmax=float(g9["lmax"]), **PARAMS["a"])
    with pytest.raises(ValueError, match="sample_densities must be set prior"):
        op.transform_new(Y)
    dens = op.fit_transform(ref, g9["labels"])
    assert _rel(dens.values, g9["dens"]) < 1e-5
    index = ["new{}".format(i) for i in range(150)]
    out = op.transform_new(pd.DataFrame(Y, index=index))
    assert list(out.columns) == list(dens.columns) == list(g9["samples"]) and list(out.index) == index and out.shape == (150, 2)
    Ka = _kernel(g9, "a", "q150")
    Ta = sparse.diags(1.0 / np.asarray(Ka.sum(1)).ravel()) @ Ka
    np.testing.assert_allclose(out.values, Ta @ dens.values, rtol=1e-9, atol=1e-14 * np.abs(dens.values).max())
    for c in range(2):
        assert np.abs(out.values[:, c] - g9["dens_q150"][:, c]).max() / np.abs(g9["dens_q150"][:, c]).max() < 1e-5
    plain = op.transform_new(Y)
    assert list(plain.index) == list(range(150))
    lik = meld_amd.utils.normalize_densities(out)
    np.testing.assert_allclose(lik.values.sum(1), 1.0)


def _hand_csr(M, N, seed):
    rng = np.random.default_rng(seed)
    lens = np.array([1, 64, 65, 130])[np.arange(M) % 4]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(N, size=n, replace=False)) for n in lens]).astype(np.int32)
    val = rng.random(int(rowptr[-1])) + 0.01
    return rowptr, col, val


@pytest.mark.parametrize("M", [3, 257])
@pytest.mark.parametrize("p", [1, 64])
def test_extend_apply_abi_on_a_hand_made_csr(M, p):
    """``meld_extend_apply`` through the C-ABI: rows of 1, 64, 65 and 130 entries against torch fp64, with and without the
    column translation."""
    from meld_amd._lib import check, get_lib, ptr

    lib, dev, N = get_lib(), torch.device("cuda"), 1000
    rowptr, col, val = _hand_csr(M, N, seed=M + p)
    rng = np.random.default_rng(1)
    F = rng.normal(size=(N, p))
    dense = torch.zeros(M, N, dtype=torch.float64)
    rows = np.repeat(np.arange(M), np.diff(rowptr))
    dense[rows, col.astype(np.int64)] = torch.from_numpy(val)
    rowsum = dense.sum(1)
    want = (dense / rowsum[:, None]) @ torch.from_numpy(F)
    t = [torch.from_numpy(a).to(dev) for a in (rowptr, col, val)]
    rs, Fd = rowsum.to(dev), torch.from_numpy(F).to(dev)
    out = torch.full((M, p), float("nan"), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    check(lib.meld_extend_apply(ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(rs), M, ptr(Fd), N, p, None, ptr(out), st), "meld_extend_apply")
    np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), rtol=1e-12, atol=1e-13)
    perm = torch.from_numpy(rng.permutation(N)).to(dev)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(N, device=dev)
    out2 = torch.full((M, p), float("nan"), dtype=torch.float64, device=dev)
    check(lib.meld_extend_apply(ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(rs), M, ptr(Fd.index_select(0, perm).contiguous()), N, p, ptr(inv), ptr(out2), st),
          "meld_extend_apply")
    assert torch.equal(out, out2)
    assert lib.meld_extend_apply(None, None, None, None, M, None, N, p, None, None, st) == -1  # null pointers: rejected before any launch


def test_extend_rows_abi_sorts_rows_of_any_length():
    """``meld_extend_rows`` through the C-ABI: a shuffled COO stream (rows of 0, 1, 64, 65, 130 and 300 entries -- beyond one LDS
    tile --, entries of foreign rows and columns in between) -> sorted rows, doubled values, row sums."""
    from meld_amd.extend import extend_rows

    rng = np.random.default_rng(4)
    N, row_begin = 5000, 700
    lens = np.array([0, 1, 64, 65, 130, 300, 5, 0, 257, 256])
    rows = np.repeat(np.arange(len(lens)), lens)
    cols = np.concatenate([rng.choice(N, size=n, replace=False) for n in lens])
    vals = rng.random(rows.shape[0])
    # foreign entries: a row in front of the slice, one behind it, a column beyond n_cols
    rows_all = np.concatenate([rows + row_begin, [row_begin - 1, row_begin + len(lens), row_begin + 2]])
    cols_all = np.concatenate([cols, [3, 4, N + 5]])
    vals_all = np.concatenate([vals, [9.0, 9.0, 9.0]])
    o = rng.permutation(rows_all.shape[0])
    keys = torch.from_numpy((rows_all[o].astype(np.int64) << 32) | cols_all[o].astype(np.int64)).cuda()
    rowptr, col, val, rowsum = extend_rows(keys, torch.from_numpy(vals_all[o]).cuda(), row_begin, len(lens), N)
    want = sparse.csr_matrix((2.0 * vals, (rows, cols)), shape=(len(lens), N))
    want.sort_indices()
    nnz = int(rowptr[-1])
    assert nnz == want.nnz
    np.testing.assert_array_equal(rowptr.cpu().numpy(), want.indptr)
    np.testing.assert_array_equal(col.cpu().numpy()[:nnz], want.indices)
    np.testing.assert_array_equal(val.cpu().numpy()[:nnz], want.data)
    np.testing.assert_allclose(rowsum.cpu().numpy(), np.asarray(want.sum(1)).ravel(), rtol=1e-14)
