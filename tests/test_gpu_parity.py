"""GPU parity tests: the HIP path (through the C-ABI) against the CPU oracle on the same seeded
inputs.  Tolerances: graph weights 1e-10 relative (fp64 both sides, different but exact distance
formulas amplified by the decay exponent), densities 1e-5 relative to the column maximum as
BASELINE.json's north_star states (measured ~1e-12 with a common lmax)."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy import sparse

pytestmark = pytest.mark.gpu


def _oracle():
    from oracle import meld_oracle as mo

    return mo


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _csr_close(A, B, rtol):
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
def cells5k():
    mo = _oracle()
    X, labels = mo.synthetic_cells(5000, n_dims=50, seed=0)
    G = mo.build_graph(X, knn=15, decay=40, thresh=1e-4, anisotropy=1, algorithm="brute")
    return X, labels, G


def test_library_loads_on_gpu():
    from meld_amd import _lib

    lib = _lib.get_lib()
    assert lib.meld_device_count() >= 1


@pytest.mark.parametrize("p", [1, 2, 3, 4, 6])
def test_chebyshev_recurrence_matches_oracle(cells5k, p):
    """A10: fused recurrence kernel vs pygsp-style scipy loop on the SAME (oracle-built) W."""
    mo = _oracle()
    import meld_amd
    from meld_amd.filter import chebyshev_apply, chebyshev_coefficients, spectral_kernel

    X, labels, G = cells5k
    rng = np.random.default_rng(1)
    sig = rng.random((G.N, p))
    sig /= sig.sum(0)
    lmax = 1.01 * float(sparse.linalg.eigsh(G.L, k=1, return_eigenvectors=False)[0])
    h = mo.filter_kernel_fn("heat", 60, 0, 1, lmax)
    c = mo.cheby_coeff(h, lmax, 30)
    c2 = chebyshev_coefficients(spectral_kernel("heat", 60, 0, 1, lmax), lmax, 30)
    np.testing.assert_allclose(c2, c, rtol=1e-13, atol=1e-16)
    ref = mo.cheby_op(G.L, lmax, c, sig)
    DG = meld_amd.DeviceGraph.from_scipy(G.W)
    out = chebyshev_apply(DG, torch.from_numpy(sig).cuda(), c, lmax).cpu().numpy()
    assert _rel(out, ref) < 1e-12


def test_knn_candidates_contain_true_neighbours():
    """A2: the MFMA search returns, for every row, a superset of its 32 nearest (fp64 brute force)."""
    mo = _oracle()
    from meld_amd._lib import check, get_lib, ptr

    lib = get_lib()
    X, _ = mo.synthetic_cells(3000, n_dims=50, seed=3)
    N, d = X.shape
    Xd = torch.from_numpy(X).cuda()
    st = torch.cuda.current_stream().cuda_stream
    KP, TS, BQ = lib.meld_knn_padded_dim(d), lib.meld_knn_tile_refs(), lib.meld_knn_block_queries()
    ksel = 64
    cap = lib.meld_knn_row_capacity(ksel)
    sums = torch.empty(d, dtype=torch.float64, device="cuda")
    check(lib.meld_col_sums_f64(ptr(Xd), N, d, ptr(sums), st))
    np.testing.assert_allclose(sums.cpu().numpy(), X.sum(0), rtol=1e-12)
    mean = sums / N
    n_tiles = (N + TS - 1) // TS
    Rt = torch.empty(n_tiles * KP * TS, dtype=torch.float32, device="cuda")
    norm2 = torch.empty(N, dtype=torch.float32, device="cuda")
    nmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    check(lib.meld_knn_prepare_refs(ptr(Xd), N, d, ptr(mean), KP, ptr(Rt), ptr(norm2), ptr(nmax), st))
    q_pad = ((N + BQ - 1) // BQ) * BQ
    Q = torch.empty(q_pad * KP, dtype=torch.float32, device="cuda")
    check(lib.meld_knn_prepare_queries(ptr(Xd), N, d, ptr(mean), KP, 0, N, ptr(Q), st))
    ci = torch.empty(q_pad * cap, dtype=torch.int32, device="cuda")
    cd = torch.empty(q_pad * cap, dtype=torch.float32, device="cuda")
    cc = torch.empty(q_pad, dtype=torch.int32, device="cuda")
    check(lib.meld_knn_topk(ptr(Q), ptr(Rt), N, KP, N, ksel, ptr(ci), ptr(cd), ptr(cc), st))
    torch.cuda.synchronize()
    Xc = X - X.mean(0)
    np.testing.assert_allclose(norm2.cpu().numpy(), (Xc**2).sum(1), rtol=1e-5)
    assert abs(float(nmax.item()) - (Xc**2).sum(1).max()) < 1e-3
    ci = ci.cpu().numpy().reshape(q_pad, cap)[:N, :ksel]
    cd = cd.cpu().numpy().reshape(q_pad, cap)[:N, :ksel]
    cc = cc.cpu().numpy()[:N]
    assert np.all(cc == ksel)
    D2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1) if N <= 1000 else None
    from scipy.spatial.distance import cdist

    D = cdist(X, X, "sqeuclidean")
    true32 = np.argsort(D, axis=1, kind="stable")[:, :32]
    for i in range(N):
        assert set(true32[i]).issubset(set(ci[i])), i
    # rows are sorted by (d2, idx) and d2 agrees with the exact value to fp32 accuracy
    assert np.all(np.diff(cd, axis=1) >= 0)
    exact = np.take_along_axis(D, ci.astype(np.int64), axis=1)
    assert np.abs(cd - exact).max() < 2e-4 * (Xc**2).sum(1).max()


@pytest.mark.parametrize("n,d,knn", [(5000, 50, 15), (2000, 10, 5), (777, 3, 7)])
def test_graph_matches_oracle(n, d, knn):
    """A2-A5: W (CSR, canonical order) and degrees equal the oracle's."""
    mo = _oracle()
    import meld_amd

    X, _ = mo.synthetic_cells(n, n_dims=d, seed=5)
    G = mo.build_graph(X, knn=knn, decay=40, thresh=1e-4, anisotropy=1, algorithm="brute")
    DG = meld_amd.build_knn_graph(torch.from_numpy(X).cuda(), knn=knn, decay=40, thresh=1e-4, anisotropy=1)
    _csr_close(DG.W, G.W, rtol=1e-9)
    np.testing.assert_allclose(DG.dw, G.dw, rtol=1e-9)
    _csr_close(DG.K, G.K, rtol=1e-9)
    np.testing.assert_allclose(DG.bandwidth_host, G.info["bandwidth"], rtol=1e-12)


@pytest.mark.parametrize("two_pass", [False, True], ids=["one-kernel", "filter+search"])
@pytest.mark.parametrize("n,d,knn", [(20000, 50, 15), (24000, 14, 10), (24000, 58, 10), (33555, 32, 5), (40000, 100, 15)])
def test_graph_in_the_principal_frame_matches_oracle(n, d, knn, two_pass, monkeypatch):
    """A2-A5 on the kernel that carries the headline -- the list-driven first pass in the cells' principal frame with the
    partial-distance test behind the first K block (``knn16_topk_kernel<.., LIST, EE>``; the product takes it from 262144 cells
    on, ``MELD_KNN_ROTATE_MIN=0`` asks for it here) -- against the ORACLE itself (brute-force kNN, [UPSTREAM graphtools
    ``build_kernel_to_data``] as restated at oracle/meld_oracle.py, reached from reference meld/meld.py:273), not against this
    library's plain path: W, K (CSR, canonical order), degrees and bandwidths.  Shapes: C2's width; one and four K blocks' worth
    of coordinates behind K block 0 (d = 14, 58); an odd number of K blocks searched in reference slices (33555 x 32, the shape
    of round 5's staging bug); the reference's default width n_pca = 100.  Both forms of the pass: the one kernel that tests and
    searches (what launches with few query blocks take, reference slices included) and the round-6 pair -- the list-filter pass
    (``meld_knn16_partial_filter``) + the search over the thinned lists -- which the product takes from ~400 000 cells on and
    ``MELD_KNN_TWO_PHASE=2`` asks for at these sizes (sliced search over thinned lists included)."""
    mo = _oracle()
    import meld_amd

    monkeypatch.setenv("MELD_KNN_ROTATE_MIN", "0")
    monkeypatch.setenv("MELD_KNN_TWO_PHASE", "2" if two_pass else "0")
    X, _ = mo.synthetic_cells(n, n_dims=d, seed=7)
    G = mo.build_graph(X, knn=knn, decay=40, thresh=1e-4, anisotropy=1, algorithm="brute", n_jobs=-1)
    DG = meld_amd.build_knn_graph(torch.from_numpy(X).cuda(), knn=knn, decay=40, thresh=1e-4, anisotropy=1)
    info = DG.info
    assert info["principal_frame"] and info["step_lists"] and info["prune"], info
    assert bool(info["two_phase"]) == two_pass, info
    if two_pass:
        assert 0 < info["pairs_past_filter"] < info["wave_tiles_done"]  # the filter pass dropped pairs, and not all of them
    assert info["blocks_past_partial_test"] is not None
    assert info["blocks_past_partial_test"] < 2 * info["wave_tiles_done"]  # the test dropped something
    _csr_close(DG.W, G.W, rtol=1e-9)
    np.testing.assert_allclose(DG.dw, G.dw, rtol=1e-9)
    _csr_close(DG.K, G.K, rtol=1e-9)
    np.testing.assert_allclose(DG.bandwidth_host, G.info["bandwidth"], rtol=1e-12)


@pytest.mark.parametrize("n,d,knn", [(6000, 50, 15), (20000, 10, 5)])
@pytest.mark.parametrize("opt", ["scale0.6", "scale0.93", "scale1.3", "fixed", "fixed_per_cell", "fixed_scaled"])
def test_bandwidth_options_match_the_oracle(n, d, knn, opt):
    """graphtools' ``bandwidth`` / ``bandwidth_scale`` (forwarded by reference meld/meld.py:106,117-118): a scaled adaptive
    bandwidth -- also below 1 / rf, where the kernel radius lies inside the bandwidth entry -- and a given bandwidth (one
    number, one per cell, scaled): W, K and the degrees equal the oracle's restatement of ``build_kernel_to_data``; at
    20000 cells the pruned, list-driven search runs with the start thresholds the options imply."""
    mo = _oracle()
    import meld_amd

    X, labels = mo.synthetic_cells(n, n_dims=d, seed=6)
    base = mo.knn_kernel(X, knn=knn, algorithm="brute", return_intermediates=True)[1]["bandwidth"]
    rng = np.random.default_rng(1)
    kw = {
        "scale0.6": dict(bandwidth_scale=0.6), "scale0.93": dict(bandwidth_scale=0.93), "scale1.3": dict(bandwidth_scale=1.3),
        "fixed": dict(bandwidth=float(np.median(base))),
        "fixed_per_cell": dict(bandwidth=base * rng.uniform(0.7, 1.2, size=n)),
        "fixed_scaled": dict(bandwidth=float(np.median(base)), bandwidth_scale=0.8),
    }[opt]
    G = mo.build_graph(X, knn=knn, decay=40, thresh=1e-4, anisotropy=1, algorithm="brute", **kw)
    DG = meld_amd.build_knn_graph(torch.from_numpy(X).cuda(), knn=knn, decay=40, thresh=1e-4, anisotropy=1, **kw)
    _csr_close(DG.W, G.W, rtol=1e-9)
    np.testing.assert_allclose(DG.dw, G.dw, rtol=1e-9)
    _csr_close(DG.K, G.K, rtol=1e-9)
    np.testing.assert_allclose(DG.bandwidth_host, G.info["bandwidth"], rtol=1e-12)
    if n >= 16384:
        assert DG.info["prune"] and DG.info["step_lists"]
    # and through the estimator, as the reference forwards them
    if n == 6000 and opt in ("scale0.93", "fixed"):
        samples, dens, Go = mo.fit_transform(X, labels, knn=knn, chebyshev_order=20, return_graph=True, algorithm="brute")  # (lmax only)
        Gk = mo.build_graph(X, knn=knn, algorithm="brute", **kw)
        ind = mo.sample_indicators(labels)[1]
        dens = mo.meld_filter(ind, Gk, chebyshev_order=20)
        out = meld_amd.MELD(knn=knn, chebyshev_order=20, lmax=Gk.lmax, verbose=0, **kw).fit_transform(X, labels)
        assert _rel(out.values, dens) < 1e-5


@pytest.mark.parametrize("opt", ["number", "per_cell", "scale", "callable"])
def test_dense_graph_bandwidth_options_match_the_oracle(opt):
    """``thresh=0`` (graphtools' TraditionalGraph, the graph of the reference's known-answer test) with graphtools' ``bandwidth`` --
    a number, one value per cell, or a CALLABLE of the pairwise-distance matrix (the one graph class that takes one) -- and
    ``bandwidth_scale``: W, degrees and densities against the oracle's restatement of ``TraditionalGraph.build_kernel``; a callable
    on the sparse builder is refused as upstream refuses it."""
    mo = _oracle()
    import meld_amd

    X, labels = mo.synthetic_cells(900, n_dims=8, seed=9)
    rng = np.random.default_rng(2)
    kw = {"number": dict(bandwidth=0.7), "per_cell": dict(bandwidth=rng.uniform(0.5, 1.0, size=900)), "scale": dict(bandwidth_scale=0.7),
          "callable": dict(bandwidth=lambda pdx: np.sort(pdx, axis=1)[:, 4], bandwidth_scale=1.2)}[opt]
    G = mo.build_graph(X, knn=7, decay=10, thresh=0, anisotropy=1, **kw)
    op = meld_amd.MELD(knn=7, decay=10, thresh=0, chebyshev_order=20, verbose=0, **kw).fit(X)
    np.testing.assert_allclose(np.asarray(op.graph.W.todense()), np.asarray(G.W.todense() if hasattr(G.W, "todense") else G.W), rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(op.graph.dw, G.dw, rtol=1e-10)
    ind = mo.sample_indicators(labels)[1]
    lmax = mo.estimate_lmax(G.L, G.dw)
    op.graph.lmax = lmax
    dens = op.transform(labels)
    ref = mo.meld_filter(ind, G, chebyshev_order=20, lmax=lmax)
    assert _rel(dens.values, ref) < 1e-5
    if opt == "callable":
        with pytest.raises(NotImplementedError):
            meld_amd.MELD(knn=7, verbose=0, bandwidth=lambda pdx: pdx[:, 1]).fit(X)
    with pytest.raises(NotImplementedError):
        meld_amd.MELD(knn=7, thresh=0, verbose=0, knn_max=9).fit(X)


@pytest.mark.parametrize("kind", ["distance", "affinity", "auto_distance", "auto_affinity"])
def test_precomputed_matrices_match_the_oracle(kind):
    """``MELD(distance="precomputed_distance" | "precomputed_affinity" | "precomputed").fit_transform(M, labels)``: graphtools'
    route for a square matrix of pairwise distances / affinities (TraditionalGraph), restated by the oracle."""
    mo = _oracle()
    from scipy.spatial.distance import cdist

    import meld_amd

    X, labels = mo.synthetic_cells(900, n_dims=8, seed=8)
    D = cdist(X, X)
    if "distance" in kind:
        M, k = D, "distance"
    else:
        M, k = np.exp(-(D / np.median(D)) ** 2), "affinity"   # some symmetric affinity with a unit diagonal
    Kd = mo.precomputed_kernel(M, k, knn=7, decay=20, thresh=1e-4)
    K = mo.apply_anisotropy(mo.symmetrize(Kd), 1)
    W = mo.weights_from_kernel(K)
    L, dw = mo.laplacian(W)
    Go = mo.OracleGraph(Kd, K, W, L, dw)
    ind = mo.sample_indicators(labels)[1]
    dens = mo.meld_filter(ind, Go, chebyshev_order=20)
    name = "precomputed" if kind.startswith("auto") else "precomputed_" + k
    op = meld_amd.MELD(distance=name, knn=7, decay=20, chebyshev_order=20, lmax=Go.lmax, verbose=0)
    out = op.fit_transform(M, labels)
    np.testing.assert_allclose(np.asarray(op.graph.W.todense()), np.asarray(W.todense() if hasattr(W, "todense") else W), rtol=1e-10, atol=1e-300)
    assert _rel(out.values, dens) < 1e-5
    with pytest.raises(ValueError):
        meld_amd.MELD(distance=name, verbose=0).fit(M[:, :5])


@pytest.mark.parametrize("case", ["mixture", "low_d", "iid_100d", "large_knn_max", "uncapped_corner", "capped_corner"])
def test_knn_max_matches_the_oracle(case):
    """graphtools' ``knn_max``: a row keeps its knn_max nearest cells (besides itself) at most -- through the candidate lists
    (ranked in refine) and, on iid 100-d data where the lists cannot certify the radius, through the certified top ranks or the
    exact sweep; against the oracle's restatement of ``build_kernel_to_data(knn_max=)``.  The two ``corner`` cases: knn = 1 with
    36 (knn + 1) < knn_max + 1, where upstream's re-search ends in an UNCAPPED radius search when no more than N // 10 rows hold
    6 (knn + 1) cells inside their radius (decay 40: few do) and in the cap when more do (decay 2: wide radii) -- the builder
    follows upstream in both (``build_knn_graph``)."""
    mo = _oracle()
    import meld_amd

    rng = np.random.default_rng(4)
    if case == "mixture":
        X, knn, kmax = mo.synthetic_cells(6000, n_dims=50, seed=3)[0], 15, 20
    elif case == "low_d":
        X, knn, kmax = mo.synthetic_cells(3000, n_dims=5, seed=3)[0], 5, 8
    elif case == "iid_100d":
        X, knn, kmax = rng.normal(size=(600, 100)), 5, 9
    elif case == "large_knn_max":
        X, knn, kmax = mo.synthetic_cells(4000, n_dims=20, seed=3)[0], 10, 100
    elif case == "capped_corner":
        X, knn, kmax = rng.normal(size=(3000, 2)), 1, 100
    else:  # a jittered grid (five cells inside every radius) and ONE cell with 120 others at its nearest-neighbour distance
        grid = np.stack(np.meshgrid(np.arange(54.0), np.arange(54.0)), -1).reshape(-1, 2) + rng.normal(0, 0.02, size=(2916, 2))
        ang = np.linspace(0, 2 * np.pi, 120, endpoint=False)
        centre = np.array([-3.0, -3.0])
        ring = centre + 0.5 * np.stack([np.cos(ang), np.sin(ang)], 1) * (1 + rng.normal(0, 1e-3, size=(120, 1)))
        X, knn, kmax = np.concatenate([grid, centre[None], ring]), 1, 100
    decay = {"capped_corner": 2, "uncapped_corner": 10}.get(case, 40)
    # (the corner cases: tree search, exact differences -- sklearn's brute force forms |x|^2 + |y|^2 - 2 x.y, too coarse for the
    # ring's tiny distances under the decay exponent)
    G = mo.build_graph(X, knn=knn, decay=decay, algorithm="ball_tree" if "corner" in case else "brute", knn_max=kmax)
    if case != "uncapped_corner":
        assert (np.diff(G.K_directed.indptr) <= kmax + 1).all()
    else:
        assert (np.diff(G.K_directed.indptr) > kmax + 1).any()  # (upstream's uncapped radius search: the oracle follows it)
    DG = meld_amd.build_knn_graph(torch.from_numpy(X).cuda(), knn=knn, decay=decay, knn_max=kmax)
    _csr_close(DG.W, G.W, rtol=1e-9)
    np.testing.assert_allclose(DG.dw, G.dw, rtol=1e-9)
    full = meld_amd.build_knn_graph(torch.from_numpy(X).cuda(), knn=knn, decay=decay)
    assert bool(DG.info.get("knn_max_uncapped_as_upstream")) == (case == "uncapped_corner")
    if case == "capped_corner":
        assert (np.diff(G.K_directed.indptr) == kmax + 1).any()  # (the cap bites)
    assert DG.nnz <= full.nnz and (case in ("large_knn_max", "uncapped_corner") or DG.nnz < full.nnz)
    with pytest.raises(ValueError):
        meld_amd.build_knn_graph(torch.from_numpy(X).cuda(), knn=knn, knn_max=knn - 1)


@pytest.mark.parametrize("symm", [("*", None), ("mnn", None), ("mnn", 0.3), ("mnn", 0.0)])
def test_kernel_symmetrisation_modes_match_the_oracle(symm):
    """graphtools' ``kernel_symm`` / ``theta`` (reference meld/meld.py:106,117-118 forwards them): K o K^T and
    theta min + (1 - theta) max instead of the default (K + K^T) / 2 -- in the row-bucket merge of the sparse builder and in
    the dense builder -- against the oracle; W stays bitwise symmetric (the folded recurrence layout relies on it)."""
    mo = _oracle()
    import meld_amd

    ks, th = symm
    X, labels = mo.synthetic_cells(7000, n_dims=30, seed=12)
    G = mo.build_graph(X, knn=9, algorithm="brute", kernel_symm=ks, theta=th)
    op = meld_amd.MELD(knn=9, kernel_symm=ks, theta=th, verbose=0).fit(X)
    _csr_close(op.graph.W, G.W, rtol=1e-9)
    W = op.graph.W
    assert abs(W - W.T).max() == 0
    np.testing.assert_allclose(op.graph.dw, G.dw, rtol=1e-9)
    Gd = mo.build_graph(X[:900], knn=9, thresh=0, decay=20, kernel_symm=ks, theta=th)
    Wd = meld_amd.MELD(knn=9, thresh=0, decay=20, kernel_symm=ks, theta=th, verbose=0).fit(X[:900]).graph.W
    np.testing.assert_allclose(np.asarray(Wd.todense()), np.asarray(Gd.W), rtol=1e-10, atol=1e-300)
    with pytest.raises(ValueError):
        meld_amd.MELD(kernel_symm="mnn", theta=1.5, verbose=0).fit(X[:500])
    with pytest.raises(NotImplementedError):
        meld_amd.MELD(kernel_symm=None, verbose=0).fit(X[:500])


def test_knn_beyond_the_candidate_lists_takes_the_dense_route():
    """knn = 150 (the search kernel's lists hold 128): the same kernel semantics evaluated densely, against the oracle."""
    mo = _oracle()
    import meld_amd

    X, labels = mo.synthetic_cells(1500, n_dims=10, seed=2)
    G = mo.build_graph(X, knn=150, algorithm="brute")
    op = meld_amd.MELD(knn=150, verbose=0).fit(X)
    assert op.graph.info.get("dense_knn")
    _csr_close(op.graph.W, G.W, rtol=1e-9)
    np.testing.assert_allclose(op.graph.dw, G.dw, rtol=1e-9)


def test_bandwidth_options_are_refused_where_they_are_not_built():
    import meld_amd

    X = np.random.default_rng(0).normal(size=(400, 5))
    for extra in (dict(sample_idx=np.arange(400) % 2), dict(distance="cosine")):
        with pytest.raises(NotImplementedError):
            meld_amd.MELD(bandwidth_scale=0.5, verbose=0, **extra).fit(X)
    # decay=None: upstream's unweighted kNN graph never looks at the bandwidth options -- accepted, no effect
    Wa = meld_amd.MELD(decay=None, bandwidth_scale=0.5, knn_max=9, verbose=0).fit(X).graph.W
    Wb = meld_amd.MELD(decay=None, verbose=0).fit(X).graph.W
    assert Wa.nnz == Wb.nnz and abs(Wa - Wb).max() == 0
    meld_amd.MELD(bandwidth_scale=0.5, thresh=0, verbose=0).fit(X)  # (round 6: the dense graph takes them, test_dense_graph_bandwidth_options_match_the_oracle)
    with pytest.raises(NotImplementedError):
        meld_amd.MELD(knn_max=9, thresh=0, verbose=0).fit(X)
    with pytest.raises(ValueError):
        meld_amd.MELD(bandwidth_scale=-1.0, verbose=0).fit(X)
    with pytest.raises(ValueError):
        meld_amd.MELD(bandwidth=np.ones(7), verbose=0).fit(X)


def test_graph_exact_sweep_path_matches_main_path():
    """Rows sent through the exact fp64 sweep give the same graph as certified candidate rows."""
    mo = _oracle()
    import meld_amd

    X, _ = mo.synthetic_cells(1500, n_dims=20, seed=9)
    Xd = torch.from_numpy(X).cuda()
    A = meld_amd.build_knn_graph(Xd, knn=10)
    B = meld_amd.build_knn_graph(Xd, knn=10, force_fallback=True)
    assert A.info["n_flagged_rows"] == 0 and B.info["n_flagged_rows"] == 1500
    _csr_close(A.W, B.W, rtol=1e-12)
    G = mo.build_graph(X, knn=10, algorithm="brute")
    _csr_close(B.W, G.W, rtol=1e-9)


def test_readme_toy_goes_through_radius_fallback():
    """C1 (README.md:51-57): iid 100-d data -- most rows have more radius neighbours than the
    candidate list holds, which exercises the flagged-row sweep like graphtools' re-search."""
    mo = _oracle()
    import meld_amd

    rng = np.random.default_rng(0)
    X = rng.normal(size=(500, 100))
    labels = rng.choice(["treatment", "control"], size=500)
    samples, dens, G = mo.fit_transform(X, labels, return_graph=True, algorithm="brute")
    op = meld_amd.MELD(lmax=G.lmax)
    out = op.fit_transform(X, labels)
    assert op.graph.info["n_flagged_rows"] > 0
    _csr_close(op.graph.W, G.W, rtol=1e-9)
    assert list(out.columns) == list(samples)
    assert _rel(out.values, dens) < 1e-5


def test_fit_transform_parity_50k_config_scaled():
    """C2-shaped (d=50, knn=15, beta=60, M=30) at N=20k so the oracle finishes in seconds; the full
    50k case is test_fit_transform_parity_50k_config below.  Common injected lmax ('lmax')."""
    mo = _oracle()
    import meld_amd

    X, labels = mo.synthetic_cells(20000, n_dims=50, seed=0)
    samples, dens, G = mo.fit_transform(X, labels, knn=15, beta=60, chebyshev_order=30, return_graph=True,
                                        algorithm="brute", n_jobs=-1)
    op = meld_amd.MELD(knn=15, beta=60, chebyshev_order=30, lmax=G.lmax)
    out = op.fit_transform(X, labels)
    assert out.shape == dens.shape
    # N >= 8192: the device arrays are in the cache-locality order; exports come back in input order
    assert op.graph.perm is not None and sorted(op.graph.perm.cpu().tolist()) == list(range(20000))
    _csr_close(op.graph.W, G.W, rtol=1e-9)
    np.testing.assert_allclose(op.graph.dw, G.dw, rtol=1e-9)
    np.testing.assert_allclose(op.graph.bandwidth_host, G.info["bandwidth"], rtol=1e-12)
    for c in range(dens.shape[1]):
        assert np.abs(out.values[:, c] - dens[:, c]).max() / np.abs(dens[:, c]).max() < 1e-5
    np.testing.assert_allclose(out.values, dens, rtol=1e-5, atol=1e-5 * dens.max())
    # native lmax: converged Lanczos vs ARPACK(tol=5e-3): same spectral bound to ~1e-3
    op2 = meld_amd.MELD(knn=15, beta=60, chebyshev_order=30)
    op2.fit_transform(X, labels)
    lam = float(sparse.linalg.eigsh(G.L, k=1, tol=1e-10, return_eigenvectors=False)[0])
    assert abs(op2.graph.lmax / 1.01 - lam) / lam < 2e-5  # default Lanczos tolerance 1e-3 (eigenvalue error ~ tol^2)
    assert abs(op2.graph.lmax - G.lmax) / G.lmax < 5e-3


def test_mass_conservation_and_laplacian_filter():
    """Invariant pinned by reference test/test_meld.py:78-81: 1^T h(L) x = h(0) 1^T x."""
    mo = _oracle()
    import meld_amd

    X, labels = mo.synthetic_cells(4000, n_dims=30, seed=11)
    for filt in ("heat", "laplacian"):
        op = meld_amd.MELD(knn=10, filter=filt, sample_normalize=False, chebyshev_order=40)
        out = op.fit_transform(X, labels)
        samples, dens, G = mo.fit_transform(X, labels, knn=10, filter=filt, sample_normalize=False,
                                            chebyshev_order=40, return_graph=True, lmax=op.graph.lmax, algorithm="brute")
        assert _rel(out.values, dens) < 1e-9
        counts = np.array([(labels == s).sum() for s in samples], dtype=float)
        np.testing.assert_allclose(out.values.sum(0), dens.sum(0), rtol=1e-10)
        np.testing.assert_allclose(out.values.sum(0), counts, rtol=1e-3)


def test_normalize_densities_kernel():
    mo = _oracle()
    import pandas as pd

    import meld_amd

    rng = np.random.default_rng(2)
    a = rng.normal(size=(1000, 3))
    a[5] = 0
    np.testing.assert_allclose(meld_amd.normalize_densities(a), mo.normalize_densities(a), rtol=1e-15)
    df = pd.DataFrame(np.abs(a[:, :2]), index=["c%d" % i for i in range(1000)], columns=["A", "B"])
    out = meld_amd.utils.normalize_densities(df)
    assert list(out.index) == list(df.index) and list(out.columns) == ["A", "B"]
    np.testing.assert_allclose(out.values.sum(1)[6:], 1.0, rtol=1e-14)


def test_sharded_driver_on_one_gpu_matches_single_gpu_path(tmp_path):
    """The row-sharded driver with HipOps over NCCL (=RCCL) and a 1-rank group must reproduce
    the single-GPU path: identical graph (same kernels), lmax / densities to rounding (the
    reductions go through all-reduce instead of a local sum)."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %r)
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", RANK="0", WORLD_SIZE="1")
torch.cuda.set_device(0)
dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
import meld_amd
from meld_amd import distributed as mdist
from oracle import meld_oracle as mo
X, labels = mo.synthetic_cells(6000, n_dims=50, seed=2)
a = meld_amd.MELD(knn=15, chebyshev_order=30)
da = mdist.fit_transform_sharded(a, torch.from_numpy(X).cuda(), labels)
b = meld_amd.MELD(knn=15, chebyshev_order=30)
db = b.fit_transform(X, labels)
assert a.graph.nnz == b.graph.nnz and a.graph.info["nnz_global"] == b.graph.nnz
assert torch.equal(a.graph.val, b.graph.val) and torch.equal(a.graph.col, b.graph.col)
assert abs(a.graph.lmax - b.graph.lmax) <= 1e-13 * b.graph.lmax, (a.graph.lmax, b.graph.lmax)
assert np.abs(da.values - db.values).max() <= 1e-11 * np.abs(db.values).max()
dist.destroy_process_group()
print("SHARDED_OK")
""" % root
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert "SHARDED_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]


@pytest.mark.parametrize("n,d", [(70001, 50), (5000, 3), (1000, 141)])
def test_column_statistics_in_one_pass_and_the_scale_they_imply(n, d):
    """meld_col_stats_f64 (sums, minima, maxima of the columns in one pass, fixed-order reduction) against torch, and
    meld_knn16_prepare_scaled -- the operand scale from the columns' extremes -- against meld_knn16_prepare's own pass over
    X: the same operands, bit for bit."""
    from meld_amd._lib import check, get_lib, ptr
    from meld_amd.graph import HipOps

    lib = get_lib()
    rng = np.random.default_rng(d)
    X = rng.normal(size=(n, d)) * rng.uniform(0.1, 30.0, size=d)[None, :] + rng.normal(size=d)[None, :] * 5.0
    Xd = torch.from_numpy(X).cuda()
    sums, mins, maxs = HipOps().col_stats(Xd)
    np.testing.assert_allclose(sums.cpu().numpy(), X.sum(0), rtol=1e-12, atol=1e-9)
    assert torch.equal(mins, Xd.min(0).values) and torch.equal(maxs, Xd.max(0).values)
    s2 = HipOps().col_stats(Xd)[0]
    assert torch.equal(sums, s2)  # reproducible bits
    st = torch.cuda.current_stream().cuda_stream
    TS, BQ = lib.meld_knn16_tile_refs(), lib.meld_knn16_block_queries()
    mean = sums / n
    n_tiles, q_pad = (n + TS - 1) // TS, ((n + BQ - 1) // BQ) * BQ
    outs = []
    for scaled in (False, True):
        Rt = torch.zeros(n_tiles * lib.meld_knn16_tile_bytes(d), dtype=torch.uint8, device="cuda")
        Q = torch.zeros(q_pad * lib.meld_knn16_query_bytes(d), dtype=torch.uint8, device="cuda")
        Qn = torch.zeros(q_pad, dtype=torch.float32, device="cuda")
        norm2 = torch.zeros(n, dtype=torch.float32, device="cuda")
        nmax = torch.zeros(1, dtype=torch.float32, device="cuda")
        sinfo = torch.zeros(4, dtype=torch.float32, device="cuda")
        if scaled:
            check(lib.meld_knn16_prepare_scaled(ptr(Xd), n, d, ptr(mean), ptr(mins), ptr(maxs), 0, n, ptr(Rt), ptr(Q), ptr(Qn), ptr(norm2), ptr(nmax), ptr(sinfo), st))
        else:
            check(lib.meld_knn16_prepare(ptr(Xd), n, d, ptr(mean), 0, n, ptr(Rt), ptr(Q), ptr(Qn), ptr(norm2), ptr(nmax), ptr(sinfo), st))
        outs.append((Rt, Q, Qn, norm2, nmax, sinfo))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n", [9000, 80000])
def test_sharded_recurrences_enqueued_from_c_equal_the_python_loops(n):
    """On an RCCL group the sharded Chebyshev filter and the sharded Lanczos iterations are ONE C call each
    (meld_cheby_run / meld_lanczos_steps_sharded on the library's own communicator: kernel + ncclAllGather (+ the one
    all-reduce) per step, enqueued back to back); MELD_SHARDED_C_LOOPS=0 restores the per-step Python loops over
    torch.distributed.  Same lmax and densities either way -- on the CSR-stream kernel (9000 cells) and on the panel-tiled
    layout (80000 cells) -- and the C path is the one that ran."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %r)
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29543", RANK="0", WORLD_SIZE="1")
torch.cuda.set_device(0)
dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
import meld_amd
from meld_amd import distributed as mdist, graph as mgraph
from oracle import meld_oracle as mo
n = %d
X, labels = mo.synthetic_cells(n, n_dims=50, seed=4)
Xd = torch.from_numpy(X).cuda()
calls = dict(cheby=0, lanczos=0)
orig_c, orig_l = mgraph.HipOps.cheby_run_sharded, mgraph.HipOps.lanczos_steps_sharded
def count_c(self, *a, **k):
    out = orig_c(self, *a, **k); calls["cheby"] += out is not None; return out
def count_l(self, *a, **k):
    out = orig_l(self, *a, **k); calls["lanczos"] += bool(out); return out
mgraph.HipOps.cheby_run_sharded, mgraph.HipOps.lanczos_steps_sharded = count_c, count_l
a = meld_amd.MELD(knn=15, chebyshev_order=30)
da = mdist.fit_transform_sharded(a, Xd, labels)
assert mdist.Comm().rccl() is not None and calls["cheby"] == 1 and calls["lanczos"] >= 1, calls
assert a.graph.info["spmm"] == ("tiled" if n >= 65536 else "csr"), a.graph.info["spmm"]
os.environ["MELD_SHARDED_C_LOOPS"] = "0"
mdist.Comm._RCCL.clear()
calls.update(cheby=0, lanczos=0)
b = meld_amd.MELD(knn=15, chebyshev_order=30)
db = mdist.fit_transform_sharded(b, Xd, labels)
assert calls == dict(cheby=0, lanczos=0), calls
assert abs(a.graph.lmax - b.graph.lmax) <= 1e-12 * b.graph.lmax, (a.graph.lmax, b.graph.lmax)
assert np.abs(da.values - db.values).max() <= 1e-12 * np.abs(db.values).max()
c = meld_amd.MELD(knn=15, chebyshev_order=31, lmax=b.graph.lmax)   # an odd number of steps on the single-GPU path
dc = c.fit_transform(X, labels)
os.environ["MELD_SHARDED_C_LOOPS"] = "1"
mdist.Comm._RCCL.clear()
e = meld_amd.MELD(knn=15, chebyshev_order=31, lmax=b.graph.lmax)
de = mdist.fit_transform_sharded(e, Xd, labels)
assert np.abs(de.values - dc.values).max() <= 1e-11 * np.abs(dc.values).max()
dist.destroy_process_group()
print("SHARDED_C_OK")
""" % (root, n)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert "SHARDED_C_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]


@pytest.mark.parametrize("nprod", [3, 1])
@pytest.mark.parametrize("n,d", [(3000, 50), (1500, 100), (2000, 3)])
def test_knn16_candidates_contain_true_neighbours(n, d, nprod):
    """A2, split-fp16 search: superset of the 32 nearest of every row, rows sorted, d2 within the
    error budget that refine's completeness test assumes (meld_knn16_error_coef * max |x~|^2)."""
    mo = _oracle()
    from scipy.spatial.distance import cdist

    from meld_amd._lib import check, get_lib, ptr

    lib = get_lib()
    X, _ = mo.synthetic_cells(n, n_dims=d, seed=3)
    X = X * 37.5 + 11.0  # arbitrary units and offset: the kernel centres and rescales internally
    N = n
    Xd = torch.from_numpy(X).cuda()
    st = torch.cuda.current_stream().cuda_stream
    KB, TS, BQ = lib.meld_knn16_kblocks(d), lib.meld_knn16_tile_refs(), lib.meld_knn16_block_queries()
    ksel = 64
    cap = lib.meld_knn16_row_capacity(ksel)
    sums = torch.empty(d, dtype=torch.float64, device="cuda")
    check(lib.meld_col_sums_f64(ptr(Xd), N, d, ptr(sums), st))
    mean = sums / N
    n_tiles = (N + TS - 1) // TS
    q_pad = ((N + BQ - 1) // BQ) * BQ
    Rt = torch.empty(n_tiles * lib.meld_knn16_tile_bytes(d), dtype=torch.uint8, device="cuda")
    Q = torch.empty(q_pad * lib.meld_knn16_query_bytes(d), dtype=torch.uint8, device="cuda")
    Qn = torch.empty(q_pad, dtype=torch.float32, device="cuda")
    norm2 = torch.empty(N, dtype=torch.float32, device="cuda")
    nmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    sinfo = torch.empty(4, dtype=torch.float32, device="cuda")
    check(lib.meld_knn16_prepare(ptr(Xd), N, d, ptr(mean), 0, N, ptr(Rt), ptr(Q), ptr(Qn), ptr(norm2), ptr(nmax), ptr(sinfo), st))
    ci = torch.empty(q_pad * cap, dtype=torch.int32, device="cuda")
    cd = torch.empty(q_pad * cap, dtype=torch.float32, device="cuda")
    cc = torch.empty(q_pad, dtype=torch.int32, device="cuda")
    check(lib.meld_knn16_topk(ptr(Q), ptr(Qn), ptr(Rt), ptr(sinfo), N, d, N, ksel, nprod, 1, None, None, 0, None, 0, 1.0, ptr(ci), ptr(cd), ptr(cc), None, None, None, st))
    torch.cuda.synchronize()
    Xc = X - X.mean(0)
    n2 = (Xc**2).sum(1)
    np.testing.assert_allclose(norm2.cpu().numpy(), n2, rtol=1e-5)
    assert abs(float(sinfo[2].item()) - np.abs(Xc).max()) < 1e-5 * np.abs(Xc).max()
    ci = ci.cpu().numpy().reshape(q_pad, cap)[:N, :ksel]
    cd = cd.cpu().numpy().reshape(q_pad, cap)[:N, :ksel]
    assert np.all(cc.cpu().numpy()[:N] == ksel)
    D = cdist(X, X, "sqeuclidean")
    true32 = np.argsort(D, axis=1, kind="stable")[:, :32]
    n_true = 32 if nprod == 3 else 24  # the hi-only search may permute candidates near the cut
    for i in range(N):
        assert set(true32[i][:n_true]).issubset(set(ci[i])), i
        assert len(set(ci[i])) == ksel
    assert np.all(np.diff(cd, axis=1) >= 0)
    exact = np.take_along_axis(D, ci.astype(np.int64), axis=1)
    err = np.abs(cd - exact).max() / n2.max()
    print("knn16 nprod=%d max |d2 - exact| / max|x|^2 = %.3e (budget %.3e)" % (nprod, err, lib.meld_knn16_error_coef(nprod, d)))
    assert err < 0.5 * lib.meld_knn16_error_coef(nprod, d)  # the budget is a worst-case bound


def test_both_search_kernels_build_the_same_graph():
    import meld_amd
    from meld_amd.graph import HipOps

    mo = _oracle()
    X, _ = mo.synthetic_cells(4000, n_dims=50, seed=12)
    Xd = torch.from_numpy(X).cuda()
    graphs = {}
    for search, nprod in (("f32", 3), ("f16x3", 3), ("f16x3", 1)):
        ops = HipOps(search=search, nprod=nprod)
        keys, vals, bw, info = ops.directed_kernel_coo(Xd, 0, 4000, 15, 40, 1e-4, 64)
        rowptr, col, val = ops.assemble_rows(keys, vals, 0, 4000, 4000)
        graphs[(search, nprod)] = (rowptr, col, val, bw)
        assert info["search"] == search
    for key in (("f16x3", 3), ("f16x3", 1)):
        for a, b in zip(graphs[("f32", 3)], graphs[key]):
            assert torch.equal(a, b)


def test_fit_transform_parity_50k_config():
    """BASELINE.json configs[1] at full size: 50k cells x 50 dims, knn=15, beta=60, Chebyshev order 30 on one
    MI355X against the CPU oracle (brute-force kNN on all host cores so that it finishes in seconds): graph
    weights / degrees to 1e-9, sample densities within the north star's 1e-5 relative (fp64), common lmax."""
    mo = _oracle()
    import meld_amd

    X, labels = mo.synthetic_cells(50000, n_dims=50, seed=0)
    samples, dens, G = mo.fit_transform(X, labels, knn=15, beta=60, chebyshev_order=30, return_graph=True,
                                        algorithm="brute", n_jobs=-1)
    op = meld_amd.MELD(knn=15, beta=60, chebyshev_order=30, lmax=G.lmax)
    out = op.fit_transform(X, labels)
    assert list(out.columns) == list(samples)
    assert op.graph.info["wave_tiles_done"] < (50000 / 64) ** 2  # the pruned search was the one that ran
    _csr_close(op.graph.W, G.W, rtol=1e-9)
    np.testing.assert_allclose(op.graph.dw, G.dw, rtol=1e-9)
    assert _rel(out.values, dens) < 1e-5


@pytest.mark.parametrize("search,nprod", [("f16x3", 1), ("f16x3", 3), ("f32", 3)])
def test_query_ranges_compose_to_the_full_graph(search, nprod):
    """What a rank of the row-sharded driver computes (queries [r0, r0 + n) against all references)
    must be the corresponding rows of the single-range result, for ragged ranges that do not start
    at a tile or workgroup boundary."""
    from meld_amd.graph import HipOps

    mo = _oracle()
    N = 9000
    X, _ = mo.synthetic_cells(N, n_dims=24, seed=21)
    Xd = torch.from_numpy(X).cuda()
    ops = HipOps(search=search, nprod=nprod)
    keys, vals, bw, _ = ops.directed_kernel_coo(Xd, 0, N, 7, 40, 1e-4, 32)
    M = keys.shape[0] // 2
    full = dict(zip(keys[:M].tolist(), vals[:M].tolist()))
    got = {}
    for r0, n in ((0, 2999), (2999, 3002), (6001, 2999)):
        k, v, b, _ = ops.directed_kernel_coo(Xd, r0, n, 7, 40, 1e-4, 32)
        m = k.shape[0] // 2
        rows = (k[:m] >> 32)
        assert int(rows.min()) >= r0 and int(rows.max()) < r0 + n
        assert torch.equal((k[m:] & 0xFFFFFFFF), rows)  # transposed half: (j, i) of the same entries
        assert torch.equal(b, bw[r0 : r0 + n])
        got.update(zip(k[:m].tolist(), v[:m].tolist()))
    assert got == full


@pytest.mark.parametrize("n,d,knn", [(3000, 20, 9), (9000, 50, 5)])
def test_unweighted_knn_graph_decay_none(n, d, knn):
    """decay=None: graphtools' unweighted kNN graph (binary connectivity of the knn + 1 nearest, self
    included), symmetrised and anisotropy-normalised like the weighted one."""
    import meld_amd

    mo = _oracle()
    X, labels = mo.synthetic_cells(n, n_dims=d, seed=31)
    op = meld_amd.MELD(knn=knn, decay=None, verbose=0).fit(X)
    G = mo.build_graph(X, knn=knn, decay=None)
    W = op.graph.W
    assert W.nnz == G.W.nnz and abs(W - G.W).max() <= 1e-12
    # thresh = 0 with decay=None is still the kNN graph (graphtools' api.Graph looks at decay first): the same W
    W0 = meld_amd.MELD(knn=knn, decay=None, thresh=0, verbose=0).fit(X).graph.W
    assert W0.nnz == W.nnz and abs(W0 - W).max() == 0
    lmax = mo.estimate_lmax(G.L, G.dw)
    op.graph.lmax = lmax
    dens = op.transform(labels)
    ref = mo.meld_filter(mo.sample_indicators(labels)[1], G, beta=60, chebyshev_order=50, lmax=lmax)
    assert np.abs(dens.values - ref).max() <= 1e-5 * np.abs(ref).max()


@pytest.mark.parametrize("world", [2, 3])
def test_two_ranks_on_one_gpu(tmp_path, world):
    """All ranks of a 2- (3-) rank group run the real HIP kernels on this GPU (collectives staged through host
    memory over gloo, see tests/dist_worker_gpu.py): every rank must return the single-GPU result."""
    import socket
    import subprocess

    import meld_amd

    mo = _oracle()
    n, d, knn = 20011, 16, 9
    from tests.conftest import run_ranks

    out = str(tmp_path / "res")
    run_ranks("dist_worker_gpu.py", [out, n, d, knn], world)
    ranks = [np.load(out + ".rank{}.npz".format(r)) for r in range(world)]
    X, labels = mo.synthetic_cells(n, n_dims=d, seed=7)
    single = meld_amd.MELD(knn=knn, beta=40, chebyshev_order=25, verbose=0)
    ref = single.fit_transform(X, labels)
    per = -(-(-(-n // world)) // 256) * 256  # shards = whole search workgroups
    assert [int(r["row_begin"]) for r in ranks] == [min(i * per, n) for i in range(world)]
    assert int(ranks[0]["nnz_global"]) == single.graph.nnz
    assert bool(ranks[0]["device_resident"])  # the phase-wise Lanczos ran, not the host loop
    assert int(ranks[0]["all_reduces"]) == 1  # ... in its one-reduction form
    assert all(str(r["exchange"]) == "fixed" for r in ranks)  # meld_coo_partition_remote + one equal-split all-to-all
    assert all(bool(r["perm_equal"]) for r in ranks)  # sharded assignment passes of the ordering: same permutation
    for r in ranks:
        assert abs(float(r["lmax"]) - single.graph.lmax) <= 1e-9 * single.graph.lmax
        assert np.abs(r["dens"] - ref.values).max() <= 1e-9 * np.abs(ref.values).max()


@pytest.mark.parametrize("mode", ["vfc", "mnn", "unweighted"])
def test_two_ranks_on_one_gpu_vfc_and_graph_options(tmp_path, mode):
    """The sharded driver beyond the plain kNN graph, with the real HIP kernels on both ranks of a 2-rank group (collectives
    staged through host memory, tests/dist_worker_gpu.py): the filter-bank VertexFrequencyCluster (BASELINE configs[4]),
    sample_idx (MNN graph: built whole on every rank, rows sharded for the recurrences) and decay=None (unweighted kNN
    graph) -- every rank must return what one GPU computes alone."""
    import socket
    import subprocess

    import meld_amd

    mo = _oracle()
    n, d, knn, world = 20011, 16, 9, 2
    from tests.conftest import run_ranks

    out = str(tmp_path / "res")
    run_ranks("dist_worker_gpu.py", [out, n, d, knn, mode], world)
    ranks = [np.load(out + ".rank{}.npz".format(r)) for r in range(world)]
    X, labels = mo.synthetic_cells(n, n_dims=d, seed=7)
    kw = dict(sample_idx=np.random.default_rng(3).choice(["s0", "s1"], size=n)) if mode == "mnn" else {}
    single = meld_amd.MELD(knn=knn, beta=40, chebyshev_order=25, verbose=0, decay=None if mode == "unweighted" else 40, **kw)
    ref = single.fit_transform(X, labels)
    assert int(ranks[0]["nnz_global"]) == single.graph.nnz
    for r in ranks:
        assert abs(float(r["lmax"]) - single.graph.lmax) <= 1e-9 * single.graph.lmax
        assert np.abs(r["dens"] - ref.values).max() <= 1e-9 * np.abs(ref.values).max()
    if mode == "vfc":
        vfc = meld_amd.VertexFrequencyCluster(method="filterbank", n_probes=24, n_bands=6, window_sizes=np.array([1, 2, 4, 8]),
                                              chebyshev_order=48, random_state=3, n_clusters=3)
        vfc.fit(single.graph)
        spec = vfc._fb_spectrogram.cpu().numpy()
        assert spec.shape == (n, 24 + 6) and np.isfinite(spec).all()
        for r in ranks:
            np.testing.assert_array_equal(r["spec"], ranks[0]["spec"])  # every rank ends with the whole spectrogram
            assert np.abs(r["ritz"] - vfc._fb["ritz"].cpu().numpy()).max() < 1e-7 * single.graph.lmax
            assert np.abs(r["spec"] - spec).max() < 1e-6


@pytest.mark.parametrize("opts,n", [({"bandwidth_scale": 0.8, "knn_max": 14}, 20011), ({"kernel_symm": "mnn", "theta": 0.3}, 20011),
                                    ({"bandwidth": 0.9}, 20011), ({"thresh": 0}, 1500)])
def test_two_ranks_on_one_gpu_with_graph_keywords(tmp_path, opts, n):
    """graphtools' graph keywords on the row-sharded driver (reference meld/meld.py:106,117-118 forwards them): the builder does not
    shard these graphs itself -- every rank builds the graph whole with the single-GPU builder and keeps its rows, the filter is
    sharded.  Two ranks with the real HIP kernels (collectives staged through host memory): every rank returns what one GPU
    computes alone."""
    import json
    import socket
    import subprocess

    import meld_amd

    mo = _oracle()
    d, knn, world = 16, 9, 2
    from tests.conftest import run_ranks

    out = str(tmp_path / "res")
    run_ranks("dist_worker_gpu.py", [out, n, d, knn, "opt:" + json.dumps(opts)], world)
    ranks = [np.load(out + ".rank{}.npz".format(r)) for r in range(world)]
    X, labels = mo.synthetic_cells(n, n_dims=d, seed=7)
    kw = dict(opts)
    thresh = kw.pop("thresh", 1e-4)
    single = meld_amd.MELD(knn=knn, beta=40, chebyshev_order=25, verbose=0, thresh=thresh, **kw)
    ref = single.fit_transform(X, labels)
    assert [int(r["n_rows"]) for r in ranks] != [n, n]  # (the filter ran on row shards)
    assert sum(int(r["n_rows"]) for r in ranks) == n
    for r in ranks:
        assert abs(float(r["lmax"]) - single.graph.lmax) <= 1e-9 * single.graph.lmax
        assert np.abs(r["dens"] - ref.values).max() <= 1e-9 * np.abs(ref.values).max()


def test_locality_reordering_does_not_change_results():
    """The permutation is a memory-layout decision only: identical graph and densities (to
    rounding: summation order inside a row changes) with and without it."""
    mo = _oracle()
    import meld_amd

    X, labels = mo.synthetic_cells(12000, n_dims=50, seed=21)
    Xd = torch.from_numpy(X).cuda()
    A = meld_amd.build_knn_graph(Xd, knn=15, reorder=True)
    B = meld_amd.build_knn_graph(Xd, knn=15, reorder=False)
    assert A.perm is not None and B.perm is None
    _csr_close(A.W, B.W, rtol=1e-13)
    A.lmax = B.lmax = 0.11
    samples, ind = mo.sample_indicators(labels)
    from meld_amd.filter import filter as mfilter

    da = mfilter(ind, A, "heat", 60, chebyshev_order=30)
    db = mfilter(ind, B, "heat", 60, chebyshev_order=30)
    assert np.abs(da - db).max() / np.abs(db).max() < 1e-12


def test_tile_pruning_is_exact():
    """Skipping reference tiles by the bounding-sphere lower bound must not change a single
    candidate: identical graph with and without pruning, on clustered data in locality order
    (where most tiles are skipped) and on unordered data (where almost none are)."""
    mo = _oracle()
    import meld_amd
    from meld_amd.graph import HipOps
    from meld_amd.reorder import locality_permutation

    for dims, knn in ((50, 15), (3, 5)):  # (d <= 6 runs the full hi/lo split from the first pass)
        X, _ = mo.synthetic_cells(30000, n_dims=dims, seed=31)
        Xd = torch.from_numpy(X).cuda()
        for ordered in (True, False):
            Xs = Xd.index_select(0, locality_permutation(Xd)) if ordered else Xd
            outs = []
            # pruning and the radius cut (rows cut at the kernel radius their knn-th neighbour implies) are
            # independent switches of the search; the graph must not depend on either
            # (the last two: the seeded search without the per-query test of the table against the seeds, and without
            # the longest-first dispatch order of the query blocks)
            for prune, cut, seed, sb, bo in ((False, False, False, True, True), (True, False, False, True, True),
                                             (False, True, False, True, True), (True, True, False, True, True),
                                             (True, True, True, True, True), (False, True, True, True, True),
                                             (True, True, True, False, True), (True, True, True, True, False)):
                ops = HipOps(prune=prune)
                ops.radius_cut = cut
                ops.seed = seed  # thresholds started from every row's own block (meld_knn16_seed_thresholds_mfma)
                ops.seeded_bounds = sb
                ops.block_order = bo
                keys, vals, bw, info = ops.directed_kernel_coo(Xs, 0, 30000, knn, 40, 1e-4, 64)
                outs.append(ops.assemble_rows(keys, vals, 0, 30000, 30000) + (bw,))
            for other in outs[1:]:
                for a, b in zip(outs[0], other):
                    assert torch.equal(a, b)


@pytest.mark.parametrize("case", ["outliers", "duplicates", "offset", "tiny", "grid_ties", "isotropic"])
def test_pruning_and_radius_cut_on_awkward_data(case):
    """The pruned / radius-cut search against the plain one (bit for bit) on data that stresses the bounds:
    far outliers (huge error allowance), duplicated cells (zero-radius tiles, zero distances), a large offset,
    tiny scale, an integer grid (masses of exact distance ties at every threshold) and full-rank isotropic
    noise (nothing can be pruned)."""
    from meld_amd.graph import HipOps
    from meld_amd.reorder import locality_permutation

    rng = np.random.default_rng(7)
    N = 20000
    if case == "outliers":
        X = rng.normal(size=(N, 8))
        X[:5] *= 1000.0
    elif case == "duplicates":
        base = rng.normal(size=(N // 4, 5))
        X = np.concatenate([base, base, base[: N // 4], base[: N // 4] + 1e-9])
    elif case == "offset":
        X = rng.normal(size=(N, 10)) * 1.0e3 + 3.0e6
    elif case == "tiny":
        X = rng.normal(size=(N, 10)) * 1.0e-7
    elif case == "grid_ties":
        X = rng.integers(0, 12, size=(N, 4)).astype(np.float64)
    else:
        X = rng.normal(size=(N, 40))
    Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    perm = locality_permutation(Xd)
    Xd = Xd.index_select(0, perm).contiguous()
    knn = 5
    outs = []
    for prune, cut in ((False, False), (True, True)):
        ops = HipOps(prune=prune)
        ops.radius_cut = cut
        ops.seed = cut
        try:
            keys, vals, bw, info = ops.directed_kernel_coo(Xd, 0, N, knn, 40, 1e-4, 64)
        except Exception as e:  # (degenerate ties are refused loudly by both variants, never answered wrongly)
            outs.append(("raised", type(e).__name__))
            continue
        outs.append(ops.assemble_rows(keys, vals, 0, N, N) + (bw,))
    if outs[0][0] == "raised" or outs[1][0] == "raised":
        assert outs[0][0] == outs[1][0] == "raised", outs
        return
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_mfma_threshold_seeds_bound_the_kernel_radius():
    """meld_knn16_seed_thresholds_mfma: every seed is at least the squared kernel radius of its row (scaled units), so no
    wanted neighbour can fail `d2 < threshold`; and it is tight enough to be useful (within 3x of it in locality order)."""
    from meld_amd._lib import check, get_lib, ptr

    mo = _oracle()
    lib = get_lib()
    from meld_amd.reorder import locality_permutation

    N, d, knn = 16500, 50, 15
    X, _ = mo.synthetic_cells(N, n_dims=d, seed=8)
    Xd = torch.from_numpy(X).cuda()
    Xd = Xd.index_select(0, locality_permutation(Xd)).contiguous()  # blocks = spatial neighbourhoods, as in fit
    st = torch.cuda.current_stream().cuda_stream
    BQ = lib.meld_knn16_block_queries()
    sums = torch.empty(d, dtype=torch.float64, device="cuda")
    check(lib.meld_col_sums_f64(ptr(Xd), N, d, ptr(sums), st))
    mean = sums / N
    n_tiles = (N + 63) // 64
    q_pad = ((N + BQ - 1) // BQ) * BQ
    Rt = torch.empty(n_tiles * lib.meld_knn16_tile_bytes(d), dtype=torch.uint8, device="cuda")
    Q = torch.empty(q_pad * lib.meld_knn16_query_bytes(d), dtype=torch.uint8, device="cuda")
    Qn = torch.empty(q_pad, dtype=torch.float32, device="cuda")
    norm2 = torch.empty(N, dtype=torch.float32, device="cuda")
    nmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    sinfo = torch.empty(4, dtype=torch.float32, device="cuda")
    check(lib.meld_knn16_prepare(ptr(Xd), N, d, ptr(mean), 0, N, ptr(Rt), ptr(Q), ptr(Qn), ptr(norm2), ptr(nmax), ptr(sinfo), st))
    rf = (-np.log(1e-4)) ** (1 / 40)
    torch.cuda.synchronize()
    s2 = float(sinfo[0]) ** 2
    D = torch.cdist(Xd, Xd)
    bw = torch.kthvalue(D, knn + 1, dim=1).values  # true bandwidth (self counted)
    radius2 = ((bw * rf) ** 2 * s2).to(torch.float32)
    # no seed where the register lists cannot hold knn + 1 entries (knn + 1 > 64): every row +inf, the padding rows of the last
    # block included (the padding queries of the operands repeat the last cell, so a seeded launch gives them that cell's seed)
    seeds2 = torch.zeros(q_pad, dtype=torch.float32, device="cuda")
    check(lib.meld_knn16_seed_thresholds_mfma(ptr(Q), ptr(Qn), ptr(Rt), ptr(sinfo), ptr(nmax), N, d, 0, N, 64, rf, 1, 0, ptr(seeds2), st))
    torch.cuda.synchronize()
    assert bool(torch.isinf(seeds2).all())
    # the matrix-pipe version over the own tiles and four on either side (the default of the graph builder)
    seeds2 = torch.empty(q_pad, dtype=torch.float32, device="cuda")
    prev = None
    for side in (0, 4, 16):  # (0 = automatic; a wider neighbourhood can only lower a seed)
        check(lib.meld_knn16_seed_thresholds_mfma(ptr(Q), ptr(Qn), ptr(Rt), ptr(sinfo), ptr(nmax), N, d, 0, N, knn, rf, 1, side, ptr(seeds2), st))
        torch.cuda.synchronize()
        got2 = seeds2[:N].clone()
        assert bool((got2 >= radius2).all())
        assert float((got2 / radius2).median()) < 3.0
        if side == 16:
            assert bool((got2 <= prev).all())
        prev = got2


def test_pruned_search_on_shard_ranges():
    """A rank of the sharded driver searches a tile-aligned query range against all references with its own
    slice of the pruning table: same rows as the unpruned full-range search (ragged last range included)."""
    from meld_amd.graph import HipOps
    from meld_amd.reorder import locality_permutation

    mo = _oracle()
    N = 40000
    X, _ = mo.synthetic_cells(N, n_dims=50, seed=33)
    Xd = torch.from_numpy(X).cuda()
    Xd = Xd.index_select(0, locality_permutation(Xd)).contiguous()
    plain = HipOps(prune=False)
    plain.radius_cut = False
    keys, vals, bw, _ = plain.directed_kernel_coo(Xd, 0, N, 15, 40, 1e-4, 64)
    M = keys.shape[0] // 2
    full = dict(zip(keys[:M].tolist(), vals[:M].tolist()))
    ops = HipOps(prune=True)
    got = {}
    for r0, n in ((0, 13568), (13568, 13568), (27136, N - 27136)):
        k, v, b, info = ops.directed_kernel_coo(Xd, r0, n, 15, 40, 1e-4, 64)
        m = k.shape[0] // 2
        assert torch.equal(b, bw[r0 : r0 + n])
        assert info["wave_tiles_done"] < 0.9 * ((n + 63) // 64) * ((N + 63) // 64)  # tiles really were skipped
        got.update(zip(k[:m].tolist(), v[:m].tolist()))
    assert got == full


def test_knn16_reference_slices_merge_to_the_same_rows():
    """Cutting the references into slices + meld_knn16_merge_slices == one full scan."""
    mo = _oracle()
    from meld_amd._lib import check, get_lib, ptr

    lib = get_lib()
    X, _ = mo.synthetic_cells(2500, n_dims=50, seed=17)
    N, d = X.shape
    Xd = torch.from_numpy(X).cuda()
    st = torch.cuda.current_stream().cuda_stream
    KB, TS, BQ = lib.meld_knn16_kblocks(d), lib.meld_knn16_tile_refs(), lib.meld_knn16_block_queries()
    ksel = 64
    cap = lib.meld_knn16_row_capacity(ksel)
    sums = torch.empty(d, dtype=torch.float64, device="cuda")
    check(lib.meld_col_sums_f64(ptr(Xd), N, d, ptr(sums), st))
    mean = sums / N
    n_tiles = (N + TS - 1) // TS
    nq = 700  # a subset of the rows as queries, through the row-list form
    rows = torch.arange(100, 100 + nq, dtype=torch.int32, device="cuda")
    q_pad = ((nq + BQ - 1) // BQ) * BQ
    Rt = torch.empty(n_tiles * lib.meld_knn16_tile_bytes(d), dtype=torch.uint8, device="cuda")
    Qall = torch.empty(((N + BQ - 1) // BQ) * BQ * lib.meld_knn16_query_bytes(d), dtype=torch.uint8, device="cuda")
    Qnall = torch.empty(((N + BQ - 1) // BQ) * BQ, dtype=torch.float32, device="cuda")
    norm2 = torch.empty(N, dtype=torch.float32, device="cuda")
    nmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    sinfo = torch.empty(4, dtype=torch.float32, device="cuda")
    check(lib.meld_knn16_prepare(ptr(Xd), N, d, ptr(mean), 0, N, ptr(Rt), ptr(Qall), ptr(Qnall), ptr(norm2), ptr(nmax), ptr(sinfo), st))
    Q = torch.empty(q_pad * lib.meld_knn16_query_bytes(d), dtype=torch.uint8, device="cuda")
    Qn = torch.empty(q_pad, dtype=torch.float32, device="cuda")
    check(lib.meld_knn16_prepare_rows(ptr(Xd), N, d, ptr(mean), ptr(sinfo), 0, ptr(rows), nq, ptr(Q), ptr(Qn), st))
    res = {}
    for S in (1, 3):
        ci = torch.zeros(S * q_pad * cap, dtype=torch.int32, device="cuda")
        cd = torch.zeros(S * q_pad * cap, dtype=torch.float32, device="cuda")
        cc = torch.zeros(S * q_pad, dtype=torch.int32, device="cuda")
        check(lib.meld_knn16_topk(ptr(Q), ptr(Qn), ptr(Rt), ptr(sinfo), N, d, nq, ksel, 3, S, None, ptr(nmax), 0, None, 0, 1.0, ptr(ci), ptr(cd), ptr(cc), None, None, None, st))
        if S > 1:
            mi = torch.zeros(q_pad * cap, dtype=torch.int32, device="cuda")
            md = torch.zeros(q_pad * cap, dtype=torch.float32, device="cuda")
            mc = torch.zeros(q_pad, dtype=torch.int32, device="cuda")
            check(lib.meld_knn16_merge_slices(ptr(ci), ptr(cd), ptr(cc), nq, ksel, S, ptr(mi), ptr(md), ptr(mc), st))
            ci, cd, cc = mi, md, mc
        torch.cuda.synchronize()
        res[S] = (ci.view(-1, cap)[:nq, :ksel].clone(), cd.view(-1, cap)[:nq, :ksel].clone(), cc[:nq].clone())
    for a, b in zip(res[1], res[3]):
        assert torch.equal(a, b)
    # row 0 of the subset is global row 100: its nearest candidate is itself
    assert int(res[1][0][0, 0]) == 100


def test_partition_of_remote_entries_matches_numpy():
    """meld_coo_partition_remote: every entry owed to another rank lands in that rank's segment exactly once (keys and
    value bits side by side), own entries are left out, unused slots carry the sentinel key, counts say what was owed
    even when it did not fit."""
    import meld_amd
    from meld_amd.graph import HipOps

    ops = HipOps()
    rng = np.random.default_rng(3)
    n, R, world, rank = 200000, 4096, 5, 2
    rows = rng.integers(0, R * world - 100, n)
    cols = rng.integers(0, R * world, n)
    keys = torch.from_numpy((rows << 32) | cols).cuda()
    vals = torch.from_numpy(rng.normal(size=n)).cuda()
    owner = np.minimum(rows // R, world - 1)
    for cap in (65536, 1000):
        send, counts = ops.partition_remote(keys, vals, R, world, rank, cap)
        send = send.cpu().numpy().reshape(world, 2, cap)
        counts = counts.cpu().numpy()
        for o in range(world):
            want = np.nonzero(owner == o)[0] if o != rank else np.empty(0, dtype=np.int64)
            assert counts[o] == want.shape[0]
            got_k, got_v = send[o, 0], send[o, 1].view(np.float64)
            used = got_k != -1
            assert used.sum() == min(want.shape[0], cap)
            pairs = set(zip(keys.cpu().numpy()[want].tolist(), vals.cpu().numpy()[want].tolist()))
            assert set(zip(got_k[used].tolist(), got_v[used].tolist())) <= pairs
            if want.shape[0] <= cap:
                assert len(set(zip(got_k[used].tolist(), got_v[used].tolist()))) == len(pairs)


@pytest.mark.parametrize("n,d,npg,n_groups", [(20000, 50, 64, 1), (30011, 50, 32, 37), (5000, 7, 13, 300), (9000, 128, 64, 5)])
def test_assign_nearest_on_the_matrix_pipe_matches_brute_force(n, d, npg, n_groups):
    """meld_assign_nearest (|c|^2 - 2 x.c on the fp32 MFMA): every point gets its nearest centroid of its group; where it
    differs from an fp64 brute force the two distances are a near-tie (fp32 products, keys without their low 6 bits)."""
    from meld_amd._lib import check, get_lib, ptr

    lib = get_lib()
    rng = np.random.default_rng(n + d)
    X = rng.normal(size=(n, d)) * 3.0 + rng.normal(size=(1, d))
    cents = rng.normal(size=(n_groups * npg, d)) * 3.0
    Xd, Cd = torch.from_numpy(X).cuda(), torch.from_numpy(cents).cuda()
    out = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if n_groups == 1:
        grp = np.zeros(n, dtype=np.int64)
        check(lib.meld_assign_nearest(ptr(Xd), n, d, ptr(Cd), npg, None, None, ptr(out), st), "meld_assign_nearest")
    else:
        sizes = rng.multinomial(n - n_groups, np.ones(n_groups) / n_groups) + 1  # ragged groups, none empty
        sizes[3] += sizes[4] - 1
        sizes[4] = 1
        grp = rng.permutation(np.repeat(np.arange(n_groups), sizes))
        g32 = torch.from_numpy(grp.astype(np.int32)).cuda()
        order = torch.from_numpy(np.argsort(grp, kind="stable")).cuda()
        check(lib.meld_assign_nearest(ptr(Xd), n, d, ptr(Cd), npg, ptr(g32), ptr(order), ptr(out), st), "meld_assign_nearest")
    got = out.cpu().numpy().astype(np.int64)
    assert got.min() >= 0 and got.max() < npg
    C = cents.reshape(n_groups, npg, d)[grp]                    # [n, npg, d]
    d2 = ((X[:, None, :] - C) ** 2).sum(-1)
    best = d2.argmin(1)
    diff = np.nonzero(best != got)[0]
    assert diff.shape[0] < 0.002 * n
    scale = (X ** 2).sum(1) + (C ** 2).sum(-1).max(1)
    assert np.all(d2[diff, got[diff]] - d2[diff, best[diff]] <= 2e-5 * scale[diff])


def test_ordering_glue_kernels_match_numpy():
    """meld_argsort_u32 (stable, over the key bits only), meld_order_starts, meld_order_pick_centroids and
    meld_order_update_keys against their NumPy definitions, groups of every size including empty ones."""
    from meld_amd._lib import check, get_lib, ptr

    lib = get_lib()
    rng = np.random.default_rng(11)
    n, d, n_groups, f = 70001, 9, 300, 7
    key = rng.integers(0, n_groups - 5, n).astype(np.int32)  # (the last groups stay empty)
    key[key == 17] = 18                                       # ... and one in the middle
    X = rng.normal(size=(n, d))
    st = torch.cuda.current_stream().cuda_stream
    kd, Xd = torch.from_numpy(key).cuda(), torch.from_numpy(X).cuda()
    order = torch.empty(n, dtype=torch.int64, device="cuda")
    skeys = torch.empty(n, dtype=torch.int32, device="cuda")
    tb = lib.meld_argsort_u32_temp_bytes(n)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    check(lib.meld_argsort_u32(ptr(kd), n, int(n_groups - 1).bit_length(), ptr(order), ptr(skeys), ptr(tmp), tb, st), "argsort")
    want = np.argsort(key, kind="stable")
    np.testing.assert_array_equal(order.cpu().numpy(), want)
    np.testing.assert_array_equal(skeys.cpu().numpy(), key[want])
    starts = torch.empty(n_groups + 1, dtype=torch.int64, device="cuda")
    check(lib.meld_order_starts(ptr(skeys), n, n_groups, ptr(starts), st), "starts")
    s_np = np.searchsorted(key[want], np.arange(n_groups + 1), side="left")
    np.testing.assert_array_equal(starts.cpu().numpy(), s_np)
    cents = torch.empty(n_groups * f, d, dtype=torch.float64, device="cuda")
    check(lib.meld_order_pick_centroids(ptr(Xd), n, d, ptr(order), ptr(starts), n_groups, f, ptr(cents), st), "picks")
    cnt = np.diff(s_np)
    frac = (np.arange(f) + 0.5) / f
    pick = s_np[:-1, None] + (frac[None, :] * cnt[:, None]).astype(np.int64)
    pick = np.minimum(pick, (s_np[:-1] + np.maximum(cnt - 1, 0))[:, None]).clip(0, n - 1)
    np.testing.assert_array_equal(cents.cpu().numpy(), X[want[pick.reshape(-1)]])
    child = rng.integers(0, f, n).astype(np.int32)
    rank = np.stack([rng.permutation(f) for _ in range(n_groups)]).astype(np.int32)
    cd, rd = torch.from_numpy(child).cuda(), torch.from_numpy(rank.reshape(-1)).cuda()
    check(lib.meld_order_update_keys(ptr(kd), ptr(cd), ptr(rd), n, f, st), "update")
    np.testing.assert_array_equal(kd.cpu().numpy(), key * f + rank[key, child])


def test_direct_step_lists_equal_the_table_driven_ones():
    """meld_knn16_step_lists_direct (bounds kept as two bits per (wave, tile), transposed and ANDed) must write the lists
    meld_knn16_bounds + meld_knn16_step_lists write from the symmetrised fp16 table: same counts, same entries; and the graph
    built on them is the graph of the table-driven search."""
    mo = _oracle()
    import meld_amd

    X, _ = mo.synthetic_cells(400000, n_dims=50, seed=5)  # (enough query blocks for the list-driven pass: 2 x the resident workgroups)
    Xd = torch.from_numpy(X).cuda()
    graphs = {}
    # (in the principal frame the direct lists take their bounds from the first K block of the operands alone -- lower bounds all the
    # same, a few more blocks computed: "lead"; MELD_KNN16_LEAD_BOUNDS=0 gives them the full distances the table is built from)
    for direct, lead in (("1", "0"), ("0", "0"), ("1", "1")):
        os.environ["MELD_KNN_LIST_DIRECT"] = direct
        os.environ["MELD_KNN16_LEAD_BOUNDS"] = lead
        try:
            graphs[direct if lead == "0" else "lead"] = meld_amd.build_knn_graph(Xd, knn=15)
        finally:
            os.environ.pop("MELD_KNN_LIST_DIRECT", None)
            os.environ.pop("MELD_KNN16_LEAD_BOUNDS", None)
        assert graphs[direct if lead == "0" else "lead"].info["step_lists"]
    A, B, L = graphs["1"], graphs["0"], graphs["lead"]
    assert torch.equal(A.rowptr, L.rowptr) and torch.equal(A.col, L.col) and torch.equal(A.val, L.val)
    assert 0 <= L.info["wave_tiles_done"] - A.info["wave_tiles_done"] <= 0.02 * A.info["wave_tiles_done"]
    assert torch.equal(A.rowptr, B.rowptr) and torch.equal(A.col, B.col) and torch.equal(A.val, B.val)
    # the same (wave, tile) blocks were computed -- except by the padding waves of the last query block (128 padding queries here),
    # which the direct lists leave out of every step and the table keeps at whatever their padding seeds say
    n_tiles = -(-400000 // 64)
    pad_waves = (-(-400000 // 256) * 256 - 400000) // 64
    assert 0 <= B.info["wave_tiles_done"] - A.info["wave_tiles_done"] <= pad_waves * n_tiles
