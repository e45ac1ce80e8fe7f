"""Partial Fourier basis on the GPU: ``DeviceGraph.compute_fourier_basis(n_eigenvectors=k)`` / ``fourier_basis`` /
``fourier_basis_device`` (meld_amd/spectrum.py) against dense and shift-invert host eigensolvers, and the three block kernels
of csrc/subspace.hip against NumPy through ``HipOps``."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-6  # the default
EPS = float(np.finfo(np.float64).eps)


def _mixture(n, d=5, seed=0):
    rng = np.random.default_rng(seed)
    cent = 3.0 * rng.normal(size=(5, d))
    return cent[rng.integers(0, 5, n)] + rng.normal(size=(n, d))


def _graph(X, knn):
    import torch

    import meld_amd

    return meld_amd.build_knn_graph(torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).cuda(), knn=knn)


def _ub(G):
    from meld_amd.spectrum import upper_bound

    return upper_bound(G)[0]


def _check_pairs(L, e, U, e_ref, ub):
    k = e.shape[0]
    assert e.shape == (k,) and U.shape == (L.shape[0], k) and e.dtype == np.float64 and U.dtype == np.float64
    assert np.all(np.diff(e) >= 0)
    err = np.abs(e - e_ref[:k]).max()
    res = np.linalg.norm(L @ U - U * e[None, :], axis=0).max()
    orth = np.abs(U.T @ U - np.eye(k)).max()
    print("k={} |e - e_ref|/ub={:.3e} residual/ub={:.3e} max|U^T U - I|={:.3e}".format(k, err / ub, res / ub, orth))
    assert err <= TOL * ub
    assert res <= 2 * TOL * ub
    assert orth <= 1e-10
    # sign convention: the entry of largest magnitude of every column is positive, the lowest row wins a tie
    for j in range(k):
        assert U[np.argmax(np.abs(U[:, j])), j] > 0


@pytest.fixture(scope="module")
def mix3001():
    G = _graph(_mixture(3001), knn=7)
    L = G.L
    return G, L, np.linalg.eigvalsh(L.toarray())


@pytest.mark.parametrize("k", [1, 5, 33, 48])
def test_against_dense_eigh(mix3001, k):
    G, L, e_ref = mix3001
    assert G.N == 3001 and G.N % 64 != 0
    assert G.compute_fourier_basis(n_eigenvectors=k) is None
    e, U = G.fourier_basis(k)
    assert G.fourier_partial_info["iterations"] >= 1 and G.fourier_partial_info["block"] == 64
    _check_pairs(L, e, U, e_ref, _ub(G))
    assert G.fourier_basis(k)[1] is U  # kept per (k, tol, seed)


def test_disconnected_graph_counts_its_components():
    from scipy.sparse.csgraph import connected_components

    from tests.golden.make_golden import make_batches

    X, _ = make_batches(100)  # six well-separated blobs
    G = _graph(X, knn=5)
    n_comp = connected_components(G.W, directed=False)[0]
    assert 1 < n_comp < 8  # (6 with the oracle's graph of the same cells)
    e, U = G.fourier_basis(8)
    assert int((e <= TOL * _ub(G)).sum()) == n_comp
    L = G.L
    assert np.linalg.norm(L @ U - U * e[None, :], axis=0).max() <= 2 * TOL * _ub(G)


def test_rows_are_in_the_callers_order_under_the_locality_permutation():
    from scipy.sparse.linalg import eigsh

    n, k = 8192, 6  # the smallest size the locality permutation reorders (meld_amd/reorder.py)
    G = _graph(_mixture(n, seed=1), knn=7)
    assert G.perm is not None
    ub = _ub(G)
    e, U = G.fourier_basis(k)
    L = G.L  # host export, caller's order
    e_ref = np.sort(eigsh(L.tocsc(), k, sigma=-1e-3 * ub, which="LM", return_eigenvectors=False))
    _check_pairs(L, e, U, e_ref, ub)


def test_determinism_and_isolation():
    import torch

    X = _mixture(700, seed=2)
    G = _graph(X, knn=7)
    assert G._lmax is None and G.lmax_info == {}
    e1, U1 = (a.copy() for a in G.fourier_basis(6))
    assert G._lmax is None and G.lmax_info == {}  # no estimate left behind
    e2, U2 = G.fourier_basis(6, recompute=True)
    assert np.array_equal(e1, e2) and np.array_equal(U1, U2)
    ed, Ud = G.fourier_basis_device(6)
    assert ed.is_cuda and Ud.is_cuda and Ud.shape == (700, 6)
    assert np.array_equal(ed.cpu().numpy(), e2) and np.array_equal(Ud.cpu().numpy(), U2)
    # an injected lmax is neither used (far too small here: a filter that trusted it would diverge) nor changed
    H = _graph(X, knn=7)
    H.lmax = 1e-3
    e3, U3 = H.fourier_basis(6)
    assert H._lmax == 1e-3 and H.lmax_info == {"method": "injected"}
    assert H.fourier_partial_info["ub_rule"] == "gershgorin" and np.abs(e3 - e1).max() <= TOL * _ub(H)
    # ... and a Lanczos estimate is used as it is
    K = _graph(X, knn=7)
    lm = K.estimate_lmax()
    info = dict(K.lmax_info)
    K.compute_fourier_basis(n_eigenvectors=6)
    assert K.fourier_partial_info["ub_rule"] == "lanczos" and K.fourier_partial_info["ub"] == lm
    assert K._lmax == lm and K.lmax_info == info
    # the full basis is still the full basis
    assert getattr(G, "_U", None) is None
    assert G.U.shape == (700, 700) and G.e.shape == (700,)
    assert np.abs(G.e[:6] - e1).max() <= TOL * _ub(H)
    assert torch.equal(G.fourier_basis_device(6)[1], Ud)


def test_refusals_and_the_dense_slice():
    G = _graph(_mixture(100, seed=3), knn=5)
    with pytest.raises(ValueError, match=r"\[1, 48\]"):
        G.compute_fourier_basis(n_eigenvectors=0)
    with pytest.raises(ValueError, match=r"\[1, 48\]"):
        G.fourier_basis(49)
    with pytest.raises(TypeError, match="integer"):
        G.fourier_basis(2.5)
    e, U = G.fourier_basis(10)
    assert G.fourier_partial_info["method"] == "dense" and G._lmax is None and getattr(G, "_U", None) is None
    L = G.L
    w, Q = np.linalg.eigh(L.toarray())
    ub = _ub(G)
    # a dense decomposition: backward error ~ N eps |L|
    assert np.abs(e - w[:10]).max() <= 1e-12 * ub
    assert np.linalg.norm(L @ U - U * e[None, :], axis=0).max() <= 1e-12 * ub
    assert np.abs(U.T @ U - np.eye(10)).max() <= 1e-12
    for j in range(10):
        assert U[np.argmax(np.abs(U[:, j])), j] > 0
    # non-convergence is an error that states the residual, and nothing is kept
    B = _graph(_mixture(700, seed=2), knn=7)
    with pytest.raises(RuntimeError, match=r"worst residual .* > tol \* ub"):
        B.fourier_basis(6, max_iter=0)
    assert not B._partial_fourier


@pytest.mark.parametrize("m", [1, 2, 33, 64])
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 4097])
def test_block_kernel_contracts(n_rows, m):
    """meld_block_gram_f64 / _rotate_f64 / _residuals_f64 through HipOps, tight (ld = m) and padded (ld = m + 3) rows.  The padding
    holds NaN on the way in (a NaN in a result: it was read) and a sentinel on the way out (it must survive)."""
    import torch

    from meld_amd.graph import HipOps

    ops = HipOps(torch.device("cuda"))
    rng = np.random.default_rng(1000 * n_rows + m)
    A, B = rng.normal(size=(n_rows, m)), rng.normal(size=(n_rows, m))
    S = rng.normal(size=(m, m))
    theta = rng.normal(size=m)
    ld_ref = np.longdouble
    gram_ref = (A.astype(ld_ref).T @ B.astype(ld_ref)).astype(np.float64)
    gram_tol = n_rows * EPS * np.outer(np.linalg.norm(A, axis=0), np.linalg.norm(B, axis=0))
    rot_ref = (A.astype(ld_ref) @ S.astype(ld_ref)).astype(np.float64)
    rot_tol = m * EPS * (np.abs(A) @ np.abs(S))
    res_ref = (((A.astype(ld_ref) - theta.astype(ld_ref)[None, :] * B.astype(ld_ref)) ** 2).sum(0)).astype(np.float64)
    # every term d = lv - theta v carries <= eps (|lv| + |theta v|) =: eps s, its square 2 |d| eps s + eps d^2, the sum n eps / 2 more
    res_tol = (n_rows + 2) * EPS * ((np.abs(A) + np.abs(theta)[None, :] * np.abs(B)) ** 2).sum(0)
    for ld in (m, m + 3):
        def dev(a, fill):
            t = torch.full((a.shape[0], ld), fill, dtype=torch.float64, device="cuda")
            t[:, :m] = torch.from_numpy(a).cuda()
            return t

        Ad, Bd = dev(A, float("nan")), dev(B, float("nan"))
        nb = ops.block_n_blocks(n_rows)
        assert 1 <= nb <= ops.lib.meld_block_max_blocks()
        part = torch.empty(nb * m * m, dtype=torch.float64, device="cuda")
        C = [torch.full((m, m), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)]
        for c in C:
            ops.block_gram(Ad, Bd, n_rows, m, part, nb, c)
        assert torch.equal(C[0], C[1])  # the same bits every run
        assert np.all(np.abs(C[0].cpu().numpy() - gram_ref) <= gram_tol)
        # rotation, into another block and in place
        Sd = torch.from_numpy(S).cuda()
        out = torch.full((n_rows, ld), 7.5, dtype=torch.float64, device="cuda")
        ops.block_rotate(Ad, Sd, n_rows, m, out)
        assert np.all(np.abs(out[:, :m].cpu().numpy() - rot_ref) <= rot_tol) and bool((out[:, m:] == 7.5).all())
        Ac = dev(A, 7.5)
        ops.block_rotate(Ac, Sd, n_rows, m, Ac)
        assert torch.equal(Ac[:, :m], out[:, :m]) and bool((Ac[:, m:] == 7.5).all())
        # residuals (LV = A, V = B)
        r = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
        ops.block_residuals(Ad, Bd, torch.from_numpy(theta).cuda(), n_rows, m, part, nb, r)
        assert np.all(np.abs(r.cpu().numpy() - res_ref) <= res_tol)
    # more partial slots than rows, and a single one: the same contract
    for nb in (1, 7):
        part = torch.empty(nb * m * m, dtype=torch.float64, device="cuda")
        c = torch.empty(m, m, dtype=torch.float64, device="cuda")
        ops.block_gram(Ad, Bd, n_rows, m, part, nb, c)
        assert np.all(np.abs(c.cpu().numpy() - gram_ref) <= gram_tol)
    # the entry points check their arguments before any launch
    assert ops.lib.meld_block_gram_f64(None, m, None, m, n_rows, m, None, 1, None, None) == -1
    assert ops.lib.meld_block_rotate_f64(Ad.data_ptr(), m - 1, Sd.data_ptr(), n_rows, m, out.data_ptr(), m, None) == -1
    assert ops.lib.meld_block_residuals_f64(Ad.data_ptr(), Bd.data_ptr(), m, r.data_ptr(), n_rows, 65, part.data_ptr(), 1, r.data_ptr(), None) == -1
