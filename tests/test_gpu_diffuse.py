"""Diffusion of cell signals on the device (meld_amd/diffuse.py, csrc/diffuse.hip) against scipy: ``P = G.diff_op`` on the host,
``ref = P @ (... @ F)``.

Tolerance, derived: ``P`` is row-stochastic and non-negative, so a step never amplifies an error; a step of a row with ``m`` entries
commits at most ``(m + 3) 2^-53 max|x|`` (m products and sums, the diagonal term, the division), and scipy's own sums the same.
After ``t`` steps ``|device - host| <= 2 t (m_max + 3) 2^-53 max|F|``, with ``m_max`` read from the graph's ``rowptr``.

Geometry of ``diffuse_step_kernel``: 8 consecutive rows per wave, 32 per workgroup (as ``cheby_step_wide_kernel``), lanes = columns
with a second column per lane beyond 64 and a panel per 128: N in {1, 31, 32, 33, 257, 4097} straddles the row boundaries, p in
{63, 64, 65, 127, 128, 129, 257} the column ones; N = 100 003 wraps the XCD interleaving of the workgroups many times."""
import numpy as np
import pytest
import torch
from scipy import sparse

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
P_MAX = 257


def _path(n):
    i = np.arange(n - 1)
    w = np.random.default_rng(n).uniform(0.1, 1.0, n - 1)
    W = sparse.coo_matrix((np.r_[w, w], (np.r_[i, i + 1], np.r_[i + 1, i])), shape=(n, n)).tocsr()
    W.sort_indices()
    return W


def _star(n):
    j = np.arange(1, n)
    w = np.random.default_rng(n + 1).uniform(0.1, 1.0, n - 1)
    hub = n // 3  # (not the first row)
    j[j == hub] = 0
    W = sparse.coo_matrix((np.r_[w, w], (np.r_[np.full(n - 1, hub), j], np.r_[j, np.full(n - 1, hub)])), shape=(n, n)).tocsr()
    W.sort_indices()
    return W


def _random(n, seed, dyadic=False):
    """About 12 entries per row among the connected vertices, and up to 50 isolated ones (rows without entries: y = x).
    ``dyadic``: weights k / 1024, so that every sum of a row's weights is exact in any order."""
    rng = np.random.default_rng(seed)
    iso = min(50, n // 4)
    live = rng.permutation(n)[: n - iso]
    if live.size < 2:
        return sparse.csr_matrix((n, n))
    a, b = rng.choice(live, 12 * live.size), rng.choice(live, 12 * live.size)
    keep = a < b
    a, b = a[keep], b[keep]
    w = rng.integers(1, 1025, a.size) / 1024.0 if dyadic else rng.uniform(0.05, 1.0, a.size)
    A = sparse.coo_matrix((w, (a, b)), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A = sparse.triu(A, k=1)
    W = (A + A.T).tocsr()
    W.sort_indices()
    return W


_MAKERS = {"path": _path, "star": _star, "random": lambda n: _random(n, 100 + n), "dyadic": lambda n: _random(n, 200 + n, dyadic=True)}
_CACHE = {}


def _case(kind, n):
    """One graph, its host operator, a seeded signal of P_MAX columns and the reference powers computed so far (shared by the
    tests, never changed)."""
    key = (kind, n)
    if key not in _CACHE:
        from meld_amd.graph import DeviceGraph

        W = _MAKERS[kind](n)
        G = DeviceGraph.from_scipy(W)
        m_max = int(np.diff(G.rowptr.cpu().numpy()).max()) if n else 0
        F = np.random.default_rng(7 * n + len(kind)).standard_normal((n, P_MAX))
        _CACHE[key] = dict(G=G, W=W, P=G.diff_op, m_max=m_max, F=F, F_dev=torch.from_numpy(F).cuda(), refs={0: F})
    return _CACHE[key]


def _ref(c, t, p):
    """``P^t F[:, :p]`` on the host (columns are independent: the powers are kept for the widest request so far)."""
    refs = c["refs"]
    have = max(k for k in refs if k <= t and refs[k].shape[1] >= p)
    cur = refs[have][:, :p]
    for k in range(have, t):
        cur = c["P"] @ cur
        if k + 1 not in refs or refs[k + 1].shape[1] < p:
            refs[k + 1] = cur
    return cur


def _bound(c, t, fmax):
    return 2 * t * (c["m_max"] + 3) * U * fmax


def _check(c, p, t):
    F = c["F_dev"][:, :p].contiguous()
    out = c["G"].diffuse_device(F, t=t)
    assert out.dtype == torch.float64 and tuple(out.shape) == tuple(F.shape)
    ref = _ref(c, t, p)
    err = float(np.abs(out.cpu().numpy() - ref).max()) if ref.size else 0.0
    tol = _bound(c, t, float(np.abs(c["F"][:, :p]).max()))
    print("N={} p={} t={}: |device - host| = {:.3e}, bound {:.3e}".format(c["F"].shape[0], p, t, err, tol))
    if t == 0:
        assert torch.equal(out, F) and out.data_ptr() != F.data_ptr()
    assert err <= tol


# 1. step and powers against scipy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0, 1, 2, 5])
@pytest.mark.parametrize("p", [1, 2, 63, 64, 65, 100, 127, 128, 129, 200, 257])
def test_powers_on_the_random_graph(p, t):
    _check(_case("random", 4097), p, t)


@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("p", [1, 65, 129])
@pytest.mark.parametrize("kind,n", [("path", n) for n in (1, 31, 32, 33, 257, 4097)] + [("random", n) for n in (1, 31, 32, 33, 257)]
                         + [("star", 4097), ("random", 100003)])
def test_powers_on_the_other_graphs(kind, n, p, t):
    c = _case(kind, n)
    if kind == "star":
        assert c["m_max"] == n - 1 and int(np.diff(c["W"].indptr).min()) == 1
    _check(c, p, t)


def test_one_dimensional_and_host_input():
    c = _case("random", 4097)
    G = c["G"]
    out = G.diffuse_device(c["F_dev"][:, 5], t=2)
    assert tuple(out.shape) == (4097,)
    assert np.abs(out.cpu().numpy() - _ref(c, 2, 6)[:, 5]).max() <= _bound(c, 2, float(np.abs(c["F"][:, 5]).max()))
    host = G.diffuse(c["F"][:, :3], t=2)
    assert isinstance(host, np.ndarray) and np.array_equal(host, G.diffuse_device(c["F_dev"][:, :3], t=2).cpu().numpy())
    import pandas as pd

    df = pd.DataFrame(c["F"][:, :3], index=["c%d" % i for i in range(4097)], columns=["a", "b", "c"])
    back = G.diffuse(df, t=2)
    assert isinstance(back, pd.DataFrame) and list(back.index) == list(df.index) and list(back.columns) == ["a", "b", "c"]
    assert np.array_equal(back.values, host)


# 2. columns do not see each other -------------------------------------------------------------------------------------------------
def test_columns_are_independent_and_runs_repeat():
    c = _case("random", 4097)
    G, F = c["G"], c["F_dev"]
    wide = G.diffuse_device(F[:, :257], t=2)
    assert torch.equal(wide, G.diffuse_device(F[:, :257], t=2))  # the same bits every run
    for j in (0, 63, 64, 127, 128, 200, 256):
        assert torch.equal(wide[:, j], G.diffuse_device(F[:, j], t=2)), j


# 3. leading dimensions -----------------------------------------------------------------------------------------------------------
def test_leading_dimensions_through_the_c_entry():
    from meld_amd import _lib
    from meld_amd.diffuse import walk_vectors

    c = _case("random", 4097)
    G = c["G"]
    N, ld, p, off = 4097, 300, 100, 37
    lib = _lib.get_lib()
    kd, s = walk_vectors(G)
    st = torch.cuda.current_stream().cuda_stream
    xb = torch.from_numpy(np.random.default_rng(11).standard_normal((N, ld))).cuda()
    yb = torch.full((N, ld), -777.0, dtype=torch.float64, device="cuda")
    args = [_lib.ptr(G.rowptr), _lib.ptr(G.col), _lib.ptr(G.val), _lib.ptr(kd), _lib.ptr(s), N]
    _lib.check(lib.meld_diffuse_step(*args, xb.data_ptr() + 8 * off, ld, yb.data_ptr() + 8 * off, ld, p, st), "meld_diffuse_step")
    xc = xb[:, off:off + p].contiguous()
    yc = torch.empty_like(xc)
    _lib.check(lib.meld_diffuse_step(*args, _lib.ptr(xc), p, _lib.ptr(yc), p, p, st), "meld_diffuse_step")
    torch.cuda.synchronize()
    assert torch.equal(yb[:, off:off + p], yc)
    assert bool((yb[:, :off] == -777.0).all()) and bool((yb[:, off + p:] == -777.0).all())
    ref = c["P"] @ xc.cpu().numpy()
    assert np.abs(yc.cpu().numpy() - ref).max() <= _bound(c, 1, float(xc.abs().max()))


# 4. row-stochastic properties ----------------------------------------------------------------------------------------------------
def test_constants_are_kept():
    """``P^t 1 = 1`` within ``4 t 2^-53``.  The bound counts the roundings of the step itself (the diagonal term, the division); it
    presumes that ``s`` is the sum the kernel forms.  With arbitrary weights ``dw`` (numpy's blocked sum) and the kernel's sum in
    storage order differ by up to ``(m - 1) 2^-53`` of a row of ``m`` entries, so the graphs here have weights ``k / 1024`` (every
    partial sum exact) or at most two entries per row (one order only); arbitrary weights are held to the bound of the module."""
    for kind, n in (("dyadic", 4097), ("path", 257)):
        G = _case(kind, n)["G"]
        for t in (1, 2, 5):
            ones = G.diffuse_device(torch.ones(n, 3, dtype=torch.float64, device="cuda"), t=t)
            dev = float((ones - 1.0).abs().max())
            print("{} t={}: |P^t 1 - 1| = {:.3e}".format(kind, t, dev))
            assert dev <= 4 * t * U
    c = _case("random", 4097)
    for t in (1, 2, 5):
        ones = c["G"].diffuse_device(torch.ones(4097, dtype=torch.float64, device="cuda"), t=t)
        dev = float((ones - 1.0).abs().max())
        print("random t={}: |P^t 1 - 1| = {:.3e}".format(t, dev))
        assert dev <= _bound(c, t, 1.0)


@pytest.mark.parametrize("kind,n", [("random", 4097), ("star", 4097), ("path", 257)])
def test_steps_stay_inside_the_range_of_the_signal(kind, n):
    c = _case(kind, n)
    G = c["G"]
    for t in (1, 2, 5):
        F = c["F_dev"][:, :70].contiguous()
        out = G.diffuse_device(F, t=t)
        tol = _bound(c, t, float(F.abs().max()))
        assert bool((out >= F.min(dim=0).values - tol).all()) and bool((out <= F.max(dim=0).values + tol).all())
        assert bool((G.diffuse_device(F.abs(), t=t) >= 0).all())  # a non-negative signal stays non-negative


# 5. fitted graphs: the kernel's diagonal is not 1 ----------------------------------------------------------------------------------
def _mixture(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)) + np.repeat([0.0, 6.0, 12.0], n // 3)[:, None]
    return X[rng.permutation(n)]


def _fitted_check(G, t=3, p=100):
    N = G.N
    F = np.random.default_rng(N).standard_normal((N, p))
    P = G.diff_op
    ref = F
    for _ in range(t):
        ref = P @ ref
    m_max = int(np.diff(G.rowptr.cpu().numpy()).max())
    tol = 2 * t * (m_max + 3) * U * float(np.abs(F).max())
    F_dev = torch.from_numpy(F).cuda()
    out = G.diffuse_device(F_dev, t=t)
    err = float(np.abs(out.cpu().numpy() - ref).max())
    print("fitted N={} anisotropy={}: |device - host| = {:.3e}, bound {:.3e}".format(N, G.anisotropy, err, tol))
    assert err <= tol
    return F_dev, out


@pytest.mark.parametrize("anisotropy", [1, 0])
def test_fitted_graph(anisotropy):
    import meld_amd

    op = meld_amd.MELD(knn=5, anisotropy=anisotropy, verbose=False).fit(_mixture(3000, 20, 1))
    kd = op.graph.kernel_diagonal().cpu().numpy()
    if anisotropy:
        assert float(np.abs(kd - 1.0).max()) > 1e-3  # (what this test is about)
    _fitted_check(op.graph)


def test_fitted_graph_in_the_locality_order():
    """9,000 cells: above the 8,192 from which the builder permutes the cells (tests/test_gpu_parity.py)."""
    import meld_amd

    op = meld_amd.MELD(knn=5, verbose=False).fit(_mixture(9000, 20, 2))
    G = op.graph
    assert G.perm is not None
    F_dev, out = _fitted_check(G)
    in_order = G.diffuse_device(F_dev.index_select(0, G.perm), t=3, device_order=True)
    assert torch.equal(in_order, out.index_select(0, G.perm))


# 6. impute -----------------------------------------------------------------------------------------------------------------------
def _impute_ref(op, idx, t=3):
    """``P^t X_s`` mapped back with the stored model on the host, and the tolerance: the diffusion bound on the scores plus the
    ``2 d 2^-53 max|X_t| max|V|`` of a ``d``-term fp64 dot product per element."""
    G = op.graph
    st = G._extend_state
    Xs = st.X.cpu().numpy()
    Xt = Xs
    for _ in range(t):
        Xt = G.diff_op @ Xt
    m_max = int(np.diff(G.rowptr.cpu().numpy()).max())
    tol = 2 * t * (m_max + 3) * U * float(np.abs(Xs).max())
    if st.model is None:
        return Xt[:, idx], tol
    V = st.model["V"].cpu().numpy()
    ref = Xt @ V[idx].T
    if st.model["kind"] == "pca":
        ref = ref + st.model["mean"].cpu().numpy().reshape(-1)[idx][None, :]
    tol += 2 * Xs.shape[1] * U * float(np.abs(Xt).max()) * float(np.abs(V).max())
    return ref, tol


@pytest.fixture(scope="module")
def gene_data():
    rng = np.random.default_rng(4)
    X = _mixture(3000, 60, 3) + 8.0
    thin = X * (rng.random(X.shape) < 0.3)
    return dict(dense=X, thin=sparse.csr_matrix(thin))


@pytest.mark.parametrize("kind", ["pca", "svd", "none"])
def test_impute_against_the_stored_model(kind, gene_data):
    import pandas as pd

    import meld_amd

    names = ["g%d" % j for j in range(60)]
    cells = ["cell%d" % i for i in range(3000)]
    if kind == "pca":
        op = meld_amd.MELD(knn=5, n_pca=10, verbose=False).fit(pd.DataFrame(gene_data["dense"], index=cells, columns=names))
    elif kind == "svd":
        op = meld_amd.MELD(knn=5, n_pca=10, verbose=False).fit(gene_data["thin"])
    else:
        op = meld_amd.MELD(knn=5, n_pca=None, verbose=False).fit(gene_data["dense"])
    st = op.graph._extend_state
    assert (st.model or {}).get("kind") == (None if kind == "none" else kind)
    assert int(st.X.shape[1]) == (60 if kind == "none" else 10)
    mask = np.zeros(60, dtype=bool)
    mask[[2, 3, 59]] = True
    requests = {"integers": ([5, 0, 17, 5], [5, 0, 17, 5]), "mask": (mask, [2, 3, 59]), "all": (None, list(range(60)))}
    if kind == "pca":
        requests["names"] = (["g7", "g0", "g59"], [7, 0, 59])
    for what, (genes, idx) in requests.items():
        out = op.impute(genes, t=3)
        ref, tol = _impute_ref(op, idx)
        assert isinstance(out, pd.DataFrame) and out.shape == (3000, len(idx))
        err = float(np.abs(out.values - ref).max())
        print("impute {} / {}: |device - host| = {:.3e}, bound {:.3e}".format(kind, what, err, tol))
        assert err <= tol, what
        if kind == "pca":
            assert list(out.index) == cells and list(out.columns) == [names[j] for j in idx]
        else:
            assert list(out.index) == list(range(3000)) and list(out.columns) == idx
    if kind != "pca":
        with pytest.raises(ValueError, match="name"):
            op.impute(["g1"])
    else:  # a fitted graph handed to another estimator keeps its cells, its model and their names
        again = meld_amd.MELD().fit(op.graph).impute(["g7"], t=3)
        assert list(again.columns) == ["g7"] and list(again.index) == cells
        assert np.array_equal(again.values, op.impute(["g7"], t=3).values)
    with pytest.raises(ValueError, match="out of range"):
        op.impute([60])
    with pytest.raises(NotImplementedError, match="auto"):
        op.impute([0], t="auto")
    # t = 0: the model's own reconstruction of the data
    ref0, tol0 = _impute_ref(op, [1, 2], t=0)
    assert np.abs(op.impute([1, 2], t=0).values - ref0).max() <= tol0


def test_impute_refusals(gene_data):
    import meld_amd
    from meld_amd.graph import DeviceGraph
    from scipy.spatial.distance import pdist, squareform

    X = gene_data["dense"][:400, :12]
    given = meld_amd.MELD().fit(DeviceGraph.from_scipy(_random(257, 1)))
    with pytest.raises(NotImplementedError, match="graph.diffuse"):
        given.impute()
    cosine = meld_amd.MELD(knn=5, distance="cosine", verbose=False).fit(X)
    with pytest.raises(NotImplementedError, match="cosine"):
        cosine.impute()
    pre = meld_amd.MELD(knn=5, distance="precomputed_distance", verbose=False).fit(squareform(pdist(X)))
    with pytest.raises(NotImplementedError, match="precomputed"):
        pre.impute()


# 7. errors on the device path ----------------------------------------------------------------------------------------------------
def test_shape_errors_and_undefined_walks():
    from types import SimpleNamespace

    from meld_amd.graph import DeviceGraph

    c = _case("random", 257)
    G = c["G"]
    with pytest.raises(ValueError, match="First dimension should be the number of nodes G.N = 257"):
        G.diffuse_device(torch.zeros(256, 4, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="At most 2 dimensions"):
        G.diffuse_device(torch.zeros(257, 4, 2, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match=r"\bt\b"):
        G.diffuse_device(c["F_dev"][:, :4], t=-1)
    with pytest.raises(NotImplementedError, match="auto"):
        G.diffuse(c["F"][:, :4], t="auto")
    # an adopted graph whose kernel has a zero diagonal: its isolated vertices have no walk
    W = c["W"]
    n_isolated = int((np.diff(W.indptr) == 0).sum())
    assert n_isolated >= 50
    adopted = DeviceGraph.from_foreign(SimpleNamespace(W=W, K=W.copy()))
    assert float(adopted.kernel_diagonal().abs().max()) == 0.0
    with pytest.raises(ValueError, match="^{} cells".format(n_isolated)):
        adopted.diffuse_device(c["F_dev"][:, :4])
    assert getattr(adopted, "_walk_vectors", None) is None
