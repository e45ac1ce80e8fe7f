"""The one stopping rule of the Lanczos drivers (``meld_amd.filter._first_converged``) against a dense reference, on
tridiagonal entries from a plain numpy Lanczos: no GPU, no ops object."""
import numpy as np
import pytest

N, TOL, CHECK_EVERY, MAX_ITER = 200, 1e-3, 5, 150


def _path_laplacian(n=N):
    L = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    L[0, 0] = L[-1, -1] = 1.0
    return L


def _lanczos(L, start, m):
    """alphas[0..m), betas[0..m) of m Lanczos steps with full re-orthogonalisation; betas[k - 1] closes the prefix k."""
    V = np.zeros((m + 1, L.shape[0]))
    V[0] = start / np.linalg.norm(start)
    alphas, betas = np.zeros(m), np.zeros(m)
    for k in range(m):
        w = L @ V[k]
        alphas[k] = w @ V[k]
        for _ in range(2):
            w -= V[: k + 1].T @ (V[: k + 1] @ w)
        betas[k] = np.linalg.norm(w)
        V[k + 1] = w / betas[k]
    return alphas, betas


def _dense(alphas, betas, k):
    """(theta, relative residual) of the prefix k by a dense eigendecomposition of the k x k tridiagonal."""
    T = np.diag(alphas[:k]) + np.diag(betas[: k - 1], 1) + np.diag(betas[: k - 1], -1)
    ev, evec = np.linalg.eigh(T)
    return ev[-1], abs(betas[k - 1] * evec[-1, -1]) / abs(ev[-1])


@pytest.fixture(scope="module")
def rule():
    from meld_amd.filter import _first_converged

    return _first_converged


@pytest.fixture(scope="module")
def tri():
    """One entry more than MAX_ITER: the folded driver reads its arrays one iteration past the prefix it examines."""
    start = np.random.default_rng(0).normal(size=N)
    alphas, betas = _lanczos(_path_laplacian(), start, MAX_ITER + 1)
    assert np.isfinite(betas).all() and (betas > 1e-14 * np.abs(alphas)).all()  # no breakdown: residuals alone decide
    return alphas, betas


@pytest.fixture(scope="module")
def expected(tri):
    """(k, theta) of the first prefix that is a multiple of CHECK_EVERY (or MAX_ITER) with a dense residual <= TOL."""
    alphas, betas = tri
    for k in range(1, MAX_ITER + 1):
        theta, resid = _dense(alphas, betas, k)
        if (k % CHECK_EVERY == 0 or k == MAX_ITER) and resid <= TOL:
            assert k < MAX_ITER  # the recurrence converges before the cap on this matrix
            return k, theta
    raise AssertionError("the reference Lanczos did not reach {} in {} iterations".format(TOL, MAX_ITER))


def _feed(rule, alphas, betas, cuts, max_iter=MAX_ITER, extra=0):
    """The rule over consecutive (lo, hi] cuts, each fed the arrays up to hi + extra; stops where the rule does."""
    out = None
    for lo, hi in cuts:
        out = rule(alphas[: hi + extra], betas[: hi + extra], lo, hi, CHECK_EVERY, max_iter, TOL)
        if out[3]:
            break
    return out


def test_stops_where_the_dense_reference_does(rule, tri, expected):
    alphas, betas = tri
    k, theta, resid, stopped = rule(alphas[:MAX_ITER], betas[:MAX_ITER], 0, MAX_ITER, CHECK_EVERY, MAX_ITER, TOL)
    print("stopped at k = {} (expected {}), theta = {!r}, resid = {:.3e}".format(k, expected[0], theta, resid))
    assert stopped and k == expected[0]
    assert abs(theta - expected[1]) <= 1e-12 * abs(expected[1])
    assert resid <= TOL and abs(resid - _dense(alphas, betas, k)[1]) <= 1e-9 * TOL


def test_same_answer_however_the_prefixes_are_cut(rule, tri, expected):
    alphas, betas = tri
    first = 4 * CHECK_EVERY
    batches = [(0, first)] + [(lo, lo + CHECK_EVERY) for lo in range(first, MAX_ITER, CHECK_EVERY)]
    whole = _feed(rule, alphas, betas, [(0, MAX_ITER)])
    assert whole[0] == expected[0] and whole[3]
    assert _feed(rule, alphas, betas, batches) == whole  # the device and phases drivers
    assert _feed(rule, alphas, betas, [(k, k + 1) for k in range(MAX_ITER)]) == whole
    assert _feed(rule, alphas, betas, batches, extra=1) == whole  # the folded driver: one iteration late


def test_the_iteration_cap_is_examined(rule, tri, expected):
    alphas, betas = tri
    cap = 23
    assert cap < expected[0] and cap % CHECK_EVERY
    k, theta, resid, stopped = rule(alphas[:cap], betas[:cap], 0, cap, CHECK_EVERY, cap, TOL)
    theta_ref, resid_ref = _dense(alphas, betas, cap)
    assert k == cap and not stopped and resid > TOL
    assert abs(theta - theta_ref) <= 1e-12 * theta_ref and abs(resid - resid_ref) <= 1e-9 * resid_ref


def test_breakdown_stops_at_once(rule):
    L = _path_laplacian()
    evec = np.linalg.eigh(L)[1]
    alphas, betas = _lanczos(L, evec[:, 10] + evec[:, 90] + evec[:, 170], 8)
    assert betas[2] <= 1e-14 * abs(alphas[2]) and (betas[:2] > 1e-3).all()
    k, theta, resid, stopped = rule(alphas, betas, 0, 8, CHECK_EVERY, MAX_ITER, TOL)
    assert (k, stopped) == (3, True)
    assert abs(theta - _dense(alphas, betas, 3)[0]) <= 1e-12 * theta


def test_a_non_finite_beta_stops_at_once(rule, tri, expected):
    alphas, betas = tri[0].copy(), tri[1].copy()
    assert expected[0] > 7
    betas[6] = np.nan
    k, theta, resid, stopped = rule(alphas, betas, 0, MAX_ITER, CHECK_EVERY, MAX_ITER, TOL)
    assert (k, stopped) == (7, True)


def test_an_ops_object_without_a_lanczos_driver_is_a_type_error():
    import torch
    from types import SimpleNamespace

    from meld_amd.filter import lanczos_lmax

    class NoRecurrence:
        def dot_slots(self):
            return 4

    G = SimpleNamespace(ops=NoRecurrence(), comm=None, val=torch.zeros(1, dtype=torch.float64), N=8, n_pad=8)
    with pytest.raises(TypeError, match="NoRecurrence.*lanczos_steps.*lanczos_fold.*lanczos_spmv"):
        lanczos_lmax(G)
