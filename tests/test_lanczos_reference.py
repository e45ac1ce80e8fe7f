"""Host tests of tests/lanczos_reference.py: the per-step contract of the Lanczos recurrence behind ``lmax`` (no GPU).

  * the contract holds for three independent fp64 implementations of the step -- the numpy twin of ``meld_lanczos_steps`` and the
    phases / folded forms of ``tests.cpu_ops.CpuOps``, driven as ``filter._lanczos_lmax_phases`` / ``_folded`` drive them -- on every
    step of every matrix;
  * it is sharp: a dropped entry, beta of the wrong iteration and fp32-rounded weights against the fp64 reference each exceed the
    componentwise bound on w on every matrix from M70 up;
  * the long-double recurrence itself is sound against a dense eigensolver;
  * the conditions tests/test_gpu_lanczos_contract.py relies on hold for the reference alone: no breakdown inside the window
    (beta >= 1e-6 max(dw) on every step used), K = min(16, n - 1) steps on every matrix but M3, and the estimates that test runs to
    convergence converge long before the recurrence reaches n iterations.
"""
import numpy as np
import pytest
import torch

from tests import lanczos_reference as lr
from tests.cpu_ops import CpuOps

U = lr.U


def _twin_fractions(name, W_run=None, fp32_ref=False, stale_beta=False):
    """Per step (fa, fw, fb) of the twin run on ``W_run`` (default: the matrix itself) against the reference on the matrix."""
    W, dw, k = lr.matrix(name)
    Wref = lr.weights(name, fp32_ref)
    V, state, alphas, betas = lr.twin_setup(lr.start_vector(W.shape[0]), k)
    out = []
    for it in range(k):
        lr.twin_lanczos_steps(W if W_run is None else W_run, dw, V, state, alphas, betas, it, 1, stale_beta=stale_beta)
        out.append(lr.check_after(Wref, dw, V, it, alphas[it], betas[it])[0])
    return np.array(out, dtype=np.float64)


def test_long_double_is_extended_or_the_fallback_is_stated():
    """The guard of the reference: a 64-bit mantissa, or fp64 with exactly rounded sums -- either way every test below runs."""
    assert lr.EXTENDED == bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)
    x = np.array([1.0, 2.0 ** -60, -1.0])
    assert float(lr._sum(x)) == 2.0 ** -60  # (a plain fp64 sum loses it)
    # rows without entries between rows with entries
    got = lr._row_sums(np.array([1.0, 2.0, 4.0], dtype=lr.LD), np.array([0, 0, 2, 2, 3, 3]))
    assert got.tolist() == [0.0, 3.0, 0.0, 4.0, 0.0]


def test_matrices_are_what_the_contract_tests_assume():
    for name in lr.NAMES:
        W, dw, k = lr.matrix(name)
        n = W.shape[0]
        assert abs(W - W.T).max() == 0.0 and W.diagonal().max() == 0.0 and W.has_sorted_indices
        assert k == (2 if name == "M3" else min(16, n - 1))
        assert np.array_equal(dw, np.ravel(W.sum(1)))
    from tests.test_gpu_tiled import _awkward_matrix

    for name, n, density in (("M70", 70, 0.3), ("M257", 257, 0.05), ("M4481", 4481, 0.004)):  # the same matrices as there
        T = _awkward_matrix(n, density)[0]
        W = lr.matrix(name)[0]
        assert np.array_equal(T.indptr, W.indptr) and np.array_equal(T.indices, W.indices) and np.array_equal(T.data, W.data)
    W = lr.matrix("M257log")[0]
    assert (lr.matrix("M257")[0] != 0).toarray().tolist() == (W != 0).toarray().tolist()
    assert 1e-4 <= W.data.min() < 2e-4 and 0.5 < W.data.max() <= 1.0
    for name in ("M4481", "M20000"):
        W = lr.matrix(name)[0]
        rows = np.diff(W.indptr)
        assert rows[5] == 0 and rows[7] >= 290 and rows.max() == rows[7]
    # workgroups: CSR-stream kernel 32 rows each, axpy 256 rows each, against 64 slots
    assert -(-4481 // 32) == 141 and -(-20000 // 256) == 79


@pytest.mark.parametrize("name", lr.NAMES)
def test_no_breakdown_inside_the_window(name):
    """Every step used has beta_ref >= 1e-6 max(dw): the recurrence is nowhere near a breakdown in the window the GPU tests check
    (if a matrix ever violates this, its seed changes -- not this assertion or the cap)."""
    W, dw, k = lr.matrix(name)
    for fp32 in (False, True):
        _, betas = lr.reference_run(lr.weights(name, fp32), dw, lr.start_vector(W.shape[0]), k)
        assert len(betas) == k and np.all(betas >= 1e-6 * dw.max()), (name, fp32, betas)


@pytest.mark.parametrize("name", lr.NAMES)
def test_twin_of_the_device_loop_keeps_the_contract(name):
    f = _twin_fractions(name)
    print("%s twin: alpha %.2e  w %.2e  beta %.2e of the bounds" % (name, f[:, 0].max(), f[:, 1].max(), f[:, 2].max()))
    assert f.shape[0] == lr.matrix(name)[2] and np.all(f <= 1.0), f
    # cut into calls of 3, 1, 4, ... iterations: the same numbers, bit for bit (the scalars live in ``state``)
    W, dw, k = lr.matrix(name)
    one, cut = lr.twin_setup(lr.start_vector(W.shape[0]), k), lr.twin_setup(lr.start_vector(W.shape[0]), k)
    lr.twin_lanczos_steps(W, dw, *one, 0, k)
    it = 0
    for m in (3, 1, 4, 1, 5, 2):
        m = min(m, k - it)
        lr.twin_lanczos_steps(W, dw, *cut, it, m)
        it += m
    assert it == k and all(np.array_equal(a, b) for a, b in zip(one, cut))


def _cpu_graph(name):
    from meld_amd.graph import DeviceGraph

    return DeviceGraph.from_scipy(lr.matrix(name)[0], device="cpu")


@pytest.mark.parametrize("name", lr.NAMES)
def test_phases_form_of_the_host_stand_in_keeps_the_contract(name):
    W, dw, k = lr.matrix(name)
    G, Wref = _cpu_graph(name), lr.weights(name, False)
    assert np.array_equal(G.dw_dev.numpy(), dw)
    worst = np.zeros(3)
    for it, V, alphas, betas in lr.drive_phases(CpuOps(), G, torch.from_numpy(lr.start_vector(W.shape[0])), k):
        f, _ = lr.check_after(Wref, dw, V, it, float(alphas[it]), float(betas[it]))
        worst = np.maximum(worst, f)
        assert max(f) <= 1.0, (name, it, f)
    assert it == k - 1
    print("%s phases: alpha %.2e  w %.2e  beta %.2e of the bounds" % ((name,) + tuple(worst)))


@pytest.mark.parametrize("name", lr.NAMES)
def test_folded_form_of_the_host_stand_in_keeps_the_contract(name):
    """beta_k is known at iteration k + 1 and checked then, against the reference of step k."""
    W, dw, k = lr.matrix(name)
    G, Wref = _cpu_graph(name), lr.weights(name, False)
    worst = np.zeros(3)
    prev = None
    for it, V, alphas, betas in lr.drive_folded(CpuOps(), G, torch.from_numpy(lr.start_vector(W.shape[0])), k):
        (fa, fw, _), ref = lr.check_after(Wref, dw, V, it, float(alphas[it]))
        fb = 0.0
        if prev is not None:
            fb = float(lr._fraction(lr.LD(float(betas[it - 1])) - prev.beta, lr.beta_bound(prev)))
        assert float(betas[it]) == 0.0  # not known yet
        worst = np.maximum(worst, (fa, fw, fb))
        assert max(fa, fw, fb) <= 1.0, (name, it, fa, fw, fb)
        prev = ref
    assert it == k - 1
    print("%s folded: alpha %.2e  w %.2e  beta %.2e of the bounds" % ((name,) + tuple(worst)))


@pytest.mark.parametrize("name", lr.FROM_M70)
def test_a_dropped_entry_exceeds_the_bound_on_w(name):
    """One entry (i, j) of weight ~0.1 missing from row i: w[i] is off by W_ij v_j at every step."""
    W, dw, k = lr.matrix(name)
    Wd, i, j, wgt = lr.drop_entry(W)
    assert Wd.nnz == W.nnz - 1 and 0.05 < wgt < 0.2 and Wd[j, i] == W[j, i] != 0
    f = _twin_fractions(name, W_run=Wd)
    print("%s dropped (%d, %d) = %.3f: w bound exceeded %.1e .. %.1e times" % (name, i, j, wgt, f[:, 1].min(), f[:, 1].max()))
    assert f[:, 1].max() > 1.0
    assert np.all(f[:, 1] > 1.0), f[:, 1]


@pytest.mark.parametrize("name", lr.FROM_M70)
def test_beta_of_the_wrong_iteration_exceeds_the_bound_on_w(name):
    """beta_{k-2} in place of beta_{k-1} from iteration 2 on (the wrong parity buffer): steps 0 and 1 pass, every later one fails."""
    f = _twin_fractions(name, stale_beta=True)
    print("%s stale beta: w bound exceeded %.1e .. %.1e times from step 2" % (name, f[2:, 1].min(), f[2:, 1].max()))
    assert np.all(f[:2] <= 1.0)
    assert np.all(f[2:, 1] > 1.0), f[:, 1]


@pytest.mark.parametrize("name", lr.FROM_M70)
def test_fp32_weights_exceed_the_bound_on_w_of_the_fp64_reference(name):
    """The twin on the fp32-rounded weights against the fp64 reference fails; against the fp32-rounded reference -- what the tiled
    layout is held to -- it passes."""
    W32 = lr.weights(name, True).csr
    f = _twin_fractions(name, W_run=W32)
    print("%s fp32 weights: bounds exceeded alpha %.1e  w %.1e  beta %.1e times" % (name, f[:, 0].max(), f[:, 1].max(), f[:, 2].max()))
    assert np.all(f[:, 1] > 1.0), f[:, 1]
    assert np.all(_twin_fractions(name, W_run=W32, fp32_ref=True) <= 1.0)


@pytest.mark.parametrize("name", ["M70", "M257log", "M4481"])
def test_long_double_recurrence_is_sound(name):
    """The top Ritz value of every k-prefix of the long-double recurrence has an eigenvalue of the dense Lref within |beta_k s_k|
    and never exceeds lambda_max, both up to delta = 64 * 2^-53 * lambda_max: the eigenvalues compared with come from an fp64
    solver, and on M257log the residual falls to 1e-14 (a third of an ulp of lambda_max = 32.2) at k = 15, below what any such
    solver resolves.  The yardstick itself is good to a quarter of delta (``laplacian_spectrum``)."""
    W, dw, k = lr.matrix(name)
    for fp32 in (False, True):
        lam = lr.laplacian_spectrum(name, fp32)
        delta = 64 * U * lam[-1]
        print("%s fp32=%s: lambda_max %.15g, residual of its eigenpair %.2e = %.1f * 2^-53 lambda_max" % (
            name, fp32, lam[-1], lr.top_residual(name, fp32), lr.top_residual(name, fp32) / (U * lam[-1])))
        assert lr.top_residual(name, fp32) <= 16 * U * lam[-1]
        alphas, betas = lr.reference_run(lr.weights(name, fp32), dw, lr.start_vector(W.shape[0]), k)
        for m in range(1, k + 1):
            theta, resid = lr.ritz_top(alphas, betas, m)
            assert np.abs(lam - theta).min() <= resid + delta, (name, fp32, m, theta, resid)
            assert theta <= lam[-1] + delta, (name, fp32, m, theta, lam[-1])


@pytest.mark.parametrize("name", ["M70", "M257log", "M4481"])
def test_estimates_converge_long_before_n_iterations(name):
    """``_lanczos_lmax_device(G, ops, u, 3e-4, 300, 5)`` is run on these matrices with max_iter beyond n for the two small ones: the
    stopping rule must fire, with everything the overlapped driver enqueues behind it (two checks' worth), well inside n."""
    from meld_amd.filter import _first_converged

    W, dw, _ = lr.matrix(name)
    n = W.shape[0]
    kmax = min(60, n - 1)
    V, state, alphas, betas = lr.twin_setup(lr.start_vector(n), kmax)
    lr.twin_lanczos_steps(W, dw, V, state, alphas, betas, 0, kmax)
    k, theta, resid, stopped = _first_converged(alphas, betas, 0, kmax, 5, 300, 3e-4)
    assert stopped and k + 10 <= min(kmax, n // 2), (name, k, resid)
