"""The pure parts of the PHATE embedding (meld_amd/phate.py) against the host reference tests/phate_reference.py, the reference's own
properties, and the argument contracts that need no device."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
from scipy.spatial.distance import cdist

from tests import phate_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _spectrum(n, seed):
    """Singular values like a diffusion operator's: 1, then a decay with a gap."""
    rng = np.random.default_rng(seed)
    s = np.sort(rng.uniform(0.0, 1.0, n))[::-1] ** 2
    s[0] = 1.0
    s[1:5] = 0.97 - 0.01 * np.arange(4)
    return s


@pytest.mark.parametrize("n,t_max", [(5, 3), (64, 100), (257, 100), (2000, 40)])
def test_entropy_curve_against_the_reference(n, t_max):
    """Both sides take the same powers; the sums of n non-negative terms differ by their order: ``2 (n + 2) u`` relative on the
    normalising sum, and the entropy, a sum of ``-p log p`` over terms of mixed sign around p = 1/e, within ``2 (n + 4) u sum |p log
    p|``."""
    from meld_amd.phate import entropy_curve

    s = _spectrum(n, n)
    h, want = entropy_curve(s, t_max), ref.entropy_curve(s, t_max)
    assert h.shape == (t_max,) and h.dtype == np.float64
    scale = np.empty(t_max)
    for i in range(t_max):
        p = s ** (i + 1)
        p = p / p.sum() + np.finfo(float).eps
        scale[i] = np.abs(p * np.log(p)).sum() + np.abs(np.log(p) + 1).max()  # (the second term: d(p log p) of the perturbed sum)
    err = np.abs(h - want)
    print("entropy: worst {:.2e} of its bound".format(float((err / (2 * (n + 4) * U * scale)).max())))
    assert np.all(err <= 2 * (n + 4) * U * scale)
    assert np.all(np.diff(want) <= 1e-12) and want[0] <= np.log(n) + 1e-9  # (the powers concentrate: the entropy falls)


def _two_lines(n, b, slope1, slope2):
    x = np.arange(n, dtype=np.float64)
    return np.where(x <= b, slope1 * (x - b), slope2 * (x - b)) + 3.0


@pytest.mark.parametrize("n,b", [(3, 1), (10, 1), (10, 8), (100, 15), (100, 50), (101, 98)])
def test_knee_of_two_exact_lines(n, b):
    """Two lines with dyadic slopes meeting at ``b``: both fits are exact there and nowhere else."""
    from meld_amd.phate import knee, knee_errors

    h = _two_lines(n, b, -2.0, -0.25)
    assert knee(h) == b == ref.knee(h)
    err, want = knee_errors(h), ref.knee_errors(h)
    assert err[b] <= 1e-12 and np.isinf(err[0]) and np.isinf(err[-1])
    others = np.delete(np.arange(1, n - 1), b - 1)
    assert np.all(err[others] > 1e-3) or others.size == 0
    assert np.allclose(err[1:-1], want[1:-1], rtol=1e-9, atol=1e-9)


def test_knee_ties_go_to_the_lowest_break_point():
    """A curve of zeros is fitted exactly at every break point, in the package and in the reference (``lstsq`` of a zero right-hand
    side is zero): all errors are exactly 0 and the knee is 1.  Any constant curve is exact in the package's centred form."""
    from meld_amd.phate import knee, knee_errors

    h = np.zeros(100)
    assert np.all(knee_errors(h)[1:-1] == 0) and np.all(ref.knee_errors(h)[1:-1] == 0)
    assert knee(h) == 1 == ref.knee(h)
    h = np.full(7, 2.5)
    assert np.all(knee_errors(h)[1:-1] == 0) and knee(h) == 1 and np.all(ref.knee_errors(h)[1:-1] <= 1e-12)
    with pytest.raises(ValueError, match="3 points"):
        knee_errors(np.zeros(2))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_knee_against_the_reference_on_entropy_curves(seed):
    from meld_amd.phate import knee, knee_errors

    h = ref.entropy_curve(_spectrum(300, seed), 100)
    err, want = knee_errors(h), ref.knee_errors(h)
    assert np.allclose(err[1:-1], want[1:-1], rtol=1e-9, atol=1e-12)
    best = np.sort(want[1:-1])
    if best[1] - best[0] > 1e-6 * best[0]:  # (the condition under which the knee may be compared)
        assert knee(h) == ref.knee(h)


def test_sign_columns():
    from meld_amd.phate import sign_columns

    Z = np.array([[1.0, -3.0, 2.0], [-2.0, 3.0, -2.0], [0.5, 1.0, 1.0]])
    out = sign_columns(Z)
    assert np.array_equal(out[:, 0], -Z[:, 0])  # (largest magnitude -2: flipped)
    assert np.array_equal(out[:, 1], -Z[:, 1])  # (a tie of magnitude 3: the lowest index, -3, decides)
    assert np.array_equal(out[:, 2], Z[:, 2])  # (a tie of magnitude 2: the lowest index, +2, decides)


def test_argument_checks():
    from meld_amd.phate import SMACOF_MAX_DIM, check_arguments, check_t

    a = check_arguments()
    assert a == dict(n_components=2, t="auto", gamma=1.0, mds="metric", max_iter=3000, eps=1e-6, t_max=100)
    assert check_t(np.int64(7)) == 7 and isinstance(check_t(np.int64(7)), int)
    for bad in (0, -1, 2.0, True, "Auto", None):
        with pytest.raises(ValueError, match="t="):
            check_t(bad)
    for bad in (0, SMACOF_MAX_DIM + 1, 2.0, True):
        with pytest.raises(ValueError, match="n_components={!r}".format(bad)):
            check_arguments(n_components=bad)
    for bad in (-1.5, 1.01, "1"):
        with pytest.raises(ValueError, match="gamma="):
            check_arguments(gamma=bad)
    for bad in (2, 0, 10.0):
        with pytest.raises(ValueError, match="t_max={!r}".format(bad)):
            check_arguments(t_max=bad)
    for bad in ("sgd", "nonmetric", None):
        with pytest.raises(ValueError, match="mds="):
            check_arguments(mds=bad)
    with pytest.raises(ValueError, match="max_iter=-1"):
        check_arguments(max_iter=-1)
    with pytest.raises(ValueError, match="eps=-1"):
        check_arguments(eps=-1)


def test_phate_refuses_before_touching_the_device():
    """A stub with the attributes the checks read: none of these calls gets as far as a tensor."""
    from meld_amd.landmark import LANDMARK_MAX
    from meld_amd.phate import phate

    G = SimpleNamespace(N=100, n_rows=100, comm=None, n_landmark=None)
    with pytest.raises(ValueError, match="n_components=9"):
        phate(G, n_components=9)
    with pytest.raises(ValueError, match="mds='sgd'"):
        phate(G, mds="sgd")
    with pytest.raises(ValueError, match="n_landmark"):
        phate(G, n_landmark=0)
    shard = SimpleNamespace(N=100, n_rows=50, comm=None, n_landmark=None)
    with pytest.raises(ValueError, match="only defined for an unsharded graph"):
        phate(shard)
    big = SimpleNamespace(N=LANDMARK_MAX + 1, n_rows=LANDMARK_MAX + 1, comm=None, n_landmark=None)
    with pytest.raises(ValueError, match="above the {} landmarks".format(LANDMARK_MAX)):
        phate(big, n_landmark=LANDMARK_MAX + 1)


def test_estimator_delegates_and_needs_a_fit():
    import meld_amd

    op = meld_amd.MELD()
    with pytest.raises(ValueError, match="must be `fit` before running `phate`"):
        op.phate()


def test_cap_and_argument_contract_of_the_library():
    """``meld_smacof_max_dim()`` is what the Python layer refuses above; every bad call returns -1 with the entry's name in the
    message.  The addresses are host memory: nothing may touch them, and nothing does -- the checks come before any launch."""
    from meld_amd._lib import get_lib
    from meld_amd.phate import SMACOF_MAX_DIM

    lib = get_lib()
    assert lib.meld_smacof_max_dim() == SMACOF_MAX_DIM == 8
    buf = (ctypes.c_double * 64)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 256
    bad = dict(
        null_D=(None, 4, 4, 2, a, b, a), null_Z=(a, 4, 4, 2, None, b, a), null_out=(a, 4, 4, 2, a, None, a), null_stress=(a, 4, 4, 2, a, b, None),
        dim_0=(a, 4, 4, 0, a, b, a), dim_9=(a, 4, 4, 9, a, b, a), ld=(a, 3, 4, 2, a, b, a), negative=(a, 4, -1, 2, a, b, a),
        same=(a, 4, 4, 2, a, a, a))
    for what, args in bad.items():
        lib.meld_scale_f64(None, 1.0, None, 10, None)  # (leaves another entry's message behind)
        assert lib.meld_smacof_step(*args, None) == -1, what
        assert lib.meld_last_error().decode().startswith("meld_smacof_step:"), (what, lib.meld_last_error())
    assert lib.meld_smacof_step(a, 0, 0, 2, a, b, a, None) == 0  # (n = 0: a no-op, nothing is launched)


def test_smacof_kernels_do_not_spill():
    """One kernel per dimension 1 .. 8 as hipcc compiles them with the build's flags: no private memory, two waves per SIMD at
    least (the figures tests/test_kernel_resources.py reads for the search kernels)."""
    from tests.test_kernel_resources import _resource_usage

    rows = _resource_usage(os.path.join(ROOT, "meld_amd", "csrc", "mds.hip"))
    kernels = {k: v for k, v in rows.items() if "smacof_step_kernel" in k}
    assert len(kernels) == 8, sorted(rows)
    for name, r in kernels.items():
        assert r["ScratchSize [bytes/lane]:"] == 0 and r["Occupancy [waves/SIMD]:"] >= 2, (name, r)


# -- the reference's own properties --------------------------------------------------------------------------------------------
def _tree(n_branch, d, seed):
    """Three noisy branches from a common root in ``d`` dimensions."""
    rng = np.random.default_rng(seed)
    dirs = rng.normal(size=(3, d))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    X = np.concatenate([np.linspace(0, 1, n_branch)[:, None] * dirs[b][None, :] for b in range(3)])
    return X + 0.01 * rng.normal(size=X.shape)


def test_reference_stress_never_rises():
    """SMACOF majorises the stress: 64 steps from a random start never raise it (beyond rounding: 1e-12 relative)."""
    X = _tree(40, 10, 0)
    Dm = cdist(X, X)
    Z = np.random.default_rng(1).normal(size=(X.shape[0], 2))
    last = ref.stress(Dm, Z)
    for _ in range(64):
        Z = ref.smacof_step(Dm, Z)[0]
        now = ref.stress(Dm, Z)
        assert now <= last * (1 + 1e-12)
        last = now
    _, final, k, log = ref.smacof(Dm, np.random.default_rng(1).normal(size=(X.shape[0], 2)), max_iter=64, eps=0)
    assert k == 64 and log.shape == (65,) and final == log[-1] and abs(final - last) <= 1e-12 * last
    _, _, k, log = ref.smacof(Dm, ref.classical_mds(Dm, 2), max_iter=3000, eps=1e-3)
    assert k % ref.CHECK_EVERY == 0 and k < 3000 and log[k - 2] - log[k - 1] <= 1e-3 * log[k - 2]


def test_reference_classical_step_recovers_a_configuration_and_smacof_keeps_it():
    """257 points drawn in R^3: classical MDS of their distances reproduces the distances (1.1e-15 of the diameter measured, 1e-12
    asserted), and that configuration is a fixed point of the step with zero stress."""
    X = np.random.default_rng(5).normal(size=(257, 3))
    Dm = cdist(X, X)
    Z = ref.classical_mds(Dm, 3)
    err = np.abs(cdist(Z, Z) - Dm).max() / Dm.max()
    print("classical MDS: distances to {:.2e} of the diameter".format(err))
    assert err <= 1e-12
    for c in range(3):
        assert Z[np.argmax(np.abs(Z[:, c])), c] > 0
    Zn, rs, _ = ref.smacof_step(Dm, Z)
    assert np.abs(Zn - Z).max() <= 1e-12 * np.abs(Z).max()
    assert rs.sum() <= 1e-24 * (Dm * Dm).sum()


def test_reference_step_special_cases():
    """Coincident points contribute nothing to Z' and D^2 to the stress; the whole configuration at one point gives Z' = 0."""
    rng = np.random.default_rng(2)
    n = 9
    Dm = cdist(rng.normal(size=(n, 2)), rng.normal(size=(n, 2)))
    Dm = Dm + Dm.T
    np.fill_diagonal(Dm, 0)
    Z = np.ones((n, 2))
    Zn, rs, scale = ref.smacof_step(Dm, Z)
    assert np.all(Zn == 0) and np.all(scale == 0) and np.allclose(rs, (Dm * Dm).sum(axis=1), rtol=1e-15)


# -- Benchmarker.fit_phate without the phate package -----------------------------------------------------------------------------
def test_fit_phate_falls_back_to_the_device_embedding(monkeypatch):
    """With ``phate`` not importable, ``fit_phate`` fits a ``MELD`` graph with PHATE's defaults and calls ``graph.phate(n_components=3,
    ...)``: graph keywords go to the graph, the rest to ``phate()``.  The graph is a stub: no device is needed."""
    import meld_amd
    import meld_amd.meld as meld_module

    seen = {}
    coords = np.random.default_rng(0).normal(size=(50, 3)) + 4.0

    class Graph:
        def phate(self, **kwargs):
            seen["phate"] = kwargs
            return SimpleNamespace(embedding=coords)

    class Estimator:
        def __init__(self, **kwargs):
            seen["graph"] = kwargs

        def fit(self, data):
            seen["data"] = data
            self.graph = Graph()
            return self

    monkeypatch.setitem(sys.modules, "phate", None)  # (``import phate`` raises ImportError)
    monkeypatch.setattr(meld_module, "MELD", Estimator)
    bm = meld_amd.Benchmarker(seed=7)
    data = np.zeros((50, 4))
    out = bm.fit_phate(data, knn=9, t=12, gamma=0, n_landmark=20)
    assert seen["data"] is data
    assert seen["graph"] == dict(n_pca=100, knn=9, decay=40, anisotropy=0, verbose=False, n_landmark=20, random_state=7)
    assert seen["phate"] == dict(n_components=3, t=12, gamma=0)
    assert out is bm.data_phate and out.shape == (50, 3)
    assert np.allclose(out.mean(axis=0), 0, atol=1e-12) and np.allclose(out.std(axis=0), 1)  # (set_phate standardised it)
    bm.fit_phate(data)
    assert seen["graph"] == dict(n_pca=100, knn=5, decay=40, anisotropy=0, verbose=False, random_state=7)
    assert seen["phate"] == dict(n_components=3)
