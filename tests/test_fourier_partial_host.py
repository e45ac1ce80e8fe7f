"""Partial Fourier basis, host side (no GPU): argument validation on a stub graph, the rule for the upper end of the spectrum,
the scalars of the filter interval, the degree policy and the host half of the orthonormalisation (meld_amd/spectrum.py)."""
import math

import numpy as np
import pytest
import torch


def _stub_graph(dw=(1.0, 3.0, 2.0, 0.5, 0.5, 1.0)):
    from meld_amd.graph import DeviceGraph

    n = len(dw)
    return DeviceGraph(torch.zeros(n + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.float64),
                       torch.tensor(dw, dtype=torch.float64))


def test_argument_validation_comes_before_any_device_work():
    G = _stub_graph()
    calls = (lambda k: G.compute_fourier_basis(n_eigenvectors=k), lambda k: G.fourier_basis(k), lambda k: G.fourier_basis_device(k))
    for call in calls:
        for k in (0, 49, -1, 10**6):
            with pytest.raises(ValueError, match=r"n_eigenvectors must be in \[1, 48\]"):
                call(k)
        for k in (2.5, "3", True, 4.0):
            with pytest.raises(TypeError, match="n_eigenvectors must be an integer"):
                call(k)
    G.N = 12  # (a shard: six of twelve rows)
    for call in calls:
        with pytest.raises(ValueError, match="the Fourier basis is only defined for an unsharded graph"):
            call(np.int64(3))
    assert not getattr(G, "_partial_fourier", None) and getattr(G, "_U", None) is None


def test_upper_bound_rule():
    """An injected lmax (or the host ARPACK estimate, converged to 5e-3 only) is ignored, the device Lanczos one is used, otherwise
    Gershgorin's 2 max(dw); nothing is written to the graph."""
    from meld_amd.spectrum import upper_bound

    G = _stub_graph()
    assert upper_bound(G) == (6.0, "gershgorin")
    assert G._lmax is None and G.lmax_info == {}
    G.lmax = 0.25  # (too small on purpose: a filter on [cut, 0.25] would diverge)
    assert G.lmax_info == {"method": "injected"}
    assert upper_bound(G) == (6.0, "gershgorin")
    G._lmax, G.lmax_info = 5.5, dict(method="arpack", tol=5e-3)
    assert upper_bound(G) == (6.0, "gershgorin")
    G._lmax, G.lmax_info = 5.5, dict(method="lanczos", iterations=35)
    assert upper_bound(G) == (5.5, "lanczos")
    assert G._lmax == 5.5 and G.lmax_info == dict(method="lanczos", iterations=35)


def test_filter_interval_scalars_are_the_chebyshev_recurrence_on_cut_ub():
    from meld_amd.spectrum import filter_interval

    c, h, first, later = filter_interval(1.0, 3.0)
    assert (c, h) == (2.0, 1.0) and first == (1.0, -2.0, 0.0) and later == (2.0, -4.0, -1.0)
    cut, ub, d = 0.37, 5.2, 17
    c, h, (a1, b1, g1), (a2, b2, g2) = filter_interval(cut, ub)
    assert g1 == 0.0 and g2 == -1.0
    for lam in (0.0, 0.1, cut, 1.0, 3.3, ub):
        t0, t1 = 1.0, a1 * lam + b1  # (the step is y = alpha L x + beta x + gamma z; L acts on an eigenvector as lam)
        for _ in range(2, d + 1):
            t0, t1 = t1, a2 * lam * t1 + b2 * t1 + g2 * t0
        x = (lam - c) / h
        want = math.cos(d * math.acos(x)) if abs(x) <= 1 else math.copysign(1.0, x) ** d * math.cosh(d * math.acosh(abs(x)))
        assert abs(t1 - want) <= 1e-10 * max(1.0, abs(want)), (lam, t1, want)
        assert abs(t1) <= 1.0 + 1e-10 if cut <= lam <= ub else abs(t1) > 1.0  # damped on [cut, ub], growing below
    for bad in ((3.0, 3.0), (4.0, 3.0), (0.0, 0.0)):
        with pytest.raises(ValueError, match="cut < ub"):
            filter_interval(*bad)


def test_degree_policy():
    from meld_amd import spectrum as sp

    ub = 2.0
    last = 0
    for cut in (0.95 * ub, 0.5 * ub, 0.1 * ub, 1e-2 * ub, 1e-3 * ub, 1e-5 * ub):
        d = sp.filter_degree(cut, ub)
        assert sp.DEGREE_MIN <= d <= sp.DEGREE_MAX and d >= last  # a narrower wanted interval: a longer filter
        last = d
        growth = math.cosh(d * math.acosh((ub + cut) / (ub - cut)))  # |p(0)| against max |p| = 1 on [cut, ub]
        assert growth >= sp.AMPLIFICATION or d == sp.DEGREE_MAX
        if d > sp.DEGREE_MIN:
            assert math.cosh((d - 1) * math.acosh((ub + cut) / (ub - cut))) < sp.AMPLIFICATION  # ... and no longer than needed
    assert sp.filter_degree(1e-5 * ub, ub) == sp.DEGREE_MAX and sp.K_MAX + 16 <= sp.BLOCK == 64


def test_orthonormaliser_applied_twice():
    """The host half of the orthonormalisation on a block whose columns differ by 1e6 in norm and are nearly parallel (what the
    filter leaves): the first application is accurate to the Gram matrix's rounding, the second to fp64."""
    from meld_amd.spectrum import orthonormaliser

    rng = np.random.default_rng(0)
    V = rng.normal(size=(500, 64))
    V = V[:, :1] + 1e-4 * V  # nearly parallel columns
    V *= np.logspace(0, 6, 64)[None, :]
    for _ in range(2):
        V = V @ orthonormaliser(V.T @ V)
    assert np.abs(V.T @ V - np.eye(64)).max() <= 64 * math.sqrt(500) * np.finfo(float).eps
