"""The PHATE embedding on the device (meld_amd/phate.py, csrc/mds.hip) against the host reference tests/phate_reference.py (whose own
properties tests/test_phate_host.py holds).

Tolerances, derived.  u = 2^-53; a value that passes through k roundings is within ``(1 + u)^k - 1`` of the exact one, and two
computations of k1 and k2 roundings are within ``(k1 + k2) u`` of each other to first order -- written below as ``2 (m + 1) u`` with
``m + 1 >= max(k1, k2)``, the form of tests/test_gpu_landmark.py.

* ``row_stress[i] = sum_{j != i} (d_ij - D_ij)^2``: non-negative terms, so relative errors add and never cancel.  ``d_ij``: ``dim``
  roundings for the sum of squares (an fma chain on the device, a pairwise sum in scipy) and one for the root -- halved by it; the
  difference, its square and the sum over ``n`` columns (a lane's chain of ``n / 64`` additions and a six-level butterfly on the
  device; any order on the host): at most ``n + dim + 4`` roundings either side, ``2 (n + dim + 4) u`` relative.  (The subtraction
  ``d - D`` amplifies the error of ``d`` by ``d / |d - D|``; the cases keep the two configurations at different scales, so that this
  factor is of order 1 -- the worst ratio to the bound is printed.)
* ``Z'[i, c] = (1 / n) sum_j (D_ij / d_ij) (Z[i, c] - Z[j, c])``: terms of mixed signs, so the bound is relative to the sum of their
  magnitudes, not to the result.  A term carries ``d_ij`` (above), one division, one exact-input difference and one product (fused on
  the device), the sum ``n`` additions, the division by ``n`` one: ``2 (n + dim + 6) u * sum_j |term_j| / n`` per component.
* Potential distances: a sum of ``n`` squares of direct differences, one root: ``(n + 4) u`` relative between any two orders.
* ``P^t`` by any multiplication tree: every entry is a sum of products of ``t`` non-negative factors; a product of two matrices with
  entries of relative error e1 and e2 has entries within ``e1 + e2 + n u``; ``t - 1`` products: ``(t - 1) n u`` on either side,
  ``2 t (n + 1) u`` relative per entry.  ``U = -log(Pt + 1e-7)``: the derivative of the log is at most ``1 / Pt``, so the relative
  bound of ``Pt`` is an absolute one of ``U``; the rounding of the log itself (``|U| <= 16.2``) is far inside it.
* 64 SMACOF steps: the sum of the 64 step bounds times 16.  The step is non-expansive on this input: a 1e-12 relative perturbation
  of ``Z0`` is 4.7e-13 after 64 steps (measured on the host), so errors of earlier steps do not grow; 16 is the margin for their
  accumulation through ``d_ij`` of the later ones.
* Products with transitions: the dot-product bounds of tests/test_gpu_extend.py, ``rtol = 1e-12, atol = 1e-14``.

Shapes: the step kernel takes 8 rows per workgroup (two per wave), 256 columns per LDS tile, 64 per wave instruction (n in {1, 2,
3, 63, 64, 65, 257, 1000}: fewer rows than a wave's, one short of / exactly / one past a wave instruction, one past a tile, several
tiles and 125 workgroups) and one instantiation per ``dim`` (1, 2, 3 and the largest, 8)."""
import numpy as np
import pytest
import torch
from scipy.spatial.distance import cdist

from tests import phate_reference as ref
from tests.test_gpu_diffuse import _MAKERS
from tests.test_phate_host import _tree

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SIZES = (1, 2, 3, 63, 64, 65, 257, 1000)
DIMS = (1, 2, 3, 8)
CASES = ("random", "coincident", "collapsed", "zeros", "wide")
_TARGETS, _STEPS = {}, {}


def _target(n, zeros=False):
    """Target distances: those of a random configuration in R^5 at twice the scale of ``Z``; ``zeros``: a tenth of the pairs at 0."""
    key = (n, zeros)
    if key not in _TARGETS:
        rng = np.random.default_rng(10 * n + zeros)
        X = 2.0 * rng.normal(size=(n, 5))
        Dm = cdist(X, X)
        if zeros:
            drop = np.triu(rng.uniform(size=(n, n)) < 0.1, 1)
            Dm[drop | drop.T] = 0.0
        _TARGETS[key] = Dm
    return _TARGETS[key]


def _step_case(n, dim, case):
    key = (n, dim, case)
    if key not in _STEPS:
        rng = np.random.default_rng(1000 * n + 10 * dim + len(case))
        Z = rng.normal(size=(n, dim))
        if case == "coincident":  # (pairs of points on one spot, the odd one out alone)
            Z[1::2] = Z[0:2 * (n // 2):2]
        elif case == "collapsed":
            Z[:] = Z[0]
        Dm = _target(n, zeros=case == "zeros")
        _STEPS[key] = (Dm, Z, ref.smacof_step(Dm, Z))
    return _STEPS[key]


def _run_step(Dm, Z, wide=False):
    from meld_amd.phate import smacof_step_device

    n, dim = Z.shape
    if wide:  # (a view of a wider buffer: ldD = n + 5, the columns beyond n poisoned)
        buf = torch.full((n, n + 5), float("nan"), dtype=torch.float64, device="cuda")
        buf[:, :n] = torch.from_numpy(Dm)
        D_dev = buf[:, :n]
    else:
        D_dev = torch.from_numpy(Dm).cuda()
    Z_dev = torch.from_numpy(Z).cuda()
    out = torch.full((n, dim), float("nan"), dtype=torch.float64, device="cuda")
    rs = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    smacof_step_device(D_dev, Z_dev, out, rs)
    assert torch.equal(Z_dev.cpu(), torch.from_numpy(Z))  # (the input is not written)
    return out.cpu().numpy(), rs.cpu().numpy()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_step_kernel(n, dim, case):
    Dm, Z, (want, want_rs, scale) = _step_case(n, dim, case)
    got, rs = _run_step(Dm, Z, wide=case == "wide")
    again, rs_again = _run_step(Dm, Z, wide=case == "wide")
    assert np.array_equal(got, again) and np.array_equal(rs, rs_again), "two runs differ"
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(rs))
    tol_rs = 2 * (n + dim + 4) * U * want_rs
    tol = 2 * (n + dim + 6) * U * scale / n
    err_rs, err = np.abs(rs - want_rs), np.abs(got - want)
    print("step n={} dim={} {}: row_stress {:.2e}, Z' {:.2e} of their bounds".format(
        n, dim, case, float((err_rs / np.maximum(tol_rs, 1e-300)).max()), float((err / np.maximum(tol, 1e-300)).max())))
    assert np.all(err_rs <= tol_rs)
    assert np.all(err <= tol)
    if case == "collapsed":
        assert np.all(got == 0)
        assert np.all(np.abs(rs - (Dm * Dm).sum(axis=1)) <= tol_rs)
    if n == 1:
        assert np.all(got == 0) and np.all(rs == 0)


def test_step_argument_checks_leave_the_output_alone():
    from meld_amd._lib import get_lib, ptr

    lib = get_lib()
    n, dim = 6, 2
    D = torch.zeros(n, n, dtype=torch.float64, device="cuda")
    Z = torch.ones(n, dim, dtype=torch.float64, device="cuda")
    out = torch.full((n, dim), 7.0, dtype=torch.float64, device="cuda")
    rs = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    bad = dict(null_D=(None, n, n, dim, ptr(Z), ptr(out), ptr(rs)), null_Z=(ptr(D), n, n, dim, None, ptr(out), ptr(rs)),
               null_out=(ptr(D), n, n, dim, ptr(Z), None, ptr(rs)), null_stress=(ptr(D), n, n, dim, ptr(Z), ptr(out), None),
               dim_0=(ptr(D), n, n, 0, ptr(Z), ptr(out), ptr(rs)), dim_9=(ptr(D), n, n, 9, ptr(Z), ptr(out), ptr(rs)),
               ld=(ptr(D), n - 1, n, dim, ptr(Z), ptr(out), ptr(rs)), negative=(ptr(D), n, -1, dim, ptr(Z), ptr(out), ptr(rs)),
               same=(ptr(D), n, n, dim, ptr(out), ptr(out), ptr(rs)))
    for what, args in bad.items():
        assert lib.meld_smacof_step(*args, st) == -1, what
        assert lib.meld_last_error().decode().startswith("meld_smacof_step:"), what
    assert lib.meld_smacof_step(ptr(D), n, 0, dim, ptr(Z), ptr(out), ptr(rs), st) == 0  # (n = 0: a no-op)
    torch.cuda.synchronize()
    assert torch.all(out == 7.0) and torch.all(rs == 7.0)


# -- distances -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 65, 257])
def test_potential_distances(n):
    from meld_amd.phate import distances_device

    rng = np.random.default_rng(n)
    variants = []
    pot = rng.uniform(0.5, 16.0, size=(n, n))
    if n == 2:
        a, b = pot.copy(), pot.copy()
        a[1] = a[0]
        b[1] = b[0]
        b[1, 1] = np.nextafter(b[0, 1], np.inf)
        variants = [a, b]
    else:
        pot[1] = pot[0]
        pot[n - 1] = pot[0]  # (duplicates, near and far)
        pot[3] = pot[2]
        pot[3, n // 2] = np.nextafter(pot[2, n // 2], np.inf)  # (rows that differ in the last bit of one entry)
        variants = [pot]
    for pot in variants:
        Dm = distances_device(torch.from_numpy(pot).cuda()).cpu().numpy()
        want = cdist(pot, pot)
        assert Dm.shape == (n, n) and np.all(np.diag(Dm) == 0) and np.array_equal(Dm, Dm.T)
        if n > 2:
            assert Dm[0, 1] == 0 and Dm[0, n - 1] == 0 and Dm[1, n - 1] == 0
            assert Dm[2, 3] == pot[3, n // 2] - pot[2, n // 2] > 0
        elif pot[1, 1] == pot[0, 1]:
            assert Dm[0, 1] == 0
        else:
            assert Dm[0, 1] == pot[1, 1] - pot[0, 1] > 0
        err = np.abs(Dm - want)
        print("distances n={}: worst {:.2e} of the bound".format(n, float((err / np.maximum((n + 4) * U * want, 1e-300)).max())))
        assert np.all(err <= (n + 4) * U * want)


def test_potential_distances_in_row_blocks():
    """4,096 rows (``LANDMARK_MAX``): above ``PAIRS_PER_CALL`` pairs the rows go through the library's kernel in four blocks.  Eight
    columns keep the host reference cheap; the bound is that of a sum of 8 squares, ``(8 + 4) u``."""
    from meld_amd.phate import PAIRS_PER_CALL, distances_device

    n = 4096
    assert n * n > PAIRS_PER_CALL >= 2048 * 2048
    pot = np.random.default_rng(4096).uniform(0.5, 16.0, size=(n, 8))
    pot[1500] = pot[7]  # (duplicates in different blocks)
    pot[4095] = pot[7]
    pot[2047, 3] = np.nextafter(pot[1023, 3], np.inf)
    pot[2047, [0, 1, 2, 4, 5, 6, 7]] = pot[1023, [0, 1, 2, 4, 5, 6, 7]]
    Dm = distances_device(torch.from_numpy(pot).cuda()).cpu().numpy()
    want = cdist(pot, pot)
    assert Dm.shape == (n, n) and np.all(np.diag(Dm) == 0) and np.array_equal(Dm, Dm.T)
    assert Dm[7, 1500] == 0 and Dm[7, 4095] == 0 and Dm[1500, 4095] == 0
    assert Dm[1023, 2047] == pot[2047, 3] - pot[1023, 3] > 0
    assert np.all(np.abs(Dm - want) <= (8 + 4) * U * want)


# -- operator, power, potential -------------------------------------------------------------------------------------------------------
_OPERATORS = {}


def _operator(kind):
    if kind not in _OPERATORS:
        from meld_amd.graph import DeviceGraph
        from meld_amd.phate import operator_device

        G = DeviceGraph.from_scipy(_MAKERS[kind](257))
        P = operator_device(G)
        host = P.cpu().numpy()
        want = np.asarray(G.diff_op.todense())
        inv = G._inv_perm_host()
        assert inv is None  # (257 cells: the builder does not permute)
        assert host.shape == (257, 257) and np.all(host >= 0)
        # (row sums in two orders over at most 257 entries, a division against a product with the reciprocal)
        np.testing.assert_allclose(host, want, rtol=2 * (257 + 3) * U, atol=0)
        assert np.array_equal(host == 0, want == 0)
        _OPERATORS[kind] = (P, host)
    return _OPERATORS[kind]


@pytest.mark.parametrize("t", [1, 2, 7, 16])
@pytest.mark.parametrize("kind", ["path", "star", "random"])
def test_power_and_potential(kind, t):
    from meld_amd.phate import potential_device, power_device

    P, host = _operator(kind)
    n = host.shape[0]
    Pt = power_device(P, t)
    assert Pt.data_ptr() != P.data_ptr() and torch.equal(P.cpu(), torch.from_numpy(host))  # (the operator is not written)
    want = np.linalg.matrix_power(host, t)
    bound = 2 * t * (n + 1) * U
    got = Pt.cpu().numpy()
    err = np.abs(got - want)
    print("{} t={}: P^t worst {:.2e} of the bound".format(kind, t, float((err / np.maximum(bound * want, 1e-300)).max())))
    assert np.all(err <= bound * want)
    pot = potential_device(Pt, 1).cpu().numpy()
    assert np.all(np.abs(pot - ref.potential(want, 1)) <= bound)
    assert torch.equal(potential_device(Pt, -1), Pt)
    root = potential_device(Pt, 0).cpu().numpy()
    assert np.all(np.abs(root - ref.potential(want, 0)) <= bound * ref.potential(want, 0))
    with pytest.raises(ValueError, match="gamma=1.5"):
        potential_device(Pt, 1.5)


def test_classical_step_recovers_a_configuration():
    """257 points drawn in R^3 (tests/test_phate_host.py: the reference reproduces their distances to 1.1e-15 of the diameter):
    1e-12 on the device too, the columns signed by their largest entry."""
    from meld_amd.phate import classical_mds_device

    X = np.random.default_rng(5).normal(size=(257, 3))
    Dm = cdist(X, X)
    Z, w = classical_mds_device(torch.from_numpy(Dm).cuda(), 3)
    Z = Z.cpu().numpy()
    assert Z.shape == (257, 3) and np.all(np.diff(w.cpu().numpy()) <= 0)
    assert np.abs(cdist(Z, Z) - Dm).max() <= 1e-12 * Dm.max()
    for c in range(3):
        assert Z[np.argmax(np.abs(Z[:, c])), c] > 0


# -- the whole path ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree():
    import pandas as pd

    import meld_amd

    X = _tree(200, 10, 0)
    frame = pd.DataFrame(X, index=["cell{}".format(i) for i in range(X.shape[0])])
    op = meld_amd.MELD(knn=5, decay=40, anisotropy=0, verbose=False).fit(frame)
    assert op.graph.N == 600
    return op, X


def _host_stress_check(rec):
    Dm = rec.distances_device.cpu().numpy()
    Z = rec.landmark_embedding
    n, dim = Z.shape
    want = ref.stress(Dm, Z)
    print("stress {:.6e} (host {:.6e}), normalised^2 {:.4f} -> {:.4f}, {} steps".format(
        rec.stress, want, rec.info["initial_stress"] / (0.5 * (Dm * Dm).sum()), rec.normalized_stress ** 2, rec.iterations))
    assert abs(rec.stress - want) <= 2 * (n + dim + 4) * U * want
    assert rec.stress <= rec.info["initial_stress"]
    assert abs(rec.normalized_stress - np.sqrt(want / (0.5 * (Dm * Dm).sum()))) <= 1e-12
    return Dm


def test_direct_route(tree):
    from meld_amd.phate import CHECK_EVERY, singular_values

    op, X = tree
    G = op.graph
    rec = G.phate()
    assert G.phate() is rec  # (kept per argument set)
    assert rec.landmarks is None and rec.info["route"] == "direct" and rec.info["n"] == 600
    # t: comparable where the knee's margin exceeds 1e-6 relative
    s = singular_values(rec.operator_device)
    h = ref.entropy_curve(s, 100)
    errs = np.sort(ref.knee_errors(h)[1:-1])
    margin = (errs[1] - errs[0]) / errs[0]
    print("t = {}, knee margin {:.2e}".format(rec.t, margin))
    assert margin > 1e-6
    assert rec.t == max(ref.knee(h), 1)
    np.testing.assert_allclose(rec.entropy, h, rtol=1e-12)
    # the stopping rule, read from the log
    k, log = rec.iterations, rec.stress_log
    assert log.shape == (k + 1,) and k % CHECK_EVERY == 0 and 0 < k < 3000
    assert log[k - 2] - log[k - 1] <= 1e-6 * log[k - 2]
    for c in range(CHECK_EVERY, k, CHECK_EVERY):
        assert log[c - 2] - log[c - 1] > 1e-6 * log[c - 2]
    assert np.all(np.diff(log) <= 1e-12 * log[:-1])  # (the stress never rises)
    _host_stress_check(rec)
    assert rec.embedding.shape == (600, 2) and G.perm is None and np.array_equal(rec.embedding, rec.landmark_embedding)
    assert tuple(rec.potential_device.shape) == (600, 600) and tuple(rec.distances_device.shape) == (600, 600)
    Y = X[5:55]
    np.testing.assert_allclose(rec.transform(Y), G.interpolate(rec.embedding, Y=Y), rtol=1e-12, atol=1e-14)
    classic = G.phate(mds="classic", t=rec.t)
    assert classic.iterations == 0 and classic.stress_log is None
    # (the same library calls on the same operands; GEMM and eigh promise no bit-equality between calls)
    torch.testing.assert_close(classic.landmark_embedding_device, rec.initial_embedding_device, rtol=1e-9, atol=1e-9)
    assert abs(classic.stress - rec.info["initial_stress"]) <= 1e-9 * classic.stress


def test_landmark_route_against_64_reference_steps(tree):
    op, X = tree
    G = op.graph
    lab = (np.arange(600) * 64) // 600  # (64 runs of cells along the branches)
    rec = G.phate(clusters=lab, eps=0, max_iter=64)
    lm = rec.landmarks
    assert lm is G.landmarks(clusters=lab) and lm.n_landmark == 64 and rec.iterations == 64 and rec.info["route"] == "landmarks"
    assert rec.operator_device is lm.landmark_op_device
    Dm = _host_stress_check(rec)
    Z = rec.initial_embedding_device.cpu().numpy()
    n, dim = Z.shape
    tol = np.zeros_like(Z)
    for _ in range(64):
        Z, _, scale = ref.smacof_step(Dm, Z)
        tol += 2 * (n + dim + 6) * U * scale / n
    err = np.abs(rec.landmark_embedding - Z)
    print("64 steps: worst {:.2e} of the bound".format(float((err / (16 * tol)).max())))
    assert np.all(err <= 16 * tol)
    # cells: the transitions applied to the landmark coordinates
    assert rec.embedding.shape == (600, 2)
    np.testing.assert_allclose(rec.embedding, lm.transitions @ rec.landmark_embedding, rtol=1e-12, atol=1e-14)
    Y = X[5:55]
    np.testing.assert_allclose(rec.transform(Y), lm.interpolate(rec.landmark_embedding, Y=Y), rtol=1e-12, atol=1e-14)
    assert tuple(rec.transform_device(torch.from_numpy(Y)).shape) == (50, 2)
    with pytest.raises(ValueError, match="n_components=2"):
        G.phate(clusters=np.arange(600) % 2)


def test_estimator_frame_and_benchmarker(tree):
    import meld_amd

    op, X = tree
    frame = op.phate()
    assert list(frame.columns) == ["PHATE1", "PHATE2"] and list(frame.index) == ["cell{}".format(i) for i in range(600)]
    assert np.array_equal(frame.values, op.graph.phate().embedding)
    three = op.phate(n_components=3, t=op.graph.phate().t)
    assert list(three.columns) == ["PHATE1", "PHATE2", "PHATE3"] and three.shape == (600, 3)
    bm = meld_amd.Benchmarker(seed=0)
    bm.set_phate(three.values)
    pdf = bm.generate_ground_truth_pdf()
    # (an embedding that is centred already is taken as it is -- the reference's rule -- so the logistic saturates at these scales)
    assert pdf.shape == (600,) and np.all((pdf >= 0) & (pdf <= 1)) and pdf.min() < 0.5 < pdf.max()
    assert np.array_equal(bm.data_phate, three.values)
