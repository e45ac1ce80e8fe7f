"""Contract tests of the Lanczos kernels behind ``lmax`` -- ``meld_lanczos_steps``, the phases ``meld_lanczos_spmv / _alpha / _axpy /
_beta``, the folded form ``meld_lanczos_fold / _axpy3`` (csrc/spmm.hip, csrc/spmm_tiled.hip) -- step by step against
tests/lanczos_reference.py (long double; tests/test_lanczos_reference.py shows on the host that the contract holds for three fp64
implementations and fails for a dropped entry, a beta of the wrong iteration and fp32 weights against the fp64 reference), and of the two
vector kernels ``meld_scale_f64`` / ``meld_axpby_f64``.

Every test runs on the CSR-stream kernel (``HipOps(spmm="csr")``, reference weights W in fp64) and on the tiled layout
(``spmm="tiled"``, reference weights rounded to fp32 and widened: what ``pt_step`` streams when the scalars come from the device), on
the matrices of the reference module: M3 (2 steps), M70, M257, M257log (weights 1e-4 .. 1), M4481 (an empty row, a 300-entry row, 18
tiled blocks, 141 CSR workgroups) and M20000 (256 tiled blocks, 79 axpy workgroups: the 64 dot slots are shared), 16 steps each.

After iteration ``it`` the three rotating vectors are still in ``V``; the step is recomputed from the device's own ``u_prev`` and ``u``
and compared with ``alphas[it]``, the new vector and ``betas[it]``:
    |alpha - alpha_ref| <= 4 tau A,   |w[i] - w_ref[i]| <= 8 tau g[i] for every i,   |beta - beta_ref| <= 8 tau |g|_2,
    tau = (n + longest row + 16) 2^-53, A and g the majorants of the reference module -- derived there, not measured, and not to be
widened: a step beyond them is a finding.  A beta read back later than the step that made it (the tiled loop writes ``betas[it - 1]``
from the next SpMV; the folded form knows beta one iteration late) is held to the bound of the step that made it.

Largest fraction of each bound used on the MI355X (alpha / w / beta), per form and layout, over all matrices and steps -- each test
prints its own:
    form                                   CSR-stream kernel            tiled layout
    meld_lanczos_steps, fresh calls        6.9e-3 / 2.0e-3 / 4.4e-4     6.9e-3 / 2.2e-3 / 4.4e-4
    meld_lanczos_steps, cut into calls     6.9e-3 / 2.0e-3 / 4.4e-4     6.9e-3 / 2.3e-3 / 4.4e-4
    meld_lanczos_steps, with a stop word   1.3e-3 / 9.9e-4 / 1.0e-4     1.0e-3 / 1.4e-3 / 9.2e-5
    phases                                 6.9e-3 / 2.0e-3 / 4.4e-4     6.9e-3 / 2.2e-3 / 4.4e-4
    folded                                 5.4e-2 / 1.4e-2 / 1.6e-4     5.4e-2 / 1.4e-2 / 2.0e-4
(the largest are those of M3, whose tau counts 21 roundings for sums of 3 terms; from M70 up nothing passes 1e-2.)  Earlier betas of
a multi-iteration call against the norms of the run's own vectors: at most 3.4e-2 of tau |u| (M3), 1.1e-2 from M70 up; against the
runs that verified them, where the trajectory was reproduced: at most 2.7e-4 of the bound.  ``meld_axpby_f64``: y uses up to 0.81 of
2^-52 (|a x| + |b y|) -- the bound is two roundings and the kernel makes two -- the slot sum at most 1e-2 of its bound.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import lanczos_reference as lr

pytestmark = pytest.mark.gpu

LD = lr.LD
U = lr.U
LAYOUTS = ("csr", "tiled")
WORST = {}  # (form, layout) -> largest fraction of the (alpha, w, beta) bounds seen in this process


def _note(form, layout, fractions):
    cur = WORST.setdefault((form, layout), [0.0, 0.0, 0.0])
    for i, f in enumerate(fractions):
        if f is not None:
            cur[i] = max(cur[i], float(f))


def _report(form, layout, what=""):
    print("%-8s %-5s %s: largest fraction of the bounds so far  alpha %.2e  w %.2e  beta %.2e" % ((form, layout, what) + tuple(WORST[(form, layout)])))


@pytest.fixture(scope="module", autouse=True)
def _figures():
    """The table of the module docstring, printed once the module's tests have run."""
    yield
    for (form, layout), f in sorted(WORST.items()):
        print("\n%-8s %-5s  alpha %.1e  w %.1e  beta %.1e" % ((form, layout) + tuple(f)), end="")
    print()


def _case(name, layout):
    from meld_amd.graph import DeviceGraph, HipOps

    W, dw, k = lr.matrix(name)
    G = DeviceGraph.from_scipy(W)
    assert np.array_equal(G.dw_dev.cpu().numpy(), dw)
    n = W.shape[0]
    idx = torch.arange(n, dtype=torch.float64, device="cuda")  # the driver's own start vector (filter.lanczos_lmax, seed 0)
    u0 = torch.frac(torch.sin(idx * 12.9898 + 1.0) * 43758.5453) - 0.5
    return SimpleNamespace(name=name, layout=layout, G=G, ops=HipOps(spmm=layout), W=W, dw=dw, k=k, n=n, u0=u0,
                           Wref=lr.weights(name, layout == "tiled"))


def _layout_taken(c):
    assert c.G.info["spmm"] == c.layout, c.G.info
    if c.layout == "tiled":
        assert c.G.pt["nb"] >= 1
        if c.name == "M4481":
            assert c.G.pt["nb"] > 1
        if c.name == "M20000":
            assert c.G.pt["nb"] > c.ops.dot_slots()


def _fresh(c):
    """The buffers of a run, exactly as ``filter._lanczos_lmax_device`` sets them up."""
    dev, slots = c.G.val.device, c.ops.dot_slots()
    V = torch.zeros(3, c.n, dtype=torch.float64, device=dev)
    V[1].copy_(c.u0)
    state = torch.zeros(8, dtype=torch.float64, device=dev)
    inv = 1.0 / torch.linalg.vector_norm(V[1])
    state[0] = inv
    state[3] = inv
    ab = torch.zeros(2, c.k + 1, dtype=torch.float64, device=dev)
    scratch = torch.zeros(8 * slots, dtype=torch.float64, device=dev)
    return SimpleNamespace(V=V, state=state, alphas=ab[0], betas=ab[1], scratch=scratch)


def _steps(c, r, it, m, stop=None):
    c.ops.lanczos_steps(c.G, r.V, r.state, r.alphas, r.betas, it, m, r.scratch, stop)


def _check_last(c, r, it, form="steps"):
    """Step ``it`` from the state the device left; returns (reference beta, its bound) for later reads of ``betas[it]``."""
    V, alphas, betas = r.V.cpu().numpy(), r.alphas.cpu().numpy(), r.betas.cpu().numpy()
    f, ref = lr.check_after(c.Wref, c.dw, V, it, alphas[it], betas[it])
    _note(form, c.layout, f)
    assert max(f) <= 1.0, (c.name, c.layout, form, it, f)
    return ref.beta, lr.beta_bound(ref)


def _beta_fraction(beta_dev, verified):
    return float(lr._fraction(LD(beta_dev) - verified[0], verified[1]))


def _cuts(pattern, k):
    out, it = [], 0
    for m in pattern:
        m = min(m, k - it)
        if m > 0:
            out.append((it, m))
            it += m
    assert it == k
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# meld_lanczos_steps
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", lr.NAMES)
def test_every_iteration_of_a_multi_iteration_call(name, layout):
    """For m = 1 .. K a fresh call of m iterations; step m - 1 is checked from the state it leaves: interior iterations at both
    parities, the closing beta launch, and -- ``betas[it - 1]`` of the tiled loop is written by the NEXT SpMV -- the earlier betas
    of run m, two ways:
      * the last two against the norms of the run's own vectors (beta_{m-2} = |u|, beta_{m-3} = |u_prev| as the device left them;
        the square root of a sum of n squares: within tau of it).  Over m = 2 .. K that is every write of every SpMV, twice.
      * beta_j against the reference and the bound of run j + 1, which verified step j -- wherever run m reproduced that run bit
        for bit up to step j (``alphas[:j + 1]`` equal), so that both speak of the same step.  Two runs are not the same run where
        partial sums meet in unordered atomics (workgroups sharing a dot slot, waves sharing an LDS accumulator): their iterates
        differ in the last bit from the first such sum on, and the recurrence amplifies that once the top Ritz value has
        converged (the reason the contract is per step at all).  Measured on the MI355X without the condition: up to 7e9 times the
        bound at beta_13 of M257 on the tiled layout, 1e8 on M4481 / CSR -- and 1e-4 of it wherever every slot has one writer.
        Where it has (CSR-stream kernel, at most 64 workgroups of 32 rows) every comparison must have been made."""
    c = _case(name, layout)
    verified, traj, prefix, own, past, skipped = [], [], [], [], [], 0
    for m in range(1, c.k + 1):
        r = _fresh(c)
        _steps(c, r, 0, m)
        if m == 1:
            _layout_taken(c)
        verified.append(_check_last(c, r, m - 1))
        V, alphas, betas = r.V.cpu().numpy(), r.alphas.cpu().numpy(), r.betas.cpu().numpy()
        traj.append(alphas[:m].copy())
        past.append(bool(np.any(alphas[m:] != 0.0) or np.any(betas[m:] != 0.0)))
        for j in range(m - 1):
            if np.array_equal(alphas[: j + 1], traj[j]):
                prefix.append((_beta_fraction(betas[j], verified[j]), m, j))
            else:
                skipped += 1
        u_prev, u, _ = lr.rotating(V, m - 1)
        tau = LD((c.n + c.Wref.longest + 16) * U)
        for j, x in ((m - 2, u), (m - 3, u_prev)):
            if j >= 0:
                nrm = np.sqrt(lr._dot(x.astype(LD), x.astype(LD)))
                own.append((float(lr._fraction(LD(betas[j]) - nrm, tau * nrm)), m, j))
    _report("steps", layout, name)
    print("  earlier betas against the run's own vectors: largest fraction %.2e (m = %d, beta %d); against the runs that verified them:"
          " %d compared, %d not (another trajectory), largest fraction %.2e (m = %d, beta %d)"
          % (max(own) + (len(prefix), skipped) + (max(prefix) if prefix else (0.0, 0, 0))))
    assert not any(past)  # nothing written past the iterations asked for
    assert all(f <= 1.0 for f, _, _ in own), max(own)
    assert all(f <= 1.0 for f, _, _ in prefix), max(prefix)
    if layout == "csr" and c.n <= 32 * c.ops.dot_slots():
        assert skipped == 0


@pytest.mark.parametrize("pattern", [(1,) * lr.K_STEPS, (3, 1, 4, 1, 5, 2)], ids=["ones", "314152"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", lr.NAMES)
def test_seams_between_calls(name, layout, pattern):
    """One run cut into calls: the last step of every call is checked, so the scalars must survive in ``state`` / ``scratch``
    between the calls; every beta verified earlier in the run still satisfies its bound after every later call (the tiled loop
    writes ``betas[it - 1]`` again from the first SpMV of the next call); a call with n_iter = 0 in the middle changes nothing."""
    c = _case(name, layout)
    r = _fresh(c)
    cuts = _cuts(pattern, c.k)
    verified = {}
    for i, (it, m) in enumerate(cuts):
        if i == len(cuts) // 2:
            before = (r.V.clone(), r.alphas.clone(), r.betas.clone())
            _steps(c, r, it, 0)
            torch.cuda.synchronize()
            assert torch.equal(before[0], r.V) and torch.equal(before[1], r.alphas) and torch.equal(before[2], r.betas)
        _steps(c, r, it, m)
        verified[it + m - 1] = _check_last(c, r, it + m - 1, "seams")
        betas = r.betas.cpu().numpy()
        for j, v in verified.items():
            assert _beta_fraction(betas[j], v) <= 1.0, (name, layout, "beta %d after the call ending at %d" % (j, it + m - 1))
        assert not betas[it + m :].any() and not r.alphas.cpu().numpy()[it + m :].any()
    _layout_taken(c)
    _report("seams", layout, name)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["M70", "M4481"])
def test_stop_word(name, layout):
    """Tiled: a call made with stop = 1 leaves V, alphas and betas bitwise untouched (at the start of a run and in the middle), and
    with stop = 0 the loop behaves as with None.  CSR: ``stop`` is ignored by contract -- the steps run and pass."""
    c = _case(name, layout)
    dev = c.G.val.device
    stop0, stop1 = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
    if layout == "tiled":
        r = _fresh(c)
        before = (r.V.clone(), r.alphas.clone(), r.betas.clone())
        _steps(c, r, 0, 3, stop1)
        torch.cuda.synchronize()
        _layout_taken(c)
        assert torch.equal(before[0], r.V) and torch.equal(before[1], r.alphas) and torch.equal(before[2], r.betas)
    r = _fresh(c)
    live = stop0 if layout == "tiled" else stop1
    for it, m in ((0, 2), (2, 3)):
        _steps(c, r, it, m, live)
        _check_last(c, r, it + m - 1, "stop")
    _layout_taken(c)
    if layout == "tiled":
        before = (r.V.clone(), r.alphas.clone(), r.betas.clone())
        _steps(c, r, 5, 3, stop1)
        torch.cuda.synchronize()
        assert torch.equal(before[0], r.V) and torch.equal(before[1], r.alphas) and torch.equal(before[2], r.betas)
    _report("stop", layout, name)


# ---------------------------------------------------------------------------------------------------------------------------------
# the phases and the folded form, driven as filter.py drives them (comm = None)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", lr.NAMES)
def test_phases_form(name, layout):
    c = _case(name, layout)
    for it, V, alphas, betas in lr.drive_phases(c.ops, c.G, c.u0, c.k):
        f, _ = lr.check_after(c.Wref, c.dw, V, it, float(alphas[it]), float(betas[it]))
        _note("phases", layout, f)
        assert max(f) <= 1.0, (name, layout, it, f)
    assert it == c.k - 1
    _layout_taken(c)
    _report("phases", layout, name)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", lr.NAMES)
def test_folded_form(name, layout):
    """``betas[k]`` becomes available at iteration k + 1 and is checked then, against the reference of step k."""
    c = _case(name, layout)
    prev = None
    for it, V, alphas, betas in lr.drive_folded(c.ops, c.G, c.u0, c.k):
        (fa, fw, _), ref = lr.check_after(c.Wref, c.dw, V, it, float(alphas[it]))
        fb = None if prev is None else _beta_fraction(float(betas[it - 1]), prev)
        _note("folded", layout, (fa, fw, fb))
        assert max(fa, fw, fb or 0.0) <= 1.0, (name, layout, it, fa, fw, fb)
        assert float(betas[it]) == 0.0  # not known yet
        prev = (ref.beta, lr.beta_bound(ref))
    assert it == c.k - 1
    _layout_taken(c)
    _report("folded", layout, name)


# ---------------------------------------------------------------------------------------------------------------------------------
# the converged estimate
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["M70", "M257log", "M4481"])
def test_ritz_value_of_a_converged_estimate(name, layout):
    """``_lanczos_lmax_device`` run to its stopping rule: with r = residual * theta from the returned info and
    delta = 64 * 2^-53 * lambda_max (+ 2^-24 max(dw) on the tiled layout: the norm bound of the fp32 rounding of W -- every weight
    moves by at most 2^-24 of itself, and |dW| <= its largest row sum), an eigenvalue of the dense fp64 L lies within r + delta of
    theta, and theta <= lambda_max + delta."""
    from meld_amd import filter as F

    c = _case(name, layout)
    theta, info = F._lanczos_lmax_device(c.G, c.ops, c.u0, 3e-4, 300, 5)
    torch.cuda.synchronize()
    _layout_taken(c)
    lam = lr.laplacian_spectrum(name)
    r = info["residual"] * theta
    delta = 64 * U * lam[-1] + (2.0 ** -24 * c.dw.max() if layout == "tiled" else 0.0)
    gap = float(np.abs(lam - theta).min())
    print("%s %s: theta %.12g after %d iterations, lambda_max %.12g, nearest eigenvalue at %.2e, r %.2e, delta %.2e" % (
        name, layout, theta, info["iterations"], lam[-1], gap, r, delta))
    assert info["residual"] <= 3e-4 and 0 < info["iterations"] < c.n // 2
    assert gap <= r + delta
    assert theta <= lam[-1] + delta


# ---------------------------------------------------------------------------------------------------------------------------------
# meld_scale_f64, meld_axpby_f64 (no graph: the layout does not enter)
# ---------------------------------------------------------------------------------------------------------------------------------
SIZES = [1, 255, 16385]  # one lane; one short workgroup; 65 workgroups -- slot 0 is shared -- with a last workgroup of one lane


@pytest.mark.parametrize("n", SIZES)
def test_scale_is_numpys_product_bit_for_bit(n):
    from meld_amd.graph import HipOps

    ops = HipOps()
    x = np.random.default_rng(n).normal(size=n)
    a = 0.7310585786300049
    r = torch.full((n + 1,), 7.0, dtype=torch.float64, device="cuda")
    ops.scale(torch.from_numpy(x).cuda(), a, r[:n])
    got = r.cpu().numpy()
    assert np.array_equal(got[:n], a * x) and got[n] == 7.0


@pytest.mark.parametrize("with_nrm2", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_axpby(n, with_nrm2):
    """y <- a x + b y within 2^-52 (|a x| + |b y|) per component (two rounded products and a sum, or one product and an fma: the
    compiler may contract); the slot sum within (n + 16) 2^-53 sum(y^2) of the long-double sum of the squares of the y the device
    left; the slots are zeroed by the call (they hold 7.0 before it; with one workgroup every slot but the first ends at 0)."""
    from meld_amd.graph import HipOps

    ops = HipOps()
    rng = np.random.default_rng(n + 1)
    x, y = rng.normal(size=n), rng.normal(size=n)
    a, b = 1.7, -0.3
    yd = torch.full((n + 1,), 7.0, dtype=torch.float64, device="cuda")
    yd[:n].copy_(torch.from_numpy(y))
    slots = ops.dot_slots()
    nrm2 = torch.full((slots + 1,), 7.0, dtype=torch.float64, device="cuda") if with_nrm2 else None
    ops.axpby(a, torch.from_numpy(x).cuda(), b, yd[:n], nrm2[:slots] if with_nrm2 else None)
    got = yd.cpu().numpy()
    assert got[n] == 7.0
    ax, by = LD(a) * x.astype(LD), LD(b) * y.astype(LD)
    fy = lr._fraction(got[:n].astype(LD) - (ax + by), 2.0 ** -52 * (np.abs(ax) + np.abs(by)))
    print("axpby n=%d: y uses %.2e of its bound" % (n, fy.max()))
    assert fy.max() <= 1.0
    if with_nrm2:
        s = nrm2.cpu().numpy()
        assert s[slots] == 7.0
        groups = min(2048, -(-n // 256))
        assert not s[groups:slots].any()
        ref = lr._dot(got[:n].astype(LD), got[:n].astype(LD))
        fs = float(lr._fraction(lr._sum(s[:slots].astype(LD)) - ref, (n + 16) * U * ref))
        print("axpby n=%d: slot sum uses %.2e of its bound" % (n, fs))
        assert fs <= 1.0
