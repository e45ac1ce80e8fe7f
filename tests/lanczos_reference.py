"""A plain host reference of ONE step of the Lanczos recurrence behind ``lmax`` (``meld_lanczos_steps``, the four phases
``meld_lanczos_spmv / _alpha / _axpy / _beta`` and the folded form ``meld_lanczos_fold / _axpy3``; csrc/spmm.hip, csrc/spmm_tiled.hip).

NumPy only, every sum in ``np.longdouble`` (64-bit mantissa on x86: about 2000 times finer than the kernels' fp64).  Where the platform's
long double is no finer than that (``EXTENDED`` false: eps > 2^-63) the reference stays in fp64 and forms every sum with ``math.fsum``,
i.e. exactly rounded: the products then carry one fp64 rounding each, 2^-53 of the majorants below, against bounds of at least
4 * 21 * 2^-53 of them.  Nothing is skipped in either case.

Why per step.  A whole device run cannot be compared with a long-double run: fp64 against long double on the matrices below agree to
~1e-15 in the tridiagonal entries for 5 iterations, ~1e-12 at iteration 10 and not at all by iteration 15 -- once the top Ritz value has
converged, rounding differences are amplified.  After iteration ``it`` of any of the three forms all three rotating vectors are still in
``V``: ``u_prev = V[it % 3]``, ``u = V[(it + 1) % 3]`` and the new ``w = V[(it + 2) % 3]`` (only y was overwritten), all un-normalised.
The step is recomputed here from the device's own ``u_prev`` and ``u`` and compared with what the device left; no error accumulates
from step to step and the check does not depend on the layout or on how the scalars travel (``state``, parity buffers, ``acc``).

The step (``Lref = diag(dw) - Wref``, ``dw`` as the graph holds it):
    nu = |u|, v = u / nu
    it > 0: v_prev = u_prev / |u_prev|, beta_prev = nu          it == 0: v_prev = 0, beta_prev = 0
    y = Lref v - beta_prev v_prev;  alpha = <y, v>;  w = y - alpha v;  beta = |w|
    a = dw .* |v| + |Wref| |v| + beta_prev |v_prev|;  A = <a, |v|>;  g = a + A |v|          (majorants)
    tau = (n + longest row + 16) * 2^-53
Bounds (worst-case running-error bounds: tau majorises any sum the step forms -- a dot product over n, a row of ``len`` entries; the
factors count the rounded quantities composed: the scalar, y, the product and the sum.  Derived, not measured):
    |alphas[it] - alpha| <= 4 tau A;     |V_w[i] - w[i]| <= 8 tau g[i] for every i;     |betas[it] - beta| <= 8 tau |g|_2.
``Wref`` is W in fp64 for the CSR-stream kernel; the tiled layout streams the fp32 copy of the weights whenever the scalars come from
the device and p == 1 (``pt_step``), so there ``Wref`` is W with every weight rounded to fp32 and widened again; ``dw`` stays fp64.

Also here: the matrices of the contract tests, the drivers' start vector, a numpy fp64 twin of the CSR-stream arithmetic of
``meld_lanczos_steps`` (a free function: ``filter.lanczos_lmax`` picks its driver by ``hasattr(ops, "lanczos_steps")``, so the host
stand-in ``CpuOps`` must not grow that method), and the loops of ``filter._lanczos_lmax_phases`` / ``_folded`` with ``comm = None``
written as generators that hand ``V`` back after every iteration (they run on ``CpuOps`` and on ``HipOps`` alike).
"""
import functools
import math
from collections import namedtuple

import numpy as np
from scipy import sparse

LD = np.longdouble
EXTENDED = bool(np.finfo(LD).eps <= 2.0 ** -63)  # else: fp64 with math.fsum for every sum (see above)
U = 2.0 ** -53
K_STEPS = 16  # steps checked per matrix: min(K_STEPS, n - 1), except M3 (2)

Step = namedtuple("Step", "alpha w beta a A g tau")


# ---------------------------------------------------------------------------------------------------------------------------------
# sums
# ---------------------------------------------------------------------------------------------------------------------------------
def _sum(x):
    if EXTENDED:
        return np.sum(x, dtype=LD)
    return LD(math.fsum(np.asarray(x, dtype=np.float64)))


def _dot(a, b):
    return _sum(a * b)


def _row_sums(prod, indptr):
    """Sum of every row's segment of ``prod`` (empty rows: 0)."""
    out = np.zeros(len(indptr) - 1, dtype=LD)
    nonempty = indptr[1:] > indptr[:-1]
    if not nonempty.any():
        return out
    if EXTENDED:
        # the rows without entries own no element of prod: the segments of the others are contiguous
        out[nonempty] = np.add.reduceat(prod, indptr[:-1][nonempty])
    else:
        for i in np.nonzero(nonempty)[0]:
            out[i] = math.fsum(prod[indptr[i] : indptr[i + 1]])
    return out


class RefMatrix:
    """The weights the reference multiplies by: CSR pattern of W, values in long double."""

    def __init__(self, W):
        W = sparse.csr_matrix(W).astype(np.float64)
        W.sort_indices()
        self.csr = W
        self.n = int(W.shape[0])
        self.indptr = W.indptr.astype(np.int64)
        self.indices = W.indices.astype(np.int64)
        self.data = W.data.astype(LD)
        self.absdata = np.abs(self.data)
        self.longest = int(np.diff(self.indptr).max()) if self.n else 0

    def matvec(self, x, absolute=False):
        d = self.absdata if absolute else self.data
        return _row_sums(d * np.asarray(x, dtype=LD)[self.indices], self.indptr)


def reference_weights(W, fp32):
    """``Wref``: W in fp64 (the CSR-stream kernel), or with every weight rounded to fp32 and widened again (the tiled layout)."""
    W = sparse.csr_matrix(W).astype(np.float64).copy()
    if fp32:
        W.data = W.data.astype(np.float32).astype(np.float64)
    return RefMatrix(W)


def degrees(W):
    """``dw`` as ``DeviceGraph.from_scipy`` forms it."""
    return np.ravel(sparse.csr_matrix(W).sum(1)).astype(np.float64)


def dense_laplacian(W, dw):
    """fp64 dense ``diag(dw) - W`` (``W``: scipy matrix or RefMatrix), for ``numpy.linalg.eigvalsh``."""
    W = W.csr if isinstance(W, RefMatrix) else sparse.csr_matrix(W)
    return np.diag(np.asarray(dw, dtype=np.float64)) - W.toarray()


# ---------------------------------------------------------------------------------------------------------------------------------
# the step and its check
# ---------------------------------------------------------------------------------------------------------------------------------
def step(Wref, dw, u_prev, u, it):
    """(alpha, w, beta, a, A, g, tau) of iteration ``it`` from the rotating vectors as they stood BEFORE it (module docstring)."""
    dwl = np.asarray(dw, dtype=LD)
    u = np.asarray(u, dtype=LD)
    nu = np.sqrt(_dot(u, u))
    v = u / nu
    if it > 0:
        up = np.asarray(u_prev, dtype=LD)
        v_prev = up / np.sqrt(_dot(up, up))
        beta_prev = nu
    else:
        v_prev = np.zeros_like(v)
        beta_prev = LD(0)
    y = dwl * v - Wref.matvec(v) - beta_prev * v_prev
    alpha = _dot(y, v)
    w = y - alpha * v
    beta = np.sqrt(_dot(w, w))
    av, avp = np.abs(v), np.abs(v_prev)
    a = dwl * av + Wref.matvec(av, absolute=True) + beta_prev * avp
    A = _dot(a, av)
    g = a + A * av
    tau = LD((Wref.n + Wref.longest + 16) * U)
    return Step(alpha, w, beta, a, A, g, tau)


def _fraction(diff, bound):
    """|diff| / bound, elementwise; 0 / 0 = 0, anything else over 0 = inf; not-a-number counts as inf."""
    diff, bound = np.abs(np.asarray(diff, dtype=LD)), np.asarray(bound, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(bound > 0, diff / np.where(bound > 0, bound, 1), np.where(diff == 0, 0.0, np.inf))
    return np.where(np.isnan(f), np.inf, f).astype(np.float64)


def beta_bound(ref):
    return 8 * ref.tau * np.sqrt(_dot(ref.g, ref.g))


def check_step(ref, alpha_dev, w_dev, beta_dev=None):
    """The fractions of the three bounds that (alphas[it], V_w, betas[it]) use against ``ref = step(...)``: each must be <= 1
    (the third is None when ``beta_dev`` is, i.e. where the form knows beta one iteration late)."""
    fa = float(_fraction(LD(alpha_dev) - ref.alpha, 4 * ref.tau * ref.A))
    fw = float(_fraction(np.asarray(w_dev, dtype=LD) - ref.w, 8 * ref.tau * ref.g).max())
    fb = None if beta_dev is None else float(_fraction(LD(beta_dev) - ref.beta, beta_bound(ref)))
    return fa, fw, fb


def rotating(V, it):
    """(u_prev, u, w) of iteration ``it`` in the [3, n] buffer, as numpy fp64 arrays (``V``: ndarray or tensor)."""
    Vn = V if isinstance(V, np.ndarray) else V.detach().cpu().numpy()
    return Vn[it % 3], Vn[(it + 1) % 3], Vn[(it + 2) % 3]


def check_after(Wref, dw, V, it, alpha_dev, beta_dev=None):
    """``check_step`` of iteration ``it`` from the buffer it left; returns (fractions, ref)."""
    u_prev, u, w = rotating(V, it)
    ref = step(Wref, dw, u_prev, u, it)
    return check_step(ref, alpha_dev, w, beta_dev), ref


def reference_run(Wref, dw, u0, k):
    """k steps of the recurrence entirely in long double: (alphas, betas) as fp64 arrays of the long-double values."""
    u_prev, u = np.zeros(Wref.n, dtype=LD), np.asarray(u0, dtype=LD)
    alphas, betas = np.zeros(k), np.zeros(k)
    for it in range(k):
        r = step(Wref, dw, u_prev, u, it)
        alphas[it], betas[it] = float(r.alpha), float(r.beta)
        u_prev, u = u, r.w
    return alphas, betas


def ritz_top(alphas, betas, k):
    """(theta, |beta_k s_k|) of the k-prefix of the tridiagonal: its top eigenvalue and the residual norm of its Ritz vector."""
    T = np.diag(np.asarray(alphas[:k], dtype=np.float64))
    if k > 1:
        off = np.asarray(betas[: k - 1], dtype=np.float64)
        T += np.diag(off, 1) + np.diag(off, -1)
    ev, evec = np.linalg.eigh(T)
    return float(ev[-1]), abs(float(betas[k - 1]) * float(evec[-1, -1]))


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def start_vector(n):
    """The drivers' own start vector (``filter.lanczos_lmax``, seed 0): frac(sin(12.9898 i + 1) * 43758.5453) - 0.5."""
    x = np.sin(np.arange(n, dtype=np.float64) * 12.9898 + 1.0) * 43758.5453
    return (x - np.trunc(x)) - 0.5


def awkward_matrix(n, density, seed=None, legacy_pattern=True):
    """The random symmetric matrices of ``test_gpu_tiled._awkward_matrix``, entry for entry: weights in [0.1, 1.1], and for n > 100
    an empty row (5) and a row of ~300 entries (7).  ``seed`` defaults to n, as there.  ``legacy_pattern=False`` draws the pattern
    from a ``numpy.random.Generator`` instead of the integer seed: ``sparse.random`` with an integer seed permutes all n^2
    positions, 25 s at n = 20000."""
    seed = n if seed is None else seed
    rng = np.random.default_rng(seed)
    A = sparse.random(n, n, density=density, random_state=seed if legacy_pattern else np.random.default_rng(seed + 1), format="coo",
                      dtype=np.float64)
    r, c = A.row.astype(np.int64), A.col.astype(np.int64)
    if n > 100:
        keep = (r != 5) & (c != 5)  # an empty row ...
        long_row = rng.choice(n, size=min(n, 300), replace=False)  # ... and a long one
        r, c = np.concatenate([r[keep], np.full(len(long_row), 7)]), np.concatenate([c[keep], long_row])
    A = sparse.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))  # (only the pattern is used)
    W = (A + A.T).tocsr()
    W.setdiag(0)
    W.eliminate_zeros()
    W.data = rng.random(W.nnz) + 0.1
    W = ((W + W.T) * 0.5).tocsr()
    W.sort_indices()
    return W


def _m3():
    return sparse.csr_matrix(np.array([[0, 1.0, 0], [1.0, 0, 2.0], [0, 2.0, 0]]))


def _m257log():
    """The pattern of M257 with weights 10^(-4 U) in [1e-4, 1], the range of the kernel weights (thresh = 1e-4): the smallest
    entries must count."""
    P = sparse.triu(awkward_matrix(257, 0.05), k=1).tocoo()
    rng = np.random.default_rng(2570)
    vals = 10.0 ** (-4.0 * rng.random(P.nnz))
    H = sparse.coo_matrix((vals, (P.row, P.col)), shape=P.shape).tocsr()
    W = (H + H.T).tocsr()
    W.sort_indices()
    return W


_MAKERS = {
    "M3": (_m3, 2),  # the 3-vertex path: one workgroup, rows of 1 and 2 entries
    "M70": (lambda: awkward_matrix(70, 0.3), K_STEPS),
    "M257": (lambda: awkward_matrix(257, 0.05), K_STEPS),
    "M257log": (_m257log, K_STEPS),
    "M4481": (lambda: awkward_matrix(4481, 0.004), K_STEPS),  # 18 tiled blocks, 141 CSR workgroups: the 64 dot slots are shared
    "M20000": (lambda: awkward_matrix(20000, 0.0005, legacy_pattern=False), K_STEPS),  # meld_pt_num_blocks = 256 > 64 slots, 79 axpy workgroups > 64
}
NAMES = tuple(_MAKERS)
FROM_M70 = NAMES[1:]


@functools.lru_cache(maxsize=None)
def matrix(name):
    """(W, dw, steps) of a named matrix; built once per process and not to be modified."""
    W = _MAKERS[name][0]()
    return W, degrees(W), min(_MAKERS[name][1], W.shape[0] - 1)


@functools.lru_cache(maxsize=None)
def weights(name, fp32):
    """``reference_weights`` of a named matrix, once per process."""
    return reference_weights(matrix(name)[0], fp32)


@functools.lru_cache(maxsize=None)
def laplacian_spectrum(name, fp32=False):
    """Ascending eigenvalues of the dense fp64 ``diag(dw) - Wref`` (``numpy.linalg.eigvalsh``), the largest one polished, once per
    process.  The dense solver's own error grows with n -- at n = 4481 its lambda_max is 72 * 2^-53 * lambda_max BELOW the top Ritz
    value of 8 long-double Lanczos steps, which cannot exceed lambda_max -- and the tests allow 64 * 2^-53 * lambda_max in all.  So
    the top eigenvalue is replaced by the long-double Rayleigh quotient of its eigenvector (ARPACK, fp64, fixed start): never above
    lambda_max, and short of it by at most the residual norm, which ``top_residual`` returns and the host test holds to
    16 * 2^-53 * lambda_max."""
    lam = np.linalg.eigvalsh(dense_laplacian(weights(name, fp32), matrix(name)[1])).copy()
    rho, _ = _top_rayleigh(name, fp32)
    assert abs(rho - lam[-1]) <= 1e-10 * lam[-1], (name, rho, lam[-1])  # (the same eigenvalue)
    lam[-1] = rho
    return lam


@functools.lru_cache(maxsize=None)
def _top_rayleigh(name, fp32):
    from scipy.sparse.linalg import eigsh

    Wref, dw = weights(name, fp32), matrix(name)[1]
    n = Wref.n
    if n <= 3:
        x = np.linalg.eigh(dense_laplacian(Wref, dw))[1][:, -1]
    else:
        _, x = eigsh(sparse.diags(dw) - Wref.csr, k=1, which="LA", tol=0, v0=np.ones(n), maxiter=50 * n)
    x = np.ravel(x).astype(LD)
    x /= np.sqrt(_dot(x, x))
    Lx = np.asarray(dw, dtype=LD) * x - Wref.matvec(x)
    rho = _dot(Lx, x)
    res = Lx - rho * x
    return float(rho), float(np.sqrt(_dot(res, res)))


def top_residual(name, fp32=False):
    """|L x - rho x| of the polished top eigenpair of ``laplacian_spectrum`` (long double)."""
    return _top_rayleigh(name, fp32)[1]


def drop_entry(W):
    """W without ONE stored entry (i, j) -- its mirror (j, i) stays, as when a kernel loses an entry of one row: the entry whose
    weight is closest to 0.1.  Returns (W', i, j, weight)."""
    W = sparse.csr_matrix(W).copy()
    e = int(np.argmin(np.abs(W.data - 0.1)))
    i = int(np.searchsorted(W.indptr, e, side="right") - 1)
    j, wgt = int(W.indices[e]), float(W.data[e])
    W.data[e] = 0.0
    W.eliminate_zeros()
    return W, i, j, wgt


# ---------------------------------------------------------------------------------------------------------------------------------
# numpy fp64 twin of meld_lanczos_steps, CSR-stream arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
def twin_setup(u0, k):
    """(V, state, alphas, betas) as ``filter._lanczos_lmax_device`` sets them up."""
    n = len(u0)
    V = np.zeros((3, n))
    V[1] = u0
    state = np.zeros(8)
    state[0] = state[3] = 1.0 / np.sqrt(float(V[1] @ V[1]))
    return V, state, np.zeros(k), np.zeros(k)


def twin_lanczos_steps(W, dw, V, state, alphas, betas, it_begin, n_iter, stale_beta=False):
    """Iterations [it_begin, it_begin + n_iter) in numpy fp64 with the scalars of csrc/spmm.hip: state[0] s_cur (v_k = s_cur u_k),
    [1] s_prev, [2] beta_{k-1}, [3] alpha argument of the next SpMV (= s_cur), [4] its gamma argument (= -beta_{k-1} s_prev),
    [5] a of w = y + a u (= -alpha_k s_cur).  ``stale_beta``: the mutation "beta_{k-2} for beta_{k-1}" in the gamma argument, from
    iteration 2 on."""
    for it in range(it_begin, it_begin + n_iter):
        u_prev, u, y = V[it % 3], V[(it + 1) % 3], V[(it + 2) % 3]
        y[:] = state[3] * (dw * u - W @ u) + state[4] * u_prev
        alpha = float(y @ u) * state[0]
        alphas[it] = alpha
        state[5] = -alpha * state[0]
        y += state[5] * u
        beta = float(np.sqrt(y @ y))
        betas[it] = beta
        s_cur, beta_old = state[0], state[2]
        state[1], state[2], state[0], state[3] = s_cur, beta, 1.0 / beta, 1.0 / beta
        state[4] = -(beta_old if stale_beta and it >= 1 else beta) * s_cur


# ---------------------------------------------------------------------------------------------------------------------------------
# the loops of filter._lanczos_lmax_phases / _folded, comm = None, one iteration at a time
# ---------------------------------------------------------------------------------------------------------------------------------
def drive_phases(ops, G, u0, k):
    """``filter._lanczos_lmax_phases`` for k iterations; yields (it, V, alphas, betas) after each (device tensors)."""
    import torch

    from meld_amd.filter import _local

    dev, slots = G.val.device, ops.dot_slots()
    V = torch.zeros(3, G.n_pad, dtype=torch.float64, device=dev)
    V[1].copy_(u0)
    state = torch.zeros(8, dtype=torch.float64, device=dev)
    inv = 1.0 / torch.linalg.vector_norm(V[1])
    state[0] = inv
    state[3] = inv
    alphas = torch.zeros(k + 1, dtype=torch.float64, device=dev)
    betas = torch.zeros(k + 1, dtype=torch.float64, device=dev)
    dots = torch.zeros(2 * slots, dtype=torch.float64, device=dev)
    nrm2 = torch.zeros(slots, dtype=torch.float64, device=dev)
    for i in range(k):
        u_prev, u, y = V[i % 3], V[(i + 1) % 3], V[(i + 2) % 3]
        ops.lanczos_spmv(G, u, _local(G, u_prev), _local(G, y), state, dots)
        ops.lanczos_alpha(state, dots, nrm2, alphas, i)
        ops.lanczos_axpy(_local(G, u), _local(G, y), state, nrm2)
        ops.lanczos_beta(state, nrm2, dots, betas, i)
        yield i, V, alphas, betas


def drive_folded(ops, G, u0, k):
    """``filter._lanczos_lmax_folded`` for k iterations; yields (it, V, alphas, betas) after each: ``betas[it - 1]`` is new at
    iteration ``it`` (beta is known one iteration late), ``betas[it]`` is not written yet."""
    import torch

    from meld_amd.filter import _local

    dev, slots = G.val.device, ops.dot_slots()
    V = torch.zeros(3, G.n_pad, dtype=torch.float64, device=dev)
    V[1].copy_(u0)
    state = torch.zeros(8, dtype=torch.float64, device=dev)
    state[3] = 1.0
    alphas = torch.zeros(k + 1, dtype=torch.float64, device=dev)
    betas = torch.zeros(k + 1, dtype=torch.float64, device=dev)
    acc = torch.zeros(3 * slots, dtype=torch.float64, device=dev)
    nrm2 = acc[2 * slots :]
    u_loc0 = _local(G, V[1])
    nrm2[0] = torch.dot(u_loc0, u_loc0)
    for i in range(k):
        u_prev, u, y = V[i % 3], V[(i + 1) % 3], V[(i + 2) % 3]
        ops.lanczos_spmv(G, u, _local(G, u_prev), _local(G, y), state, acc)
        ops.lanczos_fold(state, acc, alphas, betas, i)
        ops.lanczos_axpy3(_local(G, y), _local(G, u), _local(G, u_prev), state, nrm2)
        yield i, V, alphas, betas
