"""Partial Fourier basis: the k smallest eigenpairs of the combinatorial Laplacian ``L = D - W`` at any graph size.

Stands for [UPSTREAM pygsp (development line) ``Graph.compute_fourier_basis(n_eigenvectors=k)``], which runs ARPACK on one host
core.  Here: a Chebyshev-filtered subspace iteration (Zhou & Saad) on a block of ``BLOCK = 64`` columns -- the widest
``meld_cheby_step_wide`` takes; ``k <= K_MAX = 48`` of them are wanted, the rest are guard vectors.  Per outer iteration

* the block is multiplied by a degree-``d`` Chebyshev polynomial of ``L`` that is at most 1 on ``[cut, ub]`` and grows below
  ``cut`` (``cut``: the largest Ritz value of the block, ``ub``: a rigorous upper bound of the spectrum): ``d`` calls of
  ``meld_cheby_step_wide`` ping-ponging two buffers;
* Rayleigh-Ritz: the block is orthonormalised (Gram matrix + 64 x 64 ``eigh`` on the host + rotation, applied twice), ``L V``
  is one more wide step, ``H = V^T L V``, ``eigh(H)``, ``V`` and ``L V`` are rotated, and the residual norms
  ``|L v_j - theta_j v_j|`` are one pass (``meld_block_gram_f64`` / ``meld_block_rotate_f64`` / ``meld_block_residuals_f64``,
  csrc/subspace.hip: no atomics, the same bits every run).

The iteration runs in the graph's device order on ``n_pad`` rows (padding rows are zero and stay zero); the result is brought
to the caller's order with ``meld_scatter_rows_f64``.  Nothing here sets or reads-and-modifies ``lmax`` / ``lmax_info``.
"""
from __future__ import annotations

import math

import numpy as np
import torch

K_MAX = 48  # wanted eigenpairs at most; BLOCK - K_MAX >= 16 guard vectors
BLOCK = 64  # columns of the iterated block (the widest meld_cheby_step_wide takes)
DENSE_SLICE_N = 128  # up to here the dense decomposition is sliced (a 64-wide block makes no sense)
# Degree policy: the filter's growth at eigenvalue 0 relative to its bound 1 on [cut, ub] is cosh(d acosh(x0)), x0 = (ub + cut) /
# (ub - cut).  d is the smallest degree that reaches AMPLIFICATION there, within [DEGREE_MIN, DEGREE_MAX]: the block's condition
# number after the filter stays below ~AMPLIFICATION, which the Gram-matrix orthonormalisation (it squares the condition number)
# can take in fp64; and a wide interval (early iterations, cut ~ ub / 2) gets a short filter, a narrow one the full DEGREE_MAX.
AMPLIFICATION = 1e6
DEGREE_MIN = 2
DEGREE_MAX = 60
CUT_MAX = 0.95  # cut <= CUT_MAX * ub: the damped interval never degenerates


def check_k(k):
    """``k`` as an int in [1, K_MAX]; TypeError for a non-integer, ValueError naming the limit otherwise."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError("n_eigenvectors must be an integer, got {!r}".format(k))
    k = int(k)
    if k < 1 or k > K_MAX:
        raise ValueError("n_eigenvectors must be in [1, {}] (the iterated block has {} columns, {} or more of them guard vectors; more "
                         "eigenpairs need deflation), got {}".format(K_MAX, BLOCK, BLOCK - K_MAX, k))
    return k


def upper_bound(G):
    """A rigorous upper end of the spectrum, ``(ub, rule)``: the graph's ``lmax`` only where the device Lanczos estimate produced
    it (1.01 x a converged Ritz value), else Gershgorin's ``2 max(dw)``.  An injected ``lmax`` is never used -- a filter whose
    interval misses lambda_max diverges -- and nothing is written to the graph."""
    if G._lmax is not None and G.lmax_info.get("method") == "lanczos":
        return float(G._lmax), "lanczos"
    return 2.0 * float(G.dw_dev.max()), "gershgorin"


def filter_interval(cut, ub):
    """Centre ``c``, half-width ``h`` of the damped interval ``[cut, ub]`` and the ``(alpha, beta, gamma)`` of the first and of
    every later step of ``meld_cheby_step_wide``: ``T_1 = (L - c) T_0 / h``, ``T_s = 2 (L - c) T_{s-1} / h - T_{s-2}``."""
    cut, ub = float(cut), float(ub)
    if not (ub > 0.0 and cut < ub):
        raise ValueError("the damped interval needs cut < ub, ub > 0 (cut={}, ub={})".format(cut, ub))
    c, h = 0.5 * (ub + cut), 0.5 * (ub - cut)
    return c, h, (1.0 / h, -c / h, 0.0), (2.0 / h, -2.0 * c / h, -1.0)


def filter_degree(cut, ub):
    """The degree policy (see AMPLIFICATION)."""
    c, h, _, _ = filter_interval(cut, ub)
    d = math.ceil(math.acosh(AMPLIFICATION) / math.acosh(c / h))
    return int(min(DEGREE_MAX, max(DEGREE_MIN, d)))


def _sym_eigh(a):
    from .graph import _eigh_one_thread

    a = 0.5 * (a + a.T)
    return _eigh_one_thread(np.ascontiguousarray(a))


def orthonormaliser(gram):
    """``S`` with ``(V S)^T (V S) = I`` for a block with Gram matrix ``gram`` (host, fp64): columns scaled to unit norm first,
    then ``Q w^{-1/2}`` of the scaled matrix's eigendecomposition; eigenvalues are floored at 1e-14 of the largest (a direction
    lost to rounding comes back as noise, which the second application orthonormalises)."""
    g = 0.5 * (gram + gram.T)
    s = 1.0 / np.sqrt(np.maximum(np.diag(g), 1e-300))
    w, q = _sym_eigh(g * s[:, None] * s[None, :])
    w = np.maximum(w, 1e-14 * max(float(w[-1]), 1e-300))
    return np.ascontiguousarray((s[:, None] * q) / np.sqrt(w)[None, :])


def fix_signs(U):
    """Flip each column of the device tensor ``U [N, k]`` (caller's order) so that its entry of largest magnitude is positive;
    the lowest row wins a tie."""
    n = U.shape[0]
    rows = torch.arange(n, device=U.device)
    for j in range(U.shape[1]):
        a = U[:, j].abs()
        first = torch.where(a == a.max(), rows, n).min()
        if bool(U[first, j] < 0):
            U[:, j].neg_()
    return U


def _dense_slice(G, k):
    e, U = G._dense_fourier()
    dev = G.val.device
    e_d = torch.from_numpy(np.ascontiguousarray(e[:k])).to(dev)
    U_d = fix_signs(torch.from_numpy(np.ascontiguousarray(U[:, :k])).to(dev))
    return e_d, U_d, dict(method="dense", n=G.N, k=k)


def partial_basis_device(G, k, tol=1e-6, max_iter=200, seed=0):
    """The ``k`` smallest eigenpairs of ``G``'s Laplacian as device tensors ``(e [k], U [N, k], info)``, ``e`` ascending, the rows
    of ``U`` in the caller's order, signs fixed (``fix_signs``).  RuntimeError, stating the worst residual reached, when the
    ``k`` smallest Ritz pairs do not all reach ``|L v - theta v| <= tol * ub`` within ``max_iter`` filter applications."""
    from ._device_ops import stream
    from ._lib import check, get_lib, ptr
    from .filter import _ops_of
    from .graph import _EventSpan

    k = check_k(k)
    if G.n_rows != G.N:
        raise ValueError("the Fourier basis is only defined for an unsharded graph")
    if k > G.N:
        raise ValueError("n_eigenvectors={} exceeds the {} cells of the graph".format(k, G.N))
    if G.N <= DENSE_SLICE_N:
        return _dense_slice(G, k)
    ops = _ops_of(G)
    N, n_pad, m, dev = G.N, int(G.n_pad), BLOCK, G.val.device
    ub, rule = upper_bound(G)
    if not (ub > 0.0 and math.isfinite(ub)):
        raise ValueError("the graph has no positive weight: its Laplacian is zero")
    f64 = dict(dtype=torch.float64, device=dev)
    nb = ops.block_n_blocks(N)
    part = torch.empty(nb * m * m, **f64)
    C, S, theta_d, res_d = torch.empty(m, m, **f64), torch.empty(m, m, **f64), torch.empty(m, **f64), torch.empty(m, **f64)
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    V = torch.zeros(n_pad, m, **f64)
    V[:N] = torch.randn(N, m, generator=gen, **f64)
    O = torch.zeros(n_pad, m, **f64)

    def orthonormalise(F):
        for _ in range(2):
            with _EventSpan("fourier_gram", N=N, m=m):
                ops.block_gram(F, F, N, m, part, nb, C)
            S.copy_(torch.from_numpy(orthonormaliser(C.cpu().numpy())))
            with _EventSpan("fourier_rotate", N=N, m=m):
                ops.block_rotate(F, S, N, m, F)

    def rayleigh_ritz(F, LF):
        """F orthonormal -> Ritz vectors in F, L F in LF; returns (theta, residual norms) on the host"""
        with _EventSpan("fourier_filter", N=N, m=m, steps=1):
            ops.cheby_step_wide(G, m, F, 0, None, LF, 1.0, 0.0, 0.0)
        with _EventSpan("fourier_gram", N=N, m=m):
            ops.block_gram(F, LF, N, m, part, nb, C)
        theta, Q = _sym_eigh(C.cpu().numpy())
        S.copy_(torch.from_numpy(np.ascontiguousarray(Q)))
        theta_d.copy_(torch.from_numpy(np.ascontiguousarray(theta)))
        with _EventSpan("fourier_rotate", N=N, m=m):
            ops.block_rotate(F, S, N, m, F)
            ops.block_rotate(LF, S, N, m, LF)
        with _EventSpan("fourier_residuals", N=N, m=m):
            ops.block_residuals(LF, F, theta_d, N, m, part, nb, res_d)
        return theta, np.sqrt(np.maximum(res_d.cpu().numpy(), 0.0))

    degrees = []
    orthonormalise(V)
    while True:
        theta, res = rayleigh_ritz(V, O)
        worst = float(res[:k].max())
        if worst <= tol * ub:
            break
        if len(degrees) >= max_iter:
            raise RuntimeError("partial Fourier basis: the {} smallest Ritz pairs did not converge within max_iter={} filter applications: "
                               "worst residual {:.3e} > tol * ub = {:.3e}".format(k, max_iter, worst, tol * ub))
        cut = min(float(theta[-1]), CUT_MAX * ub)
        _, _, first, later = filter_interval(cut, ub)
        d = filter_degree(cut, ub)
        degrees.append(d)
        with _EventSpan("fourier_filter", N=N, m=m, steps=d):
            prev, cur = V, O
            ops.cheby_step_wide(G, m, prev, 0, None, cur, *first)
            for _ in range(2, d + 1):
                ops.cheby_step_wide(G, m, cur, 0, prev, prev, *later)  # T_s over T_{s-2}
                prev, cur = cur, prev
        V, O = cur, prev
        orthonormalise(V)
    e = theta_d[:k].clone()
    Vk = V[:N, :k].contiguous()
    if G.perm is None:
        U = Vk
    else:
        U = torch.empty_like(Vk)
        check(get_lib().meld_scatter_rows_f64(ptr(Vk), ptr(G.perm), N, k, ptr(U), stream()), "meld_scatter_rows_f64")
    info = dict(method="chebyshev-filtered subspace iteration", n=N, k=k, block=m, ub=ub, ub_rule=rule, tol=float(tol), seed=int(seed),
                iterations=len(degrees), degrees=degrees, wide_steps=sum(degrees) + len(degrees) + 1, worst_residual=worst)
    return e, fix_signs(U), info
