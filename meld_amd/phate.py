"""PHATE embedding of a fitted graph on the device: plot coordinates for every cell.

Every notebook of the reference goes from the densities to a PHATE plot, and ``Benchmarker.fit_phate`` draws its ground truth over
one.  This module restates [UPSTREAM phate 1.0.x ``phate.PHATE`` / ``phate.vne`` / ``phate.mds``, unpinned: it cannot be imported
next to this code, every stage below is this project's own definition, close to upstream as remembered].  The stages:

1. Operator ``P [n, n]``, dense, on the device: ``landmarks().landmark_op_device``, or -- where the graph has no more cells than
   ``n_landmark`` and no ``clusters`` are given (the direct route) -- the graph's ``diff_op`` made dense, rows and columns in the
   device order.
2. ``t``: a positive integer, or ``"auto"``: with ``s`` the singular values of ``P``, ``h[i] = -sum p log p`` for
   ``p = s^(i+1) / sum s^(i+1) + eps`` (``entropy_curve``), and ``t`` the knee of ``h`` (``knee``: the break point of the best fit
   by two least-squares lines).  The index shift is upstream's as remembered: ``h[0]`` belongs to power 1, the knee is read as ``t``.
3. Potential: ``Pt = P^t`` by repeated squaring (library GEMMs); ``gamma = 1``: ``U = -log(Pt + 1e-7)``; ``gamma = -1``: ``U = Pt``;
   otherwise ``U = Pt^c / c`` with ``c = (1 - gamma) / 2``.
4. Potential distances ``Dm[i, j] = |U[i] - U[j]|_2`` from direct differences (never ``|a|^2 + |b|^2 - 2ab``): equal rows are at
   distance exactly 0, the matrix is exactly symmetric.
5. Classical MDS (Torgerson): ``B = -1/2 J Dm^2 J``, the ``n_components`` largest eigenpairs, ``Z0 = V sqrt(max(lambda, 0))``, every
   column signed so that its entry of largest magnitude is positive.  (Upstream's classical step, as remembered, is a PCA of the
   centred matrix; this is the textbook form.)
6. Metric MDS by SMACOF from ``Z0`` (``csrc/mds.hip``, ``meld_smacof_step``: one launch per step, the hot loop): the Guttman
   transform with unit weights until the stress stops falling.  (Upstream's default solver is a stochastic gradient descent whose
   result cannot be reproduced; SMACOF is its documented alternative.)
7. Cells: the landmark coordinates interpolated through the transitions (``Landmarks.interpolate_device``), new cells through their
   kernel to the fitted ones.

``check_t``, ``check_arguments``, ``entropy_curve``, ``knee``, ``knee_errors`` and ``sign_columns`` are pure NumPy helpers (no
device).
"""
from __future__ import annotations

import hashlib
import numbers

import numpy as np

from ._graph_steps import require_unsharded

__all__ = ["SMACOF_MAX_DIM", "DEFAULT_N_LANDMARK", "CHECK_EVERY", "PhateEmbedding", "check_t", "check_arguments", "entropy_curve",
           "knee_errors", "knee", "sign_columns", "operator_device", "singular_values", "power_device", "potential_device",
           "distances_device", "classical_mds_device", "smacof_step_device", "smacof_device", "phate"]

SMACOF_MAX_DIM = 8  # ``meld_smacof_max_dim()`` (tests/test_phate_host.py holds the two together)
DEFAULT_N_LANDMARK = 2000  # upstream's default
CHECK_EVERY = 8  # SMACOF steps between two reads of the stress log (one sync per eight launches, as in the recurrences)
LOG_FLOOR = 1e-7  # the constant inside the log potential
PAIRS_PER_CALL = 1 << 22  # pairs of one call of the library's pairwise-distance kernel (2,048 rows of 2,048; 1,024 of 4,096)


# -- pure helpers --------------------------------------------------------------------------------------------------------------
def _is_int(x):
    return isinstance(x, (numbers.Integral, np.integer)) and not isinstance(x, (bool, np.bool_))


def check_t(t):
    """``"auto"`` or a positive integer (as ``int``); ValueError with the value otherwise."""
    if isinstance(t, str):
        if t == "auto":
            return t
        raise ValueError("t must be a positive integer or 'auto', got t={!r}".format(t))
    if not _is_int(t) or int(t) < 1:
        raise ValueError("t must be a positive integer or 'auto', got t={!r}".format(t))
    return int(t)


def check_arguments(n_components=2, t="auto", gamma=1, mds="metric", max_iter=3000, eps=1e-6, t_max=100):
    """The checked arguments of ``phate`` that do not depend on the graph, as a dict; ValueError naming the offending value."""
    if not _is_int(n_components) or not 1 <= int(n_components) <= SMACOF_MAX_DIM:
        raise ValueError("n_components must be an integer in [1, {}], got n_components={!r}".format(SMACOF_MAX_DIM, n_components))
    t = check_t(t)
    if isinstance(gamma, (bool, np.bool_)) or not isinstance(gamma, (numbers.Real, np.floating, np.integer)) or not -1 <= float(gamma) <= 1:
        raise ValueError("gamma must lie in [-1, 1], got gamma={!r}".format(gamma))
    if mds not in ("metric", "classic"):
        raise ValueError("mds must be 'metric' or 'classic' (upstream's SGD solver and non-metric MDS are not implemented), "
                         "got mds={!r}".format(mds))
    if not _is_int(max_iter) or int(max_iter) < 0:
        raise ValueError("max_iter must be an integer >= 0, got max_iter={!r}".format(max_iter))
    if isinstance(eps, (bool, np.bool_)) or not isinstance(eps, (numbers.Real, np.floating, np.integer)) or not float(eps) >= 0:
        raise ValueError("eps must be a number >= 0, got eps={!r}".format(eps))
    if not _is_int(t_max) or int(t_max) < 3:
        raise ValueError("t_max must be an integer >= 3 (the knee needs a point on either side), got t_max={!r}".format(t_max))
    return dict(n_components=int(n_components), t=t, gamma=float(gamma), mds=mds, max_iter=int(max_iter), eps=float(eps),
                t_max=int(t_max))


def entropy_curve(s, t_max=100):
    """``h [t_max]``: the von Neumann entropy of the powers 1 .. t_max of an operator with singular values ``s``:
    ``h[i] = -sum p log p`` with ``p = s^(i+1) / sum s^(i+1) + eps`` and ``eps = np.finfo(float).eps``."""
    s = np.asarray(s, dtype=np.float64).reshape(-1)
    t_max = int(t_max)
    powers = s[None, :] ** np.arange(1, t_max + 1, dtype=np.float64)[:, None]
    p = powers / powers.sum(axis=1)[:, None] + np.finfo(float).eps
    return -(p * np.log(p)).sum(axis=1)


def _line_residual(x, y):
    """Sum of the absolute residuals of the least-squares line through ``(x, y)`` (at least two distinct ``x``)."""
    xm, ym = x.mean(), y.mean()
    dx = x - xm
    slope = (dx * (y - ym)).sum() / (dx * dx).sum()
    return np.abs(y - ym - slope * dx).sum()


def knee_errors(h):
    """``err [len(h)]``: ``err[b]`` for ``b`` in ``1 .. len(h) - 2`` is the sum of the absolute residuals of two least-squares lines,
    one through the points ``0 .. b`` of ``h`` over ``x = index``, one through ``b .. len(h) - 1``; ``inf`` at both ends."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    n = h.shape[0]
    if n < 3:
        raise ValueError("the knee needs at least 3 points, got {}".format(n))
    x = np.arange(n, dtype=np.float64)
    err = np.full(n, np.inf)
    for b in range(1, n - 1):
        err[b] = _line_residual(x[: b + 1], h[: b + 1]) + _line_residual(x[b:], h[b:])
    return err


def knee(h):
    """The break point ``b`` in ``1 .. len(h) - 2`` that minimises ``knee_errors``, ties to the lowest ``b``."""
    return int(np.argmin(knee_errors(h)))


def sign_columns(Z):
    """``Z`` with every column signed so that its entry of largest magnitude is positive (the lowest index on ties)."""
    Z = np.array(Z, dtype=np.float64)
    for c in range(Z.shape[1]):
        if Z.shape[0] and Z[np.argmax(np.abs(Z[:, c])), c] < 0:
            Z[:, c] = -Z[:, c]
    return Z


# -- device side ---------------------------------------------------------------------------------------------------------------
def operator_device(G):
    """The graph's ``diff_op = D^-1 (W + diag(kd))`` as a dense fp64 device tensor ``[N, N]``, rows and columns in the device order
    (the direct route's operator)."""
    import torch

    from ._graph_steps import csr_operands
    from ._device_ops import stream
    from ._lib import check, get_lib, ptr
    from .diffuse import walk_vectors

    require_unsharded(G, "the PHATE operator is")
    kd, s = walk_vectors(G)
    N = G.N
    P = torch.empty(N, N, dtype=torch.float64, device=G.val.device)
    rowptr, col, val = csr_operands(G, G.val)
    check(get_lib().meld_csr_rows_to_dense_f64(ptr(rowptr), ptr(col), ptr(val), 1 if val.dtype == torch.float32 else 0, 0, N, N, ptr(P), N,
                                               stream()), "meld_csr_rows_to_dense_f64")
    P.diagonal().add_(kd)
    P /= s[:, None]
    return P


def singular_values(P):
    """The singular values of ``P``, descending, as a host array (one library call and one read-back)."""
    import torch

    return torch.linalg.svdvals(P).cpu().numpy()


def power_device(P, t):
    """``P^t`` for an integer ``t >= 1`` by repeated squaring (library GEMMs, binary expansion of ``t`` from the low bit)."""
    t = int(t)
    if t < 1:
        raise ValueError("t must be a positive integer, got t={!r}".format(t))
    out, base = None, P
    while True:
        if t & 1:
            out = base if out is None else out @ base
        t >>= 1
        if not t:
            break
        base = base @ base
    return out.clone() if out is P else out


def potential_device(Pt, gamma=1.0):
    """The potential of the diffused operator: ``-log(Pt + 1e-7)`` (``gamma = 1``), ``Pt`` (``gamma = -1``), else ``Pt^c / c`` with
    ``c = (1 - gamma) / 2``."""
    import torch

    gamma = float(gamma)
    if not -1 <= gamma <= 1:
        raise ValueError("gamma must lie in [-1, 1], got gamma={!r}".format(gamma))
    if gamma == 1:
        return -torch.log(Pt + LOG_FLOOR)
    if gamma == -1:
        return Pt.clone()
    c = (1.0 - gamma) / 2.0
    return torch.pow(Pt, c) / c


def distances_device(U):
    """``Dm[i, j] = |U[i] - U[j]|_2`` from direct differences (the library's pairwise kernel with its GEMM route switched off): every
    pair sums the squares of its differences in one order, so equal rows and the diagonal are exactly 0 and ``Dm`` is exactly
    symmetric.  That kernel takes one workgroup per pair and refuses a grid of 4,096^2 of them: the rows go through it in blocks of
    at most ``PAIRS_PER_CALL`` pairs (a pair's arithmetic does not depend on its block)."""
    import torch

    U = U.contiguous()
    n = int(U.shape[0])
    rows = max(1, PAIRS_PER_CALL // max(n, 1))
    if rows >= n:
        return torch.cdist(U, U, p=2.0, compute_mode="donot_use_mm_for_euclid_dist")
    Dm = torch.empty(n, n, dtype=U.dtype, device=U.device)
    for r0 in range(0, n, rows):
        Dm[r0:r0 + rows] = torch.cdist(U[r0:r0 + rows], U, p=2.0, compute_mode="donot_use_mm_for_euclid_dist")
    return Dm


def classical_mds_device(Dm, n_components):
    """Torgerson's classical MDS: ``(Z0 [n, k], eigenvalues [k])``, device tensors, from ``B = -1/2 J Dm^2 J`` (``J`` the centring
    matrix, applied as row, column and grand means), its ``k`` largest eigenpairs (``torch.linalg.eigh``), ``Z0 = V sqrt(max(lambda,
    0))``, the columns signed as by ``sign_columns``."""
    import torch

    k = int(n_components)
    D2 = Dm * Dm
    rows = D2.mean(dim=1, keepdim=True)
    cols = D2.mean(dim=0, keepdim=True)
    B = -0.5 * (D2 - rows - cols + D2.mean())
    w, V = torch.linalg.eigh(B)
    w, V = w[-k:].flip(0), V[:, -k:].flip(1)
    Z0 = V * torch.sqrt(w.clamp(min=0.0))[None, :]
    # (argmax returns the first of equal maxima: the lowest index on ties)
    lead = Z0.gather(0, Z0.abs().argmax(dim=0, keepdim=True))
    Z0 = Z0 * torch.where(lead < 0, -1.0, 1.0)
    return Z0.contiguous(), w


def smacof_step_device(Dm, Z, Z_out, row_stress):
    """One launch of ``meld_smacof_step``: ``Z_out`` <- the Guttman transform of ``Z`` towards ``Dm`` (any row stride), ``row_stress``
    <- the stress terms of ``Z``."""
    from ._device_ops import stream
    from ._lib import check, get_lib, ptr

    n, dim = int(Z.shape[0]), int(Z.shape[1])
    if Dm.dim() != 2 or int(Dm.shape[0]) != n or int(Dm.shape[1]) != n or Dm.stride(1) != 1 and n > 1:
        raise ValueError("Dm must be [n, n] with unit column stride for Z of {} rows, got shape {} strides {}".format(
            n, tuple(Dm.shape), Dm.stride()))
    if not (Z.is_contiguous() and Z_out.is_contiguous() and row_stress.is_contiguous()) or tuple(Z_out.shape) != (n, dim) \
            or int(row_stress.shape[0]) != n:
        raise ValueError("Z, Z_out [n, dim] and row_stress [n] must be contiguous and of matching shapes")
    ld = int(Dm.stride(0)) if n > 1 else max(n, 1)
    check(get_lib().meld_smacof_step(ptr(Dm), ld, n, dim, ptr(Z), ptr(Z_out), ptr(row_stress), stream()), "meld_smacof_step")


def smacof_device(Dm, Z0, max_iter=3000, eps=1e-6):
    """Metric MDS by SMACOF from ``Z0``: ``(Z, stress, iterations, log)``.  Step ``k`` (one launch) moves ``Z_{k-1}`` to ``Z_k`` and
    writes ``stress(Z_{k-1})`` into ``log[k - 1]`` on the device; the host reads the log after the steps 8, 16, ... and stops at the
    first such ``k`` with ``log[k-2] - log[k-1] <= eps * log[k-2]``, or at ``max_iter`` (``eps = 0``: exactly ``max_iter`` steps, the
    log is never read).  One more launch gives the stress of the returned ``Z`` (its transform is discarded).  ``stress``: a host
    float; ``log``: a host array ``[iterations + 1]``, the stress of ``Z_0 .. Z_iterations``."""
    import torch

    n, dim = int(Z0.shape[0]), int(Z0.shape[1])
    dev = Z0.device
    max_iter, eps = int(max_iter), float(eps)
    bufs = (Z0.to(torch.float64).contiguous().clone(), torch.empty(n, dim, dtype=torch.float64, device=dev))
    row_stress = torch.empty(n, dtype=torch.float64, device=dev)
    log = torch.zeros(max_iter + 1, dtype=torch.float64, device=dev)
    k = 0
    while k < max_iter:
        smacof_step_device(Dm, bufs[k & 1], bufs[(k + 1) & 1], row_stress)
        torch.sum(row_stress, dim=0, keepdim=True, out=log[k:k + 1])  # (twice the stress of Z_k: halved where it is read)
        k += 1
        if eps > 0 and k % CHECK_EVERY == 0:
            before, last = (float(v) for v in log[k - 2:k].cpu())  # (the one read-back of eight steps)
            if before - last <= eps * before:
                break
    Z = bufs[k & 1]
    smacof_step_device(Dm, Z, bufs[(k + 1) & 1], row_stress)
    torch.sum(row_stress, dim=0, keepdim=True, out=log[k:k + 1])
    host = 0.5 * log[: k + 1].cpu().numpy()
    return Z, float(host[k]), k, host


class PhateEmbedding:
    """The PHATE embedding of a graph for one argument set (``DeviceGraph.phate``).

    ``embedding`` (host ``[N, n_components]``, the caller's cell order) and ``embedding_device``; ``landmark_embedding`` /
    ``landmark_embedding_device`` (``[n, n_components]``: the rows of the operator -- landmarks, or on the direct route the cells in
    the device order); ``t`` and ``entropy`` (the curve ``t="auto"`` read its knee from; None for an integer ``t``);
    ``operator_device``, ``potential_device``, ``distances_device`` (``[n, n]``); ``stress`` (raw, of the returned coordinates),
    ``normalized_stress`` (``sqrt(stress / (1/2 sum Dm^2))``), ``stress_log`` (host, the stress of every iterate; None for
    ``mds="classic"``), ``iterations``; ``landmarks`` (the ``Landmarks`` record, None on the direct route); ``info``."""

    def __init__(self, G, **fields):
        self._graph = G
        self.__dict__.update(fields)
        self._embedding = None
        self._landmark_embedding = None

    @property
    def embedding(self):
        if self._embedding is None:
            self._embedding = self.embedding_device.cpu().numpy()
        return self._embedding

    @property
    def landmark_embedding(self):
        if self._landmark_embedding is None:
            self._landmark_embedding = self.landmark_embedding_device.cpu().numpy()
        return self._landmark_embedding

    def transform_device(self, Y):
        """The coordinates of new cells ``Y`` (``n_features_in`` columns, or the reduced ones), an fp64 device tensor ``[M,
        n_components]``: with landmarks ``lm.interpolate_device(Z, Y=Y)``, on the direct route ``graph.interpolate_device(embedding,
        Y)``.  NotImplementedError, naming the case, for a graph that cannot be extended to new cells."""
        if self.landmarks is not None:
            return self.landmarks.interpolate_device(self.landmark_embedding_device, Y=Y)
        return self._graph.interpolate_device(self.embedding_device, Y)

    def transform(self, Y):
        """``transform_device`` as a host ndarray."""
        return self.transform_device(Y).cpu().numpy()


def _compute(G, lm, a, info):
    import torch

    from . import filter as _filter

    P = operator_device(G) if lm is None else lm.landmark_op_device
    n = int(P.shape[0])
    if a["n_components"] >= n:
        raise ValueError("n_components={} must be below the {} rows of the operator".format(a["n_components"], n))
    t, entropy = a["t"], None
    if t == "auto":
        entropy = entropy_curve(singular_values(P), a["t_max"])
        t = max(knee(entropy), 1)
    U = potential_device(power_device(P, t), a["gamma"])
    Dm = distances_device(U)
    Z0, eigenvalues = classical_mds_device(Dm, a["n_components"])
    if a["mds"] == "metric":
        Z, stress, iterations, log = smacof_device(Dm, Z0, max_iter=a["max_iter"], eps=a["eps"])
        initial = float(log[0])
    else:
        _, initial, _, log = smacof_device(Dm, Z0, max_iter=0, eps=0.0)  # (one launch: the stress of Z0)
        Z, stress, iterations, log = Z0, initial, 0, None
    scale = 0.5 * float((Dm * Dm).sum())
    if lm is None:
        cells = _filter._to_caller_order(Z, G) if G.perm is not None else Z
    else:
        cells = lm.interpolate_device(Z)
    info = dict(info, n=n, t=int(t), route="direct" if lm is None else "landmarks", initial_stress=initial,
                eigenvalues=eigenvalues.cpu().numpy())
    return PhateEmbedding(G, embedding_device=cells, landmark_embedding_device=Z, initial_embedding_device=Z0, t=int(t), entropy=entropy,
                          operator_device=P, potential_device=U, distances_device=Dm, stress=stress,
                          normalized_stress=float(np.sqrt(stress / scale)) if scale > 0 else 0.0, stress_log=log, iterations=iterations,
                          landmarks=lm, info=info)


def phate(G, n_components=2, t="auto", gamma=1, n_landmark=None, clusters=None, n_svd=100, mds="metric", max_iter=3000, eps=1e-6,
          t_max=100, random_state=None, recompute=False, kmeans="library"):
    """``DeviceGraph.phate``: the ``PhateEmbedding`` record of the graph for the given arguments, kept on the graph per argument
    set (``kmeans``: the k-means of the default landmark clustering, ``landmarks()``'s argument)."""
    from . import landmark

    landmark.check_kmeans(kmeans)
    a = check_arguments(n_components=n_components, t=t, gamma=gamma, mds=mds, max_iter=max_iter, eps=eps, t_max=t_max)
    require_unsharded(G, "the PHATE embedding is")
    if n_landmark is None:
        n_landmark = getattr(G, "n_landmark", None)
        if n_landmark is None:
            n_landmark = DEFAULT_N_LANDMARK
    direct = False
    if clusters is None:
        if not _is_int(n_landmark) or int(n_landmark) < 1:
            raise ValueError("n_landmark must be a positive integer, got {!r}".format(n_landmark))
        direct = G.N <= int(n_landmark)
        if direct and G.N > landmark.LANDMARK_MAX:
            raise ValueError("n_landmark={} asks for every one of the {} cells as a landmark, above the {} landmarks the device "
                             "operator is built for".format(int(n_landmark), G.N, landmark.LANDMARK_MAX))
    if direct:
        lm, route = None, ("direct",)
    else:
        lm = G.landmarks(n_landmark=None if clusters is not None else n_landmark, clusters=clusters, n_svd=n_svd, random_state=random_state,
                         recompute=recompute, kmeans=kmeans)
        if clusters is not None:
            route = ("clusters", hashlib.sha1(lm.clusters.tobytes()).hexdigest())
        else:
            route = ("default", int(n_landmark), int(n_svd), None if random_state is None else int(random_state))
            if kmeans != "library":
                route = route + (kmeans,)
    key = route + tuple(a[name] for name in ("n_components", "t", "gamma", "mds", "max_iter", "eps", "t_max"))
    cache = G.__dict__.setdefault("_phate", {})
    if recompute:
        cache.pop(key, None)
    if key not in cache:
        cache[key] = _compute(G, lm, a, dict(a))
    return cache[key]
