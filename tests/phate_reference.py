"""NumPy / scipy restatement of the stages of the PHATE embedding that meld_amd/phate.py defines (the entropy curve, the knee,
the potential, the potential distances, classical MDS, the SMACOF step and its stopping rule), each in its plainest form: the host
reference of tests/test_phate_host.py and tests/test_gpu_phate.py.  Nothing is copied from phate, sklearn or s_gd2."""
import numpy as np
from scipy.spatial.distance import cdist

CHECK_EVERY = 8


def entropy_curve(s, t_max=100):
    s = np.asarray(s, dtype=np.float64)
    eps = np.finfo(float).eps
    h = np.empty(t_max)
    for i in range(t_max):
        p = s ** (i + 1)
        p = p / p.sum() + eps
        h[i] = -np.sum(p * np.log(p))
    return h


def knee_errors(h):
    """err[b], b = 1 .. len(h) - 2: one ``lstsq`` line through the points 0 .. b, one through b .. len(h) - 1, the absolute
    residuals of both added (inf at the ends)."""
    h = np.asarray(h, dtype=np.float64)
    n = h.shape[0]
    x = np.arange(n, dtype=np.float64)
    err = np.full(n, np.inf)
    for b in range(1, n - 1):
        total = 0.0
        for lo, hi in ((0, b + 1), (b, n)):
            A = np.stack([x[lo:hi], np.ones(hi - lo)], axis=1)
            coef = np.linalg.lstsq(A, h[lo:hi], rcond=None)[0]
            total += np.abs(A @ coef - h[lo:hi]).sum()
        err[b] = total
    return err


def knee(h):
    return int(np.argmin(knee_errors(h)))  # (argmin: the lowest index of equal minima)


def choose_t(s, t_max=100):
    return max(knee(entropy_curve(s, t_max)), 1)


def potential(Pt, gamma=1.0):
    if gamma == 1:
        return -np.log(Pt + 1e-7)
    if gamma == -1:
        return Pt.copy()
    c = (1.0 - gamma) / 2.0
    return Pt ** c / c


def distances(U):
    return cdist(U, U)  # (direct differences)


def classical_mds(Dm, k):
    n = Dm.shape[0]
    J = np.eye(n) - np.ones((n, n)) / n
    B = -0.5 * J @ (Dm * Dm) @ J
    B = 0.5 * (B + B.T)
    w, V = np.linalg.eigh(B)
    w, V = w[::-1][:k], V[:, ::-1][:, :k]
    Z = V * np.sqrt(np.maximum(w, 0.0))[None, :]
    for c in range(k):
        if Z[np.argmax(np.abs(Z[:, c])), c] < 0:
            Z[:, c] = -Z[:, c]
    return Z


def smacof_step(Dm, Z):
    """``(Z', row_stress, abs_terms)`` by dense arrays, the definition term by term: ``Z'[i] = (1 / n) sum_j ratio[i, j] (Z[i] -
    Z[j])`` with ``ratio[i, j] = Dm[i, j] / d_ij`` off the diagonal where ``d_ij > 0`` (else 0); ``row_stress[i] = sum_{j != i} (d_ij
    - Dm[i, j])^2``; ``abs_terms[i, c] = sum_j |ratio[i, j] (Z[i, c] - Z[j, c])|``, the scale of the error bound of ``Z'`` (not
    divided by n).  (The matrix form ``B Z / n`` with ``B = diag(ratio 1) - ratio`` is the same map, but it adds ``ratio[i, j] Z[i]``
    and ``ratio[i, j] Z[j]`` apart: between near points its rounding error is far above that of the terms it stands for.)"""
    Dm, Z = np.asarray(Dm, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    n = Z.shape[0]
    d = cdist(Z, Z)
    off = ~np.eye(n, dtype=bool)
    ratio = np.zeros_like(d)
    use = off & (d > 0)
    ratio[use] = Dm[use] / d[use]
    diff = Z[:, None, :] - Z[None, :, :]
    gap = np.where(off, d - Dm, 0.0)
    return np.einsum("ij,ijc->ic", ratio, diff) / n, (gap * gap).sum(axis=1), np.einsum("ij,ijc->ic", ratio, np.abs(diff))


def stress(Dm, Z):
    return 0.5 * smacof_step(Dm, Z)[1].sum()


def smacof(Dm, Z0, max_iter=3000, eps=1e-6):
    """``(Z, stress, iterations, log)`` under the stopping rule of meld_amd/phate.py: ``log[k-1] = stress(Z_{k-1})`` is written by
    step ``k``; after the steps 8, 16, ... the run stops where ``log[k-2] - log[k-1] <= eps * log[k-2]`` (never for ``eps = 0``)."""
    Z = np.array(Z0, dtype=np.float64)
    log = []
    k = 0
    while k < max_iter:
        Zn, rs, _ = smacof_step(Dm, Z)
        log.append(0.5 * rs.sum())
        Z = Zn
        k += 1
        if eps > 0 and k % CHECK_EVERY == 0 and log[k - 2] - log[k - 1] <= eps * log[k - 2]:
            break
    log.append(stress(Dm, Z))
    return Z, log[-1], k, np.asarray(log)
