"""Host reference of the k-means kernels (csrc/kmeans_wide.hip, meld_amd/kmeans.py): plain numpy in ``np.longdouble``.

Distances are the direct sums ``sum (y - c)^2`` -- not the expanded form the kernel scores with --, the argmin takes the lowest index
among equal distances, segment sums and one Lloyd step follow the definition.

``tau`` is the bound the GPU tests compare with.  The kernel compares candidates on ``|c|^2 - 2 y.c`` in fp64.  With ``u = 2^-53``
and ``gamma_m = m u / (1 - m u)``, a dot product of length ``d`` (any order of the additions, fused or not) is off by at most
``gamma_d |y|.|c| <= gamma_d |y| |c| <= gamma_d (|y|^2 + |c|^2) / 2``, a norm by ``gamma_d |c|^2``, and the two or three additions
that join them add ``gamma_3`` of the sum of the magnitudes, at most ``2 (|y|^2 + |c|^2)``.  One expanded distance is therefore
within ``(2 d + 6) u (|y|^2 + |c|^2)`` of the true one (first order), two candidates that are compared within twice that,
``(4 d + 12) u (|y|^2 + max |c|^2)``; ``tau_i = 8 (d + 4) u (|y_i|^2 + max_j |c_j|^2)`` is twice that again, rounded up: the derivation's
figure, not a tuned one.
"""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53


def distances(Y, C, rows=None):
    """``[n, k]`` long double: ``sum_c (Y[i, c] - C[j, c])^2``, the coordinates added in ascending order."""
    Y, C = np.asarray(Y, dtype=LD), np.asarray(C, dtype=LD)
    n, k = Y.shape[0], C.shape[0]
    out = np.empty((n, k), dtype=LD)
    Ct = np.ascontiguousarray(C.T)  # [d, k]
    step = max(1, (1 << 16) // k)  # (rows per block: the [step, k] temporaries stay in cache)
    for lo in range(0, n, step):
        Yb = Y[lo:lo + step]
        acc = np.zeros((Yb.shape[0], k), dtype=LD)
        buf = np.empty_like(acc)
        for c in range(Y.shape[1]):
            np.subtract(Yb[:, c, None], Ct[c][None, :], out=buf)
            np.multiply(buf, buf, out=buf)
            acc += buf
        out[lo:lo + step] = acc
    return out


def argmin_lowest(D):
    """Row-wise argmin, the lowest index among equal values (``np.argmin``'s rule, stated)."""
    return np.argmin(D, axis=1).astype(np.int64)


def tau(Y, C):
    """``tau_i = 8 (d + 4) 2^-53 (|y_i|^2 + max_j |c_j|^2)``, long double ``[n]``."""
    Y, C = np.asarray(Y, dtype=LD), np.asarray(C, dtype=LD)
    d = Y.shape[1]
    return LD(8 * (d + 4)) * U * ((Y * Y).sum(1) + (C * C).sum(1).max())


def gaps(D):
    """Second-smallest minus smallest distance per row (``inf`` with one centre)."""
    if D.shape[1] < 2:
        return np.full(D.shape[0], np.inf, dtype=LD)
    part = np.partition(D, 1, axis=1)
    return part[:, 1] - part[:, 0]


def close_calls(Y, C, D=None):
    """Boolean ``[n]``: the points whose best and second-best distances are closer than ``2 tau_i`` (their label is not checked)."""
    D = distances(Y, C) if D is None else D
    return gaps(D) <= 2 * tau(Y, C)


def segment_sums(Y, labels, k):
    """``(sums [k, d] long double, counts [k] int64)``: rows added in ascending row order."""
    Y = np.asarray(Y, dtype=LD)
    sums = np.zeros((k, Y.shape[1]), dtype=LD)
    np.add.at(sums, np.asarray(labels, dtype=np.int64), Y)
    return sums, np.bincount(np.asarray(labels, dtype=np.int64), minlength=k)


def inertia(Y, C, labels=None):
    D = distances(Y, C)
    if labels is None:
        return D.min(1).sum()
    return D[np.arange(D.shape[0]), np.asarray(labels, dtype=np.int64)].sum()


def lloyd_step(Y, C):
    """``(labels, new centres, inertia)``: an empty cluster keeps its centre."""
    D = distances(Y, C)
    lab = argmin_lowest(D)
    sums, cnt = segment_sums(Y, lab, C.shape[0])
    newC = np.asarray(C, dtype=LD).copy()
    has = cnt > 0
    newC[has] = sums[has] / cnt[has, None].astype(LD)
    return lab, newC, D.min(1).sum()


# -- the generated inputs of tests/test_gpu_kmeans.py (tests/test_kmeans_reference.py checks every one of them on the host) ----------
ASSIGN_SHAPES = [(1, 1, 1), (17, 3, 17), (63, 4, 16), (1000, 50, 65), (1000, 100, 1000), (257, 128, 4096), (5000, 100, 2000)]


def assign_case(n, d, k, mean=0.0):
    """Standard-normal points and centres (points shifted by ``mean`` in every coordinate), seeded by the shape."""
    rng = np.random.default_rng(1000003 * n + 1009 * d + k)
    return rng.standard_normal((n, d)) + mean, rng.standard_normal((k, d)) + mean


def assign_cases():
    """``{name: (Y, C)}``: the seven shapes, and the (1000, 50, 65) shape at mean 1e3."""
    cases = {"{}x{}x{}".format(*s): assign_case(*s) for s in ASSIGN_SHAPES}
    cases["1000x50x65@1e3"] = assign_case(1000, 50, 65, mean=1e3)
    return cases


_CASE_REFERENCE = {}


def case_reference(name):
    """``(Y, C, D, tau)`` of an assign case, computed once per process and shared (read-only) by the tests that need it."""
    if name not in _CASE_REFERENCE:
        Y, C = assign_cases()[name]
        D, t = distances(Y, C), tau(Y, C)
        for a in (Y, C, D, t):
            a.setflags(write=False)
        _CASE_REFERENCE[name] = (Y, C, D, t)
    return _CASE_REFERENCE[name]


CASE_NAMES = ["{}x{}x{}".format(*s) for s in ASSIGN_SHAPES] + ["1000x50x65@1e3"]


def duplicate_case():
    """300 points in d = 10, 40 centres: centres 5 = 21 and 7 = 33 are exact duplicates, points 0..39 sit exactly on centre i."""
    rng = np.random.default_rng(77)
    C = rng.standard_normal((40, 10))
    C[21], C[33] = C[5], C[7]
    Y = rng.standard_normal((300, 10))
    Y[:40] = C
    return Y, C


def blobs(n_blobs=80, per=50, d=10, spacing=40.0, seed=5):
    """``(X, truth)``: ``n_blobs`` unit Gaussians whose centres lie ``spacing`` apart on a line through the first coordinates'
    lattice, rows permuted."""
    rng = np.random.default_rng(seed)
    truth = np.repeat(np.arange(n_blobs), per)
    centres = np.zeros((n_blobs, d))
    centres[:, 0] = spacing * (np.arange(n_blobs) % 10)
    centres[:, 1] = spacing * (np.arange(n_blobs) // 10)
    X = rng.standard_normal((n_blobs * per, d)) + centres[truth]
    order = rng.permutation(X.shape[0])
    return X[order], truth[order]


def step_case(n=1001, d=7, seed=41):
    """``(Y, C)`` for the Lloyd steps side by side: ``n`` points (no multiple of a workgroup's 256) in four unit Gaussians 8 apart,
    five centres -- the blobs' displaced by a unit Gaussian, and one at 50 in every coordinate that no point is nearest to."""
    rng = np.random.default_rng(seed)
    means = 8.0 * np.eye(4, d)
    Y = rng.standard_normal((n, d)) + means[rng.integers(0, 4, n)]
    C = np.concatenate([means + rng.standard_normal((4, d)), np.full((1, d), 50.0)])
    return Y, C


def overlapping_blobs(n=4000, d=20, k=100, spacing=3.0, seed=6):
    rng = np.random.default_rng(seed)
    centres = spacing * rng.integers(0, 4, size=(k, d)).astype(np.float64)
    return rng.standard_normal((n, d)) + centres[rng.integers(0, k, n)]


def uniform_noise(n=4000, d=20, seed=7):
    return np.random.default_rng(seed).uniform(0.0, 1.0, size=(n, d))
