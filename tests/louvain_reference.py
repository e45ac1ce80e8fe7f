"""Host restatement of the Louvain rule of csrc/louvain.hip / meld_amd/louvain.py in numpy and scipy, fp64: the definitions, the
synchronous round, the level loop, the renumbering and the contraction, each written out once more and as plainly as possible.

``A`` is a symmetric scipy CSR matrix with non-negative entries; a stored entry ``(i, i)`` is the diagonal.  ``k = A 1``,
``2m = 1' A 1`` (the same number on every level).  Sums over a row run in storage order, sums over a community in ascending vertex
order (``np.bincount`` adds its weights in the order given).  With integer weights and a dyadic resolution every sum and every score
is exact, whatever the order: the device must then agree with these functions with no tolerance.
"""
import numpy as np
from scipy import sparse

DEFAULT_TOL = 1e-7
DEFAULT_MAX_ROUNDS = 1000
DEFAULT_MAX_LEVELS = 64
RETRY_HALVINGS = 3


def csr(A):
    A = sparse.csr_matrix(A).astype(np.float64)
    A.sort_indices()
    return A


def degrees(A):
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return np.bincount(rows, weights=A.data, minlength=A.shape[0])


def q_value(s_in, s_tot2, two_m, gamma):
    """``(sum_c in_c - gamma sum_c tot_c^2 / 2m) / 2m``, in this order of operations (the host side of the device run uses the same)."""
    two_m, gamma = float(two_m), float(gamma)
    if two_m == 0.0:
        return 0.0
    t = gamma * float(s_tot2)
    t = t / two_m
    return (float(s_in) - t) / two_m


def modularity(A, labels, gamma=1.0):
    """Q of any labelling, from the definitions: in_c = sum_{i, j in c} A_ij, tot_c = sum_{i in c} k_i."""
    A = csr(A)
    _, c = np.unique(np.asarray(labels), return_inverse=True)
    n = A.shape[0]
    k = degrees(A)
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    same = c[rows] == c[A.indices]
    s_in = np.bincount(rows[same], weights=A.data[same], minlength=n).sum()
    tot = np.bincount(c, weights=k)
    return q_value(s_in, (tot * tot).sum(), k.sum(), gamma)


def move_round(A, c, k, two_m, gamma, rnd):
    """One synchronous round from the labels ``c``: ``(new labels, own, moved)`` with ``own[i] = w_{c_i} + A_ii``."""
    n = A.shape[0]
    c = np.asarray(c, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr))
    cols = A.indices.astype(np.int64)
    off = rows != cols
    diag = np.bincount(rows[~off], weights=A.data[~off], minlength=n)
    tot = np.bincount(c, weights=k, minlength=n)
    size = np.bincount(c, minlength=n)
    # w[i, b]: the off-diagonal entries of row i whose column carries label b, added in storage order
    key = rows[off] * n + c[cols[off]]
    pair, inv = np.unique(key, return_inverse=True)
    w = np.bincount(inv, weights=A.data[off], minlength=pair.shape[0])
    pi, pb = pair // n, pair % n
    a = c[pi]
    gk = gamma * k[pi]
    own_pair = pb == a
    w_a = np.zeros(n)
    w_a[pi[own_pair]] = w[own_pair]
    g_a = w_a * two_m - (gamma * k) * (tot[c] - k)
    g = w * two_m - gk * tot[pb]
    single = size[a] == 1
    allowed = np.where(single, (size[pb] > 1) | (pb < a), (pb > a) if rnd % 2 else (pb < a)) & ~own_pair
    new = c.copy()
    if allowed.any():
        ci, cb, cg = pi[allowed], pb[allowed], g[allowed]
        order = np.lexsort((cb, -cg, ci))  # per vertex: the largest score first, the lowest id among equals
        ci, cb, cg = ci[order], cb[order], cg[order]
        first = np.r_[True, ci[1:] != ci[:-1]]
        ci, cb, cg = ci[first], cb[first], cg[first]
        go = cg > g_a[ci]
        new[ci[go]] = cb[go]
    return new, w_a + diag, new != c


def run_level(A, gamma, two_m, tol=DEFAULT_TOL, max_rounds=DEFAULT_MAX_ROUNDS):
    """The rounds of one level from singletons: ``(labels kept, Q, rounds)``.  Round r evaluates Q of the labels it read.  Labels
    whose Q lies more than ``tol`` above the accepted ones' are ACCEPTED, and the round's new labels are tried next.  Labels that
    are not are dropped, and the accepted round's moves are tried again with half the movers: at the h-th try in a row only the
    movers whose vertex number is a multiple of 2^h.  The level ends when an accepted round moved nothing, after ``RETRY_HALVINGS``
    tries in a row, when a try has no mover left, or after ``max_rounds``; the labels with the larger Q are kept."""
    n = A.shape[0]
    k = degrees(A)
    ids = np.arange(n, dtype=np.int64)
    c = ids.copy()
    base, halvings, rounds = None, 0, 0
    while True:
        new, own, moved = move_round(A, c, k, two_m, gamma, rounds)
        tot = np.bincount(c, weights=k, minlength=n)
        q = q_value(own.sum(), (tot * tot).sum(), two_m, gamma)
        rounds += 1
        if base is None or q - base[1] > tol:
            base, halvings = (c, q, new, moved), 0
            if not moved.any() or rounds >= max_rounds:
                return c, q, rounds
            c = new
            continue
        kept = (c, q) if q > base[1] else (base[0], base[1])
        halvings += 1
        mask = base[3] & (ids % (1 << halvings) == 0)
        if halvings > RETRY_HALVINGS or rounds >= max_rounds or not mask.any():
            return kept[0], kept[1], rounds
        c = np.where(mask, base[2], base[0])


def renumber(c):
    """Communities numbered by their smallest member: ``(labels in [0, L), L)``."""
    _, first, inv = np.unique(c, return_index=True, return_inverse=True)
    rank = np.empty(first.shape[0], dtype=np.int64)
    rank[np.argsort(first)] = np.arange(first.shape[0])
    return rank[inv], int(first.shape[0])


def contract(A, c, L):
    """``C' A C`` with sorted rows (the diagonal holds in_c)."""
    n = A.shape[0]
    C = sparse.csr_matrix((np.ones(n), (np.arange(n), c)), shape=(n, L))
    return csr(C.T @ A @ C)


def louvain(A, gamma=1.0, tol=DEFAULT_TOL, max_rounds=DEFAULT_MAX_ROUNDS, max_levels=DEFAULT_MAX_LEVELS):
    """The whole run: ``dict(labels, modularity, levels, level_labels)``; ``levels[l] = dict(vertices, communities, rounds, Q)``, the
    last level is the one that merged nothing (or level ``max_levels``); ``level_labels[l]``: the cells' communities after level l."""
    A = csr(A)
    n = A.shape[0]
    two_m = float(degrees(A).sum())
    cell = np.arange(n, dtype=np.int64)
    levels, level_labels, q = [], [], 0.0
    while two_m > 0.0 and len(levels) < max_levels:
        c, q, rounds = run_level(A, gamma, two_m, tol, max_rounds)
        c, L = renumber(c)
        if L == A.shape[0] and levels:
            q = levels[-1]["Q"]  # (nothing merged: the partition, and so its Q, is the level before's; summed anew it could differ in the last bit)
        levels.append(dict(vertices=int(A.shape[0]), communities=L, rounds=rounds, Q=q))
        cell = c[cell]
        level_labels.append(cell.copy())
        if L == A.shape[0]:
            break
        A = contract(A, c, L)
    return dict(labels=cell.astype(np.int32), modularity=q, levels=levels, level_labels=level_labels)
