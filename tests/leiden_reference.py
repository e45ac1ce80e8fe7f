"""Host restatement of the Leiden rule of csrc/leiden.hip / meld_amd/leiden.py in numpy and scipy, fp64: the Louvain run of
tests/louvain_reference.py with a REFINEMENT of every level's move partition before the contraction.

A level on the graph ``A`` (``k = A 1``, ``2m`` of level 0):

* the move phase of Louvain (``louvain_reference.move_round``, the same accept / retry loop), from singletons on level 0 and from
  the previous level's move partition afterwards, leaves the partition ``P``;
* the refinement starts from singletons ``sub = id`` and merges only inside the communities of ``P``: ``refine_round`` below, until
  a round moves nobody;
* the graph is contracted by the refined partition; ``P`` becomes the start of the next level's move phase.

Every merge of the refinement joins a vertex to a sub-community it has an entry to, and nobody leaves a sub-community of two or
more: every sub-community induces a connected subgraph, on every level (``refine`` asserts the three invariants behind that).  With
integer weights and a dyadic resolution every sum and every score is exact: the device must agree with no tolerance.
"""
import numpy as np

from tests import louvain_reference as lref
from tests.louvain_reference import DEFAULT_MAX_LEVELS, DEFAULT_MAX_ROUNDS, DEFAULT_TOL, RETRY_HALVINGS, contract, csr, degrees, q_value, renumber

M32 = 0xFFFFFFFF


def pri(ids, rnd):
    """The priority of a vertex in a round: a bijection of the 32-bit ids (an odd multiplier and xor-shifts), so no two are equal."""
    x = (np.asarray(ids, dtype=np.uint64) + np.uint64((int(rnd) * 0x9E3779B9) & M32)) & np.uint64(M32)
    for _ in range(2):
        x = ((x ^ (x >> np.uint64(16))) * np.uint64(0x45D9F3B)) & np.uint64(M32)
    return x ^ (x >> np.uint64(16))


def refine_round(A, P, sub, k, two_m, gamma, rnd):
    """One synchronous round of the refinement from the sub-communities ``sub`` inside the communities ``P`` (labels in [0, n)
    whose totals are addressed by label): ``(new sub, proposals, movers)``; a proposal is a label or -1."""
    n = A.shape[0]
    P, sub = np.asarray(P, dtype=np.int64), np.asarray(sub, dtype=np.int64)
    ids = np.arange(n, dtype=np.int64)
    rows = np.repeat(ids, np.diff(A.indptr))
    cols = A.indices.astype(np.int64)
    tot = np.bincount(sub, weights=k, minlength=n)
    size = np.bincount(sub, minlength=n)
    totC = np.bincount(P, weights=k, minlength=n)
    inside = (rows != cols) & (P[rows] == P[cols])
    in_c = np.bincount(rows[inside], weights=A.data[inside], minlength=n)  # (storage order)
    gk = gamma * k
    well = in_c * two_m >= gk * (totC[P] - k)
    prop = np.full(n, -1, dtype=np.int64)
    key = rows[inside] * n + sub[cols[inside]]
    pair, inv = np.unique(key, return_inverse=True)
    w = np.bincount(inv, weights=A.data[inside], minlength=pair.shape[0])
    pv, pt = pair // n, pair % n
    g = w * two_m - gk[pv] * tot[pt]
    ok = (size[sub[pv]] == 1) & well[pv] & (pt != sub[pv]) & ((size[pt] >= 2) | (pri(pt, rnd) < pri(pv, rnd))) & (g > 0)
    if ok.any():
        cv, ct, cg = pv[ok], pt[ok], g[ok]
        order = np.lexsort((ct, -cg, cv))  # per vertex: the largest score first, the lowest id among equals
        cv, ct = cv[order], ct[order]
        first = np.r_[True, cv[1:] != cv[:-1]]
        prop[cv[first]] = ct[first]
    t = np.where(prop >= 0, prop, 0)
    join = (prop >= 0) & ((size[t] >= 2) | (prop[t] < 0))
    new = np.where(join, prop, sub)
    return new, prop, int(join.sum())


def _assert_invariants(A, sub, new, prop):
    n = A.shape[0]
    present = np.unique(new)
    assert np.array_equal(new[present], present)  # a label that is not empty contains the vertex of that number
    size = np.bincount(sub, minlength=n)
    assert np.all(new[size[sub] >= 2] == sub[size[sub] >= 2])  # nobody leaves a sub-community of two or more
    movers = np.nonzero(new != sub)[0]
    B = A.tocsr()
    for v in movers[:200]:  # a joiner has an entry to the sub-community it joins (w_t > 0; the entries are positive)
        nb = B.indices[B.indptr[v]:B.indptr[v + 1]]
        assert np.any((sub[nb] == new[v]) & (nb != v))


def refine(A, P, k, two_m, gamma, max_rounds=DEFAULT_MAX_ROUNDS, check=True):
    """The refinement of ``P`` from singletons: ``(sub, rounds)``; ends at the first round without a mover or at ``max_rounds``."""
    n = A.shape[0]
    sub = np.arange(n, dtype=np.int64)
    rounds = 0
    while rounds < max_rounds:
        new, prop, movers = refine_round(A, P, sub, k, two_m, gamma, rounds)
        if check:
            _assert_invariants(A, sub, new, prop)
            assert len(set(zip(new.tolist(), np.asarray(P).tolist()))) == np.unique(new).shape[0]  # nested in P
        rounds += 1
        sub = new
        if movers == 0:
            break
    return sub, rounds


def run_level(A, gamma, two_m, tol=DEFAULT_TOL, max_rounds=DEFAULT_MAX_ROUNDS, start=None):
    """``louvain_reference.run_level`` started from the labels ``start`` (ids in [0, n); singletons for ``None``)."""
    n = A.shape[0]
    k = degrees(A)
    ids = np.arange(n, dtype=np.int64)
    c = ids.copy() if start is None else np.asarray(start, dtype=np.int64).copy()
    base, halvings, rounds = None, 0, 0
    while True:
        new, own, moved = lref.move_round(A, c, k, two_m, gamma, rounds)
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


def next_start(P, S_lab, S):
    """The start labels of the contracted graph's vertices: the smallest aggregate vertex of the ``P``-community they lie in."""
    sub_p = np.empty(S, dtype=np.int64)
    sub_p[S_lab] = P
    first = np.full(int(P.max()) + 1, S, dtype=np.int64)
    np.minimum.at(first, sub_p, np.arange(S, dtype=np.int64))
    return first[sub_p]


def singleton_q(A, two_m, gamma):
    k = degrees(A)
    return q_value(A.diagonal().sum(), (k * k).sum(), two_m, gamma)


def leiden(A, gamma=1.0, tol=DEFAULT_TOL, max_rounds=DEFAULT_MAX_ROUNDS, max_levels=DEFAULT_MAX_LEVELS, check=True):
    """The whole run: ``dict(labels, modularity, levels, level_labels, level_parts)``.
    ``levels[l] = dict(vertices, communities, subcommunities, rounds, refine_rounds, Q)`` (Q of the move partition);
    ``level_labels[l]``: the cells' refined sub-communities after level l, and for the last level the returned labels;
    ``level_parts[l] = (P, sub)`` of the level's vertices, for the levels that were refined."""
    A = csr(A)
    two_m = float(degrees(A).sum())
    cell = np.arange(A.shape[0], dtype=np.int64)
    levels, level_labels, level_parts, q, start = [], [], [], 0.0, None
    while two_m > 0.0 and len(levels) < max_levels:
        n = A.shape[0]
        k = degrees(A)
        c, q, rounds = run_level(A, gamma, two_m, tol, max_rounds, start)
        P, L = renumber(c)
        if L == n:  # every community is one vertex: the partition is the one the level before moved to
            if levels:
                q = levels[-1]["Q"]
            levels.append(dict(vertices=n, communities=L, subcommunities=n, rounds=rounds, refine_rounds=0, Q=q))
            level_labels.append(cell.copy())
            break
        sub, refine_rounds = refine(A, P, k, two_m, gamma, max_rounds, check)
        S_lab, S = renumber(sub)
        level_parts.append((P, S_lab))
        levels.append(dict(vertices=n, communities=L, subcommunities=S, rounds=rounds, refine_rounds=refine_rounds, Q=q))
        if S == n:  # the refinement merged nothing: the level's vertices, each alone
            q = singleton_q(A, two_m, gamma)
            level_labels.append(cell.copy())
            break
        if len(levels) == max_levels:  # cut: the move partition, as Louvain returns it
            cell = P[cell]
            level_labels.append(cell.copy())
            break
        cell = S_lab[cell]
        level_labels.append(cell.copy())
        start = next_start(P, S_lab, S)
        A = contract(A, S_lab, S)
    return dict(labels=cell.astype(np.int32), modularity=q, levels=levels, level_labels=level_labels, level_parts=level_parts)


def disconnected_communities(W, labels):
    """How many communities of ``labels`` induce a subgraph of ``W`` with more than one component."""
    from scipy.sparse.csgraph import connected_components

    W = csr(W)
    bad = 0
    for c in np.unique(labels):
        idx = np.nonzero(labels == c)[0]
        if idx.shape[0] > 1 and connected_components(W[idx][:, idx], directed=False)[0] > 1:
            bad += 1
    return bad
