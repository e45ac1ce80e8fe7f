"""Host restatement of the rank-sum scheme of csrc/ranksum.hip, with Python integers on the columns of a
scipy CSC matrix, and of the host arithmetic of meld_amd/diffexp.py (p-values, Benjamini-Hochberg).  Written from the definitions,
it shares no code with the package: tests/test_ranksum_reference.py holds both against scipy.

Definitions.  code[cell] in {-1, 0 .. k-1}; -1: the cell takes no part.  m = the selected cells, n_c the class sizes.  For one gene
the selected cells' values are ranked with mid-ranks, the implicit zeros included; stored +0.0 / -0.0 count as zeros; negatives rank
below the zeros.

    rank2[g][c] = twice the rank sum of class c       tie[g] = sum of t^3 - t over all tie groups, the zeros' included
    nnz[g][c]   = selected non-zero entries of c      sum[g][c] = the class's values added up (long double)
"""
import numpy as np


def rank_sums(X, code, k):
    """``X``: scipy CSC [N, G]; ``code``: int [N].  Returns rank2 [G, k], tie [G] (object arrays of Python ints), nnz [G, k] int64,
    sum [G, k] and abs_sum [G, k] (long double: the class's values and their magnitudes), n_c [k] (Python ints)."""
    X = X.tocsc()
    code = np.asarray(code).astype(np.int64)
    N, G = X.shape
    assert code.shape == (N,) and code.min() >= -1 and code.max() < k
    n_c = [int((code == c).sum()) for c in range(k)]
    m = sum(n_c)
    rank2 = np.zeros((G, k), dtype=object)
    tie = np.zeros(G, dtype=object)
    nnz = np.zeros((G, k), dtype=np.int64)
    sums = np.zeros((G, k), dtype=np.longdouble)
    abs_sums = np.zeros((G, k), dtype=np.longdouble)
    for g in range(G):
        s, e = X.indptr[g], X.indptr[g + 1]
        cells, v = X.indices[s:e], X.data[s:e].astype(np.float64)
        cls = code[cells]
        keep = (cls >= 0) & (v != 0)
        for c in range(k):
            mine = v[cls == c].astype(np.longdouble)
            sums[g, c] = mine.sum()
            abs_sums[g, c] = np.abs(mine).sum()
        v, cls = v[keep], cls[keep]
        order = np.argsort(v, kind="stable")
        v, cls = v[order], cls[order]
        cnt = len(v)
        n_neg = int((v < 0).sum())
        z = m - cnt
        r2 = [0] * k
        t_sum = z ** 3 - z
        for c in range(k):
            nnz[g, c] = int((cls == c).sum())
            r2[c] += (n_c[c] - int(nnz[g, c])) * (2 * n_neg + z + 1)  # the zeros of the class: mid-rank n_neg + (z + 1) / 2
        i = 0
        while i < cnt:
            j = i
            while j < cnt and v[j] == v[i]:
                j += 1
            t = j - i
            b = i + (z if v[i] > 0 else 0)  # ranks b + 1 .. b + t: twice their mean is 2 b + t + 1
            for c in cls[i:j]:
                r2[int(c)] += 2 * b + t + 1
            t_sum += t ** 3 - t
            i = j
        for c in range(k):
            rank2[g, c] = r2[c]
        tie[g] = t_sum
    return rank2, tie, nnz, sums, abs_sums, n_c


def pvalues(rank2, tie, n1, n2):
    """(statistic U1, two-sided asymptotic p with continuity correction) per gene, fp64; p = 1.0 where the deviation is 0."""
    from scipy import stats

    n = n1 + n2
    stat, p = [], []
    for r2, t in zip(rank2, tie):
        u1 = (int(r2) - n1 * (n1 + 1)) / 2
        u = max(u1, n1 * n2 - u1)
        s = np.sqrt(n1 * n2 / 12.0 * ((n + 1) - int(t) / (n * (n - 1.0))))
        stat.append(u1)
        if s == 0:
            p.append(1.0)
        else:
            zz = (u - n1 * n2 / 2.0 - 0.5) / s
            p.append(min(1.0, 2.0 * float(stats.norm.sf(zz))))
    return np.array(stat, dtype=np.float64), np.array(p, dtype=np.float64)


def bh(p):
    """Benjamini-Hochberg: q_(i) = min over j >= i of p_(j) G / j, at most 1."""
    p = np.asarray(p, dtype=np.float64)
    g = len(p)
    order = np.argsort(p, kind="stable")
    q = np.empty(g)
    running = 1.0
    for rank in range(g, 0, -1):
        idx = order[rank - 1]
        running = min(running, p[idx] * g / rank)
        q[idx] = running
    return q


def make_case(N, G, density, seed, kind="halves", dtype=np.float64, n_classes=3, ignore=True):
    """A CSC matrix [N, G] with the features the tests need, and codes.  ``kind``: "halves" (values rounded to halves: heavy ties,
    some negatives, some stored zeros of both signs), "real" (continuous, both signs), "counts" (small positive integers).  Gene 0 is
    all zero and gene 1 all tied non-zero where G allows."""
    from scipy import sparse

    rng = np.random.default_rng(seed)
    X = sparse.random(N, G, density=density, random_state=np.random.RandomState(seed), format="csc", dtype=np.float64)
    u = X.data
    if kind == "halves":
        vals = np.round(u * 6) / 2 - 0.5  # -0.5, 0, 0.5 ... 2.5
        vals[(vals == 0) & (rng.random(len(vals)) < 0.5)] = -0.0
    elif kind == "real":
        vals = u * 3.0 - 1.0
    else:
        vals = np.floor(u * 5.0) + 1.0
    X.data = vals
    X = X.tolil()
    if G >= 1:
        X[:, 0] = 0
    if G >= 2:
        X[:, 1] = 1.5
    X = X.tocsc()
    # (lil drops the stored zeros: put some back, of both signs, at stored positions)
    if kind == "halves" and X.nnz:
        pick = rng.random(X.nnz) < 0.08
        X.data[pick] = np.where(rng.random(int(pick.sum())) < 0.5, 0.0, -0.0)
        if G >= 2:  # gene 1 stays all tied
            X.data[X.indptr[1]:X.indptr[2]] = 1.5
    X.data = X.data.astype(dtype)
    lo = -1 if ignore else 0
    code = rng.integers(lo, n_classes, N).astype(np.int32)
    for c in range(min(n_classes, N)):  # every class has a cell
        code[c] = c
    return X, code
