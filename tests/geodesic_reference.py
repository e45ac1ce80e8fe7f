"""Host restatement of the rounds of meld_amd/geodesic.py (csrc/geodesic.hip), shared by tests/test_geodesic_host.py and
tests/test_gpu_geodesic.py: synchronous (Jacobi) Bellman-Ford on a scipy CSR matrix of lengths, every stored entry an edge."""
import numpy as np
from scipy import sparse


def minplus_round(indptr, indices, lengths, x):
    """``y[i, c] = min(x[i, c], min_{e in row i} (x[col[e], c] + len[e]))`` for an fp64 block ``x [N, p]``: one add per entry, an
    exact minimum (the order of a minimum does not matter)."""
    y = x.copy()
    if indices.size:
        cand = x[indices] + lengths[:, None]
        rows = np.flatnonzero(np.diff(indptr) > 0)  # (rows without entries have no segment: the others' segments are adjacent)
        y[rows] = np.minimum(y[rows], np.minimum.reduceat(cand, indptr[:-1][rows], axis=0))
    return y


def jacobi_host(L_csr, sources, min_only=False):
    """``(D, rounds)``: ``D [N, p]`` with column ``j`` the distances from ``sources[j]`` (``[N]``, the distance to the nearest
    source, with ``min_only``), ``+inf`` where there is no path; ``rounds`` counts every round up to and including the first one
    that lowers nothing."""
    N = L_csr.shape[0]
    indptr, indices = np.asarray(L_csr.indptr, dtype=np.int64), np.asarray(L_csr.indices, dtype=np.int64)
    lengths = np.asarray(L_csr.data, dtype=np.float64)
    sources = np.asarray(sources, dtype=np.int64).reshape(-1)
    p = 1 if min_only else sources.shape[0]
    x = np.full((N, p), np.inf)
    x[sources, 0 if min_only else np.arange(p)] = 0.0
    rounds = 0
    while True:
        y = minplus_round(indptr, indices, lengths, x)
        rounds += 1
        if not (y < x).any():
            break
        x = y
    return (y[:, 0] if min_only else y), rounds


def zero_length_graph(n=1000, seed=5):
    """About 4 symmetric pairs per vertex, a fifth of them at length 0 (explicit entries), some vertices isolated."""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n - 20, 4 * n), rng.integers(0, n - 20, 4 * n)
    keep = a < b
    pairs = np.unique(np.stack([a[keep], b[keep]], 1), axis=0)
    w = rng.uniform(0.1, 2.0, pairs.shape[0])
    w[rng.random(pairs.shape[0]) < 0.2] = 0.0
    L = sparse.coo_matrix((np.r_[w, w] + 7.0, (np.r_[pairs[:, 0], pairs[:, 1]], np.r_[pairs[:, 1], pairs[:, 0]])), shape=(n, n)).tocsr()
    L.data -= 7.0  # (the zeros stay stored entries)
    L.sort_indices()
    assert (L.data == 0).sum() > 0.15 * L.nnz and L.nnz == 2 * pairs.shape[0]
    return L
