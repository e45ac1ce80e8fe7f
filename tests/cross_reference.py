"""A plain host reference of the kernel between two point sets (the blocks between two samples of the MNN kernel, the kernel from
new cells to fitted ones), and the data set that takes the search between two point sets far from its common centre.

NumPy / SciPy only, every distance by direct fp64 differences (``scipy.spatial.distance.cdist``: sqrt(sum (x - y)^2), no GEMM form),
all pairs, no search: what ``HipOps.directed_kernel_coo(n_refs=)`` and ``mnn._cross_block`` must reproduce whatever route their search
takes.  tests/test_cross_reference.py ties it to the oracle (``oracle.kernel_to_data``) before any GPU result is judged by it.

The contract, per query row q against the references Y (the query is not among them):
  * knn is clipped to the number of references;
  * bandwidth = distance to the knn-th nearest reference, floored at eps;
  * K = exp(-(dist / bandwidth)^decay), NaN -> 1, kept where K >= thresh;
  * decay = inf: 1 for the knn nearest references (ranked by (distance, index)), nothing else.
"""
import numpy as np
from scipy import sparse
from scipy.spatial.distance import cdist

EPS = float(np.finfo(np.float64).eps)


def far_samples(d, seed, n_main=600, n_far=300, out=200.0, off=5.0):
    """Two samples (A, B) with a clump far from the common centre: most cells of either around the origin, the others ``out`` units
    along the first axis -- B's a further ``off`` units along the second, so that the far cells of one sample find their neighbours
    among a few cells of the other at distances tiny against the largest norm.  The largest centred coordinate is ~ 130 at the
    defaults: a norm taken in the search's scaled units (data / absmax) is 130^2 times too small there."""
    if d < 2:
        raise ValueError("far_samples needs two axes")
    rng = np.random.default_rng(seed)
    e0, e1 = np.zeros(d), np.zeros(d)
    e0[0], e1[1] = 1.0, 1.0
    a_main = rng.normal(size=(n_main, d))
    a_far = out * e0 + rng.normal(size=(n_far, d))
    b_main = rng.normal(size=(n_main - 50, d)) + 0.3
    b_far = out * e0 + off * e1 + rng.normal(size=(n_far + 37, d))
    return np.concatenate([a_main, a_far]), np.concatenate([b_main, b_far])


KNN, DECAY, THRESH, SEED = 5, 40, 1e-4, 1
FAR_DIMS = (10, 50)
UNIT_SCALES = (2.0 ** -12, 1.0, 2.0 ** 9)  # powers of two: every operand of the search scales exactly
EDGE_DIMS = (7, 13, 14, 29, 30, 141)
N_MAIN, N_FAR = 600, 300  # far_samples' defaults: A = 600 + 300 cells, B = 550 + 337


def far_block_cases():
    """name -> (Xq, Yr, knn, decay): the blocks the GPU tests build on ``far_samples`` (tests/test_gpu_cross_search.py, c)."""
    cases = {}
    for d in FAR_DIMS:
        A, B = far_samples(d, SEED)
        cases["far_d%d_A_to_B" % d] = (A, B, KNN, DECAY)
        cases["far_d%d_B_to_A" % d] = (B, A, KNN, DECAY)
    A, B = far_samples(10, SEED)
    main = np.concatenate([A[:N_MAIN], B[: N_MAIN - 50]])
    far = np.concatenate([A[N_MAIN:], B[N_MAIN - 50 :]])
    cases["queries_outside"] = (A[N_MAIN : N_MAIN + 40], main, KNN, DECAY)  # the queries alone set the largest norm
    cases["references_outside"] = (A[:40], far, KNN, DECAY)
    cases["decay_inf"] = (A, B, KNN, np.inf)
    cases["knn_clipped"] = (A, B[::250], KNN, DECAY)  # 4 references (3 near, 1 far): knn = 5 is clipped to 4
    return cases


def edge_samples(d, nr, nq):
    """(Xq, Yr): a shifted batch of roughly unit-scale cells on a few latent axes, in arbitrary units and off the origin
    (x 37.5 + 11, as the operand test of the search does)."""
    rng = np.random.default_rng(100000 * d + 100 * nr + nq)
    lat = min(d, 8)
    M = rng.normal(size=(lat, d))
    Xq = rng.normal(size=(nq, lat)) @ M + 0.05 * rng.normal(size=(nq, d))
    Yr = (rng.normal(size=(nr, lat)) + 0.3) @ M + 0.05 * rng.normal(size=(nr, d))
    return Xq * 37.5 + 11.0, Yr * 37.5 + 11.0


def edge_shapes(TS, BQ):
    """(nr, nq) around a reference tile (TS) and a query block (BQ) of the search, and a size that is a multiple of neither."""
    return [(nr, nq) for nr in (TS - 1, TS, TS + 1, 333) for nq in (1, BQ - 1, BQ + 1)]


def mnn_cells(d):
    """(X, batch): ``far_samples`` as one data set of two samples, interleaved by a random permutation as in real data."""
    A, B = far_samples(d, SEED)
    X = np.concatenate([A, B])
    batch = np.array(["batch_a"] * A.shape[0] + ["batch_b"] * B.shape[0])
    order = np.random.default_rng(SEED).permutation(X.shape[0])
    return X[order], batch[order]


def _distances(Xq, Yr):
    return cdist(np.ascontiguousarray(Xq, dtype=np.float64), np.ascontiguousarray(Yr, dtype=np.float64), "euclidean")


def _values(D, bw, decay):
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        v = np.exp(-np.power(D / bw[:, None], decay))
    return np.where(np.isnan(v), 1.0, v)


def cross_block_reference(Xq, Yr, knn, decay, thresh):
    """(K, bandwidth): the kernel from the rows of ``Xq`` to the rows of ``Yr`` as CSR [len(Xq), len(Yr)] with sorted columns, and
    every query's bandwidth (floored at eps)."""
    D = _distances(Xq, Yr)
    nq, nr = D.shape
    knn = int(min(knn, nr))
    order = np.argsort(D, axis=1, kind="stable")  # (distance, index)
    bw = np.maximum(np.take_along_axis(D, order[:, knn - 1 : knn], axis=1)[:, 0], EPS)
    if np.isinf(decay):
        rows = np.repeat(np.arange(nq), knn)
        K = sparse.csr_matrix((np.ones(nq * knn), (rows, order[:, :knn].reshape(-1))), shape=(nq, nr))
    else:
        V = _values(D, bw, float(decay))
        keep = V >= max(float(thresh), EPS)
        rows, cols = np.nonzero(keep)
        K = sparse.csr_matrix((V[keep], (rows, cols)), shape=(nq, nr))
    K.sort_indices()
    return K, bw


def threshold_gap(Xq, Yr, knn, decay, thresh):
    """How far the nearest undecided comparison of the reference is from flipping, relative: min |K / thresh - 1| over all pairs
    (decay = inf: the gap between the knn-th and the (knn+1)-th nearest reference over the former).  A pattern compared for
    equality is decided by the data, not by rounding, while this is far above the precision of the distances."""
    D = _distances(Xq, Yr)
    nr = D.shape[1]
    knn = int(min(knn, nr))
    S = np.sort(D, axis=1)
    if np.isinf(decay):
        if knn == nr:
            return np.inf
        return float(np.min((S[:, knn] - S[:, knn - 1]) / np.maximum(S[:, knn - 1], EPS)))
    V = _values(D, np.maximum(S[:, knn - 1], EPS), float(decay))
    return float(np.min(np.abs(V / max(float(thresh), EPS) - 1.0)))
