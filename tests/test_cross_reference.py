"""tests/cross_reference.py against the project's ground truth (host only).  Every GPU result of tests/test_gpu_cross_search.py is
judged by this reference, so it is tied to the oracle first -- and every data set those tests use is shown to keep its kernel
values clear of ``thresh``, so that comparing sparsity patterns for equality is decided by the data and never by rounding."""
import numpy as np
import pytest

from tests import cross_reference as cr

GAP = 1e-9  # relative; the distances behind the values carry ~1e-15


@pytest.mark.parametrize("d", cr.FAR_DIMS)
def test_reference_reproduces_the_oracle_on_the_far_samples(d):
    from oracle import meld_oracle as mo

    A, B = cr.far_samples(d, cr.SEED)
    assert A.shape == (900, d) and B.shape == (887, d)
    for Xq, Yr in ((A, B), (B, A)):
        K, bw = cr.cross_block_reference(Xq, Yr, cr.KNN, cr.DECAY, cr.THRESH)
        Ko = mo.kernel_to_data(Xq, Yr, knn=cr.KNN, decay=cr.DECAY, thresh=cr.THRESH)
        Ko.sort_indices()
        per_row = np.diff(K.indptr)
        print("d = %d: %d entries, %d..%d per row, max |K - oracle| = %.3e" % (d, K.nnz, per_row.min(), per_row.max(), abs(K - Ko).max()))
        assert np.array_equal(K.indptr, Ko.indptr) and np.array_equal(K.indices, Ko.indices)
        assert np.abs(K.data - Ko.data).max() <= 1e-14
        assert per_row.min() >= cr.KNN
        assert d < 50 or per_row.max() > 32  # at d = 50 some rows exceed the shortest candidate list: they must be swept
        assert np.all(bw > 0)
        # The oracle on sklearn's brute-force search, which the GPU tests of whole graphs ask for (it is the fast one): the same
        # pattern.  Its distances come in the GEMM form |x|^2 + |y|^2 - 2 x.y on the cells as given, 200 units from the origin:
        # d^2 ~ 20..100 carries up to (d + 3) u (|x|^2 + |y|^2 + 2 |x.y|) ~ 9e-10 (u = 1.1e-16, |x|^2 ~ 4.1e4, d = 50), 4.5e-11
        # relative; (dist / bw)^40 then 40 * 4.5e-11, a kernel value K x (K e^-x, x <= 9.2: K x <= 0.37) at most 7e-10 -- against
        # 1e-14 for direct differences.  Measured: 3.3e-11 / 3.9e-11 at d = 10, 1.2e-11 / 1.1e-11 at d = 50, and 6e-15 .. 9e-15
        # for this reference against long-double arithmetic.  Bound: the 1e-9 those graph tests allow.
        Kb = mo.kernel_to_data(Xq, Yr, knn=cr.KNN, decay=cr.DECAY, thresh=cr.THRESH, algorithm="brute")
        Kb.sort_indices()
        print("d = %d: max |K - oracle on the brute-force search| = %.3e" % (d, abs(K - Kb).max()))
        assert np.array_equal(K.indptr, Kb.indptr) and np.array_equal(K.indices, Kb.indices)
        assert np.abs(K.data - Kb.data).max() <= 1e-9


def test_reference_connectivity_and_clipping_follow_the_oracle():
    from oracle import meld_oracle as mo

    cases = cr.far_block_cases()
    Xq, Yr, knn, decay = cases["decay_inf"]
    K, _ = cr.cross_block_reference(Xq, Yr, knn, decay, cr.THRESH)
    Ko = mo.kernel_to_data(Xq, Yr, knn=knn, decay=None, thresh=cr.THRESH)
    Ko.sort_indices()
    assert np.array_equal(K.indptr, Ko.indptr) and np.array_equal(K.indices, Ko.indices) and np.all(K.data == 1)
    assert np.all(np.diff(K.indptr) == knn)
    Xq, Yr, knn, decay = cases["knn_clipped"]
    assert Yr.shape[0] < knn
    K, _ = cr.cross_block_reference(Xq, Yr, knn, decay, cr.THRESH)
    Ko = mo.kernel_to_data(Xq, Yr, knn=knn, decay=decay, thresh=cr.THRESH)
    Ko.sort_indices()
    assert np.array_equal(K.indptr, Ko.indptr) and np.array_equal(K.indices, Ko.indices)
    assert np.abs(K.data - Ko.data).max() <= 1e-14
    assert np.all(np.diff(K.indptr) >= 1)


def test_no_kernel_value_of_the_gpu_tests_sits_on_the_threshold():
    """The gap to ``thresh`` (decay = inf: between the knn-th and the next reference) of every block the GPU tests compare."""
    from meld_amd._lib import get_lib

    lib = get_lib()
    worst = {}
    for name, (Xq, Yr, knn, decay) in cr.far_block_cases().items():
        worst[name] = cr.threshold_gap(Xq, Yr, knn, decay, cr.THRESH)
    for d in cr.FAR_DIMS:
        A, B = cr.far_samples(d, cr.SEED)
        for t in cr.UNIT_SCALES:  # (an exact scaling: the same gap, asserted all the same)
            worst["far_d%d_times_%g" % (d, t)] = cr.threshold_gap(A * t, B * t, cr.KNN, cr.DECAY, cr.THRESH)
        # the blocks of a sample with itself in the MNN graph: the cell finds itself first, the bandwidth is its (knn+1)-th
        worst["far_d%d_A_within" % d] = cr.threshold_gap(A, A, cr.KNN + 1, cr.DECAY, cr.THRESH)
        worst["far_d%d_B_within" % d] = cr.threshold_gap(B, B, cr.KNN + 1, cr.DECAY, cr.THRESH)
    for d in cr.EDGE_DIMS:
        for nr, nq in cr.edge_shapes(lib.meld_knn16_tile_refs(), lib.meld_knn16_block_queries()):
            Xq, Yr = cr.edge_samples(d, nr, nq)
            worst["edge_d%d_nr%d_nq%d" % (d, nr, nq)] = cr.threshold_gap(Xq, Yr, cr.KNN, cr.DECAY, cr.THRESH)
    name = min(worst, key=worst.get)
    print("smallest gap: %.3e (%s) over %d data sets" % (worst[name], name, len(worst)))
    assert worst[name] > GAP, (name, worst[name])
