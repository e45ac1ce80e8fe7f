"""Landmarks without a device: the host reference of the landmark algebra (tests/landmark_reference.py) against a dense brute-force
statement of graphtools' definition, the pure helpers of meld_amd/landmark.py, the argument checks of ``landmarks()`` that raise
before anything touches the device, the argument contract of the C entries (every refusal comes before any launch), and what hipcc
reports for the kernels of csrc/landmark.hip (no private memory)."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import sparse

from tests import landmark_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _graph60(seed=0):
    """A symmetric 60-cell kernel with a positive diagonal that is not constant, one isolated cell and one hub."""
    rng = np.random.default_rng(seed)
    n = 60
    a, b = rng.integers(0, n - 1, 240), rng.integers(0, n - 1, 240)  # (cell 59 stays isolated)
    keep = a < b
    W = sparse.coo_matrix((rng.uniform(0.05, 1.0, keep.sum()), (a[keep], b[keep])), shape=(n, n)).tocsr()
    W.sum_duplicates()
    hub = sparse.coo_matrix((rng.uniform(0.1, 1.0, n - 2), (np.full(n - 2, 7), np.r_[0:7, 8:n - 1])), shape=(n, n)).tocsr()
    W = sparse.triu(W + hub + hub.T, k=1)
    W = (W + W.T).tocsr()
    return (W + sparse.diags(rng.uniform(0.2, 1.0, n))).tocsr()


@pytest.mark.parametrize("L", [1, 2, 7, 59])
def test_reference_against_the_dense_definition(L):
    K = _graph60()
    assert abs(K - K.T).max() == 0 and K[59].nnz == 1
    rng = np.random.default_rng(L)
    labels = np.r_[np.arange(L), rng.integers(0, L, 60 - L)][rng.permutation(60)]  # (every landmark present)
    got, want = ref.landmark_algebra(K, labels, L), ref.brute_force(K, labels, L)
    np.testing.assert_allclose(got["transitions"].toarray(), want["transitions"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(got["pmn"].toarray(), want["pmn"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(got["landmark_op"], want["landmark_op"], rtol=1e-13, atol=1e-300)
    op = got["landmark_op"]
    assert op.shape == (L, L) and op.min() >= 0
    np.testing.assert_allclose(op.sum(1), 1.0, rtol=1e-13)
    np.testing.assert_allclose(got["r"], np.asarray(K.sum(1)).ravel(), rtol=1e-14)
    # the merged rows hold every present label once, ascending
    A = got["A"]
    for i in range(60):
        row = A.indices[A.indptr[i]:A.indptr[i + 1]]
        assert np.all(np.diff(row) > 0)
        assert set(row) == set(labels[K.indices[K.indptr[i]:K.indptr[i + 1]]])


def test_label_compaction():
    from meld_amd.landmark import check_clusters, compact_labels

    c, values = compact_labels(np.array([7, 3, 3, 100, 7, 0]))
    assert c.dtype == np.int32 and c.tolist() == [2, 1, 1, 3, 2, 0] and values.tolist() == [0, 3, 7, 100]
    c, L = check_clusters(np.array([5, 5, 9, 2 ** 40], dtype=np.int64), 4)
    assert c.tolist() == [0, 0, 1, 2] and L == 3
    c, L = check_clusters(np.array([4, 4, 4], dtype=np.uint8), 3)
    assert c.tolist() == [0, 0, 0] and L == 1
    import torch

    c, L = check_clusters(torch.tensor([1, 0, 1]), 3)
    assert c.tolist() == [1, 0, 1] and L == 2


def test_bad_clusters():
    from meld_amd.landmark import LANDMARK_MAX, check_clusters

    with pytest.raises(ValueError, match="one entry per cell"):
        check_clusters(np.zeros(5, dtype=np.int64), 6)
    with pytest.raises(ValueError, match="negative"):
        check_clusters(np.array([0, -1, 2]), 3)
    with pytest.raises(TypeError, match="integers"):
        check_clusters(np.array([0.0, 1.0, 2.0]), 3)
    with pytest.raises(TypeError, match="integers"):
        check_clusters(np.array([True, False, True]), 3)
    with pytest.raises(ValueError, match="one-dimensional"):
        check_clusters(np.zeros((3, 1), dtype=np.int64), 3)
    with pytest.raises(ValueError, match=str(LANDMARK_MAX)):
        check_clusters(np.arange(LANDMARK_MAX + 1), LANDMARK_MAX + 1)


def test_n_landmark_checks():
    from meld_amd.landmark import LANDMARK_MAX, check_n_landmark

    assert check_n_landmark(np.int64(5), 6) == 5 and check_n_landmark(LANDMARK_MAX, 10 ** 6) == LANDMARK_MAX
    for bad in (0, -3, 2.0, "4", True, None):
        with pytest.raises(ValueError, match="positive integer"):
            check_n_landmark(bad, 100)
    with pytest.raises(ValueError, match="less than the number of cells"):
        check_n_landmark(100, 100)
    with pytest.raises(ValueError, match="above the {} landmarks".format(LANDMARK_MAX)):
        check_n_landmark(LANDMARK_MAX + 1, 10 ** 6)


def test_landmarks_refuses_before_touching_the_device():
    """A stub with the attributes the checks read: none of these calls gets as far as a tensor."""
    from meld_amd.landmark import LANDMARK_MAX, landmarks

    def stub(**kw):
        return SimpleNamespace(**dict(dict(N=100, n_rows=100, comm=None, n_landmark=None), **kw))

    with pytest.raises(ValueError, match="neither n_landmark nor clusters"):
        landmarks(stub())
    with pytest.raises(ValueError, match="less than the number of cells"):
        landmarks(stub(n_landmark=100))  # (the recorded default is used, and checked)
    with pytest.raises(ValueError, match="less than the number of cells"):
        landmarks(stub(), n_landmark=250)
    with pytest.raises(ValueError, match="above the {} landmarks".format(LANDMARK_MAX)):
        landmarks(stub(N=10 ** 6, n_rows=10 ** 6), n_landmark=LANDMARK_MAX + 1)
    with pytest.raises(ValueError, match="n_svd"):
        landmarks(stub(), n_landmark=10, n_svd=0)
    with pytest.raises(ValueError, match="only defined for an unsharded graph"):
        landmarks(stub(n_rows=50), n_landmark=10)
    with pytest.raises(ValueError, match="one entry per cell"):
        landmarks(stub(), clusters=np.zeros(99, dtype=np.int64))
    with pytest.raises(TypeError, match="integers"):
        landmarks(stub(), clusters=np.zeros(100))


def test_estimator_delegates_and_needs_a_fit():
    import meld_amd

    op = meld_amd.MELD(n_landmark=50)
    assert op.n_landmark == 50
    with pytest.raises(ValueError, match="must be `fit`"):
        op.landmarks()


def test_cap_and_argument_contract_of_the_library():
    """``meld_landmark_max()`` is what the Python layer refuses above, and at least 4096; every bad call returns -1 with the entry's
    name in the message.  The addresses are host memory: nothing may touch them, and nothing does -- the checks come before any
    launch."""
    from meld_amd import _lib
    from meld_amd.landmark import LANDMARK_MAX

    lib = _lib.get_lib()
    cap = lib.meld_landmark_max()
    assert cap >= 4096 and cap == LANDMARK_MAX
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)

    def refused(name, status):
        assert status == -1, name
        assert lib.meld_last_error().decode().startswith(name + ":"), lib.meld_last_error()

    count, fill, gram = lib.meld_landmark_merge_count, lib.meld_landmark_merge_fill, lib.meld_landmark_gram
    refused("meld_landmark_merge_count", count(None, a, 4, 4, a, 2, None, 0, a, a, None))
    refused("meld_landmark_merge_count", count(a, a, 4, 4, None, 2, None, 0, a, a, None))
    refused("meld_landmark_merge_count", count(a, a, 4, 4, a, 2, None, 0, a, None, None))
    refused("meld_landmark_merge_count", count(a, None, 4, 4, a, 2, None, 0, a, a, None))
    refused("meld_landmark_merge_count", count(a, a, 4, 4, a, 2, None, 0, None, a, None))
    refused("meld_landmark_merge_count", count(a, a, 4, 4, a, 0, None, 0, a, a, None))
    refused("meld_landmark_merge_count", count(a, a, 4, 4, a, cap + 1, None, 0, a, a, None))
    refused("meld_landmark_merge_count", count(a, a, -1, 4, a, 2, None, 0, a, a, None))
    refused("meld_landmark_merge_count", count(a, a, 4, -1, a, 2, None, 0, a, a, None))
    refused("meld_landmark_merge_count", count(a, a, 4, 5, a, 2, None, 1, a, a, None))  # (a diagonal on a matrix that is not square)
    assert count(a, None, 0, 0, a, 2, None, 0, None, a, None) == 0  # (an empty problem: a successful no-op)
    refused("meld_landmark_merge_fill", fill(None, a, None, 4, a, a, a, a, a, None))
    refused("meld_landmark_merge_fill", fill(a, a, None, 4, a, None, a, a, a, None))
    refused("meld_landmark_merge_fill", fill(a, a, None, 4, a, a, a, a, None, None))
    refused("meld_landmark_merge_fill", fill(a, None, None, 4, a, a, a, a, a, None))
    refused("meld_landmark_merge_fill", fill(a, a, None, 4, a, a, None, a, a, None))
    refused("meld_landmark_merge_fill", fill(a, a, None, -2, a, a, a, a, a, None))
    assert fill(a, None, None, 0, None, a, None, None, a, None) == 0
    refused("meld_landmark_gram", gram(None, a, a, 4, a, a, a, 2, a, a, a, None))
    refused("meld_landmark_gram", gram(a, a, a, 4, None, a, a, 2, a, a, a, None))
    refused("meld_landmark_gram", gram(a, a, a, 4, a, a, a, 2, None, a, a, None))
    refused("meld_landmark_gram", gram(a, a, a, 4, a, a, a, 2, a, None, a, None))
    refused("meld_landmark_gram", gram(a, a, a, 4, a, a, a, 2, a, a, None, None))
    refused("meld_landmark_gram", gram(a, None, a, 4, a, a, a, 2, a, a, a, None))
    refused("meld_landmark_gram", gram(a, a, a, 4, a, a, a, 0, a, a, a, None))
    refused("meld_landmark_gram", gram(a, a, a, 4, a, a, a, cap + 1, a, a, a, None))
    refused("meld_landmark_gram", gram(a, a, a, -1, a, a, a, 2, a, a, a, None))


def test_landmark_kernels_do_not_spill():
    """The three kernels as hipcc compiles them with the build's flags: no private memory (the figures tests/test_kernel_resources.py
    reads for the search kernels)."""
    from tests.test_kernel_resources import _resource_usage

    rows = _resource_usage(os.path.join(ROOT, "meld_amd", "csrc", "landmark.hip"))
    kernels = {k: v for k, v in rows.items() if "landmark_" in k and "_kernel" in k}
    assert len(kernels) == 3, sorted(rows)
    for name, r in kernels.items():
        assert r["ScratchSize [bytes/lane]:"] == 0, (name, r)
        assert r["VGPRs:"] <= 64 and r["Occupancy [waves/SIMD]:"] == 8, (name, r)  # (the kernels wait on memory: full occupancy)
