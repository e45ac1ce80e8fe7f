"""The host reference of the k-means kernels (tests/kmeans_reference.py) on cases worked by hand, and the condition the GPU tests
rest on: on every generated input they use, the points whose two nearest centres are closer than ``2 tau_i`` -- the only points
whose label the GPU tests do not compare -- are at most 0.1 % of the points."""
import numpy as np
import pytest

from tests import kmeans_reference as ref

LD = np.longdouble


def test_distances_and_argmin_by_hand():
    Y = np.array([[0.0, 0.0], [3.0, 4.0], [1.0, 1.0]])
    C = np.array([[0.0, 0.0], [3.0, 0.0], [0.0, 0.0], [2.0, 2.0]])
    D = ref.distances(Y, C)
    assert D.dtype == LD
    assert D.tolist() == [[0, 9, 0, 8], [25, 16, 25, 5], [2, 5, 2, 2]]
    assert ref.argmin_lowest(D).tolist() == [0, 3, 0]  # (ties to the lowest index: centres 0 = 2, and 0, 2, 3 at distance 2)
    assert ref.gaps(D).tolist() == [0, 11, 0]
    assert ref.inertia(Y, C) == 5 + 2 and ref.inertia(Y, C, [1, 1, 1]) == 9 + 16 + 5


def test_distances_keep_what_fp64_loses():
    """(1e8 + 1 - 1e8)^2 is 1 in the direct form; the expanded form in fp64 cannot see it."""
    Y, C = np.array([[1e8 + 1.0]]), np.array([[1e8]])
    assert ref.distances(Y, C)[0, 0] == 1
    t = ref.tau(Y, C)[0]
    assert t == LD(8 * 5) * LD(2.0) ** -53 * (LD(1e8 + 1.0) ** 2 + LD(1e8) ** 2)
    assert 80 < float(t) < 100  # (at this offset the bound allows the expanded form to be off by more than the distance)


def test_segment_sums_and_lloyd_step_by_hand():
    Y = np.array([[0.0, 1.0], [2.0, 3.0], [10.0, 10.0], [4.0, 5.0]])
    sums, cnt = ref.segment_sums(Y, [0, 0, 2, 0], 4)
    assert sums.tolist() == [[6, 9], [0, 0], [10, 10], [0, 0]] and cnt.tolist() == [3, 0, 1, 0]
    C = np.array([[1.0, 1.0], [100.0, 100.0], [9.0, 9.0]])
    lab, newC, inertia = ref.lloyd_step(Y, C)
    assert lab.tolist() == [0, 0, 2, 0]
    assert newC.tolist() == [[2, 3], [100, 100], [10, 10]]  # (the empty cluster keeps its centre)
    assert inertia == 1 + (1 + 4) + 2 + (9 + 16)


def test_one_centre_has_no_second_best():
    Y, C = ref.assign_case(1, 1, 1)
    assert np.isinf(ref.gaps(ref.distances(Y, C))[0]) and not ref.close_calls(Y, C)[0]


@pytest.mark.parametrize("name", ref.CASE_NAMES)
def test_generated_inputs_leave_few_points_out(name):
    Y, C, D, t = ref.case_reference(name)
    left_out = int((ref.gaps(D) <= 2 * t).sum())
    print(name, "points within 2 tau of a tie:", left_out, "of", Y.shape[0])
    assert left_out <= Y.shape[0] // 1000


def test_duplicate_case_is_what_it_says():
    Y, C = ref.duplicate_case()
    assert np.array_equal(C[5], C[21]) and np.array_equal(C[7], C[33])
    D = ref.distances(Y, C)
    assert np.all(D[np.arange(40), np.arange(40)] == 0)
    lab = ref.argmin_lowest(D)
    assert lab[21] == 5 and lab[33] == 7 and not np.isin(lab, [21, 33]).any()
    # away from the duplicated pairs no point of the case is within 2 tau of a tie
    D2 = np.delete(D, [21, 33], axis=1)
    assert int((ref.gaps(D2) <= 2 * ref.tau(Y, C)).sum()) == 0


def test_step_case_decides_every_point_and_leaves_one_cluster_empty():
    Y, C = ref.step_case()
    assert Y.shape == (1001, 7) and C.shape == (5, 7)
    D = ref.distances(Y, C)
    assert int((ref.gaps(D) <= 2 * ref.tau(Y, C)).sum()) == 0  # (no row is left out of a label comparison)
    lab, newC, _ = ref.lloyd_step(Y, C)
    assert np.bincount(lab, minlength=5)[:4].min() > 100 and not (lab == 4).any() and np.array_equal(newC[4], C[4])


def test_blobs_are_separate():
    X, truth = ref.blobs()
    assert X.shape == (4000, 10) and np.bincount(truth).tolist() == [50] * 80
    means = np.stack([X[truth == b].mean(0) for b in range(80)])
    lab = ref.argmin_lowest(ref.distances(X, means))
    assert np.array_equal(lab, truth)
