"""The route of the kNN build (meld_amd.knn_plan) for each shape of DESIGN.md section 4.1's route table -- no GPU: the plan reads
only the library's host-side geometry; the resident-workgroup count, the one device query, is given."""
import dataclasses

import pytest

from meld_amd import _lib
from meld_amd.knn_plan import KnnPlan, SearchOptions, plan_knn_search

RESIDENT = 768  # workgroups of the search resident at once (the order of MI355X's, 256 CUs)
OPTS = SearchOptions()
F = dict(search="f16x3", nprod=1, radius_cut=True, stage2=True)


@pytest.fixture(scope="module")
def lib():
    return _lib.get_lib()


def plan(lib, N, d, q_begin=0, q_count=None, knn=15, ksel=64, options=OPTS, **kw):
    return plan_knn_search(lib, N, d, q_begin, N if q_count is None else q_count, knn, ksel, options=options, resident=RESIDENT, **kw)


def route(**kw):
    base = dict(F, frame=False, prune=True, seed="mfma", knn_cut=15, bounds="none", seeded_bounds=True, lists="none", block_order="lists",
                main_slices=1, two_pass=False, partial_in_search=False)
    base.update(kw)
    return KnnPlan(**base)


def test_headline_1m_x_50(lib):
    p = plan(lib, 1_000_000, 50)
    assert p == route(frame=True, lists="direct", two_pass=True, partial_in_search=True)
    assert p.without_frame() == route(lists="direct")


def test_1m_x_100_frame_through_the_library_rotation(lib):
    assert 100 > lib.meld_frame_max_dims()
    p = plan(lib, 1_000_000, 100)
    assert p == route(frame=True, lists="direct", two_pass=True, partial_in_search=True)
    assert p.without_frame() == route(lists="direct")


def test_200k_x_50_below_the_frame_size(lib):
    p = plan(lib, 200_000, 50)
    assert p == route(lists="direct", main_slices=2)
    assert p.without_frame() == p


def test_few_blocks_slice_the_references(lib, monkeypatch):
    opts = dataclasses.replace(OPTS, rotate_min_cells=0)
    p = plan(lib, 33555, 32, knn=5, options=opts)
    assert p == route(frame=True, knn_cut=5, lists="direct", main_slices=4, partial_in_search=True)
    monkeypatch.setenv("MELD_KNN_TWO_PHASE", "2")
    assert plan(lib, 33555, 32, knn=5, options=opts).two_pass


def test_row_shard_with_shared_spheres(lib):
    p = plan(lib, 1_000_000, 50, 0, 500_000, world=2)
    assert p == route(frame=True, bounds="bounds_from_spheres", lists="table", two_pass=True, partial_in_search=True)


def test_row_shard_without_comm(lib):
    p = plan(lib, 1_000_000, 50, 262144, 262144)
    assert p == route(frame=True, bounds="bounds", lists="table", main_slices=2, partial_in_search=True)


def test_low_dimension_full_split_from_the_start(lib):
    p = plan(lib, 100_000, 4)
    assert p == route(nprod=3, bounds="bounds", block_order="work", main_slices=4, stage2=False)


def test_small_data_unpruned(lib):
    p = plan(lib, 10000, 50)
    assert p == route(prune=False, seeded_bounds=False, block_order="none")


def test_cross_search(lib):
    p = plan(lib, 35000, 30, 20000, 15000, knn=9, ksel=32, cross=True)
    assert p == route(prune=False, seed="none", knn_cut=9, seeded_bounds=False, block_order="none")


def test_wide_data_library_search(lib):
    assert plan(lib, 30000, 160) == KnnPlan("wide", 1, False, False, False, "none", 15, "none", False, "none", "none", 1, False, False, False)
    with pytest.raises(NotImplementedError):
        plan(lib, 30000, 160, 20000, 10000, cross=True)


def test_fp32_search(lib):
    p = plan(lib, 50000, 50, options=dataclasses.replace(OPTS, search="f32"))
    assert p == KnnPlan("f32", 1, False, False, False, "none", 15, "none", False, "none", "none", 1, False, False, False)


def test_given_bandwidth(lib):
    p = plan(lib, 200_000, 50, bandwidth=True)
    assert p == route(seed="bandwidth", knn_cut=0, lists="direct", main_slices=2)
    assert not plan(lib, 1_000_000, 50, bandwidth=True).frame


def test_retry_and_fallback_shapes(lib):
    # (the ksel = 128 retry and the forced fallback are decided by the data; the plan of the longer list and of 20000 x 10)
    assert plan(lib, 200_000, 2, ksel=128) == route(nprod=3, bounds="bounds", block_order="work", main_slices=2, stage2=False)
    assert plan(lib, 20000, 10, knn=2, ksel=128) == route(knn_cut=2, lists="direct", main_slices=4)


def test_options_switch_single_decisions(lib, monkeypatch):
    assert plan(lib, 1_000_000, 50, options=dataclasses.replace(OPTS, prune=False)) == route(prune=False, seeded_bounds=False, block_order="none")
    assert plan(lib, 200_000, 50, options=dataclasses.replace(OPTS, seeded_bounds=False)) == route(seeded_bounds=False, bounds="bounds", lists="table", main_slices=2)
    assert plan(lib, 200_000, 50, options=dataclasses.replace(OPTS, block_order=False)) == route(lists="direct", block_order="none", main_slices=2)
    no_cut = plan(lib, 200_000, 50, options=dataclasses.replace(OPTS, radius_cut=False))
    assert no_cut == route(radius_cut=False, seed="none", seeded_bounds=False, bounds="bounds", block_order="work")
    monkeypatch.setenv("MELD_KNN_LIST_DIRECT", "0")
    assert plan(lib, 200_000, 50) == route(bounds="bounds", lists="table", main_slices=2)
    monkeypatch.setenv("MELD_KNN_TWO_PHASE", "0")
    assert not plan(lib, 1_000_000, 50).two_pass


def test_partial_test_and_lead_bounds_switches(lib, monkeypatch):
    # (development switches: read under MELD_DEV=1 only, and only by the plan -- the library follows what it is handed)
    monkeypatch.setenv("MELD_DEV", "1")
    headline = route(frame=True, lists="direct", two_pass=True, partial_in_search=True)
    assert headline.lead_bounds and not route(lists="direct").lead_bounds and not route(frame=True, lists="table").lead_bounds
    monkeypatch.setenv("MELD_KNN16_EE", "0")  # the frame without the test, and no filter pass
    p = plan(lib, 1_000_000, 50)
    assert p == route(frame=True, lists="direct", partial_forced=True)
    assert p.without_frame() == route(lists="direct", partial_forced=True)
    monkeypatch.setenv("MELD_KNN16_EE", "1")  # the test in the search, frame or not, and no filter pass
    p = plan(lib, 1_000_000, 50)
    assert p == route(frame=True, lists="direct", partial_in_search=True, partial_forced=True)
    assert p.without_frame() == route(lists="direct", partial_in_search=True, partial_forced=True)
    assert plan(lib, 200_000, 50) == route(lists="direct", main_slices=2, partial_in_search=True, partial_forced=True)
    monkeypatch.delenv("MELD_KNN16_EE")
    assert plan(lib, 1_000_000, 50) == headline
    monkeypatch.setenv("MELD_KNN16_LEAD_BOUNDS", "0")  # the direct lists' bounds from all K blocks
    assert plan(lib, 1_000_000, 50) == route(frame=True, lists="direct", two_pass=True, partial_in_search=True, lead_bounds=False)
    assert not plan(lib, 1_000_000, 50).without_frame().lead_bounds
    monkeypatch.setenv("MELD_DEV", "0")  # (outside development mode neither switch is read)
    monkeypatch.setenv("MELD_KNN16_EE", "0")
    assert plan(lib, 1_000_000, 50) == headline
