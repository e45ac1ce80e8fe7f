"""Where the fused row pass behind the search (``KnnPlan.fused_rows``, ``meld_knn_refine_emit``) is planned -- no GPU: the plan reads
the library's host-side geometry only -- and the alignment check of the entry points that read rows as pairs of doubles."""
import ctypes

import pytest

from meld_amd import _lib
from meld_amd.knn_plan import SearchOptions, bucket_route, plan_fused_rows, plan_knn_search

RESIDENT = 768
FREE = 200 << 30  # free device memory handed to the plan: far more than the buckets of any case below need


@pytest.fixture(scope="module")
def lib():
    return _lib.get_lib()


def fused(lib, N, d, q_begin=0, q_count=None, knn=15, ksel=64, options=SearchOptions(), assemble=True, free_bytes=FREE, **kw):
    return plan_knn_search(lib, N, d, q_begin, N if q_count is None else q_count, knn, ksel, options=options, resident=RESIDENT,
                           assemble=assemble, free_bytes=free_bytes, **kw)


def test_headline_build_takes_the_fused_pass(lib):
    p = fused(lib, 1_000_000, 50)
    assert p.fused_rows == "sort+emit" and p.main_slices == 1 and p.lists == "direct"
    # no step lists (too few cells to prune): the search's own finish, the emit stage alone
    assert fused(lib, 3000, 2).fused_rows == "emit" and fused(lib, 3000, 140, ksel=128).fused_rows == "emit"
    # the decision does not change which search route two plans are: it is left out of their comparison, like fused_operands
    assert p == fused(lib, 1_000_000, 50, assemble=False)


def test_callers_that_keep_the_three_kernels(lib):
    # a caller that wants (keys, vals) -- the sharded builder, the MNN blocks, extend.py -- never asks for the assembled rows
    assert fused(lib, 1_000_000, 50, assemble=False).fused_rows == "off"
    # sharded builds: a slice of the rows, ranks that share the spheres
    assert fused(lib, 1_000_000, 50, 0, 500_000, world=2).fused_rows == "off"
    assert fused(lib, 1_000_000, 50, 0, 500_000).fused_rows == "off"
    assert fused(lib, 1_000_000, 50, 262144, 1_000_000 - 262144).fused_rows == "off"
    assert fused(lib, 1_000_000, 50, world=2).fused_rows == "off"
    # the cross search: queries behind the references
    assert fused(lib, 40000, 32, 20000, 20000, cross=True).fused_rows == "off"
    assert plan_fused_rows(lib, 40000, 32, 0, 40000, 64, search="f16x3", cross=True, assemble=True, free_bytes=FREE) == "off"
    # the fp32 search and the library search of wide data
    assert fused(lib, 100_000, 50, options=SearchOptions(search="f32")).fused_rows == "off"
    assert fused(lib, 100_000, 300).search == "wide" and fused(lib, 100_000, 300).fused_rows == "off"


def test_shapes_the_emitting_kernel_does_not_take(lib):
    assert fused(lib, 100_000, 51).fused_rows == "off"  # odd d: no four-chain refinement
    assert fused(lib, 100_000, 7).fused_rows == "off"
    for d in (258, 300):  # d > 256 (beyond the MFMA search as well: whatever search they get, no fused pass)
        assert plan_fused_rows(lib, 100_000, d, 0, 100_000, 64, search="f16x3", assemble=True, free_bytes=FREE) == "off"
    assert plan_fused_rows(lib, 100_000, 256, 0, 100_000, 64, search="f16x3", assemble=True, free_bytes=FREE) == "emit"
    # ksel > 128: more than two entries per lane (the search refuses such lists anyway)
    assert plan_fused_rows(lib, 100_000, 50, 0, 100_000, 129, search="f16x3", assemble=True, free_bytes=FREE) == "off"
    assert plan_fused_rows(lib, 100_000, 50, 0, 100_000, 128, search="f16x3", assemble=True, free_bytes=FREE) == "emit"
    assert fused(lib, 100_000, 50, x_aligned=False).fused_rows == "off"  # rows not 16-byte aligned


def test_sliced_search_takes_the_emit_stage(lib):
    """Few query blocks: the references are cut into slices and ``meld_knn16_merge_slices`` delivers finished rows; the refinement
    behind it emits all the same."""
    p = fused(lib, 200_000, 50)
    assert p.main_slices > 1 and p.lists != "none" and p.fused_rows == "emit"
    assert fused(lib, 400_000, 50).main_slices == 1 and fused(lib, 400_000, 50).fused_rows == "sort+emit"


def test_bucket_memory_that_does_not_fit(lib):
    B = lib.meld_csr_bucket_slots()
    N = 1_000_000
    need = N * B * 12  # tcol (4) + tval (8) per slot
    assert fused(lib, N, 50, free_bytes=4 * need).fused_rows == "sort+emit"
    assert fused(lib, N, 50, free_bytes=4 * need - 4).fused_rows == "off"
    assert fused(lib, N, 50, free_bytes=0).fused_rows == "off"
    assert bucket_route(lib, N, 0, N, 64, cross=False, assemble=True, free_bytes=4 * need)
    assert not bucket_route(lib, N, 0, N, B + 1, cross=False, assemble=True, free_bytes=FREE)  # a list longer than a bucket


def test_development_switches(lib, monkeypatch):
    monkeypatch.setenv("MELD_DEV", "1")
    monkeypatch.setenv("MELD_ROWS_FUSED", "0")
    assert fused(lib, 1_000_000, 50).fused_rows == "off"
    monkeypatch.setenv("MELD_ROWS_FUSED", "a")
    assert fused(lib, 1_000_000, 50).fused_rows == "emit"
    monkeypatch.setenv("MELD_ROWS_FUSED", "b")
    assert fused(lib, 1_000_000, 50).fused_rows == "sort+emit"
    assert fused(lib, 3000, 50).fused_rows == "emit"  # (no lists: nothing leaves the rows raw)
    assert fused(lib, 1_000_000, 51).fused_rows == "off"  # (forcing it on does not lift a condition)
    # the sort-based assembly, or the emit + scatter pair, asked for: no buckets to emit into
    monkeypatch.setenv("MELD_ASSEMBLE", "sort")
    assert fused(lib, 1_000_000, 50).fused_rows == "off"
    monkeypatch.setenv("MELD_ASSEMBLE", "bucket")
    monkeypatch.setenv("MELD_ASSEMBLE_FUSED", "0")
    assert fused(lib, 1_000_000, 50).fused_rows == "off"
    # without MELD_DEV=1 a stray MELD_ROWS_FUSED changes nothing
    monkeypatch.setenv("MELD_ASSEMBLE_FUSED", "1")
    monkeypatch.setenv("MELD_ROWS_FUSED", "0")
    monkeypatch.setenv("MELD_DEV", "0")
    assert fused(lib, 1_000_000, 50).fused_rows == "sort+emit"
    monkeypatch.delenv("MELD_DEV")
    assert fused(lib, 1_000_000, 50).fused_rows == "sort+emit"


def test_misaligned_cells_are_refused_before_any_launch(lib):
    """Even d <= 256: four lanes read 64 contiguous bytes of a row as pairs of doubles, so ``X`` must be 16-byte aligned --
    MELD_ERR_INVALID (-1) from the four entry points, naming themselves.  Every other argument is a plausible non-null address (host
    memory: nothing may touch it); odd d takes the scalar loops and is not refused for its alignment."""
    buf = (ctypes.c_double * 4096)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    x = a + 8
    calls = {
        "meld_knn_refine_emit": lambda X, d: lib.meld_knn_refine_emit(X, 16, d, a, a, a, None, 8, 8, 2, 40.0, 1e-4, a, 0.0, None, 0.0, a, a, a, a, 1.0,
                                                                      None, 0, a, a, a, None),
        "meld_knn_refine": lambda X, d: lib.meld_knn_refine(X, 16, d, 0, 16, a, a, a, None, 8, 8, 2, 40.0, 1e-4, a, 0.0, None, 0.0, a, a, a, a, a,
                                                            None, 0, None, 1.0, None, 0, None),
        "meld_knn_radius_exact": lambda X, d: lib.meld_knn_radius_exact(X, 16, d, 0, a, 1, a, 2, 40.0, 1e-4, 0, a, None, a, None, None, a, 1.0, None),
        "meld_knn_pair_distances": lambda X, d: lib.meld_knn_pair_distances(X, d, a, a, 1, 1, a, None),
    }
    for name, call in calls.items():
        for d in (2, 50, 256):
            lib.meld_scale_f64(None, 1.0, None, 10, None)  # (leaves another entry's message behind)
            assert call(x, d) == -1, (name, d)
            msg = lib.meld_last_error().decode()
            assert msg.startswith(name + ":") and "16-byte aligned" in msg, (name, d, msg)
    # the emitting entry point takes the four-chain shapes only, and says so
    lib.meld_scale_f64(None, 1.0, None, 10, None)
    assert lib.meld_knn_refine_sort_emit(x, 16, 50, a, a, a, a, a, None, 8, 16, 2, 40.0, 1e-4, a, 0.0, None, 0.0, a, a, a, a, 1.0, None, 0, a, a, a, None) == -1
    assert lib.meld_last_error().decode().startswith("meld_knn_refine_sort_emit:") and "16-byte aligned" in lib.meld_last_error().decode()
    assert lib.meld_knn_refine_emit(a, 16, 51, a, a, a, None, 8, 8, 2, 40.0, 1e-4, a, 0.0, None, 0.0, a, a, a, a, 1.0, None, 0, a, a, a, None) == -1
    assert "even d" in lib.meld_last_error().decode()
