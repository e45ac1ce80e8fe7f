"""The L1 / L-infinity graph beyond the dense route (meld_amd/metric_knn.py, csrc/metric_knn.hip), on the host: which builder
serves which request, the kernels' register budget, the library's entry points.  (CPU only: hipcc cross-compiles without a GPU.)"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ["manhattan", "cityblock", "l1", "chebyshev"]
ENTRY_POINTS = ["meld_metric_tile_rows", "meld_metric_tile_boxes", "meld_metric_topk", "meld_metric_refine", "meld_metric_radius"]


@pytest.mark.parametrize("n,expected", [(1800, "dense"), (16384, "dense"), (16385, "metric_knn"), (20000, "metric_knn"), (10**6, "metric_knn")])
def test_route_by_size(n, expected):
    from meld_amd.metric_knn import metric_route

    assert metric_route(n, 50, 7, 40, 1e-4) == expected
    assert metric_route(n, 50, 7, None, 1e-4) == expected  # decay=None: the unweighted graph takes the same route


def test_route_limits_beyond_the_dense_size():
    from meld_amd.metric_knn import metric_route

    assert metric_route(20000, 10, 126, 40, 1e-4) == "metric_knn"
    assert metric_route(20000, 10, 127, 40, 1e-4) == "dense"  # (which refuses: below)
    assert metric_route(20000, 256, 7, 40, 1e-4) == "metric_knn"
    assert metric_route(20000, 257, 7, 40, 1e-4) == "dense"
    assert metric_route(20000, 10, 7, None, 0) == "dense"  # thresh=0 with decay=None stays where it was
    for opts in (dict(sample_idx=[0, 1]), dict(bandwidth=1.0), dict(bandwidth_scale=0.5), dict(knn_max=9)):
        with pytest.raises(NotImplementedError):
            metric_route(20000, 10, 7, 40, 1e-4, opts)
    with pytest.raises(NotImplementedError):
        metric_route(20000, 10, 7, 40, 0)  # the dense "exact" graph of thresh=0


@pytest.mark.parametrize("metric", METRICS)
def test_requests_the_new_route_does_not_serve_are_refused_as_before(metric):
    """knn > 126 and d > 256 beyond 16,384 cells: the dense route's NotImplementedError, raised before anything touches a device."""
    from meld_amd.dense import build_dense_knn_graph
    from meld_amd.metric_knn import build_metric_knn_graph

    X = torch.zeros(20000, 3, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="N <= 16384"):
        build_dense_knn_graph(X, 127, 40, 1e-4, metric=metric)
    with pytest.raises(TypeError):
        build_metric_knn_graph(X, 7, 40, 1e-4, 1, metric)  # (a host tensor)


def test_euclidean_front_end_still_refuses_these_metrics():
    from meld_amd.graph import metric_front_end

    for metric in METRICS:
        with pytest.raises(NotImplementedError, match=repr(metric)):
            metric_front_end(torch.zeros(4, 2, dtype=torch.float64), metric, 40)


def _resource_usage(src):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    from meld_amd import build as mbuild  # (the flags the library is built with, per-file additions included)

    cmd = [hipcc] + mbuild.FLAGS + mbuild.FILE_FLAGS.get(os.path.basename(src), []) + [
        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.devnull]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1200).stdout
    rows, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            rows[cur] = {}
        for key in ("VGPRs:", "ScratchSize [bytes/lane]:", "Occupancy [waves/SIMD]:"):
            if cur and key in line:
                rows[cur][key] = int(line.split(key)[1].split()[0])
    return rows


@pytest.mark.timeout(1500)
def test_metric_kernels_compile_without_scratch():
    from meld_amd import build as mbuild

    assert "metric_knn.hip" in mbuild.SOURCES
    rows = _resource_usage(os.path.join(ROOT, "meld_amd", "csrc", "metric_knn.hip"))
    topk = [k for k in rows if "metric_topk_kernel" in k]
    radius = [k for k in rows if "metric_radius_kernel" in k]
    assert len(topk) == 2 and len(radius) == 2, sorted(rows)  # one instantiation per metric
    assert any("metric_tile_boxes_kernel" in k for k in rows) and any("metric_refine_kernel" in k for k in rows)
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]:"] == 0, (name, r)
    for name in topk:  # (the distances of 32 references and a chunk of 16 query coordinates live in registers)
        assert rows[name]["Occupancy [waves/SIMD]:"] >= 3, (name, rows[name])


def test_entry_points_are_declared_registered_and_exported():
    from meld_amd import _lib

    header = open(os.path.join(ROOT, "include", "meld_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b{}\(".format(name), header), name
        assert name in _lib.SIGNATURES, name
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmeld_hip.so not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    lib.meld_metric_tile_rows.restype = ctypes.c_int
    assert lib.meld_metric_tile_rows() == 64
