"""New cells on the L1 / L-infinity graphs, host side (no GPU): which graphs are extendable, the entry points, and the register
budget of the kernels of the search between two point sets (csrc/metric_knn.hip).  (hipcc cross-compiles without a GPU.)"""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["meld_metric_cross_slices", "meld_metric_cross_seed", "meld_metric_cross_topk", "meld_metric_cross_refine",
                "meld_metric_cross_radius"]


def _stub_graph(n=6, **info):
    from meld_amd.graph import DeviceGraph

    G = DeviceGraph(torch.zeros(n + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.float64),
                    torch.zeros(n, dtype=torch.float64))
    G.info.update(info)
    return G


def _with_state(G, **kw):
    from meld_amd.extend import attach_extension_state

    args = dict(X=torch.zeros(G.N, 3, dtype=torch.float64), n_features_in=3, project=None, row_fn=None, knn=2, decay=40.0, thresh=1e-4)
    args.update(kw)
    return attach_extension_state(G, **args)


@pytest.mark.parametrize("info", [dict(route="metric_knn", metric="manhattan"), dict(route="metric_knn", metric="chebyshev"),
                                  dict(dense=True, dense_knn=True, metric="l1"), dict(dense=True, dense_knn=True, metric="cityblock")])
def test_a_graph_with_an_l1_state_is_extendable(info):
    from meld_amd import extend
    from meld_amd.metric_knn import METRICS

    G = _with_state(_stub_graph(**info), metric=METRICS[info["metric"]])
    assert extend.refusal(G) is None
    assert extend.state_of(G).metric == METRICS[info["metric"]]
    # the shape check still comes first, before anything touches a device
    with pytest.raises(ValueError, match=r"Y must be of shape \(n, 3\)"):
        G.build_kernel_to_data(np.zeros((2, 4)))


def test_graphs_without_the_state_keep_their_refusals():
    from meld_amd import extend

    Y = np.zeros((2, 3))
    G = _stub_graph(route="metric_knn", metric="manhattan")
    assert extend.refusal(G) == ("the L1 / L-inf graphs (distance='manhattan') cannot be extended to new cells: the search between two "
                                 "point sets is euclidean")
    G = _stub_graph(dense=True, metric="chebyshev")
    assert "L1 / L-inf" in extend.refusal(G)
    G = _stub_graph(dense=True)
    assert extend.refusal(G).startswith("a dense graph (thresh=0, a precomputed matrix, or a kernel evaluated densely)")
    # a euclidean state does not make a dense or an L1 graph extendable
    assert "dense graph" in extend.refusal(_with_state(_stub_graph(dense=True)))
    assert "L1 / L-inf" in extend.refusal(_with_state(_stub_graph(route="metric_knn", metric="l1")))
    # what stays refused with an L1 state
    from meld_amd.metric_knn import METRICS

    code = METRICS["manhattan"]
    for G, what in [(_with_state(_stub_graph(graph="mnn", metric="manhattan"), metric=code), "MNN graph"),
                    (_with_state(_stub_graph(metric="manhattan"), metric=code, knn_max=9), "knn_max"),
                    (_with_state(_stub_graph(metric="manhattan"), metric=code, bandwidth=lambda d: d), "callable bandwidth"),
                    (_with_state(_stub_graph(metric="manhattan"), metric=code, bandwidth=np.ones(6)), "per-cell bandwidth"),
                    (_with_state(_stub_graph(metric="manhattan", adopted_from="kNNGraph"), metric=code), "adopted from kNNGraph")]:
        with pytest.raises(NotImplementedError, match=what):
            G.build_kernel_to_data(Y)
    G = _with_state(_stub_graph(metric="manhattan"), metric=code)
    G.N = 12  # (a shard)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        G.extend_to_data(Y)


def test_sparse_cells_pass_the_shape_check_before_the_device():
    from meld_amd.extend import check_extension_shape

    with pytest.raises(ValueError, match=r"Y must be of shape either \(n, 30000\) or \(n, 20\)"):
        check_extension_shape((5, 21), 30000, 20)
    assert check_extension_shape((5, 20), 30000, 20) == "reduced"  # (refused for sparse input by prepare_queries)


def test_entry_points_are_declared_and_registered():
    from meld_amd import _lib

    header = open(os.path.join(ROOT, "include", "meld_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b{}\(".format(name), header), name
        assert name in _lib.SIGNATURES, name
        n_args = len([a for a in re.search(r"\b{}\((.*?)\);".format(name), header, flags=re.S).group(1).split(",") if a.strip()])
        assert n_args == len(_lib.SIGNATURES[name][1]), (name, n_args)


@pytest.mark.timeout(1500)
def test_cross_kernels_compile_within_the_search_budget():
    from tests.test_metric_knn_host import _resource_usage

    rows = _resource_usage(os.path.join(ROOT, "meld_amd", "csrc", "metric_knn.hip"))
    search = [k for k in rows if "metric_cross_topk_kernel" in k]
    sweep = [k for k in rows if "metric_cross_radius_kernel" in k]
    seed = [k for k in rows if "metric_cross_seed_kernel" in k]
    merge = [k for k in rows if "metric_cross_merge_kernel" in k]
    refine = [k for k in rows if "metric_cross_refine_kernel" in k]
    assert len(search) == 2 and len(sweep) == 2 and len(seed) == 2, sorted(rows)  # one instantiation per metric
    assert len(merge) == 1 and len(refine) == 1, sorted(rows)
    for name in search + sweep + seed + merge + refine:
        assert rows[name]["ScratchSize [bytes/lane]:"] == 0, (name, rows[name])
    for name in search:  # (the self search's budget: 32 distances and 16 query coordinates in registers)
        assert rows[name]["Occupancy [waves/SIMD]:"] >= 3, (name, rows[name])
