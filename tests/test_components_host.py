"""Connectivity, host side (no GPU): selection validation on plain numpy input, the refusal of a row-sharded graph on a stub
object, the default round cap (meld_amd/components.py)."""
import math

import numpy as np
import pytest
import torch


def _stub_graph(n=6):
    from meld_amd.graph import DeviceGraph

    return DeviceGraph(torch.zeros(n + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.float64),
                       torch.zeros(n, dtype=torch.float64))


def test_selection_index_accepts_integers_and_masks():
    from meld_amd.components import selection_index

    for ind in ([4, 0, 2], np.array([4, 0, 2], dtype=np.int32), np.array([4, 0, 2], dtype=np.uint8), torch.tensor([4, 0, 2])):
        out = selection_index(ind, 6)
        assert isinstance(out, np.ndarray) and out.dtype == np.int64 and out.tolist() == [4, 0, 2]  # the order given is kept
    mask = np.array([True, False, True, False, True, False])
    for m in (mask, mask.tolist(), torch.from_numpy(mask)):
        out = selection_index(m, 6)
        assert out.dtype == np.int64 and out.tolist() == [0, 2, 4]
    assert selection_index(np.arange(6), 6).tolist() == list(range(6))


def test_selection_index_refusals():
    from meld_amd.components import selection_index

    with pytest.raises(ValueError, match="more than once"):
        selection_index([1, 3, 1], 6)
    for bad in ([0, 6], [-1, 2], np.array([2**40])):
        with pytest.raises(ValueError, match=r"outside \[0, 6\)"):
            selection_index(bad, 6)
    for bad in ([], np.array([], dtype=np.int64), np.zeros(6, dtype=bool)):
        with pytest.raises(ValueError, match="empty"):
            selection_index(bad, 6)
    with pytest.raises(ValueError, match="one entry per cell"):
        selection_index(np.ones(5, dtype=bool), 6)
    with pytest.raises(ValueError, match="one-dimensional"):
        selection_index(np.zeros((2, 2), dtype=np.int64), 6)
    for bad in ([1.0, 2.0], np.array([1, 2], dtype=np.float32), np.array(["a", "b"]), np.array([1 + 0j]), torch.tensor([0.5])):
        with pytest.raises(TypeError, match="integer array or a boolean mask"):
            selection_index(bad, 6)


def test_a_row_sharded_graph_is_refused_before_any_device_work():
    G = _stub_graph()
    calls = (G.connected_components_device, G.connected_components, G.is_connected, lambda: G.component_sizes, G.extract_components,
             G.largest_component, lambda: G.subgraph([0, 1]))
    G.N = 12  # (a shard: six of twelve rows)
    for call in calls:
        with pytest.raises(ValueError, match="only defined for an unsharded graph"):
            call()
    G.N = 6
    G.comm = object()  # (one rank's share of a distributed build)
    for call in calls:
        with pytest.raises(ValueError, match="only defined for an unsharded graph"):
            call()
    assert getattr(G, "_components", None) is None and not hasattr(G, "components_info")


def test_default_round_cap():
    from meld_amd.components import default_max_rounds

    for n in (1, 2, 3, 4, 5, 4096, 4097, 10**6, 2**31 - 1):
        assert default_max_rounds(n) == 4 * math.ceil(math.log2(n)) + 64, n
    assert default_max_rounds(1) == 64 and default_max_rounds(4097) == 116 and default_max_rounds(10**6) == 144
    with pytest.raises(ValueError):
        default_max_rounds(0)
