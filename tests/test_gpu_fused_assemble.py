"""The CSR is written once: row sums out of ``meld_csr_rows_sort_merge_sums`` and the anisotropy inside the compaction
(``meld_csr_compact_rows_anisotropy``) against today's sequence -- ``meld_csr_rows_sort_merge``, ``meld_csr_compact_rows_sums``,
``meld_csr_anisotropy_degrees`` -- on the same buckets: ``rowptr``, ``col``, ``val``, the degrees and the row sums bit for bit.
And one build of the benchmark's cells with the fused routes (operands and hand-over) on and off."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _sym_coo(rng, N, deg, hub=0):
    """directed entries (i, j, v), i != j, unique per (i, j), in both directions at v / 2 like meld_coo_emit; ``hub``: that many rows
    point at cell 0 (a long transposed row); a third of the pairs are mutual (both directions present: two addends)"""
    i = np.repeat(np.arange(N), deg)
    j = rng.integers(0, N, size=i.shape[0])
    if hub:
        j[np.arange(hub) * deg + deg] = 0  # row 1 .. hub: one entry each towards cell 0
    keep = i != j
    i, j = i[keep], j[keep]
    _, first = np.unique(i.astype(np.int64) << 32 | j, return_index=True)
    i, j = i[first], j[first]
    v = rng.random(i.shape[0])
    keys = np.concatenate([(i.astype(np.int64) << 32) | j, (j.astype(np.int64) << 32) | i])
    vals = np.concatenate([0.5 * v, 0.5 * v])
    p = rng.permutation(keys.shape[0])
    return keys[p], vals[p]


def _buckets(ops, keys, vals, N):
    from meld_amd._lib import check, ptr

    lib = ops.lib
    B = int(lib.meld_csr_bucket_slots())
    k, v = torch.from_numpy(keys).cuda(), torch.from_numpy(vals).cuda()
    cursor = torch.empty(N, dtype=torch.int32, device="cuda")
    tcol = torch.zeros(N * B, dtype=torch.int32, device="cuda")
    tval = torch.zeros(N * B, dtype=torch.float64, device="cuda")
    check(lib.meld_coo_scatter_rows(ptr(k), ptr(v), int(k.shape[0]), 0, N, ptr(cursor), ptr(tcol), ptr(tval), None), "meld_coo_scatter_rows")
    return cursor, tcol, tval


def _both(ops, keys, vals, N, a, symm):
    """(separate, fused): each (rowptr, col, val, dw, ksum) as numpy, or None where the bucket path declined"""
    out = []
    for fused in (False, True):
        # (the scatter's atomics place a row's entries in arrival order; the merge sorts them by column, so both runs merge the same rows)
        cursor, tcol, tval = _buckets(ops, keys, vals, N)
        done = ops._finish_buckets(cursor, tcol, tval, N, sums_diag=1.0, symm=symm, anisotropy=a if fused else None)
        if done is None:
            out.append(None)
            continue
        rowptr, col, val = done
        ksum = ops.last_row_sums[1]
        if fused:
            dw = ops.last_degrees
            assert dw is not None
        else:
            assert ops.last_degrees is None
            dw = ops.anisotropy_degrees(rowptr, col, val, N, ksum, 0, a)
        torch.cuda.synchronize()
        out.append(tuple(t.cpu().numpy() for t in (rowptr, col, val, dw, ksum)))
    return out


def _assert_same(sep, fus):
    for name, x, y in zip(("rowptr", "col", "val", "dw", "ksum"), sep, fus):
        assert x.shape == y.shape, name
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "{}: {} entries differ".format(name, int((x != y).sum()))


@pytest.mark.parametrize("a", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("symm", [(0, 0.0), (1, 0.0), (2, 0.7)], ids=["plus", "times", "mnn"])
def test_fused_compaction_equals_compaction_then_anisotropy(a, symm):
    from meld_amd.graph import HipOps

    ops = HipOps()
    N = 4000  # (40 of 4000: one pair in a hundred is mutual -- two addends under "+", all that "*" keeps)
    keys, vals = _sym_coo(np.random.default_rng(17), N, 40)
    sep, fus = _both(ops, keys, vals, N, a, symm)
    assert sep is not None and fus is not None and ops.last_assemble == "bucket"
    _assert_same(sep, fus)
    assert sep[0][-1] > 0


@pytest.mark.parametrize("a", [0.0, 0.5, 1.0])
def test_hub_row_near_the_bucket_limit(a):
    """cell 0 is the neighbour of 205 rows: with its own 20 entries and those of the rows that point at it by chance its bucket
    holds ~250 of the 256 slots (four entries per lane in the merge's network)"""
    from meld_amd.graph import HipOps

    ops = HipOps()
    N = 5000
    keys, vals = _sym_coo(np.random.default_rng(23), N, 20, hub=205)
    n0 = int(((keys >> 32) == 0).sum())
    assert 240 <= n0 <= int(ops.lib.meld_csr_bucket_slots()), n0
    sep, fus = _both(ops, keys, vals, N, a, (0, 0.0))
    assert sep is not None and fus is not None
    _assert_same(sep, fus)
    assert sep[0][1] - sep[0][0] >= 225  # (the hub row kept its entries: its own 20 and the 205)


def test_overflowing_bucket_still_routes_to_the_sort_path(monkeypatch):
    from meld_amd.graph import HipOps

    ops = HipOps()
    N = 5000
    keys, vals = _sym_coo(np.random.default_rng(29), N, 20, hub=400)
    assert int(((keys >> 32) == 0).sum()) > int(ops.lib.meld_csr_bucket_slots())
    sep, fus = _both(ops, keys, vals, N, 1.0, (0, 0.0))
    assert sep is None and fus is None  # (the flag: both forms decline, the caller sorts)
    rp, col, val = ops.assemble_rows(torch.from_numpy(keys).cuda(), torch.from_numpy(vals).cuda(), 0, N, N)
    assert ops.last_assemble == "sort" and int(rp[1] - rp[0]) > int(ops.lib.meld_csr_bucket_slots())


def test_build_with_the_fused_routes_on_and_off_gives_the_same_graph(monkeypatch):
    """``build_knn_graph`` on the benchmark's generator at 200k x 50: one pass for the operands and the anisotropy inside the
    compaction (the plan's defaults) against the separate passes (MELD_KNN_FUSED_OPERANDS=0, MELD_ASSEMBLE_FUSED_ANISO=0)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench
    from meld_amd.graph import build_knn_graph

    X, _ = bench.synthetic_cells(200_000, n_dims=50, seed=0)
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).cuda()
    graphs = []
    for on in ("1", "0"):
        monkeypatch.setenv("MELD_KNN_FUSED_OPERANDS", on)
        monkeypatch.setenv("MELD_ASSEMBLE_FUSED_ANISO", on)
        G = build_knn_graph(Xd, knn=15)
        torch.cuda.synchronize()
        assert G.info["assemble"] == "bucket"
        graphs.append(tuple(t.cpu().numpy() for t in (G.rowptr, G.col, G.val, G.dw_dev, G.ksum)))
        del G
    _assert_same(graphs[1], graphs[0])
