"""One pass over the cells for the search operands: ``meld_knn16_prepare_fused`` (reference tiles, query rows, norms and the tile
spheres from one read of every 64-row tile) against today's sequence of separate entry points on the same inputs --
``meld_knn16_prepare_scaled`` (or ``meld_knn16_prepare``) followed by ``meld_knn16_tile_spheres`` over all tiles.  Every output
array is compared byte for byte."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _cells(N, d, seed, const_col=None):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N, d)) * np.linspace(3.0, 0.2, d) + rng.normal(size=d)
    if const_col is not None:
        X[:, const_col] = 2.5
    return torch.from_numpy(X).cuda()


def _outputs(ops, X, fused, with_extremes):
    from meld_amd._lib import check, ptr

    lib = ops.lib
    N, d = int(X.shape[0]), int(X.shape[1])
    TS, BQ = lib.meld_knn16_tile_refs(), lib.meld_knn16_block_queries()
    n_tiles, q_pad = -(-N // TS), -(-N // BQ) * BQ
    sums, cmin, cmax = ops.col_stats(X)
    mean = sums / N
    u8 = dict(dtype=torch.uint8, device=X.device)
    f32 = dict(dtype=torch.float32, device=X.device)
    Rt = torch.zeros(n_tiles * lib.meld_knn16_tile_bytes(d), **u8)
    Q = torch.zeros(q_pad * lib.meld_knn16_query_bytes(d), **u8)
    Qn, norm2, nmax, scale = torch.zeros(q_pad, **f32), torch.zeros(N, **f32), torch.zeros(1, **f32), torch.zeros(4, **f32)
    temp = torch.zeros(lib.meld_knn16_bounds_temp_bytes(N, d, N), **u8)
    lo, hi = (ptr(cmin), ptr(cmax)) if with_extremes else (None, None)
    if fused:
        temp[: temp.numel() - 256].fill_(0xAB)  # (the call zeroes the arrays itself; the 256 bytes of slack behind them are nobody's)
        check(lib.meld_knn16_prepare_fused(ptr(X), N, d, ptr(mean), lo, hi, ptr(Rt), ptr(Q), ptr(Qn), ptr(norm2), ptr(nmax), ptr(scale), ptr(temp), None),
              "meld_knn16_prepare_fused")
    else:
        tail = (0, N, ptr(Rt), ptr(Q), ptr(Qn), ptr(norm2), ptr(nmax), ptr(scale), None)
        if with_extremes:
            check(lib.meld_knn16_prepare_scaled(ptr(X), N, d, ptr(mean), lo, hi, *tail), "meld_knn16_prepare_scaled")
        else:
            check(lib.meld_knn16_prepare(ptr(X), N, d, ptr(mean), *tail), "meld_knn16_prepare")
        check(lib.meld_knn16_tile_spheres(ptr(X), N, d, ptr(mean), ptr(scale), ptr(temp), 0, n_tiles, None), "meld_knn16_tile_spheres")
    torch.cuda.synchronize()
    out = dict(Rt=Rt, Q=Q, Qn=Qn, norm2=norm2, norm2_max=nmax, scale_info=scale, spheres=temp)
    return {k: v.cpu().numpy().view(np.uint8) for k, v in out.items()}, (cmin.cpu().numpy(), cmax.cpu().numpy())


@pytest.mark.parametrize("N,d,const_col,with_extremes", [
    (20000, 50, None, True),     # the benchmark's width (split layout), N not a multiple of the 64-reference tile
    (20000, 32, None, True),     # d = 32
    (64 * 37 + 1, 50, None, True),   # the last tile holds a single row
    (64 * 9 + 1, 32, None, True),
    (4096 + 17, 50, 3, True),    # a constant column
    (4096 + 17, 32, 0, True),
    (1024, 50, None, True),      # whole tiles and whole query blocks only
    (3000, 50, None, False),     # the scale from a pass of its own (meld_knn16_prepare)
    (3000, 8, None, True),       # plain layout (no split)
])
def test_fused_operands_equal_the_separate_passes_byte_for_byte(N, d, const_col, with_extremes):
    from meld_amd.graph import HipOps

    ops = HipOps()
    X = _cells(N, d, seed=N + d, const_col=const_col)
    sep, ext = _outputs(ops, X, False, with_extremes)
    fus, ext2 = _outputs(ops, X, True, with_extremes)
    # column minima and maxima: the same call feeds both routes (the rotation with its own statistics is not part of this change)
    assert np.array_equal(ext[0], ext2[0]) and np.array_equal(ext[1], ext2[1])
    for name in ("scale_info", "norm2_max", "norm2", "Qn", "Rt", "Q", "spheres"):
        a, b = sep[name], fus[name]
        assert a.shape == b.shape, name
        diff = np.flatnonzero(a != b)
        assert diff.size == 0, "{}: {} of {} bytes differ, first at {}: {} against {}".format(name, diff.size, a.size, diff[:4], a[diff[:4]], b[diff[:4]])


def test_step_lists_from_ready_spheres_equal_the_direct_lists(monkeypatch):
    """``meld_knn16_step_lists_direct_spheres`` on the spheres the fused pass left behind gives the lists of
    ``meld_knn16_step_lists_direct_lead`` entry by entry: the build with the plan's fused route on and off is compared end to end
    in tests/test_gpu_fused_assemble.py; here the two candidate searches of one HipOps on 40000 cells."""
    from meld_amd.graph import HipOps

    X = _cells(40000, 50, seed=5)
    res = []
    for fused in ("1", "0"):
        monkeypatch.setenv("MELD_KNN_FUSED_OPERANDS", fused)
        ops = HipOps()
        keys, vals, bw, info = ops.directed_kernel_coo(X, 0, 40000, 15, 40.0, 1e-4, 64)
        torch.cuda.synchronize()
        k, v = keys.cpu().numpy(), vals.cpu().numpy()
        order = np.lexsort((v, k))  # (rows of the exact sweep are emitted in arrival order)
        res.append((k[order], v[order], bw.cpu().numpy(), info["wave_tiles_done"]))
    for a, b in zip(res[0][:3], res[1][:3]):
        assert np.array_equal(a, b)
    assert res[0][3] == res[1][3]  # (the same (wave, tile) pairs computed: the same lists)
