"""Contract tests of the L1 / L-infinity kNN stages (csrc/metric_knn.hip), every entry point called on its own through
``meld_amd._lib`` as ``build_metric_knn_graph`` and ``cross_kernel_rows`` call it, both metrics, against tests/metric_reference.py
(tied to brute force and to the dense route's semantics by tests/test_metric_reference.py).

Each stage is fed the REFERENCE's output of the stage before it -- reference boxes into the search, brute-force lists into the
refinement, reference bandwidths into the sweep -- so that one fault shows in one place.  The data are the seeded sets of the
reference module: integer lattices whose whole tiles are shuffled (ties at rank ksel on nearly every row, and more than 40 % of
the tile pairs pruned), copies of a cell, continuous blobs at every tile / chunk / list edge, shifted and signed coordinates; the
conditions that keep a comparison from excusing a failure are asserted again here before anything is launched.  No index handed
to a kernel is out of range and every buffer has the size meld_amd/metric_knn.py allocates for it.

Promises
    boxes: minima and maxima by value.  search: cand_cnt = min(N, ksel); columns exact and distances BIT FOR BIT in (distance,
    column) order; +inf / column 0 behind; prune 0 and 1 the same bits; tiles_done = all pairs without pruning, with it between
    the pairs the final lists need and all pairs, and on integer data exactly the twin's count.  refinement: bw bit for bit,
    n_flag and the set of flagged rows, keep_cnt and the zero pattern exact, values within the tolerance.  sweep: count, cursor,
    column set exact, values within the tolerance, no self entry in the self family.  seeds: keys exact.

Tolerances (derived, not tuned), u = 2^-53
    Distances and bandwidths are exact.  dist / bw carries one rounding; a kept value has (dist / bw)^decay <= -ln thresh, and
    d ln v = -decay (dist / bw)^decay d ln(dist / bw); 64 u for pow and exp as in tests/test_gpu_refine_contract.py:
        |v - v_ref| <= (decay * (-ln thresh) + 64) u * v_ref          (decay 40, thresh 1e-4: 432 u; decay 2: 82 u).
    decay = inf is compared exactly.

The seed test with several parts needs more than 64 tiles, so it alone runs at 4160 cells (boxes only, d = 3); everything else
stays at N <= 2000, M <= 130.  Every test prints its largest deviation as a fraction of its bound; the largest seen on the MI355X
and the module's wall time are recorded in DESIGN.md section 4.8.
"""
import numpy as np
import pytest

from tests import metric_reference as mr

pytestmark = pytest.mark.gpu

METRIC_IDS = sorted(mr.METRICS.items())
SENT_D, SENT_I = -7.0, -9


def _t(a, dt):
    import torch

    return torch.from_numpy(np.array(a, dtype=dt, order="C")).cuda()  # (a copy: the shared reference arrays are read-only)


def _full(n, value, dt):
    import torch

    return torch.full((max(int(n), 1),), value, dtype=dt, device="cuda")


def _env():
    import torch

    from meld_amd._lib import check, get_lib, ptr
    from meld_amd.graph import _stream

    return torch, get_lib(), check, ptr, _stream()


def report(test, what, figure):
    print("metric-contract %s: %s = %.3g" % (test, what, figure))


# ---------------------------------------------------------------------------------------------------------------------------------
# launches: buffers as meld_amd/metric_knn.py allocates them, outputs pre-filled with sentinels
# ---------------------------------------------------------------------------------------------------------------------------------
def run_boxes(X):
    torch, lib, check, ptr, st = _env()
    N, d = X.shape
    n_tiles = mr.ceil_div(N, mr.TILE)
    Xd = _t(X, np.float64)
    lo, hi = _full(n_tiles * d, SENT_D, torch.float64), _full(n_tiles * d, SENT_D, torch.float64)
    check(lib.meld_metric_tile_boxes(ptr(Xd), N, d, ptr(lo), ptr(hi), st), "meld_metric_tile_boxes")
    return lo.cpu().numpy().reshape(n_tiles, d), hi.cpu().numpy().reshape(n_tiles, d)


def run_topk(X, metric, ksel, lo, hi, prune):
    torch, lib, check, ptr, st = _env()
    N, d = X.shape
    T = int(lib.meld_metric_tile_rows())
    assert T == mr.TILE
    n_tiles = mr.ceil_div(N, T)
    Xd, lod, hid = _t(X, np.float64), _t(lo.reshape(-1), np.float64), _t(hi.reshape(-1), np.float64)
    heap_d = torch.empty(ksel * n_tiles * T, dtype=torch.float64, device="cuda")
    heap_i = torch.empty(ksel * n_tiles * T, dtype=torch.int32, device="cuda")
    idx, dd, cnt = _full(N * ksel, SENT_I, torch.int32), _full(N * ksel, SENT_D, torch.float64), _full(N, SENT_I, torch.int32)
    done = torch.zeros(1, dtype=torch.int64, device="cuda")
    check(lib.meld_metric_topk(ptr(Xd), N, d, metric, ksel, ptr(lod), ptr(hid), int(prune), ptr(heap_d), ptr(heap_i), ptr(idx), ptr(dd),
                               ptr(cnt), ptr(done), st), "meld_metric_topk")
    return idx.cpu().numpy().reshape(N, ksel), dd.cpu().numpy().reshape(N, ksel), cnt.cpu().numpy(), int(done.item())


def run_refine(idx, d, cnt, ksel, knn, decay, thresh, cross=False, bw_scale=1.0):
    torch, lib, check, ptr, st = _env()
    M = idx.shape[0]
    idxd, dd, cntd = _t(idx.reshape(-1), np.int32), _t(d.reshape(-1), np.float64), _t(cnt, np.int32)
    bw, val = _full(M, SENT_D, torch.float64), _full(M * ksel, SENT_D, torch.float64)
    keep, flag_rows = _full(M, SENT_I, torch.int32), _full(M, -1, torch.int32)
    n_flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    if cross:
        check(lib.meld_metric_cross_refine(ptr(idxd), ptr(dd), ptr(cntd), M, ksel, knn, float(decay), float(thresh), float(bw_scale), ptr(bw),
                                           ptr(val), ptr(keep), ptr(flag_rows), ptr(n_flag), st), "meld_metric_cross_refine")
    else:
        check(lib.meld_metric_refine(ptr(idxd), ptr(dd), ptr(cntd), M, ksel, knn, float(decay), float(thresh), ptr(bw), ptr(val), ptr(keep),
                                     ptr(flag_rows), ptr(n_flag), st), "meld_metric_refine")
    return bw.cpu().numpy(), val.cpu().numpy().reshape(M, ksel), keep.cpu().numpy(), flag_rows.cpu().numpy(), int(n_flag.item())


def run_radius(X, metric, rows, bw, decay, thresh, Q=None):
    """Count pass, host scan, fill pass, as ``_radius_sweep`` / ``_cross_radius_sweep`` do; Q: the cross family's queries."""
    torch, lib, check, ptr, st = _env()
    N, d = X.shape
    nf = len(rows)
    Xd, rowsd, bwd = _t(X, np.float64), _t(rows, np.int32), _t(bw, np.float64)
    Qd = None if Q is None else _t(Q, np.float64)

    def call(mode, cntd, offd, curd, cold, vald):
        if Q is None:
            check(lib.meld_metric_radius(ptr(Xd), N, d, metric, ptr(rowsd), nf, ptr(bwd), float(decay), float(thresh), mode, ptr(cntd), ptr(offd),
                                         ptr(curd), ptr(cold), ptr(vald), st), "meld_metric_radius")
        else:
            check(lib.meld_metric_cross_radius(ptr(Qd), Q.shape[0], ptr(Xd), N, d, metric, ptr(rowsd), nf, ptr(bwd), float(decay), float(thresh),
                                               mode, ptr(cntd), ptr(offd), ptr(curd), ptr(cold), ptr(vald), st), "meld_metric_cross_radius")

    cntd = torch.zeros(nf, dtype=torch.int32, device="cuda")
    call(0, cntd, None, None, None, None)
    count = cntd.cpu().numpy()
    assert np.all(count >= 0) and np.all(count <= N)
    off = np.concatenate([[0], np.cumsum(count.astype(np.int64))])
    total = int(off[-1])
    cold, vald = _full(total, SENT_I, torch.int32), _full(total, SENT_D, torch.float64)
    curd = torch.zeros(nf, dtype=torch.int32, device="cuda")
    call(1, None, _t(off, np.int64), curd, cold, vald)
    return count, curd.cpu().numpy(), off, cold.cpu().numpy(), vald.cpu().numpy()


def run_cross_seed(Q, lo, hi, N, metric):
    torch, lib, check, ptr, st = _env()
    M, d = Q.shape
    Qt = _t(Q.T, np.float64)
    lod, hid = _t(lo.reshape(-1), np.float64), _t(hi.reshape(-1), np.float64)
    key = torch.full((M,), -1, dtype=torch.int64, device="cuda")
    check(lib.meld_metric_cross_seed(ptr(Qt), M, ptr(lod), ptr(hid), N, d, metric, ptr(key), st), "meld_metric_cross_seed")
    return key.cpu().numpy().view(np.uint64)


def run_cross_topk(Q, X, metric, ksel, lo, hi, seeds, prune, n_slices):
    torch, lib, check, ptr, st = _env()
    (M, d), N = Q.shape, X.shape[0]
    T = mr.TILE
    ns = int(lib.meld_metric_cross_slices(M, N, int(n_slices)))
    assert ns == min(n_slices, mr.ceil_div(N, T))
    assert seeds.shape == (M,) and seeds.min() >= 0 and seeds.max() < mr.ceil_div(N, T)
    Qt, Xd = _t(Q.T, np.float64), _t(X, np.float64)
    lod, hid, seedd = _t(lo.reshape(-1), np.float64), _t(hi.reshape(-1), np.float64), _t(seeds, np.int32)
    q_slots = mr.ceil_div(M, T) * T
    heap_d = torch.empty(ns * ksel * q_slots, dtype=torch.float64, device="cuda")
    heap_i = torch.empty(ns * ksel * q_slots, dtype=torch.int32, device="cuda")
    p_idx = p_d = p_cnt = None
    if ns > 1:
        p_idx, p_d = _full(ns * M * ksel, SENT_I, torch.int32), _full(ns * M * ksel, SENT_D, torch.float64)
        p_cnt = torch.zeros(ns * M, dtype=torch.int32, device="cuda")
    idx, dd, cnt = _full(M * ksel, SENT_I, torch.int32), _full(M * ksel, SENT_D, torch.float64), _full(M, SENT_I, torch.int32)
    done = torch.zeros(1, dtype=torch.int64, device="cuda")
    check(lib.meld_metric_cross_topk(ptr(Qt), M, ptr(Xd), N, d, metric, ksel, ptr(lod), ptr(hid), ptr(seedd), int(prune), ns, ptr(heap_d),
                                     ptr(heap_i), ptr(p_idx), ptr(p_d), ptr(p_cnt), ptr(idx), ptr(dd), ptr(cnt), ptr(done), st),
          "meld_metric_cross_topk")
    return idx.cpu().numpy().reshape(M, ksel), dd.cpu().numpy().reshape(M, ksel), cnt.cpu().numpy(), int(done.item())


# ---------------------------------------------------------------------------------------------------------------------------------
# the self family
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mr.SEARCH_SETS)
def test_tile_boxes(name):
    s = mr.data_set(name)
    lo, hi = run_boxes(s.X)
    v = mr.check_boxes(lo, hi, s.X)
    assert v.ok, v
    report("tile_boxes[%s]" % name, "deviation (exact comparison)", v.margin)


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
@pytest.mark.parametrize("name", mr.SEARCH_SETS)
def test_topk(name, mname, metric):
    c = mr.self_case(name, metric)
    if name in mr.LATTICE_SHUFFLED:  # the conditions, before anything is launched
        assert mr.tie_share(c.D, c.ksel) >= 0.5
    lo, hi = mr.tile_boxes(c.X)
    need = mr.needed_pairs(c.idx, c.cnt, c.n_tiles)
    twin = mr.twin_search(c.X, c.X, metric, c.ksel, D=c.D) if c.integer else None
    if name in mr.LATTICE_SHUFFLED:
        assert 1.0 - twin.done / twin.pairs >= 0.4
    out = {}
    for prune in (0, 1):
        idx, d, cnt, done = out[prune] = run_topk(c.X, metric, c.ksel, lo, hi, prune)
        v = mr.check_lists(idx, d, cnt, c.idx, c.dist, c.N)
        assert v.ok, (prune, v)
        w = mr.check_visits(done, need, prune, exact=twin.done if twin is not None else None)
        assert w.ok, (prune, w)
        report("topk[%s-%s] prune=%d" % (name, mname, prune), "share of the tile pairs visited", w.margin)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1].view(np.int64), out[1][1].view(np.int64))
    assert np.array_equal(out[0][2], out[1][2])


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
@pytest.mark.parametrize("name", mr.STAGE_SETS)
def test_refine(name, mname, metric):
    c = mr.self_case(name, metric)
    worst = 0.0
    for decay, thresh in mr.REFINE_PARAMS:
        ref = mr.self_refine_case(name, metric, decay, thresh)
        assert mr.assert_decidable(ref, decay, (name, decay, thresh)) == 0.0
        bw, val, keep, flag_rows, n_flag = run_refine(c.idx, c.dist, c.cnt, c.ksel, c.knn, decay, thresh)
        assert 0 <= n_flag <= c.N
        v = mr.check_refine(bw, val, keep, flag_rows, n_flag, ref, mr.val_tol(decay, thresh))
        assert v.ok, (decay, thresh, v)
        worst = max(worst, v.margin)
    report("refine[%s-%s]" % (name, mname), "largest value deviation / bound", worst)


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
@pytest.mark.parametrize("name", mr.SWEEP_SETS)
def test_radius(name, mname, metric):
    c = mr.self_case(name, metric)
    assert c.N == 2000  # two reference chunks
    worst = 0.0
    for decay, thresh in mr.REFINE_PARAMS:
        bw = mr.self_refine_case(name, metric, decay, thresh).bw
        for length in mr.SWEEP_LENGTHS:
            rows = mr.sweep_rows(c.N, length)
            ref = mr.sweep_ref(c.D[rows], rows, bw, decay, thresh)
            assert mr.assert_decidable(ref, decay, (name, decay, thresh, length)) == 0.0
            count, cursor, off, col, val = run_radius(c.X, metric, rows, bw, decay, thresh)
            v = mr.check_sweep(count, cursor, off, col, val, rows, ref, mr.val_tol(decay, thresh))
            assert v.ok, (decay, thresh, length, v)
            worst = max(worst, v.margin)
    report("radius[%s-%s]" % (name, mname), "largest value deviation / bound", worst)


# ---------------------------------------------------------------------------------------------------------------------------------
# the cross family
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,metric", METRIC_IDS)
@pytest.mark.parametrize("name", mr.CROSS_SETS)
def test_cross_seed_one_part(name, mname, metric):
    for M in mr.CROSS_M:
        c = mr.cross_case(name, metric, M)
        v = mr.check_seeds(run_cross_seed(c.Q, c.box_lo, c.box_hi, c.N, metric), c.keys)
        assert v.ok, (M, v)
    report("cross_seed[%s-%s]" % (name, mname), "deviation (exact comparison)", 0.0)


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
def test_cross_seed_several_parts(mname, metric):
    """65 tiles: the seed kernel splits them into two parts of 33 and 32 and the parts meet in an atomic minimum.  Boxes of a
    lattice (ties between tiles in both parts) and of blobs."""
    for X in (mr.lattice(4160, 3, 9, 41), mr.blobs(4160, 3, 42)):
        lo, hi = mr.tile_boxes(X)
        assert lo.shape[0] == 65
        rng = np.random.default_rng(43)
        span = X.max(0) - X.min(0)
        Q = np.concatenate([X[rng.integers(0, 4160, size=65)], np.round(X.min(0) + span * rng.uniform(-0.5, 1.5, size=(65, 3)))])
        Q = np.ascontiguousarray(Q[rng.permutation(130)])
        ref = mr.seed_keys(Q, lo, hi, metric)
        tiles = (ref & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert (tiles < 33).any() and (tiles >= 33).any()  # winners in both parts
        v = mr.check_seeds(run_cross_seed(Q, lo, hi, 4160, metric), ref)
        assert v.ok, v
    report("cross_seed_parts[%s]" % mname, "deviation (exact comparison)", 0.0)


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
def test_cross_seed_bounds_that_agree_in_fp32(mname, metric):
    """Regression: the key is the minimum of (fp32 bound, tile) over ALL tiles.  The kernel used to take the fp64 minimum of its
    part and round only that one, so a query at 0 between boxes at 2 + 2^-40 (tile 0) and at 2 (tile 1) was keyed to tile 1, and
    which tile won depended on how the tiles were split over the grid."""
    Q, X = mr.seed_tie_case()
    lo, hi = mr.tile_boxes(X)
    ref = mr.seed_keys(Q, lo, hi, metric)
    assert not mr.check_seeds(mr.seed_keys(Q, lo, hi, metric, fp64_first_per=64), ref).ok  # the case tells the two rules apart
    v = mr.check_seeds(run_cross_seed(Q, lo, hi, X.shape[0], metric), ref)
    assert v.ok, v
    report("cross_seed_fp32_ties[%s]" % mname, "deviation (exact comparison)", 0.0)


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
@pytest.mark.parametrize("name", mr.CROSS_SETS)
def test_cross_topk(name, mname, metric):
    rng = np.random.default_rng(5)
    for M in mr.CROSS_M:
        c = mr.cross_case(name, metric, M)
        need = mr.needed_pairs(c.idx, c.cnt, c.n_tiles)
        keys = run_cross_seed(c.Q, c.box_lo, c.box_hi, c.N, metric)
        seeds = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)  # the device's seeds, the queries in random order
        assert seeds.min() >= 0 and seeds.max() < c.n_tiles
        for ns in (mr.SLICE_COUNTS if M == 130 else (1, 3)):
            ns = min(ns, c.n_tiles)
            out = {}
            for prune in (0, 1):
                idx, d, cnt, done = out[prune] = run_cross_topk(c.Q, c.X, metric, c.ksel, c.box_lo, c.box_hi, seeds, prune, ns)
                v = mr.check_lists(idx, d, cnt, c.idx, c.dist, c.N)
                assert v.ok, (M, ns, prune, v)
                exact = None
                if prune and c.integer and M == 130:
                    exact = mr.twin_search(c.Q, c.X, metric, c.ksel, cross=True, seeds=seeds, n_slices=ns, D=c.D).done
                w = mr.check_visits(done, need, prune, exact=exact)
                assert w.ok, (M, ns, prune, w)
            assert np.array_equal(out[0][1].view(np.int64), out[1][1].view(np.int64))
            if M == 130:
                report("cross_topk[%s-%s] slices=%d" % (name, mname, ns), "share of the tile pairs visited", w.margin)
        # any tile is a valid seed
        for other in (np.zeros(M, np.int64), rng.integers(0, c.n_tiles, size=M)):
            idx, d, cnt, done = run_cross_topk(c.Q, c.X, metric, c.ksel, c.box_lo, c.box_hi, other, 1, min(3, c.n_tiles))
            v = mr.check_lists(idx, d, cnt, c.idx, c.dist, c.N)
            assert v.ok, (M, "seeds", v)
            assert mr.check_visits(done, need, 1).ok


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
@pytest.mark.parametrize("name", mr.CROSS_SETS)
def test_cross_refine(name, mname, metric):
    worst = 0.0
    for M in mr.CROSS_M:
        c = mr.cross_case(name, metric, M)
        for decay, thresh in mr.REFINE_PARAMS:
            for scale in (1.0, 0.5):
                ref = mr.cross_refine_case(name, metric, M, decay, thresh, scale)
                if M == 130:
                    assert mr.assert_decidable(ref, decay, (name, decay, thresh, scale)) == 0.0
                bw, val, keep, flag_rows, n_flag = run_refine(c.idx, c.dist, c.cnt, c.ksel, c.knn, decay, thresh, cross=True, bw_scale=scale)
                v = mr.check_refine(bw, val, keep, flag_rows, n_flag, ref, mr.val_tol(decay, thresh))
                assert v.ok, (M, decay, thresh, scale, v)
                worst = max(worst, v.margin)
                if np.isinf(decay):  # exactly the first knn + 1 entries at 1, never a flag
                    n = min(c.N, c.ksel, c.knn + 1)
                    assert n_flag == 0 and np.all(val[:, :n] == 1.0) and np.all(val[:, n:] == 0.0) and np.all(keep == n)
    report("cross_refine[%s-%s]" % (name, mname), "largest value deviation / bound", worst)


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
@pytest.mark.parametrize("name", mr.CROSS_SETS)
def test_cross_radius(name, mname, metric):
    c = mr.cross_case(name, metric, 130)
    worst = 0.0
    for decay, thresh in mr.REFINE_PARAMS:
        for scale in (1.0, 0.5):
            bw = mr.cross_refine_case(name, metric, 130, decay, thresh, scale).bw
            for length in (1, 8, 9, 130):
                rows = mr.sweep_rows(130, length)
                ref = mr.sweep_ref(c.D[rows], rows, bw, decay, thresh, cross=True)
                assert mr.assert_decidable(ref, decay, (name, decay, thresh, scale, length)) == 0.0
                count, cursor, off, col, val = run_radius(c.X, metric, rows, bw, decay, thresh, Q=c.Q)
                v = mr.check_sweep(count, cursor, off, col, val, rows, ref, mr.val_tol(decay, thresh), cross=True)
                assert v.ok, (decay, thresh, scale, length, v)
                worst = max(worst, v.margin)
    report("cross_radius[%s-%s]" % (name, mname), "largest value deviation / bound", worst)


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end, small
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,metric", METRIC_IDS)
@pytest.mark.parametrize("name,knn", mr.END_TO_END)
def test_builder_equals_the_dense_route(name, knn, mname, metric):
    import torch
    from scipy import sparse

    from meld_amd.dense import build_dense_knn_graph
    from meld_amd.metric_knn import build_metric_knn_graph

    c = mr.self_case(name, metric)
    assert mr.radius_population(c.D, knn, 40.0, 1e-4) <= c.N / 4  # the builder's degenerate-graph refusal does not fire
    Xd = torch.from_numpy(np.array(c.X)).cuda()
    A = build_metric_knn_graph(Xd, knn, 40, 1e-4, 1, mname, reorder=False)
    B = build_dense_knn_graph(Xd, knn, 40, 1e-4, anisotropy=1, metric=mname)
    WA, WB = sparse.csr_matrix(A.W), sparse.csr_matrix(B.W)
    WA.sort_indices()
    WB.sort_indices()
    assert WA.shape == WB.shape and WA.nnz == WB.nnz
    assert np.array_equal(WA.indptr, WB.indptr) and np.array_equal(WA.indices, WB.indices)
    np.testing.assert_allclose(WA.data, WB.data, rtol=1e-12, atol=0)
    # (the dense route records the raw (knn+1)-th distance, 0 on the copies; the kernels clip it to eps -- the same kernel values)
    np.testing.assert_allclose(A.bandwidth_host, np.maximum(B.bandwidth_host, mr.EPS), rtol=1e-12, atol=0)
    report("builder[%s-%s]" % (name, mname), "largest weight deviation / 1e-12", float(np.max(np.abs(WA.data - WB.data) / WB.data)) / 1e-12)
