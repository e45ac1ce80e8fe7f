"""tests/metric_reference.py is sound, its data sets do their job, and the wrong variants of its twin fail.  No GPU.

Soundness: the twin of ``metric_search`` returns the brute-force lists on every data set, pruned and unpruned, self and cross;
the long-double refinement agrees with meld_amd/dense.py's ``_alpha_decay_dense`` on a small dense case.

Conditions on the data (asserted here, and again in tests/test_gpu_metric_contract.py before anything is launched):
  * on each shuffled lattice set at least half of the rows have a tie exactly at rank ksel, and the twin skips at least 40 % of the
    tile pairs (measured: ties 100 / 100 / 98 %; skipped 79 / 66 / 52 % under L1 and 79 / 66 / 50 % under L-inf; lattice (2000, 5, 6)
    skips 21 % under L1 and was replaced among these sets by (2000, 4, 5));
  * no reference kernel value within 1e-6 relative of thresh, no ksel-th distance within 1e-8 relative of bw rf (1 + 1e-9),
    decay = inf: no distance within 1e-10 of the bandwidth except exact equality -- the share of undecidable decisions is 0;
  * end to end, no row's radius holds more than N / 4 cells.

Wrong variants: each must fail its ``check_*`` on a named set.  Two findings are recorded rather than hidden:
  * admission with ``<`` on the bound as the kernel computes it (scaled by 1 - 4 d eps in phase 2 and in L1's phase 1) is caught
    only where a threshold is 0 or the bound carries no margin (``lane_wants``, L-inf's phase 1): on integer data n (1 - 4 d eps) < n,
    so the margin turns ``<`` into ``<=`` for free.  On the bound without the margin it is caught on every shuffled lattice set.
  * a seed taken as the fp64 minimum of a part and rounded afterwards (what the seed kernel did until these tests) differs from the
    minimum of (fp32 bound, tile) only where two bounds agree in fp32: ``seed_tie_case`` is built for that, no other set shows it.
  * the L1 bound WITHOUT its margin is caught by no set here (``test_l1_bound_without_margin_is_not_caught``); DESIGN.md says so.
"""
import numpy as np
import pytest

from tests import metric_reference as mr

METRIC_IDS = sorted(mr.METRICS.items())


def _seeds(c):
    return (c.keys & np.uint64(0xFFFFFFFF)).astype(np.int64)


def _self_verdict(c, **kw):
    tw = mr.twin_search(c.X, c.X, c.metric, c.ksel, D=c.D, **kw)
    return mr.check_lists(tw.idx, tw.d, tw.cnt, c.idx, c.dist, c.N), tw


def _cross_verdict(c, **kw):
    tw = mr.twin_search(c.Q, c.X, c.metric, c.ksel, cross=True, seeds=kw.pop("seeds", _seeds(c)), D=c.D, **kw)
    return mr.check_lists(tw.idx, tw.d, tw.cnt, c.idx, c.dist, c.N), tw


# ---------------------------------------------------------------------------------------------------------------------------------
# soundness
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,metric", METRIC_IDS)
def test_distances_are_the_plain_sums(mname, metric):
    """``distances`` against a long-double evaluation: within d ulps, and exact on integers."""
    for name in ("blob_129_65", "shifted", "signed", "lattice_17d"):
        s = mr.data_set(name)
        X = s.X[:200]
        D = mr.distances(X, X, metric)
        t = np.abs(X[:, None, :].astype(mr.LD) - X[None, :, :].astype(mr.LD))
        E = t.sum(2) if metric == mr.L1 else t.max(2)
        assert np.all(np.abs(D - E) <= s.d * 2.0 ** -53 * E), name
        if s.integer:
            assert np.array_equal(D, E.astype(np.float64))
        assert not np.any(np.signbit(D))


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
@pytest.mark.parametrize("name", mr.SEARCH_SETS)
def test_twin_returns_the_brute_force_lists(name, mname, metric):
    c = mr.self_case(name, metric)
    need = mr.needed_pairs(c.idx, c.cnt, c.n_tiles)
    for prune in (True, False):
        v, tw = _self_verdict(c, prune=prune)
        assert v.ok, v
        assert mr.check_visits(tw.done, need, prune).ok


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
@pytest.mark.parametrize("name", mr.CROSS_SETS)
def test_cross_twin_returns_the_brute_force_lists(name, mname, metric):
    rng = np.random.default_rng(3)
    for M in mr.CROSS_M:
        c = mr.cross_case(name, metric, M)
        need = mr.needed_pairs(c.idx, c.cnt, c.n_tiles)
        for ns in (mr.SLICE_COUNTS if M == 130 else (1, 3)):
            ns = min(ns, c.n_tiles)
            for prune in (True, False):
                v, tw = _cross_verdict(c, n_slices=ns, prune=prune)
                assert v.ok, (M, ns, prune, v)
                assert mr.check_visits(tw.done, need, prune).ok
        for seeds in (np.zeros(M, np.int64), rng.integers(0, c.n_tiles, size=M)):  # any tile is a valid seed
            v, _ = _cross_verdict(c, seeds=seeds, n_slices=min(3, c.n_tiles))
            assert v.ok, (M, v)


@pytest.mark.parametrize("decay", [40.0, 2.0, mr.INF])
@pytest.mark.parametrize("mname,metric", METRIC_IDS)
def test_refinement_agrees_with_the_dense_semantics(mname, metric, decay):
    """refine_ref on complete lists (ksel = N + 1: the list holds every cell) against ``dense._alpha_decay_dense`` on the same
    distance matrix; the dense kernel keeps K_ii, the refinement zeroes it."""
    import torch

    from meld_amd.dense import _alpha_decay_dense

    X = mr.blobs(40, 3, 7)
    N, knn, thresh = 40, 5, 1e-4
    D = mr.distances(X, X, metric)
    idx, d, cnt = mr.brute_lists(D, N + 1)
    ref = mr.refine_ref(idx, d, cnt, N + 1, knn, decay, thresh)
    assert ref.complete.all()
    K, bw = _alpha_decay_dense(torch.from_numpy(D), knn, decay, thresh)
    K, bw = K.numpy().copy(), bw.numpy()
    np.fill_diagonal(K, 0.0)
    assert np.array_equal(bw, ref.bw)
    R = np.zeros((N, N))
    for q in range(N):
        R[q, idx[q, :N]] = ref.val[q, :N].astype(np.float64)
    assert np.array_equal(K != 0, R != 0)
    np.testing.assert_allclose(K, R, rtol=1e-12, atol=0)
    assert np.array_equal(ref.keep_cnt, (K != 0).sum(1))


# ---------------------------------------------------------------------------------------------------------------------------------
# conditions on the data
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,metric", METRIC_IDS)
@pytest.mark.parametrize("name", mr.LATTICE_SHUFFLED)
def test_lattice_sets_tie_and_prune(name, mname, metric):
    c = mr.self_case(name, metric)
    assert mr.tie_share(c.D, c.ksel) >= 0.5
    _, tw = _self_verdict(c)
    assert 1.0 - tw.done / tw.pairs >= 0.4, tw.done / tw.pairs


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
def test_every_decision_is_decidable(mname, metric):
    for decay, thresh in mr.REFINE_PARAMS:
        for name in mr.STAGE_SETS:
            assert mr.assert_decidable(mr.self_refine_case(name, metric, decay, thresh), decay, (name, decay, thresh)) == 0.0
        for name in mr.CROSS_SETS:
            for scale in (1.0, 0.5):
                ref = mr.cross_refine_case(name, metric, 130, decay, thresh, scale)
                assert mr.assert_decidable(ref, decay, (name, decay, thresh, scale)) == 0.0
    for name in mr.SWEEP_SETS:
        c = mr.self_case(name, metric)
        rows = mr.sweep_rows(c.N, 300)
        for decay, thresh in mr.REFINE_PARAMS:
            bw = mr.self_refine_case(name, metric, decay, thresh).bw
            assert mr.assert_decidable(mr.sweep_ref(c.D[rows], rows, bw, decay, thresh), decay, (name, decay, thresh)) == 0.0
    for name in mr.CROSS_SETS:
        c = mr.cross_case(name, metric, 130)
        rows = np.arange(130)
        for decay, thresh in mr.REFINE_PARAMS:
            for scale in (1.0, 0.5):
                bw = mr.cross_refine_case(name, metric, 130, decay, thresh, scale).bw
                ref = mr.sweep_ref(c.D, rows, bw, decay, thresh, cross=True)
                assert mr.assert_decidable(ref, decay, (name, decay, thresh, scale)) == 0.0


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
def test_stage_sets_reach_every_branch(mname, metric):
    """The refinement cases hold certified rows, flagged rows, rows whose list holds every cell and rows with the bandwidth at eps;
    far-away queries are flagged and see every fitted cell."""
    ref = mr.self_refine_case("copies", metric, 40.0, 1e-4)
    assert np.count_nonzero(ref.bw == mr.EPS) >= 70 + 130 and not ref.complete[ref.bw == mr.EPS].any()
    assert ref.complete.any() and (~ref.complete).any()
    assert mr.self_refine_case("blob_63_16", metric, 40.0, 1e-4).complete.all()  # n < ksel
    c = mr.cross_case("blob_2000_15", metric, 130)
    ref = mr.cross_refine_case("blob_2000_15", metric, 130, 40.0, 1e-4, 1.0)
    sw = mr.sweep_ref(c.D, np.arange(130), ref.bw, 40.0, 1e-4, cross=True)
    assert sum(len(s["cols"]) == c.N for s in sw) >= 30 and ref.complete.any() and (~ref.complete).any()


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
def test_end_to_end_radius_stays_small(mname, metric):
    for name, knn in mr.END_TO_END:
        c = mr.self_case(name, metric)
        assert mr.radius_population(c.D, knn, 40.0, 1e-4) <= c.N / 4


# ---------------------------------------------------------------------------------------------------------------------------------
# wrong variants of the twin: each fails its check on a named set
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,metric", METRIC_IDS)
@pytest.mark.parametrize("name", mr.LATTICE_SHUFFLED)
def test_admission_with_less_than_fails(name, mname, metric):
    v, _ = _self_verdict(mr.self_case(name, metric), admit="lt", margin=False)
    assert not v.ok and v.what == "column"


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
def test_admission_with_less_than_on_the_scaled_bound(mname, metric):
    """With the kernel's margin: caught where thresholds are 0 (lattice_1d: every list is full of copies) and in the cross
    family's per-lane test, which has no margin; NOT caught on lattice (2000, 5, 6) -- see the module docstring."""
    assert not _self_verdict(mr.self_case("lattice_1d", metric), admit="lt")[0].ok
    assert not _cross_verdict(mr.cross_case("lattice_2d", metric, 130), admit="lt")[0].ok
    assert _self_verdict(mr.self_case("lattice_5d", metric), admit="lt")[0].ok


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
@pytest.mark.parametrize("name", mr.LATTICE_SHUFFLED + ("copies",))
def test_ties_by_visiting_order_fail(name, mname, metric):
    assert not _self_verdict(mr.self_case(name, metric), tie="visit")[0].ok
    if name in mr.CROSS_SETS:
        assert not _cross_verdict(mr.cross_case(name, metric, 130), tie="visit")[0].ok


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
@pytest.mark.parametrize("name", ("lattice_4d", "copies", "shifted"))
def test_dropped_last_half_tile_fails(name, mname, metric):
    assert not _self_verdict(mr.self_case(name, metric), drop_tail=True)[0].ok


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
@pytest.mark.parametrize("name", ("lattice_2d", "lattice_4d"))
def test_merge_by_distance_only_fails(name, mname, metric):
    assert not _cross_verdict(mr.cross_case(name, metric, 130), merge="distance_last", n_slices=5)[0].ok


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
def test_wrong_refinements_fail(mname, metric):
    c = mr.self_case("lattice_4d", metric)
    for decay, kw, what in ((40.0, dict(keep_self=True), "keep_cnt"), (mr.INF, dict(first_k_self=True), "flagged rows"),
                            (40.0, dict(bw_rank=c.knn - 1), "bandwidth bits")):
        ref = mr.self_refine_case("lattice_4d", metric, decay, 1e-4)
        bad = mr.refine_ref(c.idx, c.dist, c.cnt, c.ksel, c.knn, decay, 1e-4, **kw)
        flagged = np.nonzero(~bad.complete)[0]
        v = mr.check_refine(bad.bw, bad.val.astype(np.float64), bad.keep_cnt, flagged, len(flagged), ref, mr.val_tol(decay, 1e-4))
        assert not v.ok and v.what == what, (kw, v)
        good = mr.check_refine(ref.bw, ref.val.astype(np.float64), ref.keep_cnt, np.nonzero(~ref.complete)[0], int((~ref.complete).sum()),
                               ref, mr.val_tol(decay, 1e-4))
        assert good.ok and good.margin <= 1.0
    # continuous data: the bandwidth one rank early is a different number on every row
    c = mr.self_case("blob_2000_15", metric)
    ref = mr.self_refine_case("blob_2000_15", metric, 40.0, 1e-4)
    bad = mr.refine_ref(c.idx, c.dist, c.cnt, c.ksel, c.knn, 40.0, 1e-4, bw_rank=c.knn - 1)
    assert not np.any(bad.bw == ref.bw)


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
def test_seed_by_fp64_minimum_fails(mname, metric):
    """The seed key is the minimum of (fp32 bound, tile).  Taking the fp64 minimum of a part first names another tile where two
    bounds agree in fp32 only -- ``seed_tie_case`` catches it, no other set here does (so each of them leaves both rules equal)."""
    Q, X = mr.seed_tie_case()
    lo, hi = mr.tile_boxes(X)
    ref = mr.seed_keys(Q, lo, hi, metric)
    assert int(ref[0] & np.uint64(0xFFFFFFFF)) == 0 and int(ref[1] & np.uint64(0xFFFFFFFF)) == 0
    v = mr.check_seeds(mr.seed_keys(Q, lo, hi, metric, fp64_first_per=64), ref)
    assert not v.ok and v.what == "seed key" and v.row == 0 and v.ref == 1
    for name in mr.CROSS_SETS:
        c = mr.cross_case(name, metric, 130)
        assert mr.check_seeds(mr.seed_keys(c.Q, c.box_lo, c.box_hi, metric, fp64_first_per=64), c.keys).ok


@pytest.mark.parametrize("mname,metric", METRIC_IDS)
def test_l1_bound_without_margin_is_not_caught(mname, metric):
    """Reported, not hidden: the twin without the 1 - 4 d eps margin returns the right lists on every set tried, the shifted one
    (coordinates near 1e6, spread 1e-3: the largest rounding of the box sums relative to the distances) included.  Phase 2 sums the
    box gaps in the distance's own order, where every term is at most the distance's, so only phase 1's butterfly sum needs the
    margin, and no distance here sits within d ulps of a threshold."""
    for name in ("shifted", "signed", "blob_1000_256", "lattice_4d"):
        assert _self_verdict(mr.self_case(name, metric), margin=False)[0].ok
    assert _cross_verdict(mr.cross_case("shifted", metric, 130), margin=False)[0].ok
