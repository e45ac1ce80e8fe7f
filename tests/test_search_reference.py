"""tests/search_reference.py on the host: tied to the oracle's brute-force kernel and to scipy's distances, the conditions its cases
must satisfy for the GPU contracts (tests/test_gpu_search_contract.py) not to be vacuous, and every contract function fed outputs
that are right (accepted) and outputs with one defect (rejected, with the right row and reference)."""
import numpy as np
import pytest

from tests import search_reference as sr

LD = np.longdouble


def _coefs(nprod, d):
    from meld_amd._lib import get_lib

    lib = get_lib()  # (host functions of the library: no device is touched)
    return lib.meld_knn16_error_coef_const(nprod, d), lib.meld_knn16_error_coef_lin(nprod), lib.meld_knn16_error_coef(3, d)


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference against the project's ground truth
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,knn,q_begin,q_count", [(300, 5, 5, 0, None), (411, 23, 9, 128, 200)])
def test_reference_agrees_with_the_oracle_and_with_cdist(N, d, knn, q_begin, q_count):
    from scipy.spatial.distance import cdist

    from oracle import meld_oracle as mo

    X = sr.make_data("noise", N, d, 5)
    ref = sr.Setup(X, X.mean(axis=0), q_begin, q_count)
    qs = slice(q_begin, q_begin + ref.q_count)
    np.testing.assert_allclose(ref.D, cdist(X[qs], X, "sqeuclidean"), rtol=1e-12, atol=1e-12 * ref.n_max)
    Xc = X - X.mean(axis=0)
    assert ref.s == 1.0 / np.abs(Xc).max() and ref.n_max == (Xc * Xc).sum(axis=1).max()
    K, mid = mo.knn_kernel(X, knn=knn, decay=40, thresh=1e-4, algorithm="brute", return_intermediates=True)
    K = np.asarray(K.todense()) if hasattr(K, "todense") else np.asarray(K)
    np.testing.assert_allclose(np.sqrt(ref.bandwidth2(knn)), mid["bandwidth"][qs], rtol=1e-10)
    np.testing.assert_allclose(np.sqrt(ref.radius2(knn, sr.RF).astype(np.float64)), np.asarray(mid["radius"])[qs], rtol=1e-10)
    # the oracle's neighbours of a row are the references inside the reference's kernel radius, and the reference's rows hold them
    idx, d2 = ref.true_rows(64)
    r2 = ref.radius2(knn, sr.RF).astype(np.float64)
    for i in range(ref.q_count):
        want = set(np.nonzero(K[q_begin + i])[0].tolist()) | {q_begin + i}
        got = set(np.nonzero(ref.D[i] <= r2[i])[0].tolist())
        assert got == want, i
        assert got <= set(idx[i].tolist())
        assert np.all(np.diff(d2[i]) >= 0) and idx[i, 0] == q_begin + i
    # reachability: the block minimum of the exact distances, the diagonal pairs at zero
    pm = ref.pair_min()
    assert pm.shape == (ref.n_waves, ref.n_tiles)
    w, t = ref.n_waves - 1, ref.n_tiles - 1
    assert pm[w, t] == ref.D[w * 64:, t * 64:].min() and pm[0, q_begin // 64] == 0.0


def test_scan_order_is_a_permutation_that_starts_with_the_own_tiles():
    for n in (1, 2, 4, 5, 17, 64):
        for t0 in (0, n - 1, n // 2):
            o = sr.scan_order(t0, n)
            assert sorted(o) == list(range(n)) and o[:min(4, n)] == [(t0 + k) % n for k in range(min(4, n))]
    assert sr.scan_order(10, 17)[4:8] == [14, 9, 15, 8]


# ---------------------------------------------------------------------------------------------------------------------------------
# conditions of the cases
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sr.CASES))
def test_case_conditions(name):
    c, X, mean, ref = sr.case_setup(name)
    cc, cl, _ = _coefs(1, c["d"])
    E1 = ref.allowance(cc, cl)
    E3 = ref.allowance(*_coefs(3, c["d"])[:2])
    assert ref.N >= c["ksel"] and c["knn"] < c["ksel"]
    seeds = sr.loose_seeds(ref, c["knn"], sr.RF, E1)
    free, und = sr.share_not_needed(ref, seeds, E1)
    cut1 = sr.share_cut_engages(ref, c["knn"], sr.RF, c["ksel"], E1)
    cut3 = sr.share_cut_engages(ref, c["knn"], sr.RF, c["ksel"], E3)
    beyond = sr.share_allowance_beyond_neighbour(ref, E1)
    print("CONDITIONS {}: pairs not needed {:.1%} (undecidable {:.2%}), cut engages {:.1%} (hi only) {:.1%} (full split), "
          "E > nearest d2 on {:.1%} of rows".format(name, free, und, cut1, cut3, beyond))
    assert und <= 0.01
    if c["kind"] == "clusters":
        assert free >= 0.30
    if name == "clusters":  # the cut case (128 cells of a cluster in 50 dimensions lie within a few per cent of one distance)
        assert cut3 >= 0.90
    # (hi-only products charge 2^-9 |x_i| max|x|: between clusters 40 spreads apart that exceeds the distances inside one, and the
    # hi-only cut engages on few rows -- printed, not asserted; the cut case of the GPU tests is the full split on the clusters)
    if c["kind"] == "outliers":
        assert beyond >= 0.10
    if c["kind"] == "duplicates":
        assert int((ref.Ds[:, c["knn"] + 1] == 0).sum()) >= 24  # more than knn + 1 copies: bandwidth 0
    if c["kind"] not in ("duplicates", "grid"):
        # no reference on a decision boundary of the plain search: (exact ksel-th) - 2E, and of the seeded one: seed + E
        for E in (E1, E3):
            b = ref.Ds[:, c["ksel"] - 1].astype(LD) - 2 * E
            assert not np.any(np.abs(ref.D.astype(LD) - b[:, None]) <= LD(sr.BAND) * np.abs(b)[:, None])
        b = (seeds.astype(LD) / (LD(ref.s) ** 2) + E1)
        assert not np.any(np.abs(ref.D.astype(LD) - b[:, None]) <= LD(sr.BAND) * np.abs(b)[:, None])


# ---------------------------------------------------------------------------------------------------------------------------------
# the contract functions: right outputs pass, every defect is found where it is
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def good():
    """Outputs made from the reference itself for the clusters case: rows, cut rows with thresholds, a table, lists."""
    c, X, mean, ref = sr.case_setup("clusters")
    cc, cl, e3 = _coefs(3, c["d"])
    E = ref.allowance(cc, cl)
    ksel, knn = c["ksel"], c["knn"]
    idx, d2 = ref.true_rows(ksel)
    idx, d2 = idx.astype(np.int32), d2.astype(np.float32)
    o = np.lexsort((idx, d2), axis=1)  # (distances that differ in fp64 and tie in fp32: by index, as the kernels' rows are)
    idx, d2 = np.take_along_axis(idx, o, axis=1), np.take_along_axis(d2, o, axis=1)
    g = dict(c=c, ref=ref, E=E, e3=e3, ksel=ksel, knn=knn, cnt=np.full(ref.q_count, ksel, np.int32), idx=idx, d2=d2)
    # rows cut at a threshold: everything strictly below the exact distance of rank m
    # (the exact distance of rank knn + 9, or 1 % beyond the kernel radius where that is further; a row that would be full: no cut)
    thr = np.maximum(ref.Ds[:, knn + 9], 1.01 * ref.radius2(knn, sr.RF).astype(np.float64))
    n_in = (ref.Ds < thr[:, None]).sum(axis=1)
    g["cut_thr"] = np.where(n_in < ksel, thr, np.inf)
    g["cut_cnt"] = np.minimum(n_in, ksel).astype(np.int32)
    g["cut_idx"], g["cut_d2"] = idx.copy(), d2.copy()
    # table and lists from the exact reachability
    seeds = sr.loose_seeds(ref, knn, sr.RF, E)
    need, und = ref.needed(seeds, E)
    g["need"], g["und"], g["seeds"] = need, und, seeds
    s2 = ref.s * ref.s
    g["lb2"] = np.where(need, (ref.pair_min() * s2 * (1 - 2.0 ** -10)).astype(np.float32), np.float32(np.inf))
    lst = np.zeros((ref.n_blocks, ref.n_tiles), np.uint32)
    cnt = np.zeros(ref.n_blocks, np.int32)
    for b in range(ref.n_blocks):
        k = 0
        for i, t in enumerate(sr.scan_order(sr.block_origin(ref.q_begin, b, ref.n_tiles), ref.n_tiles)):
            mask = sum(1 << w for w in range(4) if 4 * b + w < ref.n_waves and need[4 * b + w, t])
            if mask or i == 0:
                lst[b, k] = t | (mask << 24)
                k += 1
        cnt[b] = k
    g["list"], g["list_cnt"] = lst, cnt
    return g


def _rows(g, **kw):
    a = dict(idx=g["idx"], d2=g["d2"], cnt=g["cnt"], thr=None, exact_rule=True, radius2=None)
    a.update(kw)
    return sr.check_rows(g["ref"], a["idx"], a["d2"], a["cnt"], g["ksel"], g["E"], thr=a["thr"], exact_rule=a["exact_rule"], radius2=a["radius2"])


def test_right_outputs_pass(good):
    g, ref = good, good["ref"]
    v = _rows(g)
    assert v.ok and v.margin < 1e-3 and v.skipped <= 0.01, v
    v = _rows(g, idx=g["cut_idx"], d2=g["cut_d2"], cnt=g["cut_cnt"], thr=g["cut_thr"], exact_rule=False, radius2=ref.radius2(g["knn"], sr.RF))
    assert v.ok, v
    assert sr.check_bounds(ref, g["lb2"], g["need"], g["und"]).ok
    v = sr.check_lists(ref, g["list"], g["list_cnt"], ref.n_tiles, g["need"], g["und"], work=g["list_cnt"])
    assert v.ok and v.margin >= 0.30, v  # (the lists leave out what is not needed: most of the table on this case)
    assert sr.check_seeds(ref, g["seeds"], g["knn"], sr.RF).ok
    assert sr.check_seeds(ref, np.full(ref.q_count, np.inf), 64, sr.RF).ok


def _gap_row(g, lo, hi):
    """A row whose exact distances of ranks lo and hi are more than 4 E apart."""
    ref = g["ref"]
    ok = np.nonzero((ref.Ds[:, hi] - ref.Ds[:, lo]).astype(LD) > 4 * g["E"])[0]
    assert len(ok)
    return int(ok[len(ok) // 2])


def test_a_removed_candidate_is_found(good):
    g, ref, ksel = good, good["ref"], good["ksel"]
    r = _gap_row(g, 2, ksel)
    idx, d2 = g["idx"].copy(), g["d2"].copy()
    gone = int(idx[r, 2])
    idx[r, 2:ksel - 1], d2[r, 2:ksel - 1] = g["idx"][r, 3:], g["d2"][r, 3:]
    idx[r, ksel - 1], d2[r, ksel - 1] = ref.order[r, ksel], np.float32(ref.Ds[r, ksel])
    v = _rows(g, idx=idx, d2=d2)
    assert not v.ok and (v.row, v.ref) == (r, gone) and "missing" in v.what, v


def test_a_raised_threshold_is_found(good):
    g, ref = good, good["ref"]
    m = good["knn"] + 9
    r = int(np.nonzero((g["cut_thr"] == ref.Ds[:, m]) & (g["cut_cnt"] == m))[0][100])
    thr = g["cut_thr"].copy()
    thr[r] = float(LD(thr[r]) + 2 * g["E"][r])
    v = _rows(g, idx=g["cut_idx"], d2=g["cut_d2"], cnt=g["cut_cnt"], thr=thr, exact_rule=False)
    assert not v.ok and (v.row, v.ref) == (r, int(ref.order[r, m])) and "tau" in v.what, v


def test_a_moved_distance_is_found(good):
    g, ksel = good, good["ksel"]
    r = 77
    d2 = g["d2"].copy()
    d2[r, ksel - 1] = np.float32(float(LD(d2[r, ksel - 1]) + LD(1.5) * g["E"][r]))
    v = _rows(g, d2=d2)
    assert not v.ok and (v.row, v.ref) == (r, int(g["idx"][r, ksel - 1])) and "allowance" in v.what and 1.4 < v.margin < 1.6, v


def test_a_duplicate_and_a_swapped_pair_are_found(good):
    g = good
    idx = g["idx"].copy()
    idx[300, 5] = idx[300, 4]
    v = _rows(g, idx=idx)
    assert not v.ok and (v.row, v.ref) == (300, int(idx[300, 4])) and "duplicate" in v.what, v
    idx, d2 = g["idx"].copy(), g["d2"].copy()
    assert d2[301, 3] < d2[301, 4]
    idx[301, [3, 4]], d2[301, [3, 4]] = idx[301, [4, 3]], d2[301, [4, 3]]
    v = _rows(g, idx=idx, d2=d2)
    assert not v.ok and (v.row, v.ref) == (301, int(g["idx"][301, 3])) and "sorted" in v.what, v
    for cnt_bad in (0, g["ksel"] + 1):
        cnt = g["cnt"].copy()
        cnt[9] = cnt_bad
        v = _rows(g, cnt=cnt)
        assert not v.ok and v.row == 9 and "count" in v.what


def test_a_cleared_list_bit_and_a_raised_bound_are_found(good):
    g, ref = good, good["ref"]
    # a needed pair off the diagonal, of the second wave of block 5
    gw = 5 * 4 + 1
    t = int(np.nonzero(g["need"][gw] & ~g["und"][gw] & (np.arange(ref.n_tiles) != gw))[0][0])
    lst = g["list"].copy()
    k = int(np.nonzero((lst[5, :g["list_cnt"][5]] & 0xFFFFFF) == t)[0][0])
    lst[5, k] &= ~np.uint32(1 << 25)
    v = sr.check_lists(ref, lst, g["list_cnt"], ref.n_tiles, g["need"], g["und"])
    assert not v.ok and (v.row, v.ref) == (gw, t) and "missing" in v.what, v
    lst = g["list"].copy()
    lst[5, [1, 2]] = lst[5, [2, 1]]
    v = sr.check_lists(ref, lst, g["list_cnt"], ref.n_tiles, g["need"], g["und"])
    assert not v.ok and v.row == 5 and "scan order" in v.what
    work = g["list_cnt"].copy()
    work[3] += 1
    assert not sr.check_lists(ref, g["list"], g["list_cnt"], ref.n_tiles, g["need"], g["und"], work=work).ok
    # the table: a finite entry one part in a thousand above the true minimum; +inf on a needed pair
    lb = g["lb2"].copy()
    lb[gw, t] = np.float32(ref.pair_min()[gw, t] * ref.s * ref.s * 1.001)
    v = sr.check_bounds(ref, lb, g["need"], g["und"])
    assert not v.ok and (v.row, v.ref) == (gw, t) and "above" in v.what and 1.0 < v.margin < 1.01, v
    lb = g["lb2"].copy()
    lb[gw, t] = np.inf
    v = sr.check_bounds(ref, lb, g["need"], g["und"])
    assert not v.ok and (v.row, v.ref) == (gw, t) and "+inf" in v.what, v


def test_a_low_seed_and_wrong_research_thresholds_are_found(good):
    g, ref, ksel = good, good["ref"], good["ksel"]
    seeds = g["seeds"].copy()
    seeds[40] = float(ref.s ** 2 * ref.radius2(g["knn"], sr.RF)[40]) * (1 - 1e-6)
    v = sr.check_seeds(ref, seeds, g["knn"], sr.RF)
    assert not v.ok and v.row == 40, v
    rows = np.array([5, 6, 7, 900])
    cnt = g["cnt"].copy()
    cnt[6] = ksel - 1
    want = sr.research_threshold_ref(ref, rows, g["d2"], cnt, ksel, g["E"], g["e3"])
    assert np.isinf(want[1]) and np.all(np.isfinite(want[[0, 2, 3]]))
    up = 20 * 2.0 ** -24
    assert sr.check_research(ref, rows, want * (1 + 1e-6), g["d2"], cnt, ksel, g["E"], g["e3"], up).ok
    for k, f in ((0, 1 - 1e-6), (3, 1 + 1e-5)):
        thr = want.copy()
        thr[k] *= f
        v = sr.check_research(ref, rows, thr, g["d2"], cnt, ksel, g["E"], g["e3"], up)
        assert not v.ok and v.row == rows[k], v
    thr = want.copy()
    thr[1] = thr[0]
    assert not sr.check_research(ref, rows, thr, g["d2"], cnt, ksel, g["E"], g["e3"], up).ok


def test_operands_check_accepts_fp32_roundings_and_no_more(good):
    ref = good["ref"]
    f = np.float32
    s = f(1.0) / f(ref.absmax)
    si = np.array([s, f(1.0) / (s * s), f(ref.absmax), 0], np.float32)
    norm2 = ref.n.astype(np.float32)
    Qn = (norm2.astype(np.float64) * float(s) ** 2).astype(np.float32)
    assert sr.check_operands(ref, norm2, f(ref.n_max), si, Qn).ok
    bad = norm2.copy()
    bad[17] *= f(1 + 1e-4)
    v = sr.check_operands(ref, bad, f(ref.n_max), si, Qn)
    assert not v.ok and v.row == 17 and v.what == "norm2"
    bad = Qn.copy()
    bad[18] *= f(1 + 1e-5)
    v = sr.check_operands(ref, norm2, f(ref.n_max), si, bad)
    assert not v.ok and v.row == 18 and v.what == "Qn"
