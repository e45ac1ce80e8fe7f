"""Host tier of the rank-sum test (no GPU): the restatement tests/ranksum_reference.py and the host arithmetic of
meld_amd/diffexp.py (``pvalues``, ``bh_qvalues``, ``encode_classes``) against scipy's ``mannwhitneyu(method="asymptotic",
use_continuity=True, alternative="two-sided")`` and ``false_discovery_control(method="bh")``.

Tolerances.  ``statistic`` is a half-integer far below 2^53: EQUAL.  p and q to rtol 1e-10: |dp / p| ~ z |dz| on the normal tail,
z <~ 38 before p leaves the fp64 range and dz is a few ulp of z, so 1e-12 holds with margin.  Where scipy's p is below 1e-290 (the
tail's last decades, denormals next) only p < 1e-289 is required; the inputs carry random labels so that at most 5 % of a case's
genes fall there, asserted on the restatement's own p-values."""
import ctypes
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
from scipy import stats

from tests import ranksum_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-10
TINY, TINY_OK, TINY_SHARE = 1e-290, 1e-289, 0.05

CASES = {
    "halves": dict(N=700, G=40, density=0.15, seed=1, kind="halves"),
    "real": dict(N=300, G=25, density=0.4, seed=2, kind="real"),
    "counts_f32": dict(N=500, G=30, density=0.1, seed=3, kind="counts", dtype=np.float32),
}
_MADE = {}


def case(name):
    """(X CSC, codes in {-1, 0, 1, 2}, dense fp64 copy, the restatement's integers for k = 3), made once."""
    if name not in _MADE:
        X, code = ref.make_case(**CASES[name])
        _MADE[name] = (X, code, np.asarray(X.toarray(), dtype=np.float64), ref.rank_sums(X, code, 3))
    return _MADE[name]


def scipy_test(D, sel1, sel2):
    stat, p = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for g in range(D.shape[1]):
            r = stats.mannwhitneyu(D[sel1, g], D[sel2, g], use_continuity=True, alternative="two-sided", method="asymptotic")
            stat.append(r.statistic)
            p.append(r.pvalue)
    return np.array(stat), np.array(p)


def assert_p_close(ours, theirs, own_reference=None):
    ours, theirs = np.asarray(ours), np.asarray(theirs)
    tiny = theirs < TINY
    if own_reference is not None:
        assert (np.asarray(own_reference) < TINY).mean() <= TINY_SHARE
    assert tiny.mean() <= TINY_SHARE
    assert (ours[tiny] < TINY_OK).all()
    np.testing.assert_allclose(ours[~tiny], theirs[~tiny], rtol=RTOL, atol=0)


def two_group_codes(code, a, b):
    """codes of "class a against class b": everything else -1, a -> 0, b -> 1"""
    out = np.full_like(code, -1)
    out[code == a] = 0
    out[code == b] = 1
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_and_host_pvalues_equal_scipy_for_two_groups(name):
    from meld_amd import diffexp

    X, code, D, _ = case(name)
    c2 = two_group_codes(code, 0, 2)
    rank2, tie, nnz, sums, _, n_c = ref.rank_sums(X, c2, 2)
    want_stat, want_p = scipy_test(D, code == 0, code == 2)
    stat, p = ref.pvalues(rank2[:, 0], tie, n_c[0], n_c[1])
    assert (stat == want_stat).all()
    assert_p_close(p, want_p, own_reference=p)
    stat2, p2 = diffexp.pvalues(rank2[:, 0].astype(np.int64), tie.astype(np.int64), n_c[0], n_c[1])
    assert (stat2 == want_stat).all()
    assert_p_close(p2, want_p, own_reference=p)
    # the all-zero gene and the all-tied non-zero gene: every value tied, p = 1.0 from all three
    for g in (0, 1):
        assert want_p[g] == 1.0 and p[g] == 1.0 and p2[g] == 1.0
        assert tie[g] == (n_c[0] + n_c[1]) ** 3 - (n_c[0] + n_c[1])
    assert (nnz[0] == 0).all() and (nnz[1] == np.array(n_c)).all()
    # the other direction is the mirrored statistic
    stat_b, p_b = ref.pvalues(rank2[:, 1], tie, n_c[1], n_c[0])
    assert (stat_b == n_c[0] * n_c[1] - want_stat).all()
    np.testing.assert_allclose(p_b, p, rtol=1e-13)


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_run_serves_every_class_against_the_rest(name):
    from meld_amd import diffexp

    X, code, D, (rank2, tie, nnz, sums, _, n_c) = case(name)
    m = sum(n_c)
    assert (code == -1).any()  # ignored cells
    for c in range(3):
        want_stat, want_p = scipy_test(D, code == c, (code >= 0) & (code != c))
        stat, p = ref.pvalues(rank2[:, c], tie, n_c[c], m - n_c[c])
        assert (stat == want_stat).all()
        assert_p_close(p, want_p, own_reference=p)
        stat2, p2 = diffexp.pvalues(rank2[:, c].astype(np.int64), tie.astype(np.int64), n_c[c], m - n_c[c])
        assert (stat2 == want_stat).all()
        assert_p_close(p2, want_p, own_reference=p)
        np.testing.assert_allclose(sums[:, c].astype(np.float64), D[code == c].sum(axis=0), rtol=1e-12, atol=1e-12)
        assert (nnz[:, c] == (D[code == c] != 0).sum(axis=0)).all()
    # the rank sums of all classes are the ranks 1 .. m
    assert all(sum(rank2[g]) == m * (m + 1) for g in range(X.shape[1]))


def test_restatement_has_the_features_the_cases_promise():
    X, code, D, _ = case("halves")
    assert (X.data == 0).any() and np.signbit(X.data[X.data == 0]).any() and not np.signbit(X.data[X.data == 0]).all()
    assert (X.data < 0).any() and X.nnz > (D != 0).sum()
    assert (D[:, 0] == 0).all() and (D[:, 1] == 1.5).all()
    vals, counts = np.unique(X.data, return_counts=True)
    assert len(vals) <= 9 and counts.max() > 100  # heavy ties


def test_benjamini_hochberg_equals_scipy():
    from meld_amd import diffexp

    rng = np.random.default_rng(5)
    for p in (rng.random(200), np.concatenate([rng.random(50) * 1e-6, rng.random(50), np.ones(7), [0.0, 1e-300]]), np.array([0.3]),
              np.array([0.5, 0.5, 0.01, 0.01])):
        want = stats.false_discovery_control(p, method="bh")
        np.testing.assert_allclose(ref.bh(p), want, rtol=RTOL, atol=0)
        np.testing.assert_allclose(diffexp.bh_qvalues(p), want, rtol=RTOL, atol=0)
    assert diffexp.bh_qvalues(np.array([])).shape == (0,)


def test_encode_classes():
    import pandas as pd

    from meld_amd.diffexp import MAX_CLASSES, encode_classes

    g = np.array(["b", "a", None, "c", "a", "b", np.nan, "c"], dtype=object)
    codes, classes = encode_classes(g)
    assert classes == ["a", "b", "c"] and codes.dtype == np.int32
    assert codes.tolist() == [1, 0, -1, 2, 0, 1, -1, 2]
    codes, classes = encode_classes(pd.Series(g), group="c", reference="a")
    assert classes == ["c", "a"] and codes.tolist() == [-1, 1, -1, 0, 1, -1, -1, 0]
    codes, classes = encode_classes(g, group="b")
    assert classes == ["b", None] and codes.tolist() == [0, 1, -1, 1, 1, 0, -1, 1]
    f = np.array([2.0, np.nan, 0.5, 2.0])
    codes, classes = encode_classes(f)
    assert classes == [0.5, 2.0] and codes.tolist() == [1, -1, 0, 1]
    codes, classes = encode_classes(np.array([3, 1, 3]), group=3, reference=1, n_cells=3)
    assert codes.tolist() == [0, 1, 0]
    mixed = np.array([1, "x", 1, ("t", 2)], dtype=object)  # hashable, not sortable: order of appearance
    codes, classes = encode_classes(mixed)
    assert classes == [1, "x", ("t", 2)] and codes.tolist() == [0, 1, 0, 2]
    with pytest.raises(ValueError, match="absent"):
        encode_classes(g, group="z")
    with pytest.raises(ValueError, match="reference label 'z' is absent"):
        encode_classes(g, group="a", reference="z")
    with pytest.raises(ValueError, match="empty reference"):
        encode_classes(np.array(["a", "a", None], dtype=object), group="a")
    with pytest.raises(ValueError, match="empty reference"):
        encode_classes(g, group="a", reference="a")
    with pytest.raises(ValueError, match="empty group"):
        encode_classes(np.array([None, np.nan], dtype=object))
    with pytest.raises(ValueError, match="length mismatch"):
        encode_classes(g, n_cells=9)
    with pytest.raises(ValueError, match="at most {}".format(MAX_CLASSES)):
        encode_classes(np.arange(MAX_CLASSES + 1))
    assert len(encode_classes(np.arange(MAX_CLASSES))[1]) == MAX_CLASSES


def test_host_pvalues_refuse_an_empty_side():
    from meld_amd import diffexp

    with pytest.raises(ValueError, match="empty group or reference"):
        diffexp.pvalues(np.array([2]), np.array([0]), 1, 0)


def test_entries_check_their_arguments_before_any_launch():
    """Every ``meld_ranksum_*`` entry and the integer-payload sort return -1, naming themselves, for NULL pointers and sizes out of
    range (host addresses stand in for device memory: nothing may touch them)."""
    from meld_amd import _lib, diffexp

    lib = _lib.get_lib()
    assert lib.meld_ranksum_lds_max() >= 2048 and lib.meld_ranksum_lds_max() & (lib.meld_ranksum_lds_max() - 1) == 0
    assert lib.meld_ranksum_max_classes() >= 64 and lib.meld_ranksum_max_classes() == diffexp.MAX_CLASSES
    assert lib.meld_ranksum_max_selected() == diffexp.MAX_SELECTED == 2097151
    assert (diffexp.MAX_SELECTED ** 3) < 2 ** 63 <= (diffexp.MAX_SELECTED + 1) ** 3
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    kmax = lib.meld_ranksum_max_classes()
    big = diffexp.MAX_SELECTED + 1
    calls = {
        "meld_ranksum_sums": [
            lambda: lib.meld_ranksum_sums(None, a, a, 0, 4, a, 8, 2, a, None),
            lambda: lib.meld_ranksum_sums(a, a, a, 0, 4, a, 8, 2, None, None),
            lambda: lib.meld_ranksum_sums(a, a, a, 2, 4, a, 8, 2, a, None),
            lambda: lib.meld_ranksum_sums(a, a, a, 0, 0, a, 8, 2, a, None),
            lambda: lib.meld_ranksum_sums(a, a, a, 0, 4, a, 1 << 31, 2, a, None),
            lambda: lib.meld_ranksum_sums(a, a, a, 0, 4, a, 8, kmax + 1, a, None),
            lambda: lib.meld_ranksum_sums(a, a, a, 0, 4, a, 8, 0, a, None),
        ],
        "meld_ranksum_short": [
            lambda: lib.meld_ranksum_short(a, a, a, 0, 4, None, 2, a, 8, 2, a, 8, a, a, a, None),
            lambda: lib.meld_ranksum_short(a, a, a, 0, 4, a, 2, a, 8, 2, None, 8, a, a, a, None),
            lambda: lib.meld_ranksum_short(a, a, a, 0, 4, a, 2, a, 8, 2, a, 8, a, None, a, None),
            lambda: lib.meld_ranksum_short(a, a, a, 0, 4, a, 5, a, 8, 2, a, 8, a, a, a, None),
            lambda: lib.meld_ranksum_short(a, a, a, 0, 4, a, 2, a, 8, kmax + 1, a, 8, a, a, a, None),
            lambda: lib.meld_ranksum_short(a, a, a, 0, 4, a, 2, a, 8, 2, a, big, a, a, a, None),
            lambda: lib.meld_ranksum_short(a, a, a, 0, 4, a, 2, a, 8, 2, a, -1, a, a, a, None),
        ],
        "meld_ranksum_gather": [
            lambda: lib.meld_ranksum_gather(a, a, a, 0, 4, a, None, 2, 10, a, 8, 2, a, a, None),
            lambda: lib.meld_ranksum_gather(a, a, a, 0, 4, a, a, 2, 10, a, 8, 2, None, a, None),
            lambda: lib.meld_ranksum_gather(a, a, a, 0, 4, a, a, 0, 10, a, 8, 2, a, a, None),
            lambda: lib.meld_ranksum_gather(a, a, a, 0, 4, a, a, 2, -1, a, 8, 2, a, a, None),
            lambda: lib.meld_ranksum_gather(a, a, a, 0, 4, a, a, 2, 1 << 38, a, 8, 2, a, a, None),
        ],
        "meld_ranksum_scan": [
            lambda: lib.meld_ranksum_scan(None, a, a, a, 2, 4, 2, a, 8, a, a, a, None),
            lambda: lib.meld_ranksum_scan(a, a, a, None, 2, 4, 2, a, 8, a, a, a, None),
            lambda: lib.meld_ranksum_scan(a, a, a, a, 0, 4, 2, a, 8, a, a, a, None),
            lambda: lib.meld_ranksum_scan(a, a, a, a, 2, 4, kmax + 1, a, 8, a, a, a, None),
            lambda: lib.meld_ranksum_scan(a, a, a, a, 2, 4, 2, a, big, a, a, a, None),
        ],
        "meld_sort_pairs_u64_u64": [
            lambda: lib.meld_sort_pairs_u64_u64(None, a, a, a, 10, 0, 64, a, 1 << 20, None),
            lambda: lib.meld_sort_pairs_u64_u64(a, a, a, a, 10, 0, 64, None, 1 << 20, None),
            lambda: lib.meld_sort_pairs_u64_u64(a, a, a, a, 10, 32, 32, a, 1 << 20, None),
            lambda: lib.meld_sort_pairs_u64_u64(a, a, a, a, 10, 0, 65, a, 1 << 20, None),
            lambda: lib.meld_sort_pairs_u64_u64(a, a, a, a, -1, 0, 64, a, 1 << 20, None),
        ],  # (a temp that is too small needs the device's sort configuration: tests/test_gpu_ranksum.py)
    }
    for name, bad in calls.items():
        for i, call in enumerate(bad):
            lib.meld_scale_f64(None, 1.0, None, 10, None)  # (leaves another entry's message behind)
            assert call() == -1, (name, i)
            assert lib.meld_last_error().decode().startswith(name + ":"), (name, i, lib.meld_last_error())
    assert lib.meld_ranksum_scan(a, a, a, a, 2, 4, 2, a, big, a, a, a, None) == -1 and b"2097151" in lib.meld_last_error()  # names the limit
    # nothing to do is not an error and launches nothing
    assert lib.meld_ranksum_short(a, a, a, 0, 4, a, 0, a, 8, 2, a, 8, a, a, a, None) == 0
    assert lib.meld_sort_pairs_u64_u64(a, a, a, a, 0, 0, 64, a, 0, None) == 0


def test_long_route_batches_cover_the_genes_in_order():
    from meld_amd.diffexp import _long_batches

    assert _long_batches([5, 5, 5, 5], 10) == [(0, 2), (2, 4)]
    assert _long_batches([50, 1, 1, 50], 10) == [(0, 1), (1, 3), (3, 4)]  # a gene above the limit goes alone
    assert _long_batches([0, 0], 10) == [(0, 2)] and _long_batches([], 10) == []
    assert _long_batches([3], 10) == [(0, 1)]


@pytest.mark.timeout(600)
def test_rank_sum_kernels_use_no_private_memory():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    from meld_amd import build as mbuild

    src = os.path.join(ROOT, "meld_amd", "csrc", "ranksum.hip")
    cmd = [hipcc] + mbuild.FLAGS + mbuild.FILE_FLAGS.get("ranksum.hip", []) + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only",
                                                                             "-c", src, "-o", os.devnull]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=580).stdout
    rows, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            rows[cur] = {}
        for key in ("ScratchSize [bytes/lane]:", "LDS Size [bytes/block]:", "Occupancy [waves/SIMD]:"):
            if cur and key in line:
                rows[cur][key] = int(line.split(key)[1].split()[0])
    ours = {n: r for n, r in rows.items() if "ranksum_" in n}
    assert len(ours) == 7, sorted(ours)  # short, gather and sums for fp32 / fp64 values, the scan
    for n, r in ours.items():
        assert r["ScratchSize [bytes/lane]:"] == 0, (n, r)
    for n, r in ours.items():
        if "ranksum_short_kernel" in n:  # four workgroups of four waves on a CU's 160 KiB
            assert r["LDS Size [bytes/block]:"] <= 40 * 1024 and r["Occupancy [waves/SIMD]:"] == 4, (n, r)
