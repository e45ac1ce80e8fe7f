"""Rank-sum differential expression on the device (meld_amd/diffexp.py, csrc/ranksum.hip) against the host restatement
(tests/ranksum_reference.py, itself held against scipy by tests/test_ranksum_reference.py): ``rank2``, ``tie`` and ``nnz`` are integer
arithmetic and must be EQUAL, on the short route (sort in LDS), on the long route (radix sort, scan from global memory) and at the
boundary between them; ``sum`` lies within m 2^-53 sum|v| of the long-double sum (any order of m fp64 additions does) and has the same
bits on every run.  ``rank_sum_test`` end to end is held to scipy under the host tier's tolerances."""
import numpy as np
import pytest
import torch
from scipy import sparse, stats

from tests import ranksum_reference as ref
from tests.test_ranksum_reference import RTOL, TINY, TINY_OK, TINY_SHARE, scipy_test

pytestmark = pytest.mark.gpu

KINDS = ["halves", "real", "counts"]
DTYPES = [np.float64, np.float32]


def _kmax():
    from meld_amd._lib import get_lib

    return int(get_lib().meld_ranksum_max_classes())


def _cap():
    from meld_amd._lib import get_lib

    return int(get_lib().meld_ranksum_lds_max())


def _run(data, code, k, **kw):
    from meld_amd.diffexp import rank_sums_device

    res = rank_sums_device(data, code, k, **kw)
    torch.cuda.synchronize()
    return res


def _assert_equals_reference(res, want, what):
    rank2, tie, nnz, sums, abs_sums, n_c = want
    m = sum(n_c)
    got_r2, got_tie, got_nnz = res.rank2.cpu().numpy(), res.tie.cpu().numpy(), res.nnz.cpu().numpy()
    assert res.m == m and res.n_c.cpu().tolist() == n_c, what
    assert got_r2.dtype == np.int64 and got_tie.dtype == np.int64 and got_nnz.dtype == np.int32
    assert (got_r2 == rank2.astype(np.int64)).all(), (what, np.argwhere(got_r2 != rank2.astype(np.int64))[:5])
    assert (got_tie == tie.astype(np.int64)).all(), (what, np.argwhere(got_tie != tie.astype(np.int64))[:5])
    assert (got_nnz == nnz).all(), what
    err = np.abs(res.sum.cpu().numpy().astype(np.longdouble) - sums)
    assert (err <= m * 2.0 ** -53 * abs_sums).all(), (what, float(err.max()))


def _assert_same_bits(a, b, what, with_sum=True):
    assert torch.equal(a.rank2, b.rank2) and torch.equal(a.tie, b.tie) and torch.equal(a.nnz, b.nnz), what
    if with_sum:
        assert torch.equal(a.sum.view(torch.int64), b.sum.view(torch.int64)), what


@pytest.mark.parametrize("G", [1, 40, 300])
@pytest.mark.parametrize("N", [2, 63, 64, 65, 700, 5000])
def test_raw_outputs_equal_the_restatement_on_both_routes(N, G):
    i = [2, 63, 64, 65, 700, 5000].index(N) + 2 * [1, 40, 300].index(G)
    k = [2, 3, 17, _kmax()][i % 4]
    kind, dtype = KINDS[i % 3], DTYPES[(i // 2) % 2]
    X, code = ref.make_case(N, G, 0.3 if N < 100 else 0.12, seed=100 + i, kind=kind, dtype=dtype, n_classes=k)
    assert X.dtype == dtype
    want = ref.rank_sums(X, code, k)
    short = _run(X, code, k)
    long_ = _run(X, code, k, force_long=True)
    _assert_equals_reference(short, want, ("short", N, G, k, kind))
    _assert_equals_reference(long_, want, ("long", N, G, k, kind))
    _assert_same_bits(short, long_, ("short against long", N, G, k))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [2, 3, 17, "max"])
def test_every_number_of_classes(k, dtype):
    k = _kmax() if k == "max" else k
    X, code = ref.make_case(700, 40, 0.15, seed=k, kind="halves", dtype=dtype, n_classes=k)
    want = ref.rank_sums(X, code, k)
    _assert_equals_reference(_run(X, code, k), want, ("short", k))
    _assert_equals_reference(_run(X, code, k, force_long=True), want, ("long", k))


def _boundary_case(dtype):
    """N = cap + 70 cells; genes of stored length 0, 1, cap - 1, cap, cap + 1 and N (stored in every cell), heavy ties, negatives,
    stored zeros of both signs, ignored cells."""
    cap = _cap()
    N = cap + 70
    rng = np.random.default_rng(11)
    lens = [0, 1, cap - 1, cap, cap + 1, N]
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rng.choice(N, n, replace=False)) for n in lens]).astype(np.int32)
    data = (np.round(rng.random(indptr[-1]) * 8) / 2 - 1.0)  # -1, -0.5, 0 ... 3
    data[(data == 0) & (rng.random(len(data)) < 0.5)] = -0.0
    X = sparse.csc_matrix((data.astype(dtype), indices, indptr), shape=(N, len(lens)))
    code = rng.integers(-1, 3, N).astype(np.int32)
    return X, code, lens


@pytest.mark.parametrize("dtype", DTYPES)
def test_route_boundary_and_a_gene_stored_in_every_cell(dtype):
    X, code, lens = _boundary_case(dtype)
    cap = _cap()
    assert cap >= 2048 and sum(n > cap for n in lens) == 2 and sum(n <= cap for n in lens) == 4
    assert (X.data == 0).any() and (X.data < 0).any() and (code == -1).any()
    want = ref.rank_sums(X, code, 3)
    mixed = _run(X, code, 3)
    _assert_equals_reference(mixed, want, "routes by stored length")
    long_ = _run(X, code, 3, force_long=True)
    _assert_equals_reference(long_, want, "long route for every gene")
    _assert_same_bits(mixed, long_, "a gene's numbers do not depend on its route")
    # the same input twice: identical bits in every output, on either route
    _assert_same_bits(mixed, _run(X, code, 3), "twice, by stored length")
    _assert_same_bits(long_, _run(X, code, 3, force_long=True), "twice, long")


def test_long_route_in_several_batches(monkeypatch):
    from meld_amd import diffexp

    X, code = ref.make_case(700, 40, 0.15, seed=4, kind="halves", n_classes=3)
    one = _run(X, code, 3, force_long=True)
    monkeypatch.setattr(diffexp, "LONG_BATCH_ENTRIES", 500)
    assert len(diffexp._long_batches(np.diff(X.indptr), 500)) > 5
    _assert_same_bits(one, _run(X, code, 3, force_long=True), "batches of the long route")
    _assert_equals_reference(one, ref.rank_sums(X, code, 3), "long")


def test_permuting_the_cells_with_their_codes_changes_nothing():
    X, code = ref.make_case(700, 40, 0.15, seed=6, kind="halves", n_classes=3)
    perm = np.random.default_rng(0).permutation(700)
    Xp = X.tocsr()[perm].tocsc()
    assert Xp.nnz == X.nnz  # (the stored zeros survive the indexing)
    for force in (False, True):
        _assert_same_bits(_run(X, code, 3, force_long=force), _run(Xp, code[perm], 3, force_long=force), ("permuted", force), with_sum=False)


def test_every_input_form_gives_the_same_integers():
    import pandas as pd

    from meld_amd.sparse import DeviceCSR

    X, code = ref.make_case(700, 40, 0.15, seed=7, kind="halves", n_classes=3)
    want = ref.rank_sums(X, code, 3)
    D = np.asarray(X.toarray())
    base = _run(X, code, 3)  # a host CSC matrix: uploaded as the CSR of the transpose
    _assert_equals_reference(base, want, "csc")
    dcsr = DeviceCSR.from_input(X.tocsr())
    forms = {"csr": X.tocsr(), "coo": X.tocoo(), "device csr": dcsr, "device csr again (cached transpose)": dcsr, "numpy": D,
             "frame": pd.DataFrame(D), "float32": D.astype(np.float32), "device tensor": torch.from_numpy(D).cuda(),
             "torch csr": torch.from_numpy(D).cuda().to_sparse_csr(), "codes on the device": X}
    for name, data in forms.items():
        res = _run(data, torch.from_numpy(code).cuda() if name == "codes on the device" else code, 3)
        _assert_same_bits(base, res, name, with_sum=False)
        np.testing.assert_allclose(res.sum.cpu().numpy(), base.sum.cpu().numpy(), rtol=1e-13, atol=1e-13)
    assert dcsr._T is not None  # the transpose stays with the matrix the caller holds


def _assert_frame_equals_scipy(frame, D, sel1, sel2):
    want_stat, want_p = scipy_test(D, sel1, sel2)
    assert list(frame.columns) == ["statistic", "pval", "qval", "mean_group", "mean_reference", "log2fc", "nnz_group", "nnz_reference"]
    assert (frame["statistic"].to_numpy() == want_stat).all()
    for ours, theirs in ((frame["pval"].to_numpy(), want_p), (frame["qval"].to_numpy(), stats.false_discovery_control(want_p, method="bh"))):
        tiny = theirs < TINY
        assert tiny.mean() <= TINY_SHARE and (ours[tiny] < TINY_OK).all()
        np.testing.assert_allclose(ours[~tiny], theirs[~tiny], rtol=RTOL, atol=0)
    np.testing.assert_allclose(frame["mean_group"].to_numpy(), D[sel1].mean(axis=0), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(frame["mean_reference"].to_numpy(), D[sel2].mean(axis=0), rtol=1e-12, atol=1e-300)
    with np.errstate(all="ignore"):
        lfc = np.log2(frame["mean_group"].to_numpy() / frame["mean_reference"].to_numpy())
    assert np.array_equal(frame["log2fc"].to_numpy(), lfc, equal_nan=True)
    assert (frame["nnz_group"].to_numpy() == (D[sel1] != 0).sum(axis=0)).all()
    assert (frame["nnz_reference"].to_numpy() == (D[sel2] != 0).sum(axis=0)).all()


def test_rank_sum_test_end_to_end_against_scipy():
    import pandas as pd

    import meld_amd

    X, code = ref.make_case(700, 40, 0.15, seed=1, kind="halves", n_classes=3)
    D = np.asarray(X.toarray())
    names = np.array(["T", "B", "NK"], dtype=object)
    groups = np.where(code >= 0, names[np.maximum(code, 0)], None)
    genes = ["gene{}".format(g) for g in range(40)]
    frame_data = pd.DataFrame(D, columns=genes)
    # two groups
    two = meld_amd.rank_sum_test(frame_data, groups, group="T", reference="NK")
    assert list(two.index) == genes  # the gene index comes from the DataFrame's columns
    _assert_frame_equals_scipy(two, D, code == 0, code == 2)
    assert two["pval"].iloc[0] == 1.0 and two["pval"].iloc[1] == 1.0  # the all-zero and the all-tied gene
    # one group against the rest, sparse input, names given
    rest = meld_amd.rank_sum_test(X, pd.Series(groups), group="B", gene_names=genes)
    assert list(rest.index) == genes
    _assert_frame_equals_scipy(rest, D, code == 1, (code >= 0) & (code != 1))
    # every cluster against the rest, from one run; integer gene index without names
    every = meld_amd.rank_sum_test(X, groups)
    assert sorted(every) == ["B", "NK", "T"]
    for c, label in enumerate(names):
        _assert_frame_equals_scipy(every[label], D, code == c, (code >= 0) & (code != c))
        assert list(every[label].index) == list(range(40))
    pd.testing.assert_frame_equal(every["B"].set_axis(genes), rest)
    # the estimator's wrapper gives the same frames; after transform the sample labels are the groups
    op = meld_amd.MELD(knn=7, verbose=False)
    pd.testing.assert_frame_equal(op.rank_sum_test(frame_data, groups, group="T", reference="NK"), two)
    with pytest.raises(ValueError, match="transform"):
        op.rank_sum_test(frame_data)
    samples = np.where(np.arange(700) % 3 == 0, "treated", "control")
    op.fit_transform(D + np.random.default_rng(0).normal(size=D.shape) * 1e-3, samples)
    by_sample = op.rank_sum_test(frame_data, group="treated")
    _assert_frame_equals_scipy(by_sample, D, samples == "treated", samples == "control")


def test_every_refusal_comes_before_any_launch(monkeypatch):
    from meld_amd import _lib, diffexp

    X, code = ref.make_case(65, 5, 0.3, seed=9, kind="halves", n_classes=3)
    groups = np.where(code >= 0, np.array(["a", "b", "c"], dtype=object)[np.maximum(code, 0)], None)
    lib = _lib.get_lib()
    launching = ["meld_ranksum_sums", "meld_ranksum_short", "meld_ranksum_gather", "meld_ranksum_scan", "meld_sort_pairs_u64_u64"]

    def refuse(*a, **kw):
        raise AssertionError("a kernel entry was called")

    for name in launching:
        monkeypatch.setattr(lib, name, refuse)
    with pytest.raises(ValueError, match="group label 'z' is absent"):
        diffexp.rank_sum_test(X, groups, group="z")
    with pytest.raises(ValueError, match="reference label 'z' is absent"):
        diffexp.rank_sum_test(X, groups, group="a", reference="z")
    with pytest.raises(ValueError, match="empty reference"):
        diffexp.rank_sum_test(X, np.where(groups == "a", "a", None), group="a")
    with pytest.raises(ValueError, match="empty reference"):
        diffexp.rank_sum_test(X, np.where(groups == "a", "a", None))
    with pytest.raises(ValueError, match="empty group"):
        diffexp.rank_sum_test(X, np.full(65, None, dtype=object))
    with pytest.raises(ValueError, match="at most {}".format(_kmax())):
        diffexp.rank_sum_test(sparse.random(_kmax() + 1, 3, density=0.5, format="csc", random_state=0), np.arange(_kmax() + 1))
    with pytest.raises(ValueError, match="length mismatch"):
        diffexp.rank_sum_test(X, groups[:-1])
    with pytest.raises(ValueError, match="length mismatch"):
        diffexp.rank_sums_device(X, code[:-1], 3)
    with pytest.raises(ValueError, match="classes"):
        diffexp.rank_sums_device(X, code, _kmax() + 1)
    with pytest.raises(ValueError, match="classes"):
        diffexp.rank_sums_device(X, code, 0)
    # more selected cells than the tie term holds in int64: refused, the limit named
    n_big = diffexp.MAX_SELECTED + 1
    big = sparse.csc_matrix((np.ones(3), np.array([0, 5, n_big - 1]), np.array([0, 3])), shape=(n_big, 1))
    with pytest.raises(ValueError, match="2097151"):
        diffexp.rank_sums_device(big, np.zeros(n_big, dtype=np.int32), 2)
    monkeypatch.undo()
    # ... and exactly the limit is served: one gene, three ones among 2,097,151 cells of two classes
    n_ok = diffexp.MAX_SELECTED
    ok = sparse.csc_matrix((np.ones(3), np.array([0, 5, n_ok - 1]), np.array([0, 3])), shape=(n_ok, 1))
    code_ok = (np.arange(n_ok) % 2).astype(np.int32)
    for force in (False, True):
        res = _run(ok, code_ok, 2, force_long=force)
        z = n_ok - 3
        assert int(res.tie[0]) == z ** 3 - z + 3 ** 3 - 3
        # zeros: mid-rank (z + 1) / 2; the ones: ranks z + 1 .. z + 3, mid-rank z + 2; cells 0 and n_ok - 1 are class 0, cell 5 class 1
        n0 = (n_ok + 1) // 2
        assert res.rank2.cpu().tolist() == [[(n0 - 2) * (z + 1) + 2 * 2 * (z + 2), (n_ok - n0 - 1) * (z + 1) + 2 * (z + 2)]]
        assert res.nnz.cpu().tolist() == [[2, 1]]


def test_integer_payload_sort_is_stable_on_a_bit_range_and_checks_its_temp():
    from meld_amd._lib import get_lib, ptr

    lib, st = get_lib(), torch.cuda.current_stream().cuda_stream
    n = 5000
    gen = torch.Generator().manual_seed(0)
    keys = (torch.randint(0, 7, (n,), generator=gen, dtype=torch.int64) << 32 | torch.randint(0, 1 << 20, (n,), generator=gen)).cuda()
    vals = torch.arange(n, dtype=torch.int64).cuda()
    k2, v2 = torch.empty_like(keys), torch.empty_like(vals)
    tb = lib.meld_sort_temp_bytes(n)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    assert lib.meld_sort_pairs_u64_u64(ptr(keys), ptr(k2), ptr(vals), ptr(v2), n, 32, 35, ptr(tmp), tb, st) == 0
    torch.cuda.synchronize()
    order = torch.sort(keys >> 32, stable=True).indices
    assert torch.equal(v2, vals[order]) and torch.equal(k2, keys[order])
    assert lib.meld_sort_pairs_u64_u64(ptr(keys), ptr(k2), ptr(vals), ptr(v2), 1 << 22, 0, 64, ptr(tmp), 16, st) == -1
    assert lib.meld_last_error().decode().startswith("meld_sort_pairs_u64_u64: temp_bytes=16")
