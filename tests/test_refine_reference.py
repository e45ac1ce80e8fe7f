"""tests/refine_reference.py against the project's ground truth (host only): on candidate lists that ARE complete -- the true
nearest cells by brute force, no search error -- the reference must reproduce the oracle's directed kernel and bandwidths.  Every GPU
result of tests/test_gpu_refine_contract.py is judged by this reference, so it is tied to the oracle first."""
import numpy as np
import pytest

from tests import refine_reference as rr


def _cells(seed, N=700, d=4):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(N, d)) * rng.uniform(0.2, 2.0, size=d) + rng.normal(size=d)


def _reference_kernel(X, ksel, knn, decay, thresh, **opts):
    N = X.shape[0]
    idx, d2 = rr.true_lists(X, 0, N, ksel)
    cnt = np.full(N, ksel, np.int32)
    ref = rr.refine_ref(X, 0, idx.astype(np.int32), d2.astype(np.float32), cnt, None, ksel, ksel, knn, decay, thresh, 1.0, 0.0, **opts)
    return idx, ref


@pytest.mark.parametrize(
    "name,decay,okw,rkw",
    [
        ("decay40", 40, {}, {}),
        ("connectivity", None, {}, {}),
        ("decay10_scale_0.6", 10, dict(bandwidth_scale=0.6), dict(bw_scale=0.6)),
        ("decay40_scale_1.3", 40, dict(bandwidth_scale=1.3), dict(bw_scale=1.3)),
        ("fixed_bandwidth", 40, dict(bandwidth="per_cell"), dict(bw_fixed="per_cell")),
        ("fixed_bandwidth_scaled", 40, dict(bandwidth="per_cell", bandwidth_scale=0.8), dict(bw_fixed="per_cell", bw_scale=0.8)),
        ("knn_max", 40, dict(knn_max=8), dict(max_rank=9)),
    ],
)
def test_reference_reproduces_the_oracle_on_complete_lists(name, decay, okw, rkw):
    from oracle import meld_oracle as mo

    X = _cells(3)
    N, knn, thresh, ksel = X.shape[0], 5, 1e-4, 100
    if okw.get("bandwidth") == "per_cell":
        given = np.random.default_rng(7).uniform(0.25, 0.5, size=N)
        okw, rkw = dict(okw, bandwidth=given), dict(rkw, bw_fixed=given)
    K, mid = mo.knn_kernel(X, knn=knn, decay=decay, thresh=thresh, algorithm="brute", return_intermediates=True, **okw)
    idx, ref = _reference_kernel(X, ksel, knn, np.inf if decay is None else decay, thresh, **rkw)
    # the lists are complete by construction and the reference must say so (its certificate has no error allowance to pay here);
    # a row with a knn_max is complete through the rank clause even where 100 cells do not reach its radius
    assert ref["complete"].all()
    # no kernel value sits on the threshold: the comparison of the sparsity patterns below is decided, nothing is left out
    nz = ref["val"][(ref["dist"] < np.inf) & (ref["rank"] > 0)]
    if decay is not None:
        full = rr.kernel_values(ref["dist"], ref["bw"][:, None] * rkw.get("bw_scale", 1.0), decay)
        inside = np.isfinite(ref["dist"]) & (full > 0)
        assert float(np.min(np.abs(full[inside].astype(np.float64) / thresh - 1.0))) > 1e-6
    assert nz.size
    # bandwidths (the oracle reports the scaled, floored value; the reference records the unscaled one)
    used = np.maximum(ref["bw"].astype(np.float64) * rkw.get("bw_scale", 1.0), rr.EPS)
    np.testing.assert_allclose(used, mid["bandwidth"], rtol=1e-10)
    if "bw_fixed" in rkw:
        assert np.array_equal(ref["bw"].astype(np.float64), rkw["bw_fixed"])
    # the directed kernel off the diagonal: same pattern, same values
    K = K.tocsr()
    K.sort_indices()
    for i in range(N):
        cols, vals = K.indices[K.indptr[i]:K.indptr[i + 1]], K.data[K.indptr[i]:K.indptr[i + 1]]
        off = cols != i
        kept = ref["val"][i] > 0
        o = np.argsort(idx[i][kept])
        assert np.array_equal(idx[i][kept][o], cols[off]), (name, i)
        np.testing.assert_allclose(ref["val"][i][kept][o].astype(np.float64), vals[off], rtol=1e-9)
        assert ref["keep_cnt"][i] == int(off.sum())
        assert idx[i][0] == i and ref["val"][i][0] == 0  # the row itself: in the list, never kept


def test_sweep_reference_agrees_with_the_list_reference_and_counts_closer_cells():
    """The two halves of the reference against each other: a brute-force sweep of a row with the bandwidth its complete list gives
    keeps what the list keeps, counts exactly knn cells strictly closer (self among them) and confirms the bandwidth; a bandwidth
    1 % larger is not confirmed; eps with more than knn copies is."""
    X = _cells(5, N=500, d=3)
    X[10:20] = X[9]  # ten exact copies of cell 9
    knn, thresh, ksel = 5, 1e-4, 100
    idx, ref = _reference_kernel(X, ksel, knn, 40, thresh)
    rows = np.array([0, 9, 15, 77, 499])
    sw = rr.sweep_ref(X, 0, rows, ref["bw"], knn, 40, thresh)
    for r, s in zip(rows, sw):
        kept = ref["val"][r] > 0
        assert np.array_equal(np.sort(idx[r][kept]), s["cols"]) and r not in s["cols"]
        assert s["confirmed"]
        if r in (9, 15):
            assert ref["bw"][r] == rr.EPS and s["n_closer"] == 11 and len(s["cols"]) == 10 and np.all(s["vals"] == 1)
        else:
            assert s["n_closer"] == knn
    big = rr.sweep_ref(X, 0, rows, ref["bw"] * np.longdouble(1.01), knn, 40, thresh)
    assert [s["confirmed"] for s in big] == [False, False, False, False, False]
