"""k-means on the device (meld_amd/kmeans.py, csrc/kmeans_wide.hip) against the long-double host reference tests/kmeans_reference.py
(checked by hand, and for the share of near-ties of every input used here, by tests/test_kmeans_reference.py).

Tolerances, derived.  ``tau_i = 8 (d + 4) 2^-53 (|y_i|^2 + max_j |c_j|^2)`` bounds twice the error of comparing two expanded distances
``|y|^2 + |c|^2 - 2 y.c`` in fp64 (tests/kmeans_reference.py states the derivation).  So the centre the kernel picks is within
``2 tau_i`` of the nearest, equals it wherever the runner-up is more than ``2 tau_i`` away, and the distance it reports -- one
expanded distance -- is within ``tau_i`` of the true one.  Sums: ``m`` rows added in any order are within ``(m - 1) u sum |y|`` of
the exact sum to first order; the bound used is ``m u sum |y|``.  Inertia: ``n`` distances, each within ``tau_i``, summed: a step
that does not lower the true inertia can show a rise of at most ``sum tau_i``.

Shapes: the assign kernel takes 256 points per workgroup (128 for d > 96), 32 centres per tile, d padded to a multiple of 16 and
one kernel per padded width: n in {1, 17, 63, 257, 1000, 5000}, d in {1, 3, 4, 10, 50, 100, 128}, k in {1, 16, 17, 40, 65, 1000,
2000, 4096} and 4,100 centres for the chunked route; the sums kernel takes 16 slots of 4 rows per cluster."""
import numpy as np
import pytest
import torch

from tests import kmeans_reference as ref

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.array(a)).to("cuda", dtype=dtype)  # (a copy: the shared reference arrays are read-only)


def _check_assign(Y, C, D, t, lab, d2):
    n, k = D.shape
    assert lab.dtype == np.int32 and lab.min() >= 0 and lab.max() < k  # (f) a padded centre is never selected
    rows = np.arange(n)
    picked, nearest = D[rows, lab], D.min(1)
    excess = picked - nearest
    print("assign: n, d, k =", Y.shape[0], Y.shape[1], k, " max excess / tau =", float((excess / t).max()),
          " max |best_d2 - dist| / tau =", float((np.abs(d2.astype(LD) - picked) / t).max()))
    assert np.all(excess <= 2 * t)  # (a) every point
    decided = ref.gaps(D) > 2 * t
    assert int((~decided).sum()) <= n // 1000  # (the cap on what (b) leaves out)
    assert np.array_equal(lab[decided], ref.argmin_lowest(D)[decided])  # (b)
    assert np.all(d2 >= 0) and np.all(np.abs(d2.astype(LD) - picked) <= t)  # (c)


@pytest.mark.parametrize("name", ref.CASE_NAMES)
def test_assign_contract(name):
    from meld_amd.kmeans import assign

    Y, C, D, t = ref.case_reference(name)
    n, d = Y.shape
    if name == "1000x100x1000":  # (this case with a leading dimension above d: the columns beyond d hold values that would win)
        buf = torch.full((n, d + 3), -1e6, dtype=torch.float64, device="cuda")
        buf[:, :d] = _dev(Y)
        Yd = buf[:, :d]
        assert Yd.stride(0) == d + 3
    else:
        Yd = _dev(Y)
    Cd = _dev(C)
    lab, d2 = assign(Yd, Cd)
    lab2, d22 = assign(Yd, Cd)
    assert torch.equal(lab, lab2) and torch.equal(d2, d22)  # (d) the same bits
    lab_only, none = assign(Yd, Cd, want_d2=False)
    assert none is None and torch.equal(lab_only, lab)
    _check_assign(Y, C, D, t, lab.cpu().numpy(), d2.cpu().numpy())


def test_assign_duplicates_and_points_on_centres():
    from meld_amd.kmeans import assign

    Y, C = ref.duplicate_case()
    D, t = ref.distances(Y, C), ref.tau(Y, C)
    lab, d2 = assign(_dev(Y), _dev(C))
    lab, d2 = lab.cpu().numpy(), d2.cpu().numpy()
    assert not np.isin(lab, [21, 33]).any()  # (e) never the higher index of a duplicated pair
    want = np.arange(40)
    want[21], want[33] = 5, 7
    assert np.array_equal(lab[:40], want)  # a point on a centre gets that centre, or its lower-indexed duplicate
    assert np.all(d2[:40] >= 0) and np.all(d2[:40] < t[:40])
    picked = D[np.arange(300), lab]
    assert np.all(picked - D.min(1) <= 2 * t) and np.all(np.abs(d2.astype(LD) - picked) <= t)
    # every centre the same row: every point gets centre 0
    same = np.repeat(C[:1], 37, axis=0)
    lab0, _ = assign(_dev(Y), _dev(same))
    assert int(lab0.abs().max()) == 0


def test_assign_in_chunks_of_centres():
    """More centres than one launch takes: chunks of 4096, label offset added, minima combined."""
    from meld_amd.kmeans import MAX_K, assign

    rng = np.random.default_rng(11)
    Y, C = rng.standard_normal((300, 7)), rng.standard_normal((MAX_K + 200, 7))
    C[MAX_K + 2] = C[3]  # (a duplicate across the chunks: the lower index stays)
    Y[0] = C[3]
    D, t = ref.distances(Y, C), ref.tau(Y, C)
    lab, d2 = assign(_dev(Y), _dev(C))
    lab, d2 = lab.cpu().numpy(), d2.cpu().numpy()
    assert lab[0] == 3 and not (lab == MAX_K + 2).any()
    picked = D[np.arange(300), lab]
    assert np.all(picked - D.min(1) <= 2 * t) and np.all(np.abs(d2.astype(LD) - picked) <= t)
    decided = ref.gaps(np.delete(D, MAX_K + 2, axis=1)) > 2 * t
    assert np.array_equal(lab[decided], ref.argmin_lowest(D)[decided]) and (lab >= MAX_K).any()


def _sums_case(which, d):
    rng = np.random.default_rng(100 + d)
    if which == "one":  # one cluster holds all 5,000 points, k = 70
        n, k = 5000, 70
        lab = np.full(n, 41)
    elif which == "singletons":
        n = k = 100
        lab = rng.permutation(100)
    else:  # 300 points over 4,096 clusters, mostly empty
        n, k = 300, 4096
        lab = rng.integers(0, k, n)
    return rng.standard_normal((n, d)) * 10.0 ** rng.integers(-3, 4, (n, 1)), lab.astype(np.int32), k


@pytest.mark.parametrize("d", [1, 100, 128])
@pytest.mark.parametrize("which", ["one", "singletons", "sparse"])
def test_sums_contract(which, d):
    from meld_amd.kmeans import segment_sums

    Y, lab, k = _sums_case(which, d)
    Yd, labd = _dev(Y), _dev(lab, torch.int32)
    sums, cnt = segment_sums(Yd, labd, k)
    sums2, cnt2 = segment_sums(Yd, labd, k)
    assert torch.equal(sums, sums2) and torch.equal(cnt, cnt2)  # the same bits
    sums, cnt = sums.cpu().numpy(), cnt.cpu().numpy()
    want, want_cnt = ref.segment_sums(Y, lab, k)
    assert np.array_equal(cnt, want_cnt)  # counts exact
    mag, _ = ref.segment_sums(np.abs(Y), lab, k)
    assert np.all(np.abs(sums.astype(LD) - want) <= want_cnt[:, None] * LD(U) * mag)
    assert np.all(sums[want_cnt == 0] == 0)  # empty clusters exactly zero
    if which == "singletons":
        assert np.array_equal(sums[lab], Y)


@pytest.fixture(scope="module")
def blob_fit():
    from meld_amd import KMeans

    X, truth = ref.blobs()
    km = KMeans(80, random_state=0).fit(X)
    return X, truth, km


def test_kmeans_recovers_separate_blobs(blob_fit):
    X, truth, km = blob_fit
    print("KMeans(80): n_iter_", km.n_iter_, "inertia_", km.inertia_, km.info_)
    assert km.info_["lloyd"] == "device" and km.labels_.dtype == np.int32 and km.cluster_centers_.shape == (80, 10)
    pairs = set(zip(truth.tolist(), km.labels_.tolist()))
    assert len(pairs) == 80, len(pairs)  # (a partition: every blob one cluster, every cluster one blob)
    assert np.array_equal(km.labels_device_.cpu().numpy(), km.labels_)


def test_kmeans_inertia(blob_fit):
    X, truth, km = blob_fit
    hist = km.inertia_history_
    assert hist.shape == (km.n_iter_,) and km.n_iter_ >= 1
    slack = float(ref.tau(X, km.cluster_centers_).sum())
    assert np.all(np.diff(hist) <= slack), (hist, slack)
    assert km.inertia_ <= hist[-1] + slack
    want = float(ref.inertia(X, km.cluster_centers_))
    assert abs(km.inertia_ - want) <= 1e-10 * want
    assert np.array_equal(km.predict(X), km.labels_)
    T = km.transform(X[:100])
    np.testing.assert_allclose(T, np.sqrt(ref.distances(X[:100], km.cluster_centers_).astype(np.float64)), rtol=1e-9, atol=1e-9)
    assert np.array_equal(T.argmin(1), km.labels_[:100])


def test_kmeans_same_seed_same_bits(blob_fit):
    from meld_amd import KMeans

    X, truth, km = blob_fit
    again = KMeans(80, random_state=0).fit(torch.from_numpy(X).cuda())  # (a device tensor goes in as it is)
    assert np.array_equal(again.labels_, km.labels_)
    assert np.array_equal(again.cluster_centers_.view(np.uint64), km.cluster_centers_.view(np.uint64))
    assert np.array_equal(again.inertia_history_, km.inertia_history_) and again.inertia_ == km.inertia_
    import pandas as pd

    assert np.array_equal(KMeans(80, random_state=0).fit_predict(pd.DataFrame(X)), km.labels_)


def test_kmeans_from_given_centres_is_the_reference_step():
    from meld_amd import KMeans

    rng = np.random.default_rng(21)
    X = rng.standard_normal((1500, 12))
    C0 = X[rng.choice(1500, 30, replace=False)].copy()
    C0[7] = 50.0  # (a centre no point is nearest to: it keeps its place)
    lab, C1, inertia = ref.lloyd_step(X, C0)
    assert int((ref.gaps(ref.distances(X, C0)) <= 2 * ref.tau(X, C0)).sum()) == 0
    km = KMeans(30, init=C0, max_iter=0).fit(X)
    assert km.n_iter_ == 0 and np.array_equal(km.labels_, lab) and np.array_equal(km.cluster_centers_, C0)
    km = KMeans(30, init=C0, max_iter=1).fit(X)
    assert km.n_iter_ == 1 and km.inertia_history_.shape == (1,)
    assert abs(km.inertia_history_[0] - float(inertia)) <= float(ref.tau(X, C0).sum())
    np.testing.assert_allclose(km.cluster_centers_, C1.astype(np.float64), rtol=1e-13, atol=1e-13)
    assert np.array_equal(km.cluster_centers_[7], C0[7])
    with pytest.raises(ValueError, match="columns"):
        KMeans(30, init=C0).fit(X[:, :5])
    with pytest.raises(ValueError, match="fewer than n_clusters"):
        KMeans(30).fit(X[:20])


def test_kmeans_wider_than_the_kernel_runs_on_the_library():
    from meld_amd import KMeans

    rng = np.random.default_rng(22)
    truth = np.repeat(np.arange(6), 40)
    X = rng.standard_normal((240, 130)) + 30.0 * np.eye(6, 130)[truth]
    km = KMeans(6, random_state=0, n_init=2).fit(X)
    assert km.info_["lloyd"] == "library"
    assert len(set(zip(truth.tolist(), km.labels_.tolist()))) == 6
    assert np.array_equal(km.predict(X), km.labels_)


def _steps(Yd, k):
    from meld_amd import kmeans

    return {"lds": kmeans.lds_step(Yd, k), "wide": kmeans.lloyd_step, "library": kmeans.library_step}


def test_the_three_back_ends_agree_on_one_step():
    """One step of every back end through the common signature on 1,001 points (no multiple of 256), d = 7, k = 5, one centre that
    no point is nearest to.  No point of the case is within ``2 tau`` of a tie (tests/test_kmeans_reference.py), so every label
    is compared.  Centres: 1e-12, the bound tests/test_gpu_cluster.py holds the LDS and library steps to; inertia: 1e-9 relative."""
    Y, C = ref.step_case()
    want = ref.argmin_lowest(ref.distances(Y, C))
    Yd, Cd = _dev(Y), _dev(C)
    out = {name: step(Yd, Cd) for name, step in _steps(Yd, 5).items()}
    newC, inertia, lab = out["wide"]
    for name, (newC_b, inertia_b, lab_b) in out.items():
        print(name, "largest centre difference to wide", float((newC_b - newC).abs().max()), "inertia", float(inertia_b))
        assert lab_b.dtype == torch.int32 and np.array_equal(lab_b.cpu().numpy(), want), name
        assert torch.allclose(newC_b, newC, rtol=1e-12, atol=1e-12), name
        assert torch.equal(newC_b[4], Cd[4]), name  # (the empty cluster keeps its centre, bit for bit)
        assert abs(float(inertia_b) - float(inertia)) <= 1e-9 * float(inertia), name
    np.testing.assert_allclose(newC.cpu().numpy(), ref.lloyd_step(Y, C)[1].astype(np.float64), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("backend", ["lds", "wide", "library"])
def test_lloyd_over_every_step(backend):
    """``lloyd`` with ``max_iter`` 0, 1 and 20 on the case above: the step count follows ``max_iter`` and the stopping rule (looked
    at after steps 8 and 16 only; the plain loop below says where it holds), the history has one entry per step, the labels and the
    inertia are those of the returned centres; the wide back end gives the same bits twice."""
    from meld_amd.kmeans import CHECK_EVERY, lloyd, lloyd_step

    Y, C = ref.step_case()
    Yd, Cd = _dev(Y), _dev(C)
    step = _steps(Yd, 5)[backend]
    var_tol = 1e-4 * float(np.var(Y, axis=0).mean())
    Cs, expected = Cd, {0: 0, 1: 1, 20: 20}
    for it in range(20):
        newC = lloyd_step(Yd, Cs)[0]
        shift, Cs = float(((newC - Cs) ** 2).sum()), newC
        if it % CHECK_EVERY == CHECK_EVERY - 1:
            assert not 0.5 * var_tol < shift < 2.0 * var_tol  # (far from the threshold: rounding cannot move the stop)
            if shift <= var_tol:
                expected[20] = it + 1
                break
    assert expected[20] == 8  # (four separate blobs: settled long before the first look)
    for max_iter, steps in expected.items():
        run = lloyd(Yd, Cd, step, max_iter=max_iter, tol=1e-4)
        centres = run["centres"].cpu().numpy()
        assert run["iterations"] == steps and tuple(run["history"].shape) == (steps,) and run["history"].dtype == torch.float64
        assert int((ref.gaps(ref.distances(Y, centres)) <= 2 * ref.tau(Y, centres)).sum()) == 0
        assert run["labels"].dtype == torch.int32
        assert np.array_equal(run["labels"].cpu().numpy(), ref.argmin_lowest(ref.distances(Y, centres)))
        want = float(ref.inertia(Y, centres))
        assert abs(run["inertia"] - want) <= 1e-9 * want
        assert np.array_equal(centres[4], C[4])
        if max_iter == 0:
            assert np.array_equal(centres, C)
        if backend == "wide":
            again = lloyd(Yd, Cd, step, max_iter=max_iter, tol=1e-4)
            assert torch.equal(again["centres"], run["centres"]) and torch.equal(again["labels"], run["labels"])
            assert torch.equal(again["history"], run["history"]) and again["inertia"] == run["inertia"]


@pytest.mark.parametrize("which", ["overlapping", "uniform"])
def test_quality_against_the_parent_kmeans(which):
    """The yardstick is the parent route, ``kmeans_device`` with k-means++ seeding and the LDS step preferred (here: the library Lloyd
    step), with seeds 0-4: the device route with seed 0 may not exceed its worst inertia by more than its own spread over the seeds."""
    from meld_amd import KMeans
    from meld_amd.kmeans import kmeans_device

    X = ref.overlapping_blobs() if which == "overlapping" else ref.uniform_noise()
    Xd = _dev(X)
    parent = []
    for seed in range(5):
        info = {}
        kmeans_device(Xd, 100, n_init=1, max_iter=300, tol=1e-4, seed=seed, info=info, seeding="k-means++", prefer="lds")
        parent.append(info["inertia"])
    km = KMeans(100, random_state=0).fit(Xd)
    print("quality[{}]: parent min {:.6g} max {:.6g}, device {:.6g}, device / parent max {:.5f}, device / parent min {:.5f}".format(
        which, min(parent), max(parent), km.inertia_, km.inertia_ / max(parent), km.inertia_ / min(parent)))
    assert km.inertia_ <= max(parent) + (max(parent) - min(parent))


@pytest.fixture(scope="module")
def cells():
    import meld_amd

    X = np.random.default_rng(31).standard_normal((3000, 10))
    return meld_amd.MELD(knn=5, verbose=False).fit(X)


def test_landmarks_by_the_device_route(cells, monkeypatch):
    import meld_amd.kmeans

    def not_this_one(*a, **kw):
        raise AssertionError("kmeans='device' must not run the k-means++ seeder")

    G = cells.graph
    with monkeypatch.context() as m:
        m.setattr(meld_amd.kmeans, "seed_plusplus", not_this_one)
        lm = G.landmarks(200, random_state=1, kmeans="device")
        with pytest.raises(AssertionError, match="must not run"):  # (and the default route does run it)
            G.landmarks(199, random_state=1)
    print("landmarks(200, kmeans='device'):", lm.info)
    L = lm.n_landmark
    assert 1 <= L <= 200 and np.array_equal(np.unique(lm.clusters), np.arange(L))
    np.testing.assert_allclose(lm.landmark_op.astype(LD).sum(1).astype(np.float64), 1.0, rtol=1e-12)
    assert lm.info["kmeans"] == "device" and lm.info["kmeans_iterations"] >= 1
    assert lm is G.landmarks(200, random_state=1, kmeans="device")
    again = G.landmarks(200, random_state=1, kmeans="device", recompute=True)
    assert again is not lm and np.array_equal(again.clusters, lm.clusters)


def test_landmarks_library_keyword_is_the_default(cells):
    G = cells.graph
    default = G.landmarks(200, random_state=1)
    assert G.landmarks(200, random_state=1, kmeans="library") is default and "kmeans" not in default.info
    assert G.landmarks(200, random_state=1, kmeans="device") is not default
    fresh = G.landmarks(200, random_state=1, kmeans="library", recompute=True)
    assert np.array_equal(fresh.clusters, default.clusters)
    with pytest.raises(ValueError, match="kmeans must be"):
        cells.landmarks(n_landmark=200, kmeans="hip")


def test_device_route_recovers_separate_blobs():
    import meld_amd

    rng = np.random.default_rng(8)
    truth = np.repeat(np.arange(4), 200)
    X = rng.normal(size=(800, 10)) + 40.0 * np.eye(4, 10)[truth]
    order = rng.permutation(800)
    X, truth = X[order], truth[order]
    op = meld_amd.MELD(knn=5, n_landmark=50, verbose=False).fit(X)
    lm = op.landmarks(n_landmark=4, random_state=0, kmeans="device")
    assert lm.n_landmark == 4 and lm.info["kmeans"] == "device"
    assert len(set(zip(truth.tolist(), lm.clusters.tolist()))) == 4


def test_phate_by_the_device_route(cells):
    emb = cells.phate(n_landmark=200, kmeans="device", t=5)
    Z = np.asarray(emb)
    assert Z.shape == (3000, 2) and np.isfinite(Z).all()
