"""tests/hvg_reference.py checks itself against numpy and scipy (no device, no import of meld_amd)."""
import numpy as np
import pytest
from scipy.signal import medfilt

from tests import hvg_reference as hvg
from tests import preprocess_reference as ref


@pytest.fixture(scope="module")
def X():
    return ref.standard_matrix()


@pytest.mark.parametrize("ddof", [0, 1])
def test_moments_agree_with_numpy_on_the_dense_matrix(X, ddof):
    D = X.toarray()
    m = hvg.moments_long(X, ddof=ddof)
    assert np.array_equal(m.count, (D != 0).sum(axis=0)) and m.n_kept == 300
    assert np.allclose(m.mean.astype(np.float64), D.mean(axis=0), rtol=1e-12, atol=0)
    assert np.allclose(m.var.astype(np.float64), D.var(axis=0, ddof=ddof), rtol=1e-12, atol=0)
    assert np.allclose(m.abs_sum.astype(np.float64), np.abs(D).sum(axis=0), rtol=1e-12, atol=0)
    assert np.allclose(m.ss.astype(np.float64), ((D - D.mean(axis=0)) ** 2).sum(axis=0), rtol=1e-12, atol=0)


def test_moments_with_cells_dropped_values_mapped_and_genes_masked(X):
    rng = np.random.default_rng(1)
    keep = rng.random(300) < 0.7
    scale = ref.abs_library_size(X)
    scale[np.flatnonzero(keep)[0]] = 0.0  # a kept cell without a scale keeps its values, rescale still multiplies
    gmask = rng.random(500) < 0.8
    m = hvg.moments_long(X, keep, scale, 1e4, "sqrt", 5.0, gmask, 1)
    safe = np.where(scale == 0, 1.0, scale)
    D = np.sqrt((X.toarray() / safe[:, None]) * 1e4)[keep]
    first = X.toarray()[np.flatnonzero(keep)[0]]
    assert first.sum() > 0 and np.array_equal(D[0], np.sqrt(first * 1e4))
    assert np.array_equal(m.count[gmask], (D != 0).sum(axis=0)[gmask]) and (m.count[~gmask] == -1).all()
    assert np.allclose(m.mean.astype(np.float64)[gmask], D.mean(axis=0)[gmask], rtol=1e-12, atol=0)
    assert np.allclose(m.var.astype(np.float64)[gmask], D.var(axis=0, ddof=1)[gmask], rtol=1e-12, atol=0)
    assert (m.mean[~gmask] == 0).all() and (m.var[~gmask] == 0).all()
    eta, tol = hvg.moment_bounds(m)
    assert (eta[~gmask] == 0).all() and (eta[gmask & (m.count > 0)] > 0).all() and float(tol.max()) < 1e-10


def test_rolling_median_and_smoothing_on_nine_genes():
    """Worked by hand.  Sorted by mean the variances are y = 1 5 2 8 3 9 4 7 6; the median of three with zeros beyond the ends is
    1 2 5 3 8 4 7 6 6; one three-point mean with the ends replicated gives 4/3 8/3 10/3 16/3 5 19/3 17/3 19/3 6; y minus that is
    -1/3 7/3 -4/3 8/3 -2 8/3 -5/3 2/3 0, scattered back to the genes' own order."""
    mean = np.array([3.0, 0.0, 8.0, 1.0, 6.0, 2.0, 7.0, 4.0, 5.0])
    var = np.array([8.0, 1.0, 6.0, 5.0, 4.0, 2.0, 7.0, 3.0, 9.0])
    order = np.argsort(mean)
    assert var[order].tolist() == [1, 5, 2, 8, 3, 9, 4, 7, 6]
    assert medfilt(var[order], 3).tolist() == [1, 2, 5, 3, 8, 4, 7, 6, 6]
    assert hvg.smooth_once(np.array([1.0, 2, 5, 3, 8, 4, 7, 6, 6])).tolist() == pytest.approx([4 / 3, 8 / 3, 10 / 3, 16 / 3, 5, 19 / 3, 17 / 3, 19 / 3, 6], abs=1e-15)
    want = np.array([8 / 3, -1 / 3, 0, 7 / 3, -5 / 3, -4 / 3, 2 / 3, -2, 8 / 3])
    got = hvg.variability(mean, var, kernel_size=3, smooth=1)
    assert np.abs(got - want).max() <= 4e-15
    # a fraction of the genes gives the next odd length: 0.4 * 9 = 3.6 -> 3; 0.005 * 9 -> 1, the identity, and then nothing is left
    assert hvg.kernel_length(0.4, 9) == 3 and hvg.kernel_length(0.005, 9) == 1 and hvg.kernel_length(0.05, 500) == 25
    assert np.array_equal(hvg.variability(mean, var, kernel_size=0.4, smooth=1), got)
    assert np.array_equal(hvg.variability(mean, var, kernel_size=0.005, smooth=0), np.zeros(9))
    with pytest.raises(ValueError):
        hvg.kernel_length(4, 9)


def test_equal_means_go_to_the_lower_gene_index():
    """means 2 1 1 1 0: sorted order 4 1 2 3 0 (the three equal ones by index), y = 7 1 9 3 5, medians 1 7 3 5 3"""
    mean = np.array([2.0, 1.0, 1.0, 1.0, 0.0])
    var = np.array([5.0, 1.0, 9.0, 3.0, 7.0])
    assert hvg.variability(mean, var, kernel_size=3, smooth=0).tolist() == [2.0, -6.0, 6.0, -2.0, 6.0]


def test_the_three_rules_and_their_ties():
    v = np.array([1.0, 3.0, 3.0, 0.0, 3.0])
    assert hvg.select_genes(v, n_top_genes=2)[0].tolist() == [1, 2] and hvg.select_genes(v, n_top_genes=2)[1] == 3.0
    assert hvg.select_genes(v, n_top_genes=3)[0].tolist() == [1, 2, 4]
    assert hvg.select_genes(v, n_top_genes=4)[0].tolist() == [0, 1, 2, 4]
    assert hvg.select_genes(v, cutoff=3.0)[0].tolist() == [] and hvg.select_genes(v, cutoff=1.0)[0].tolist() == [1, 2, 4]  # strict
    kept, cut = hvg.select_genes(v, percentile=50)
    assert cut == 3.0 and kept.tolist() == []
    assert hvg.select_genes(v, percentile=25)[0].tolist() == [1, 2, 4]
    for bad in (dict(), dict(cutoff=1.0, n_top_genes=2), dict(n_top_genes=0), dict(n_top_genes=6)):
        with pytest.raises(ValueError):
            hvg.select_genes(v, **bad)


def test_run_with_hvg_selects_from_the_step_by_step_matrix(X):
    out = hvg.run_with_hvg(X, n_top_genes=50, library_size_percentile=10, min_cells=5, rescale=10000, transform="sqrt")
    assert out.data.shape == (268, 50) and out.full.data.shape == (268, 331) and len(out.genes) == 50
    assert np.array_equal(out.genes, out.genes_before[out.kept]) and (np.diff(out.genes) > 0).all()
    assert (out.data != out.full.data[:, out.kept]).nnz == 0
    D = out.full.data.toarray()
    assert np.allclose(out.moments.var.astype(np.float64), D.var(axis=0, ddof=1), rtol=1e-12, atol=0)
    assert out.variability[out.kept].min() == out.cutoff and (np.delete(out.variability, out.kept) < out.cutoff).all()
