"""The host restatement of the preprocessing (tests/preprocess_reference.py) against independent implementations: sklearn's
``normalize``, scipy's slicing and comparison operators.  No GPU."""
import numpy as np
import pytest
from scipy import sparse

from tests import preprocess_reference as ref


@pytest.fixture(scope="module")
def X():
    return ref.standard_matrix()


def test_standard_matrix_is_not_trivial(X):
    N, G = X.shape
    assert (N, G) == (300, 500) and X.has_canonical_format
    lens = np.diff(X.indptr)
    assert round(100.0 * X.nnz / (N * G), 1) == 7.4 and (lens.min(), lens.max()) == (10, 104)
    assert (X.data == np.round(X.data)).all() and X.data.min() >= 1 and X.data.max() > 3
    Y, cells = ref.filter_library_size(X, percentile=10)
    Z, genes = ref.filter_rare_genes(Y, min_cells=5)
    assert (len(cells), len(genes)) == (268, 331)
    assert np.diff(Z.indptr).min() > 0  # no kept cell loses every gene
    out = ref.run(X, library_size_percentile=10, min_cells=5)
    assert out.data.shape == (268, 331) and np.array_equal(out.cells, cells) and np.array_equal(out.genes, genes)
    # the capture counts over the kept cells differ from those over all cells: the order of the two filters matters
    assert (ref.gene_capture_count(X) != ref.gene_capture_count(Y)).any()


@pytest.mark.parametrize("rescale", [10000, 1, "median", "mean"])
def test_normalisation_has_sklearns_bits(X, rescale):
    from sklearn.preprocessing import normalize

    got, lib = ref.library_size_normalize(X, rescale, return_library_size=True)
    r = ref.rescale_value(rescale, np.asarray(X.sum(axis=1)).ravel())
    want = normalize(X, "l1") * r
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(got.data.view(np.uint64), want.data.view(np.uint64))
    assert np.array_equal(lib, np.asarray(X.sum(axis=1)).ravel())


def test_normalisation_leaves_a_row_without_magnitude_alone():
    from sklearn.preprocessing import normalize

    A = sparse.csr_matrix((np.array([0.0, 0.0, 3.0, -1.0]), np.array([0, 2, 1, 3]), np.array([0, 2, 2, 4])), shape=(3, 4))
    got = ref.library_size_normalize(A, 100.0)
    want = normalize(A, "l1") * 100.0
    assert np.array_equal(got.data.view(np.uint64), want.data.view(np.uint64))
    assert np.array_equal(got.data, [0.0, 0.0, 75.0, -25.0])
    assert np.array_equal(ref.library_size(A), [0.0, 0.0, 2.0])  # the plain sum, not the norm


def test_selection_is_scipys_slicing(X):
    rng = np.random.default_rng(1)
    rows = np.sort(rng.choice(X.shape[0], 120, replace=False))
    cols = np.sort(rng.choice(X.shape[1], 60, replace=False))
    for r, c, want in ((rows, cols, X[rows][:, cols]), (rows, None, X[rows]), (None, cols, X[:, cols])):
        got = ref.select(X, r, c)
        want.sort_indices()
        assert got.shape == want.shape
        assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices) and np.array_equal(got.data, want.data)
    rare = np.sort(np.argsort(ref.gene_capture_count(X), kind="stable")[:40])  # the 40 rarest genes: kept cells lose all their entries
    got, want = ref.select(X, rows, rare), X[rows][:, rare]
    assert (np.diff(got.indptr) == 0).any() and got.nnz > 0
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices) and np.array_equal(got.data, want.data)


@pytest.mark.parametrize("cutoff", [0, 1, 2.5])
def test_capture_counts(X, cutoff):
    want = np.asarray((X > cutoff).sum(axis=0)).ravel()
    assert np.array_equal(ref.gene_capture_count(X, cutoff), want)
    rows = np.arange(X.shape[0]) % 3 != 0
    assert np.array_equal(ref.gene_capture_count(X, cutoff, rows=rows), np.asarray((X[rows] > cutoff).sum(axis=0)).ravel())


def test_gene_set_expression(X):
    genes = np.arange(0, 500, 7)
    want = np.asarray(X[:, genes].sum(axis=1)).ravel()
    assert np.array_equal(ref.gene_set_expression(X, genes), want)
    mask = np.zeros(500, dtype=bool)
    mask[genes] = True
    assert np.array_equal(ref.gene_set_expression(X, mask), want)


def test_comparisons_are_strict_at_the_cutoff(X):
    lib = ref.library_size(X)
    cut = float(np.sort(lib)[100])
    n_eq = int((lib == cut).sum())
    assert n_eq >= 1
    above = ref.filter_library_size(X, cutoff=cut, keep_cells="above")[1]
    below = ref.filter_library_size(X, cutoff=cut, keep_cells="below")[1]
    assert len(above) + len(below) + n_eq == X.shape[0]
    assert (lib[above] > cut).all() and (lib[below] < cut).all()
    lo, hi = float(np.sort(lib)[50]), float(np.sort(lib)[250])
    between = ref.filter_library_size(X, cutoff=(lo, hi))[1]
    assert np.array_equal(between, np.flatnonzero((lib > lo) & (lib < hi))) and lo not in lib[between] and hi not in lib[between]
    # a percentile is numpy's, and the rule stays strict
    kept = ref.filter_library_size(X, percentile=10)[1]
    assert np.array_equal(kept, np.flatnonzero(lib > np.percentile(lib, 10)))
    with pytest.raises(ValueError):
        ref.filter_library_size(X, cutoff=1, percentile=10)
    with pytest.raises(ValueError):
        ref.filter_library_size(X)


def test_transforms_and_long_sums(X):
    assert np.array_equal(ref.sqrt(X).data, np.sqrt(X.data))
    assert np.array_equal(ref.log(X, base=2).data, np.log2(X.data + 1.0))
    assert np.array_equal(ref.arcsinh(X, 5).data, np.arcsinh(X.data / 5.0))
    s, a, count, m = ref.row_stats_long(X)
    assert np.array_equal(s.astype(np.float64), ref.library_size(X)) and np.array_equal(a, s)
    assert np.array_equal(count, np.diff(X.indptr)) and np.array_equal(m, np.diff(X.indptr))
