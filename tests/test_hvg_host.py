"""The host side of the highly-variable-gene functions of meld_amd/preprocess.py: the rule itself against tests/hvg_reference.py, bit
for bit, and the argument checks, which raise before any device call (no GPU: a call that got as far as the device would fail here
with another error)."""
import numpy as np
import pytest
from scipy import sparse

from meld_amd import preprocess as pp
from tests import hvg_reference as hvg
from tests import preprocess_reference as ref


@pytest.fixture(scope="module")
def X():
    return sparse.random(20, 30, density=0.2, format="csr", random_state=np.random.default_rng(0))


@pytest.fixture(scope="module")
def moments():
    m = hvg.moments_long(ref.standard_matrix())
    tied_mean = np.repeat(np.arange(40, dtype=np.float64), 5)[np.random.default_rng(2).permutation(200)]
    tied_var = np.random.default_rng(3).gamma(2.0, size=200)
    return {"standard": (m.mean.astype(np.float64), m.var.astype(np.float64)), "tied": (tied_mean, tied_var)}


def test_new_names_are_public():
    for name in ("gene_moments_device", "gene_mean", "gene_variance", "variability_from_moments", "gene_variability", "highly_variable_genes"):
        assert name in pp.__all__ and callable(getattr(pp, name))


@pytest.mark.parametrize("smooth", [0, 5])
@pytest.mark.parametrize("kernel_size", [0.005, 0.05, 7])
@pytest.mark.parametrize("which", ["standard", "tied"])
def test_variability_has_the_bits_of_the_reference(moments, which, kernel_size, smooth):
    mean, var = moments[which]
    if which == "tied":
        assert np.unique(mean).shape[0] < mean.shape[0]
    got = pp.variability_from_moments(mean, var, kernel_size, smooth)
    want = hvg.variability(mean, var, kernel_size, smooth)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.abs(want).max() > 0 or hvg.kernel_length(kernel_size, mean.shape[0]) == 1


def test_selection_rules_have_the_reference_answers(moments):
    v = hvg.variability(*moments["standard"], 0.05, 5)
    for rule, kw in ((("n_top_genes", 50), dict(n_top_genes=50)), (pp._hvg_rule("f", 0.01, None, None), dict(cutoff=0.01)),
                     (pp._hvg_rule("f", None, 80, None), dict(percentile=80))):
        mask, cut = pp._hvg_keep("f", v, rule)
        kept, cut_ref = hvg.select_genes(v, **kw)
        assert np.array_equal(np.flatnonzero(mask), kept) and cut == cut_ref and 0 < len(kept) < 500
    tied = np.array([1.0, 3.0, 3.0, 0.0, 3.0])
    assert np.flatnonzero(pp._hvg_keep("f", tied, ("n_top_genes", 2))[0]).tolist() == [1, 2]


@pytest.mark.parametrize("kwargs", [dict(cutoff=1.0, n_top_genes=5), dict(cutoff=1.0, percentile=50), dict(percentile=50, n_top_genes=5),
                                    dict(percentile=None)])
def test_exactly_one_rule(X, kwargs):
    with pytest.raises(ValueError, match="highly_variable_genes.*exactly one"):
        pp.highly_variable_genes(X, **kwargs)
    run_kwargs = {{"cutoff": "hvg_cutoff", "percentile": "hvg_percentile"}.get(k, k): v for k, v in kwargs.items()}
    if len([v for v in kwargs.values() if v is not None]) == 2:
        with pytest.raises(ValueError, match=r"run \(highly_variable_genes\).*exactly one"):
            pp.run(X, **run_kwargs)


def test_even_kernels_and_bad_smoothing(X):
    for bad in (4, 0, -3, 0.0, 1.5, "wide"):
        with pytest.raises(ValueError, match="kernel_size"):
            pp.gene_variability(X, kernel_size=bad)
        with pytest.raises(ValueError, match="kernel_size"):
            pp.highly_variable_genes(X, kernel_size=bad)
        with pytest.raises(ValueError, match="kernel_size"):
            pp.run(X, n_top_genes=5, hvg_kernel_size=bad)
        with pytest.raises(ValueError, match="kernel_size"):
            pp.variability_from_moments(np.arange(9.0), np.arange(9.0), bad)
    with pytest.raises(ValueError, match="smooth"):
        pp.gene_variability(X, smooth=-1)
    with pytest.raises(ValueError, match="smooth"):
        pp.run(X, hvg_percentile=80, hvg_smooth=1.5)
    with pytest.raises(ValueError, match="one length"):
        pp.variability_from_moments(np.arange(9.0), np.arange(8.0))


@pytest.mark.parametrize("n", [0, -1, 31, 2.5])
def test_n_top_genes_out_of_range(X, n):
    with pytest.raises(ValueError, match="n_top_genes"):
        pp.highly_variable_genes(X, n_top_genes=n)
    with pytest.raises(ValueError, match="n_top_genes"):
        pp.run(X, n_top_genes=n)


def test_ddof_percentile_and_value_map(X):
    for bad in (2, -1, 0.5, True):
        with pytest.raises(ValueError, match="ddof"):
            pp.gene_variance(X, ddof=bad)
        with pytest.raises(ValueError, match="ddof"):
            pp.gene_moments_device(X, ddof=bad)
    for bad in (101, -1):
        with pytest.raises(ValueError, match="percentile"):
            pp.highly_variable_genes(X, percentile=bad)
        with pytest.raises(ValueError, match="percentile"):
            pp.run(X, hvg_percentile=bad)
    with pytest.raises(ValueError, match="highly_variable_genes"):
        pp.highly_variable_genes(X, percentile=(20, 80))
    with pytest.raises(ValueError, match="unknown transform"):
        pp.gene_moments_device(X, transform="cube root")
    with pytest.raises(ValueError, match="cofactor"):
        pp.gene_moments_device(X, transform="arcsinh", cofactor=0)
    with pytest.raises(ValueError, match="rescale"):
        pp.gene_moments_device(X, rescale="median")
