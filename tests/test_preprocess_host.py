"""Argument validation of meld_amd/preprocess.py that raises before any device call (no GPU: a call that got as far as the device
would fail here with another error)."""
import numpy as np
import pytest
from scipy import sparse

import meld_amd
from meld_amd import preprocess as pp


@pytest.fixture(scope="module")
def X():
    return sparse.random(20, 30, density=0.2, format="csr", random_state=np.random.default_rng(0))


def test_module_is_reachable_lazily():
    assert meld_amd.preprocess is pp
    assert "preprocess" in meld_amd.__all__


@pytest.mark.parametrize("kwargs", [dict(), dict(cutoff=10, percentile=5), dict(cutoff=(1, 2, 3)), dict(percentile=101)])
def test_exactly_one_of_cutoff_and_percentile(X, kwargs):
    with pytest.raises(ValueError, match="filter_library_size"):
        pp.filter_library_size(X, **kwargs)
    with pytest.raises(ValueError, match="filter_gene_set_expression"):
        pp.filter_gene_set_expression(X, [0, 1], **kwargs)


def test_unknown_keep_cells(X):
    with pytest.raises(ValueError, match="keep_cells"):
        pp.filter_library_size(X, cutoff=3, keep_cells="around")
    with pytest.raises(ValueError, match="between"):
        pp.filter_library_size(X, cutoff=3, keep_cells="between")


def test_log_takes_pseudocount_one_only(X):
    with pytest.raises(ValueError, match="pseudocount"):
        pp.log(X, pseudocount=0.5)
    with pytest.raises(ValueError, match="base"):
        pp.log(X, base=3)


def test_unknown_transform_and_rescale(X):
    with pytest.raises(ValueError, match="unknown transform"):
        pp.run(X, transform="cube root")
    with pytest.raises(ValueError, match="rescale"):
        pp.run(X, rescale="mode")
    with pytest.raises(ValueError, match="rescale"):
        pp.library_size_normalize(X, rescale="mode")
    with pytest.raises(ValueError, match="not both"):
        pp.run(X, min_library_size=5, library_size_percentile=10)
    with pytest.raises(ValueError, match="cofactor"):
        pp.arcsinh(X, cofactor=0)


def test_rules_resolve_as_scprep_does():
    assert pp._cutoff_rule("f", 5, None, "above") == ("cutoff", 5.0, "above")
    assert pp._cutoff_rule("f", None, (5, 95), "above") == ("percentile", [5.0, 95.0], "between")
    v = np.array([1.0, 2.0, 3.0, 4.0])
    assert pp._keep_mask(v, "cutoff", 2.0, "above")[0].tolist() == [False, False, True, True]
    assert pp._keep_mask(v, "cutoff", 2.0, "below")[0].tolist() == [True, False, False, False]
    assert pp._keep_mask(v, "cutoff", [1.0, 4.0], "between")[0].tolist() == [False, True, True, False]
    mask, cut = pp._keep_mask(v, "percentile", 50.0, "above")
    assert cut == 2.5 and mask.tolist() == [False, False, True, True]
