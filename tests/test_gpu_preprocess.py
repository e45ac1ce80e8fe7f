"""Preprocessing on the device CSR (meld_amd/preprocess.py, csrc/preprocess.hip) against the host restatement
(tests/preprocess_reference.py, itself checked against scipy and sklearn): the row statistics, the column counts, the rewrite,
the value map, the fused route against the step-by-step calls, and the result handed to MELD and to the rank-sum test.

Paths of the kernels the shapes below are chosen for.  ``meld_prep_row_stats`` takes a wave per row for EVERY matrix -- there is no
lane-group choice and so no boundary in ``nnz / n_rows``; its plain form runs a four-deep unrolled loop while at least 193 entries
are left (all lanes from 256 on) and the masked form drains a 128-slot ring whenever 64 counted entries are pending: lengths 63 /
64 / 65, 127 / 128 / 129, 192 / 193 and 255 / 256 / 257 sit on those edges.  ``meld_prep_col_counts`` gives a workgroup a contiguous
range of rows (one workgroup up to 16 rows, 256 workgroups from 4,081 rows on) and runs one launch per panel of
``meld_prep_panel_cols()`` columns."""
import numpy as np
import pytest
from scipy import sparse

from tests import preprocess_reference as ref

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256, 257, 1000, 0, 1200]
G_ROWS = 1200


def _pp():
    from meld_amd import preprocess

    return preprocess


def _dev(X):
    from meld_amd.sparse import DeviceCSR

    return DeviceCSR.from_input(X)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_csr(A, S, bits=True):
    """a DeviceCSR against a scipy CSR: structure equal, values bit for bit"""
    assert A.shape == S.shape
    assert np.array_equal(A.rowptr.cpu().numpy(), S.indptr), "rowptr"
    assert np.array_equal(A.col.cpu().numpy(), S.indices), "col"
    if bits:
        assert np.array_equal(_bits(A.val.cpu().numpy()), _bits(S.data)), "val"


def _ulps(got, want):
    """the largest difference in units of the last place of the expected value"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - want) / np.spacing(np.abs(want))).max())


@pytest.fixture(scope="module")
def X():
    return ref.standard_matrix()


def _hand_built(kind, dtype, seed=3):
    """rows of the lengths above over 1,200 columns; stored zeros and negative entries; integer- or real-valued"""
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(LENGTHS)])
    indices = np.concatenate([np.sort(rng.choice(G_ROWS, n, replace=False)) for n in LENGTHS]).astype(np.int32)
    if kind == "int":
        data = rng.integers(-5, 10, size=indptr[-1]).astype(np.float64)
    else:
        data = rng.normal(size=indptr[-1]) * np.exp(rng.normal(size=indptr[-1]) * 3)
    data[rng.random(indptr[-1]) < 0.1] = 0.0
    A = sparse.csr_matrix((data.astype(dtype), indices, indptr), shape=(len(LENGTHS), G_ROWS))
    assert A.has_canonical_format and (A.data == 0).any() and (A.data < 0).any()
    return A


# ---- 1. row statistics ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("mask", [None, "random", "all", "none"])
def test_row_stats(kind, dtype, mask):
    import torch

    pp = _pp()
    A = _hand_built(kind, dtype)
    D = _dev(A)
    assert D.val.dtype == (torch.float32 if dtype == np.float32 else torch.float64) and D.nnz == A.nnz  # (stored zeros went up)
    rng = np.random.default_rng(5)
    m = {None: None, "random": rng.random(G_ROWS) < 0.6, "all": np.ones(G_ROWS, bool), "none": np.zeros(G_ROWS, bool)}[mask]
    md = None if m is None else torch.from_numpy(m).cuda()
    cutoff = 0.5
    s, a, c = (t.cpu().numpy() for t in pp.row_stats_device(D, md, cutoff))
    Aw = A.astype(np.float64)
    s_ref, a_ref, c_ref, n = ref.row_stats_long(Aw, m, cutoff)
    assert c.dtype == np.int32 and np.array_equal(c, c_ref)
    if mask == "random":
        assert (n < 64).any() and ((n > 64) & (n < 128)).any() and (n > 128).any()  # counted entries around both ring halves
    if kind == "int":
        assert np.array_equal(s, s_ref.astype(np.float64)) and np.array_equal(a, a_ref.astype(np.float64))
    else:
        bound = n * 2.0 ** -53 * a_ref
        err_s, err_a = np.abs(s.astype(np.longdouble) - s_ref), np.abs(a.astype(np.longdouble) - a_ref)
        print("row sums: largest error / bound = {:.3f} (sum), {:.3f} (abs_sum)".format(
            float((err_s[bound > 0] / bound[bound > 0]).max(initial=0)), float((err_a[bound > 0] / bound[bound > 0]).max(initial=0))))
        assert (err_s <= bound).all() and (err_a <= bound).all()
    s2, a2, c2 = (t.cpu().numpy() for t in pp.row_stats_device(D, md, cutoff))
    assert np.array_equal(_bits(s), _bits(s2)) and np.array_equal(_bits(a), _bits(a2)) and np.array_equal(c, c2)
    if mask == "all":  # the masked kernel numbers the counted entries as the plain one numbers all of them: equal bits
        s0, a0, c0 = (t.cpu().numpy() for t in pp.row_stats_device(D, None, cutoff))
        assert np.array_equal(_bits(s), _bits(s0)) and np.array_equal(_bits(a), _bits(a0)) and np.array_equal(c, c0)
    if mask == "random":  # ... and as the plain one numbers the entries of the matrix without the dropped columns
        B = pp.select(D, cols=np.flatnonzero(m))
        s0, a0, c0 = (t.cpu().numpy() for t in pp.row_stats_device(B, None, cutoff))
        assert np.array_equal(_bits(s), _bits(s0)) and np.array_equal(_bits(a), _bits(a0)) and np.array_equal(c, c0)


def test_measures_on_the_standard_matrix(X):
    pp = _pp()
    D = _dev(X)
    assert np.array_equal(pp.library_size(D), ref.library_size(X))
    assert np.array_equal(pp.library_size(X.astype(np.float32)), ref.library_size(X))
    genes = np.arange(0, 500, 7)
    assert np.array_equal(pp.gene_set_expression(D, genes), ref.gene_set_expression(X, genes))
    mask = np.zeros(500, bool)
    mask[genes] = True
    assert np.array_equal(pp.gene_set_expression(D, mask), ref.gene_set_expression(X, genes))
    assert np.array_equal(pp.library_size(X.toarray()), ref.library_size(X))  # dense input: compressed on the device
    back = D.to_scipy()
    assert (back != X).nnz == 0 and np.array_equal(back.indptr, X.indptr) and back.data.dtype == np.float64


# ---- 2. column counts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", ["all", "mask", "none"])
@pytest.mark.parametrize("cutoff", [0, 1])
def test_col_counts_standard(X, keep, cutoff):
    import torch

    pp = _pp()
    D = _dev(X)
    rows = {"all": None, "mask": np.arange(300) % 3 != 1, "none": np.zeros(300, bool)}[keep]
    got = pp.col_counts_device(D, None if rows is None else torch.from_numpy(rows).cuda(), cutoff).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, ref.gene_capture_count(X, cutoff, rows))
    if keep == "all":
        c = pp.gene_capture_count(D, cutoff)
        assert c.dtype == np.int64 and np.array_equal(c, ref.gene_capture_count(X, cutoff))
        assert np.array_equal(pp.gene_capture_count(X.astype(np.float32), cutoff), c)


def test_col_counts_across_the_panel_seam():
    from meld_amd._lib import get_lib

    pp = _pp()
    panel = get_lib().meld_prep_panel_cols()
    assert panel >= 30000 and panel * 4 <= 160 * 1024  # 30,000 genes are one panel, the panel fits the LDS of a CU
    G = panel + 1
    rng = np.random.default_rng(2)
    fixed = np.unique([0, panel - 1, panel, G - 1])  # (G - 1 is the one column of the second panel)
    rows = []
    for _ in range(64):
        extra = rng.choice(np.setdiff1d(np.arange(1, G - 1), fixed), 5, replace=False)
        rows.append(np.sort(np.concatenate([fixed, extra])))
    indices = np.concatenate(rows).astype(np.int32)
    A = sparse.csr_matrix((rng.integers(0, 4, size=indices.shape[0]).astype(np.float64), indices, np.arange(65) * 8), shape=(64, G))
    assert len(fixed) == 3 and A.has_canonical_format
    got = pp.col_counts_device(_dev(A), None, 0).cpu().numpy()
    want = ref.gene_capture_count(A, 0)
    assert np.array_equal(got, want) and want[[0, panel - 1, panel]].min() > 20


def test_col_counts_under_contention():
    import torch

    pp = _pp()
    rng = np.random.default_rng(4)
    N, G = 5000, 50
    dense = (rng.random((N, G)) < 0.08) * rng.integers(1, 4, size=(N, G))
    dense[:, 17] = 1 + rng.integers(0, 3, size=N)  # every row hits counter 17
    A = sparse.csr_matrix(dense.astype(np.float64))
    D = _dev(A)
    got = pp.col_counts_device(D, None, 0).cpu().numpy()
    assert got[17] == N and np.array_equal(got, ref.gene_capture_count(A, 0))
    keep = rng.random(N) < 0.5
    got = pp.col_counts_device(D, torch.from_numpy(keep).cuda(), 1).cpu().numpy()
    assert np.array_equal(got, ref.gene_capture_count(A, 1, keep))


# ---- 3. the rewrite -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_select_matches_scipy_slicing(X, dtype):
    pp = _pp()
    A = X.tolil()
    A[40, :] = 0  # an input row of length 0 that is kept
    A = A.tocsr().astype(dtype)
    A.sort_indices()
    cells = np.union1d(ref.filter_library_size(X, percentile=10)[1], [40])
    genes = ref.filter_rare_genes(X[ref.filter_library_size(X, percentile=10)[1]], min_cells=5)[1]
    rare = np.sort(np.argsort(ref.gene_capture_count(X), kind="stable")[:40])
    D = _dev(A)
    assert np.diff(A.indptr)[40] == 0
    for rows, cols in ((cells, genes), (cells, None), (None, genes), (None, None), (cells, rare), (np.array([40]), None)):
        want = A.astype(np.float64)
        want = want if rows is None else want[rows]
        want = want if cols is None else want[:, cols]
        got = pp.select(D, rows=rows, cols=cols)
        _same_csr(got, want)
        assert np.array_equal(got.to_scipy().data, want.data)
    lost = ref.select(A.astype(np.float64), cells, rare)
    assert (np.diff(lost.indptr)[np.diff(A.indptr)[cells] > 0] == 0).any()  # a kept row with entries loses all of them


def test_select_keeps_stored_zeros():
    pp = _pp()
    A = _hand_built("int", np.float64)
    cols = np.arange(0, G_ROWS, 2)
    want = ref.select(A, None, cols)
    got = pp.select(_dev(A), cols=cols)
    _same_csr(got, want)
    assert (want.data == 0).any()


# ---- 4. the value map -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescale", [10000, "median", "mean"])
def test_normalised_values_have_the_reference_bits(X, rescale):
    pp = _pp()
    got, lib = pp.library_size_normalize(_dev(X), rescale, return_library_size=True)
    want, lib_ref = ref.library_size_normalize(X, rescale, return_library_size=True)
    assert np.array_equal(lib, lib_ref)
    _same_csr(got, want)


def test_transforms_within_the_documented_bounds(X):
    """sqrt is correctly rounded on both sides up to 1 ulp; the logarithms and asinh are documented to 1 ulp by the device math
    library (HIP's table of double-precision functions) and by the host's libm each: 2 ulp between them.  No document installed
    with the toolchain states another bound."""
    pp = _pp()
    N = ref.library_size_normalize(X, 10000)
    D = pp.library_size_normalize(_dev(X), 10000)
    seen = {}
    for name, got, want, bound in (
        ("sqrt", pp.sqrt(D), ref.sqrt(N), 1), ("log e", pp.log(D, base="e"), ref.log(N, base="e"), 2),
        ("log2", pp.log(D, base=2), ref.log(N, base=2), 2), ("log10", pp.log(D), ref.log(N), 2),
        ("arcsinh", pp.arcsinh(D), ref.arcsinh(N), 2), ("arcsinh 150", pp.arcsinh(D, cofactor=150), ref.arcsinh(N, 150), 2),
    ):
        _same_csr(got, want, bits=False)
        seen[name] = _ulps(got.val.cpu().numpy(), want.data)
        print("largest difference, {}: {:.2f} ulp".format(name, seen[name]))
    assert seen["sqrt"] <= 1
    assert all(v <= 2 for v in seen.values()), seen
    with pytest.raises(ValueError, match="negative"):
        pp.sqrt(_dev(_hand_built("int", np.float64)))


def test_zero_scale_rows_and_the_normalised_output(X):
    import torch

    pp = _pp()
    # a row of stored zeros has no magnitude: sklearn leaves it alone
    A = sparse.csr_matrix((np.array([0.0, 0.0, 3.0, -1.0, 2.0]), np.array([0, 2, 1, 3, 0]), np.array([0, 2, 2, 4, 5])), shape=(4, 4))
    _same_csr(pp.library_size_normalize(_dev(A), 100.0), ref.library_size_normalize(A, 100.0))
    # the kernel's rule itself: scale 0 keeps v, rescale still multiplies
    scale = torch.tensor([2.0, 0.0, 0.0, 4.0], dtype=torch.float64, device="cuda")
    got = pp.select(_dev(A), scale=scale, rescale=3.0)
    assert np.array_equal(got.val.cpu().numpy(), [0.0, 0.0, 9.0, -3.0, 1.5])
    # out_val_norm: the normalised values of the unfused call, next to the transformed ones, one structure
    D = _dev(X)
    s, a, _ = pp.row_stats_device(D)
    data, norm = pp.select(D, scale=a, rescale=10000.0, transform="sqrt", keep_normalized=True)
    unfused = pp.library_size_normalize(D, 10000)
    assert norm.rowptr is data.rowptr and norm.col is data.col
    assert torch.equal(norm.val, unfused.val) and torch.equal(norm.col, unfused.col) and torch.equal(norm.rowptr, unfused.rowptr)
    assert torch.equal(data.val, pp.sqrt(unfused).val)


# ---- 5. the fused route ---------------------------------------------------------------------------------------------------------------------
def _step_by_step(pp, D, percentile, min_cells, rescale, transform):
    A, cells = pp.filter_library_size(D, percentile=percentile)
    B, genes = pp.filter_rare_genes(A, min_cells=min_cells)
    Nrm, lib = pp.library_size_normalize(B, rescale, return_library_size=True)
    T = {"sqrt": pp.sqrt, "log2": lambda M: pp.log(M, base=2), "arcsinh": pp.arcsinh}[transform](Nrm)
    return T, Nrm, cells, genes, lib


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("rescale,transform", [(10000, "sqrt"), ("median", "log2"), ("mean", "arcsinh")])
def test_run_equals_the_single_functions_and_the_reference(X, rescale, transform, real):
    import torch

    pp = _pp()
    if real:  # real-valued data: the sums round, and the fused route still has the bits of the single functions
        X = X.copy()
        X.data = X.data * np.exp(np.random.default_rng(9).normal(size=X.nnz))
    D = _dev(X)
    out = pp.run(D, library_size_percentile=10, min_cells=5, rescale=rescale, transform=transform)
    T, Nrm, cells, genes, lib = _step_by_step(pp, D, 10, 5, rescale, transform)
    assert np.array_equal(out.cells, cells) and np.array_equal(out.genes, genes) and out.cells.dtype == np.int64
    assert np.array_equal(_bits(out.library_size), _bits(lib))
    for a, b in ((out.data, T), (out.normalized, Nrm)):
        assert a.shape == b.shape and torch.equal(a.rowptr, b.rowptr) and torch.equal(a.col, b.col)
        assert torch.equal(a.val.view(torch.int64), b.val.view(torch.int64))
    assert out.normalized.rowptr is out.data.rowptr and out.normalized.col is out.data.col
    assert out.info["shape_before"] == (300, 500) and out.info["shape_after"] == out.data.shape and out.info["nnz_after"] == out.data.nnz
    assert out.cell_index is None and out.gene_names is None
    if not real:
        want = ref.run(X, library_size_percentile=10, min_cells=5, rescale=rescale, transform=transform)
        assert out.data.shape == (268, 331)
        assert np.array_equal(out.cells, want.cells) and np.array_equal(out.genes, want.genes)
        assert np.array_equal(out.library_size, want.library_size)
        _same_csr(out.normalized, want.normalized)
        _same_csr(out.data, want.data, bits=False)
        assert _ulps(out.data.val.cpu().numpy(), want.data.data) <= (1 if transform == "sqrt" else 2)
    slim = pp.run(D, library_size_percentile=10, min_cells=5, rescale=rescale, transform=transform, keep_normalized=False)
    assert slim.normalized is None and torch.equal(slim.data.val, out.data.val)


def test_run_with_cutoffs_and_labels(X):
    import pandas as pd

    pp = _pp()
    frame = pd.DataFrame(X.toarray(), index=["cell%d" % i for i in range(300)], columns=["g%d" % j for j in range(500)])
    out = pp.run(frame, min_library_size=20, max_library_size=80, min_cells=3, gene_cutoff=1, rescale=None, transform=None)
    want = ref.run(X, min_library_size=20, max_library_size=80, min_cells=3, gene_cutoff=1, rescale=None, transform=None)
    assert 0 < len(want.cells) < 300 and 0 < len(want.genes) < 500
    assert np.array_equal(out.cells, want.cells) and np.array_equal(out.genes, want.genes)
    _same_csr(out.data, want.data)
    assert list(out.cell_index) == ["cell%d" % i for i in want.cells] and list(out.gene_names) == ["g%d" % j for j in want.genes]
    assert list(out.normalized.gene_names) == list(out.gene_names)
    sp = pp.run(pd.DataFrame.sparse.from_spmatrix(X, index=frame.index, columns=frame.columns), min_library_size=20, min_cells=None)
    assert list(sp.cell_index) == ["cell%d" % i for i in sp.cells] and list(sp.gene_names) == list(frame.columns)
    assert sp.data.shape[1] == 500 and np.array_equal(sp.cells, ref.run(X, min_library_size=20, min_cells=None).cells)
    # names select a gene set where the matrix carries them
    assert np.array_equal(pp.gene_set_expression(frame, ["g3", "g10"]), ref.gene_set_expression(X, [3, 10]))
    kept = pp.filter_gene_set_expression(frame, ["g3", "g10"], cutoff=2)[1]
    assert np.array_equal(kept, ref.filter_gene_set_expression(X, [3, 10], cutoff=2)[1])


def test_filters_that_keep_nothing_raise(X):
    pp = _pp()
    D = _dev(X)
    with pytest.raises(ValueError, match="filter_library_size"):
        pp.run(D, min_library_size=1e9)
    with pytest.raises(ValueError, match="filter_rare_genes"):
        pp.run(D, min_cells=301)
    with pytest.raises(ValueError, match="filter_library_size"):
        pp.filter_library_size(D, cutoff=1e9)
    with pytest.raises(ValueError, match="filter_rare_genes"):
        pp.filter_rare_genes(D, min_cells=301)
    A, kept = pp.filter_empty_genes(D)
    assert np.array_equal(kept, ref.filter_empty_genes(X)[1]) and len(kept) < 500
    B, kept = pp.filter_empty_cells(D)
    assert len(kept) == 300


def test_entries_refuse_bad_arguments(X):
    from meld_amd._lib import get_lib

    lib = get_lib()
    D = _dev(X)
    p = D.rowptr.data_ptr()
    assert lib.meld_prep_row_stats(None, p, p, 0, 300, 500, None, 0.0, p, p, p, None) == -1
    assert lib.meld_last_error().decode().startswith("meld_prep_row_stats:")
    assert lib.meld_prep_row_stats(p, p, p, 2, 300, 500, None, 0.0, p, p, p, None) == -1
    assert lib.meld_prep_col_counts(p, p, p, 0, -1, 500, None, 0.0, p, None) == -1
    assert lib.meld_last_error().decode().startswith("meld_prep_col_counts:")
    assert lib.meld_prep_col_counts(p, p, p, 0, 300, 500, None, 0.0, None, None) == -1
    assert lib.meld_prep_select_count(p, p, 300, 500, None, 10, None, p, None) == -1
    assert lib.meld_prep_select_count(p, p, 300, 500, p, 0, None, p, None) == -1
    assert lib.meld_prep_select_fill(p, p, p, 0, 300, 500, p, 10, None, None, 1.0, 6, 5.0, p, p, p, None, None) == -1
    assert b"transform=6" in lib.meld_last_error()
    assert lib.meld_prep_select_fill(p, p, p, 0, 300, 500, p, 10, None, None, 1.0, 5, 0.0, p, p, p, None, None) == -1
    assert lib.meld_prep_select_fill(p, p, p, 0, 300, 500, p, 10, None, None, 1.0, 0, 5.0, p, None, p, None, None) == -1


# ---- 6. through the product -----------------------------------------------------------------------------------------------------------------
def test_preprocessed_matrix_goes_through_meld_and_the_rank_sum_test(X):
    import pandas as pd

    import meld_amd

    pp = _pp()
    out = pp.run(X, library_size_percentile=10, min_cells=5)
    rng = np.random.default_rng(0)
    labels = np.where(rng.random(300) > 0.5, "treat", "ctrl")[out.cells]
    dens = meld_amd.MELD(n_pca=20, knn=5, verbose=False).fit_transform(out.data, labels)
    host = meld_amd.MELD(n_pca=20, knn=5, verbose=False).fit_transform(out.data.to_scipy(), labels)
    assert dens.shape == (268, 2) and list(dens.columns) == list(host.columns)
    diff = np.abs(dens.values - host.values).max()
    print("densities, device matrix against its host copy: largest difference {:.3e} of {:.3e}".format(diff, np.abs(host.values).max()))
    assert diff <= 1e-5 * np.abs(host.values).max()
    groups = np.where(rng.random(300) > 0.4, "a", "b")[out.cells]
    de = meld_amd.rank_sum_test(out.normalized, groups, group="a", reference="b")
    de_host = meld_amd.rank_sum_test(out.normalized.to_scipy(), groups, group="a", reference="b")
    pd.testing.assert_frame_equal(de, de_host, check_exact=True)
    assert len(de) == 331 and (de["pval"] < 1).any()
    # the estimator takes a DeviceCSR wherever it takes sparse input: new cells of the same genes
    op = meld_amd.MELD(n_pca=20, knn=5, verbose=False)
    op.fit_transform(out.data, labels)
    new = pp.select(out.data, rows=np.arange(10))
    got = op.transform_new(new)
    want = op.transform_new(new.to_scipy())
    assert got.shape == (10, 2) and np.abs(got.values - want.values).max() <= 1e-5 * np.abs(want.values).max()
