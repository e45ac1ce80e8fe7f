"""Per-gene moments and highly variable genes on the device (meld_amd/preprocess.py, ``meld_prep_gene_moments`` in csrc/preprocess.hip)
against the host restatement (tests/hvg_reference.py, itself checked against numpy and scipy): the kernel's contract, the fused
value map, the selection end to end, the refusals of the entry and the hand-over to MELD.

Paths of the kernel the GENE lengths below are chosen for.  A workgroup of 1,024 owns 16 consecutive genes.  A gene of at most
``MELD_PREP_MOMENTS_WAVE_MAX`` = 2,048 stored entries is taken by one wave, lane l adding the entries l, l + 64, ...: 63 / 64 / 65
sit on the lane count, the four-deep unrolled loop runs while at least 193 entries are left to the first lane (192 / 193) and for
all lanes from 256 on (255 / 256 / 257).  A longer gene is walked by the whole workgroup (2,048 / 2,049 on the threshold), whose
unrolled loop is entered by its first thread from 3,073 entries (3,072 / 3,073) and by all of them from 4,096 (4,095 / 4,096 /
4,097); one gene is stored in every one of the 5,000 cells.  23 genes are two workgroups, the second one partly filled, with long
genes in both.

The tolerances are those of tests/hvg_reference.py (``moment_bounds``): derived, not measured."""
import numpy as np
import pytest
from scipy import sparse

from tests import hvg_reference as hvg
from tests import preprocess_reference as ref

pytestmark = pytest.mark.gpu

N_CELLS = 5000
LENGTHS = [0, 1, 2, 63, 64, 65, 192, 193, 255, 256, 257, 2047, 2048, 2049, 3072, 3073, 4095, 4096, 4097, 5000, 0, 1000, 2500]
WAVE_MAX = 2048


def _pp():
    from meld_amd import preprocess

    return preprocess


def _dev(X):
    from meld_amd.sparse import DeviceCSR

    return DeviceCSR.from_input(X)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _host(triple):
    return tuple(t.cpu().numpy() for t in triple)


@pytest.fixture(scope="module")
def X():
    return ref.standard_matrix()


def _hand_built(kind, dtype, seed=3):
    """genes of the lengths above over 5,000 cells, as a CSR [cells, genes]; stored zeros and negative entries"""
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(LENGTHS)])
    indices = np.concatenate([np.sort(rng.choice(N_CELLS, n, replace=False)) for n in LENGTHS]).astype(np.int32)
    if kind == "int":
        data = rng.integers(-5, 10, size=indptr[-1]).astype(np.float64)
    else:
        data = rng.normal(size=indptr[-1]) * np.exp(rng.normal(size=indptr[-1]) * 3)
    data[rng.random(indptr[-1]) < 0.1] = 0.0
    C = sparse.csc_matrix((data.astype(dtype), indices, indptr), shape=(N_CELLS, len(LENGTHS)))
    A = C.tocsr()
    assert A.has_canonical_format and A.nnz == C.nnz and (A.data == 0).any() and (A.data < 0).any()
    assert np.array_equal(np.diff(A.tocsc().indptr), LENGTHS)
    return A


def _within_bounds(got, m, what):
    """count exact; mean and variance within the derived bounds of the long-double reference ``m``; returns the largest ratios"""
    count, mean, var = got
    assert count.dtype == np.int32 and mean.dtype == np.float64 and var.dtype == np.float64
    assert np.array_equal(count, m.count), what
    eta, tol = hvg.moment_bounds(m)
    err_m = np.abs(mean.astype(np.longdouble) - m.mean)
    err_v = np.abs(var.astype(np.longdouble) - m.var)
    rm = float((err_m[eta > 0] / eta[eta > 0]).max(initial=0))
    rv = float((err_v[tol > 0] / tol[tol > 0]).max(initial=0))
    print("{}: largest error / bound = {:.3f} (mean), {:.3f} (variance); largest bounds {:.2e}, {:.2e}".format(
        what, rm, rv, float(eta.max()), float(tol.max())))
    assert (err_m <= eta).all(), (what, "mean", rm)
    assert (err_v <= tol).all(), (what, "variance", rv)
    masked = m.count < 0
    assert (mean[masked] == 0).all() and (var[masked] == 0).all()
    return rm, rv


# ---- 1. the kernel's contract ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("keep", [None, "random", "all", "one"])
def test_gene_moments_contract(kind, dtype, keep):
    import torch

    pp = _pp()
    A = _hand_built(kind, dtype)
    D = _dev(A)
    assert D.val.dtype == (torch.float32 if dtype == np.float32 else torch.float64) and D.nnz == A.nnz  # (stored zeros went up)
    G = len(LENGTHS)
    assert np.array_equal(np.diff(D.T.rowptr.cpu().numpy()), LENGTHS) and max(LENGTHS) == N_CELLS
    assert {WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1} <= set(LENGTHS)
    rng = np.random.default_rng(5)
    only = int(A.tocsc().indices[-1])  # a cell the last gene is stored in
    rows = {None: None, "random": rng.random(N_CELLS) < 0.6, "all": np.ones(N_CELLS, bool), "one": np.arange(N_CELLS) == only}[keep]
    gmask = rng.random(G) < 0.7
    gmask[LENGTHS.index(N_CELLS)] = True
    assert 0 < gmask.sum() < G and (~gmask & (np.asarray(LENGTHS) > WAVE_MAX)).any()  # a long gene is masked too
    Aw = A.astype(np.float64)
    for gene_mask in (None, gmask):
        for ddof in (0, 1):
            what = "{} {} keep={} mask={} ddof={}".format(kind, np.dtype(dtype).name, keep, gene_mask is not None, ddof)
            if keep == "one" and ddof == 1:  # one kept cell leaves no degree of freedom: refused before the launch
                with pytest.raises(ValueError, match="ddof=1"):
                    pp.gene_moments_device(D, row_keep=rows, gene_mask=gene_mask, ddof=1)
                continue
            got = _host(pp.gene_moments_device(D, row_keep=rows, gene_mask=gene_mask, ddof=ddof))
            m = hvg.moments_long(Aw, rows, gene_mask=gene_mask, ddof=ddof)
            _within_bounds(got, m, what)
            live = m.count >= 0
            if kind == "int":  # integer sums are exact: the mean is THE quotient of the exact sum, so mean * n_kept is that sum
                exact = np.array([int(Aw[:, g].toarray()[:, 0][np.ones(N_CELLS, bool) if rows is None else rows].sum()) for g in range(G)])
                assert np.array_equal(_bits(got[1][live]), _bits(exact[live].astype(np.float64) / m.n_kept))
                assert np.array_equal(np.rint(got[1][live] * m.n_kept).astype(np.int64), exact[live])
            again = _host(pp.gene_moments_device(D, row_keep=rows, gene_mask=gene_mask, ddof=ddof))
            assert np.array_equal(got[0], again[0]) and np.array_equal(_bits(got[1]), _bits(again[1])) and np.array_equal(_bits(got[2]), _bits(again[2]))
            if dtype == np.float32:  # the transposition widens; the CSC arrays go up as fp32 and are widened on load: the same bits
                C = A.tocsc()
                assert C.data.dtype == np.float32 and C.nnz == A.nnz
                direct = _host(pp.gene_moments_device(C, row_keep=rows, gene_mask=gene_mask, ddof=ddof))
                assert np.array_equal(got[0], direct[0]) and np.array_equal(_bits(got[1]), _bits(direct[1])) and np.array_equal(_bits(got[2]), _bits(direct[2]))
            if keep == "all":  # a mask of ones, no scale: the bits of the plain call
                plain = _host(pp.gene_moments_device(D, gene_mask=gene_mask, ddof=ddof))
                assert np.array_equal(got[0], plain[0]) and np.array_equal(_bits(got[1]), _bits(plain[1])) and np.array_equal(_bits(got[2]), _bits(plain[2]))
    if keep == "random":
        cnt = hvg.moments_long(Aw, rows).count
        assert (cnt == 0).any() and (cnt < np.asarray(LENGTHS)).any() and (cnt > WAVE_MAX).any()


def test_csc_input_goes_up_as_the_gene_major_copy_and_the_host_measures():
    pp = _pp()
    A = _hand_built("real", np.float64)
    D = _dev(A)
    from_csr = _host(pp.gene_moments_device(D))
    from_csc = _host(pp.gene_moments_device(A.tocsc()))
    for a, b in zip(from_csr, from_csc):
        assert np.array_equal(a, b) and a.dtype == b.dtype
    assert np.array_equal(_bits(pp.gene_mean(D)), _bits(from_csr[1]))
    assert np.array_equal(_bits(pp.gene_variance(D)), _bits(from_csr[2]))
    m0 = hvg.moments_long(A, ddof=0)
    _within_bounds((from_csr[0], pp.gene_mean(D), pp.gene_variance(D, ddof=0)), m0, "gene_mean / gene_variance(ddof=0)")
    v, means = pp.gene_variability(D, kernel_size=5, smooth=2, return_means=True)
    assert np.array_equal(_bits(means), _bits(from_csr[1]))
    assert np.array_equal(_bits(v), _bits(hvg.variability(from_csr[1], from_csr[2], 5, 2)))


# ---- 2. the fused value map -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transform", [None, "sqrt", "log", "log2", "log10", "arcsinh"])
def test_moments_of_the_values_the_rewrite_would_leave(X, transform):
    import torch

    pp = _pp()
    X = X.copy()
    X.data[X.indptr[7]:X.indptr[8]] = 0.0  # a kept cell of stored zeros only: its scale is 0 and it is left alone
    rng = np.random.default_rng(11)
    keep = rng.random(300) < 0.8
    keep[7] = True
    cells = np.flatnonzero(keep)
    genes = np.flatnonzero(ref.gene_capture_count(X, 0, keep) >= 5)
    gmask = np.zeros(500, bool)
    gmask[genes] = True
    D = _dev(X)
    a = pp.row_stats_device(D, torch.from_numpy(gmask).cuda())[1]
    assert float(a[7]) == 0.0 and X.indptr[8] > X.indptr[7]
    got = _host(pp.gene_moments_device(D, row_keep=keep, row_scale=a, rescale=10000.0, transform=transform, cofactor=5.0, gene_mask=gmask))
    assert (got[0][~gmask] == -1).all() and (got[1][~gmask] == 0).all() and (got[2][~gmask] == 0).all()
    # the matrix the step-by-step reference leaves: select, normalise, transform
    Y = ref.select(X, rows=cells, cols=genes)
    T = ref.TRANSFORMS[transform](ref.library_size_normalize(Y, 10000))
    m = hvg.moments_long(T)
    assert m.n_kept == len(cells) and 0 < len(genes) < 500
    _within_bounds(tuple(g[gmask] for g in got), m, "fused map, {}".format(transform))
    # the kernel's own rule: a scale of 0 on a cell WITH values keeps them, rescale still multiplies
    scale = a.cpu().numpy().copy()
    busy = int(cells[np.argmax(np.diff(X.indptr)[cells])])
    scale[busy] = 0.0
    got = _host(pp.gene_moments_device(D, row_keep=keep, row_scale=scale, rescale=3.0, transform=transform, cofactor=150.0, gene_mask=gmask))
    m = hvg.moments_long(X, keep, scale, 3.0, transform, 150.0, gmask, 1)
    _within_bounds(got, m, "zero scale on a busy cell, {}".format(transform))


# ---- 3. selection end to end ----------------------------------------------------------------------------------------------------------------
def _largest_tolerance(m):
    eta, tol = hvg.moment_bounds(m)
    return max(float(eta.max()), float(tol.max()))


def _assert_not_on_a_knife_edge(m, v, kw, cut, G):
    """On the REFERENCE alone: the selection cannot hinge on rounding.  The variability gap at the cutoff (at the n_top_genes edge)
    and the smallest gap between distinct sorted means each exceed 1e6 times the largest tolerance of the moments.  A percentile
    that lands exactly on an order statistic makes the cutoff that gene's own variability, whatever its rounding, and `>` drops
    the gene either way: the gap is then taken over the other genes."""
    T = _largest_tolerance(m)
    mean = np.sort(m.mean.astype(np.float64))
    d = np.diff(mean)
    mean_gap = d[d > 0].min()
    if "n_top_genes" in kw:
        s = np.sort(v)[::-1]
        gap = s[kw["n_top_genes"] - 1] - s[kw["n_top_genes"]]
    else:
        on_cut = v == cut
        if on_cut.any():
            assert "percentile" in kw and on_cut.sum() == 1, "the cutoff sits on a gene's variability: the fixture is wrong"
            pos = kw["percentile"] / 100.0 * (G - 1)
            assert pos == int(pos)
        gap = np.abs(v[~on_cut] - cut).min()
    print("selection {}: variability gap {:.2e}, smallest mean gap {:.2e}, largest tolerance {:.2e}".format(kw, gap, mean_gap, T))
    assert gap > 1e6 * T and mean_gap > 1e6 * T, "the fixture hinges on rounding: choose another seed"


@pytest.mark.parametrize("rule", ["percentile", "cutoff", "n_top_genes"])
def test_highly_variable_genes_on_the_standard_matrix(X, rule):
    pp = _pp()
    m = hvg.moments_long(X)
    v = hvg.variability(m.mean.astype(np.float64), m.var.astype(np.float64), 0.05, 5)
    s = np.sort(v)
    i = 350 + int(np.argmax(np.diff(s[350:451])))  # the cutoff: the middle of the widest gap among the positive variabilities
    assert s[350] > 0                              # (146 genes of the raw matrix have a variability of exactly 0: no cutoff there)
    kw = {"percentile": dict(percentile=80), "cutoff": dict(cutoff=float((s[i] + s[i + 1]) / 2)), "n_top_genes": dict(n_top_genes=50)}[rule]
    want, kept_ref, extra = hvg.highly_variable_genes(X, **kw)
    _assert_not_on_a_knife_edge(m, v, kw, extra.cutoff, 500)
    D = _dev(X)
    got, kept = pp.highly_variable_genes(D, **kw)
    assert kept.dtype == np.int64 and np.array_equal(kept, kept_ref) and 0 < len(kept) < 500
    assert got.shape == want.shape and np.array_equal(got.rowptr.cpu().numpy(), want.indptr)
    assert np.array_equal(got.col.cpu().numpy(), want.indices) and np.array_equal(_bits(got.val.cpu().numpy()), _bits(want.data))
    if rule == "percentile":  # the default rule; scipy input and a CSC input give the same genes
        assert np.array_equal(pp.highly_variable_genes(X)[1], kept_ref)
        assert np.array_equal(pp.highly_variable_genes(X.tocsc())[1], kept_ref)
    if rule == "n_top_genes":
        with pytest.raises(ValueError, match="n_top_genes"):
            pp.highly_variable_genes(D, n_top_genes=501)


@pytest.mark.parametrize("rule", [dict(n_top_genes=50), dict(hvg_percentile=80)])
def test_run_with_a_rule_equals_the_steps_then_the_selection(X, rule):
    import torch

    pp = _pp()
    steps = dict(library_size_percentile=10, min_cells=5, rescale=10000, transform="sqrt")
    want = hvg.run_with_hvg(X, **steps, **rule)
    kw = {"n_top_genes": rule.get("n_top_genes")} if "n_top_genes" in rule else {"percentile": rule["hvg_percentile"]}
    _assert_not_on_a_knife_edge(want.moments, want.variability, kw, want.cutoff, len(want.genes_before))
    D = _dev(X)
    out = pp.run(D, **steps, **rule)
    full = pp.run(D, **steps)
    assert D._T is not None
    assert np.array_equal(out.genes, want.genes) and out.genes.dtype == np.int64 and np.array_equal(out.cells, want.cells)
    assert np.array_equal(full.genes, want.genes_before) and np.array_equal(out.info["hvg"]["genes"], want.genes_before)
    assert np.array_equal(_bits(out.library_size), _bits(full.library_size)) and np.array_equal(out.library_size, want.library_size)
    # the matrix: `select` of the step-by-step result, values bit for bit (normalise, then select)
    for a, whole, r in ((out.data, full.data, want.data), (out.normalized, full.normalized, want.normalized)):
        b = pp.select(whole, cols=want.kept)
        assert a.shape == b.shape == r.shape and torch.equal(a.rowptr, b.rowptr) and torch.equal(a.col, b.col)
        assert torch.equal(a.val.view(torch.int64), b.val.view(torch.int64))
        assert np.array_equal(a.rowptr.cpu().numpy(), r.indptr) and np.array_equal(a.col.cpu().numpy(), r.indices)
    assert np.array_equal(_bits(out.normalized.val.cpu().numpy()), _bits(want.normalized.data))
    assert out.info["shape_after"] == (268, len(want.genes)) and out.data.shape == (268, len(want.genes))
    info = out.info["hvg"]
    _within_bounds((want.moments.count.astype(np.int32), info["mean"], info["variance"]), want.moments, "run, info['hvg']")
    # the variability is the host rule on those moments; against the reference's it moves by a few tolerances at the most
    assert np.array_equal(_bits(info["variability"]), _bits(hvg.variability(info["mean"], info["variance"], 0.05, 5)))
    assert np.abs(info["variability"] - want.variability).max() <= 4 * _largest_tolerance(want.moments)
    assert info["rule"] == ("n_top_genes" if "n_top_genes" in rule else "percentile")
    assert abs(info["cutoff"] - want.cutoff) <= 4 * _largest_tolerance(want.moments)
    with pytest.raises(ValueError, match=r"run \(highly_variable_genes\): the filter leaves no gene"):
        pp.run(D, **steps, hvg_cutoff=1e9)


def test_run_without_a_rule_makes_no_transposition(X):
    pp = _pp()
    D = _dev(X)
    out = pp.run(D, library_size_percentile=10, min_cells=5)
    assert D._T is None and "hvg" not in out.info and out.data.shape == (268, 331)


# ---- 4. the entry refuses bad arguments -----------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments(X):
    from meld_amd._lib import get_lib

    lib = get_lib()
    D = _dev(X)
    p = D.rowptr.data_ptr()

    def call(rowptr=p, col=p, val=p, f32=0, genes=500, cells=300, transform=0, cofactor=5.0, n_kept=300, ddof=1, count=p, mean=p, var=p):
        lib.meld_scale_f64(None, 1.0, None, 10, None)  # (leaves another entry's message behind)
        rc = lib.meld_prep_gene_moments(rowptr, col, val, f32, genes, cells, None, None, 1.0, transform, cofactor, None, n_kept, ddof,
                                        count, mean, var, None)
        return rc, lib.meld_last_error().decode()

    bad = [dict(rowptr=None), dict(col=None), dict(val=None), dict(count=None), dict(mean=None), dict(var=None), dict(f32=2), dict(f32=-1),
           dict(genes=0), dict(genes=2 ** 31), dict(cells=0), dict(cells=2 ** 31), dict(transform=6), dict(transform=-1),
           dict(transform=5, cofactor=0.0), dict(transform=5, cofactor=-1.0), dict(ddof=2), dict(ddof=-1), dict(n_kept=0), dict(n_kept=1, ddof=1)]
    for kwargs in bad:
        rc, msg = call(**kwargs)
        assert rc == -1 and msg.startswith("meld_prep_gene_moments:"), (kwargs, rc, msg)
    assert "transform=6" in call(transform=6)[1] and "ddof=2" in call(ddof=2)[1]
    assert lib.meld_abi_version() == 1


# ---- 5. through the product -----------------------------------------------------------------------------------------------------------------
def test_selected_matrix_goes_through_meld(X):
    import meld_amd

    pp = _pp()
    out = pp.run(X, library_size_percentile=10, min_cells=5, n_top_genes=100)
    labels = np.where(np.random.default_rng(0).random(300) > 0.5, "treat", "ctrl")
    dens = meld_amd.MELD(n_pca=20, knn=5, verbose=False).fit_transform(out.data, labels[out.cells])
    assert out.data.shape == (268, 100) and dens.shape == (268, 2) and np.isfinite(dens.values).all()
