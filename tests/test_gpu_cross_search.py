"""The search between two point sets (``meld_knn16_prepare_cross`` -> ``meld_knn16_topk`` -> refinement / exact sweep, reached through
``HipOps.directed_kernel_coo(n_refs=)`` by the MNN graph and by the extension to new cells) far from the common centre of the data.

The operand contract (include/meld_hip.h): ``norm2`` / ``norm2_max`` hold |x - mean|^2 in INPUT units for references and queries
alike, ``Qn`` the queries' norms in the search's scaled units.  Refinement certifies a row from ``norm2`` / ``norm2_max``; a query
norm in the wrong unit makes its allowance too small by the factor absmax and lets a row through with neighbours missing.  The data
(tests/cross_reference.py: ``far_samples``) put a clump of cells 200 units from the rest, so that absmax ~ 130.  Blocks are compared
with a plain fp64 all-pairs reference that tests/test_cross_reference.py ties to the oracle on the host."""
import functools

import numpy as np
import pytest
import torch

from tests import cross_reference as cr

pytestmark = pytest.mark.gpu


def _lib():
    from meld_amd._lib import get_lib

    return get_lib()


def _stacked(name):
    """[references B; queries A] of far_samples(10) for the operand tests: (X, nr, nq)."""
    A, B = cr.far_samples(10, cr.SEED)
    A = A.copy()
    shift = 0.0
    if name == "far_shifted":
        shift = 3.0e6  # the centring happens in fp64, before anything is rounded to fp32
    elif name == "query_farthest":
        A[5, 2] += 1000.0  # one query far beyond every reference: it alone sets absmax and the largest norm
    else:
        assert name == "far"
    return np.concatenate([B, A]) + shift, B.shape[0], A.shape[0]


def _prepare_cross(X, nr, nq):
    """``meld_knn16_prepare_cross`` called directly on the stacked cells, as the operand test of the search calls ``meld_knn16_prepare``."""
    from types import SimpleNamespace

    from meld_amd._lib import check, ptr

    lib = _lib()
    N, d = X.shape
    assert N == nr + nq
    Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    TS, BQ = lib.meld_knn16_tile_refs(), lib.meld_knn16_block_queries()
    sums = torch.empty(d, dtype=torch.float64, device="cuda")
    check(lib.meld_col_sums_f64(ptr(Xd), N, d, ptr(sums), st))
    mean = sums / N
    n_tiles, q_pad = (nr + TS - 1) // TS, ((nq + BQ - 1) // BQ) * BQ
    o = SimpleNamespace(Xd=Xd, mean=mean, q_pad=q_pad, st=st)
    o.Rt = torch.empty(n_tiles * lib.meld_knn16_tile_bytes(d), dtype=torch.uint8, device="cuda")
    o.Q = torch.empty(q_pad * lib.meld_knn16_query_bytes(d), dtype=torch.uint8, device="cuda")
    o.Qn = torch.empty(q_pad, dtype=torch.float32, device="cuda")
    o.norm2 = torch.full((N,), float("nan"), dtype=torch.float32, device="cuda")
    o.nmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    o.sinfo = torch.empty(4, dtype=torch.float32, device="cuda")
    check(lib.meld_knn16_prepare_cross(ptr(Xd), nr, N, d, ptr(mean), nr, nq, ptr(o.Rt), ptr(o.Q), ptr(o.Qn), ptr(o.norm2), ptr(o.nmax), ptr(o.sinfo), st),
          "meld_knn16_prepare_cross")
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("name", ["far", "far_shifted", "query_farthest"])
def test_prepare_cross_writes_every_norm_in_input_units(name):
    """a. norm2 of references AND queries = numpy's centred norms, norm2_max their maximum over both sets, Qn = the queries' norms
    times scale^2, scale_info[2] = absmax (rtol 1e-5: the tolerance of the operand test of the search within one set)."""
    X, nr, nq = _stacked(name)
    o = _prepare_cross(X, nr, nq)
    Xc = X - X.mean(0)
    n2 = (Xc**2).sum(1)
    absmax = np.abs(Xc).max()
    norm2 = o.norm2.cpu().numpy().astype(np.float64)
    nmax = float(o.nmax.item())
    sinfo = o.sinfo.cpu().numpy().astype(np.float64)
    Qn = o.Qn.cpu().numpy().astype(np.float64)[:nq]
    print("%s: absmax %.6g (library %.6g), max norm2 references %.6g queries %.6g, norm2_max %.6g; worst relative error of norm2: references %.2e, "
          "queries %.2e; of Qn against norm2 * scale^2: %.2e" % (name, absmax, sinfo[2], n2[:nr].max(), n2[nr:].max(), nmax,
                                                                 np.abs(norm2[:nr] / n2[:nr] - 1).max(), np.abs(norm2[nr:] / n2[nr:] - 1).max(),
                                                                 np.abs(Qn / (norm2[nr:] * sinfo[0] ** 2) - 1).max()))
    assert absmax > 100.0  # the data are what they are meant to be: the two units differ by four orders of magnitude
    np.testing.assert_allclose(norm2[:nr], n2[:nr], rtol=1e-5)
    np.testing.assert_allclose(norm2[nr:], n2[nr:], rtol=1e-5)
    np.testing.assert_allclose(nmax, n2.max(), rtol=1e-5)
    assert nmax == norm2.max()  # the maximum of what was written, over both point sets
    np.testing.assert_allclose(Qn, norm2[nr:] * sinfo[0] ** 2, rtol=1e-5)
    assert abs(sinfo[2] - absmax) < 1e-5 * absmax
    np.testing.assert_allclose(sinfo[0], 1.0 / absmax, rtol=1e-5)
    if name == "query_farthest":
        assert int(np.argmax(n2)) == nr + 5 and n2[nr + 5] > 4.0 * n2[:nr].max()
        assert nmax == norm2[nr + 5]


@pytest.mark.parametrize("nprod", [1, 3])
@pytest.mark.parametrize("name", ["far", "far_shifted", "query_farthest"])
def test_search_error_stays_inside_the_allowance_refine_assumes(name, nprod):
    """b. Every candidate's approximate d2 lies within E_q = c_const nmax + c_lin sqrt(n_q nmax) of the exact one, with n_q and
    nmax the TEST's norms in input units -- the allowance ``meld_knn_refine`` grants when it is handed true norms; rows sorted by
    (d2, idx), complete, indices among the references."""
    from scipy.spatial.distance import cdist

    from meld_amd._lib import check, ptr

    lib = _lib()
    X, nr, nq = _stacked(name)
    d, ksel = X.shape[1], 32
    o = _prepare_cross(X, nr, nq)
    cap = lib.meld_knn16_row_capacity(ksel)
    ci = torch.full((o.q_pad * cap,), -1, dtype=torch.int32, device="cuda")
    cd = torch.full((o.q_pad * cap,), float("nan"), dtype=torch.float32, device="cuda")
    cc = torch.empty(o.q_pad, dtype=torch.int32, device="cuda")
    check(lib.meld_knn16_topk(ptr(o.Q), ptr(o.Qn), ptr(o.Rt), ptr(o.sinfo), nr, d, nq, ksel, nprod, 1, None, None, 0, None, 0, 1.0, ptr(ci), ptr(cd),
                              ptr(cc), None, None, None, o.st), "meld_knn16_topk")
    torch.cuda.synchronize()
    ci = ci.cpu().numpy().reshape(o.q_pad, cap)[:nq, :ksel].astype(np.int64)
    cd = cd.cpu().numpy().reshape(o.q_pad, cap)[:nq, :ksel].astype(np.float64)
    assert np.all(cc.cpu().numpy()[:nq] == min(ksel, nr))
    assert ci.min() >= 0 and ci.max() < nr
    assert all(len(set(row)) == ksel for row in ci)
    dd, di = np.diff(cd, axis=1), np.diff(ci, axis=1)
    assert np.all((dd > 0) | ((dd == 0) & (di > 0)))  # sorted by (d2, idx)
    Xc = X - X.mean(0)
    n2 = (Xc**2).sum(1)
    nmax = n2.max()
    exact = np.take_along_axis(cdist(X[nr:], X[:nr], "sqeuclidean"), ci, axis=1)
    E = lib.meld_knn16_error_coef_const(nprod, d) * nmax + lib.meld_knn16_error_coef_lin(nprod) * np.sqrt(n2[nr:] * nmax)
    err = np.abs(cd - exact)
    print("%s nprod=%d: max |d2 - exact| = %.3e, smallest allowance %.3e, largest share of a row's allowance used %.3f" % (
        name, nprod, err.max(), E.min(), (err / E[:, None]).max()))
    assert np.all(err <= E[:, None])


@functools.lru_cache(maxsize=None)
def _far_case(name):
    Xq, Yr, knn, decay = cr.far_block_cases()[name]
    return Xq, Yr, knn, decay, cr.cross_block_reference(Xq, Yr, knn, decay, cr.THRESH)[0]


def _block_direct(ops, Xq, Yr, knn, decay):
    """The block through ``HipOps.directed_kernel_coo(n_refs=)``: (rows, cols, vals) as ``mnn._cross_block`` returns them, the
    bandwidths and the route's record."""
    from meld_amd.graph import default_ksel

    nq, nr = int(Xq.shape[0]), int(Yr.shape[0])
    knn_c = int(min(knn, nr))
    Xcat = torch.cat([Yr, Xq], dim=0).contiguous()
    keys, vals, bw, info = ops.directed_kernel_coo(Xcat, nr, nq, knn_c - 1, decay, cr.THRESH, default_ksel(knn_c), n_refs=nr)
    M = keys.shape[0] // 2
    return (keys[:M] >> 32) - nr, keys[:M] & 0xFFFFFFFF, 2.0 * vals[:M], bw, info, (keys, vals)


def _assert_block_is_the_reference(what, rows, cols, vals, K, knn):
    nq, nr = K.shape
    K = K.tocoo()
    ref_key = K.row.astype(np.int64) * nr + K.col.astype(np.int64)
    o_ref = np.argsort(ref_key, kind="stable")
    key = (rows * nr + cols).cpu().numpy()
    o = np.argsort(key, kind="stable")
    v = vals.cpu().numpy()
    per_row = np.bincount(rows.cpu().numpy(), minlength=nq)
    missing, extra = np.setdiff1d(ref_key, key).size, np.setdiff1d(key, ref_key).size
    print("%s: %d entries (reference %d), %d missing, %d extra, fewest per query %d" % (what, key.size, ref_key.size, missing, extra, per_row.min()))
    assert key.size == ref_key.size and np.array_equal(key[o], ref_key[o_ref]), (what, missing, extra)
    assert np.abs(v[o] - K.data[o_ref]).max() <= 1e-12, what
    assert per_row.min() >= min(knn, nr), what  # every query reaches its knn nearest references


def _both_routes(what, Xq, Yr, knn, decay, K):
    from meld_amd.graph import HipOps
    from meld_amd.mnn import _cross_block

    Xq_d, Yr_d = torch.from_numpy(np.ascontiguousarray(Xq)).cuda(), torch.from_numpy(np.ascontiguousarray(Yr)).cuda()
    ops = HipOps()
    rows, cols, vals, _, info, _ = _block_direct(ops, Xq_d, Yr_d, knn, decay)
    assert info["search"] == "f16x3"
    print("%s: %d rows flagged, %d searched again" % (what, info["n_flagged_rows"], info["n_researched_rows"]))
    _assert_block_is_the_reference(what + " (directed_kernel_coo)", rows, cols, vals, K, knn)
    rows, cols, vals = _cross_block(ops, Xq_d, Yr_d, knn, decay, cr.THRESH)
    _assert_block_is_the_reference(what + " (_cross_block)", rows, cols, vals, K, knn)


@pytest.mark.parametrize("name", sorted(cr.far_block_cases()))
def test_blocks_far_from_the_centre_equal_the_plain_reference(name):
    """c. far_samples in both directions at d = 10 and 50, queries / references alone outside, decay = inf, knn clipped."""
    Xq, Yr, knn, decay, K = _far_case(name)
    _both_routes(name, Xq, Yr, knn, decay, K)


@pytest.mark.parametrize("d", cr.EDGE_DIMS)
def test_blocks_at_tile_and_block_edges_equal_the_plain_reference(d):
    """c. Shape edges: references around one tile, queries around one block, d at the first hi-only first pass (7), at the K-block
    boundaries of ceil((d + 3) / 16) (13 / 14 -- where the split layout starts -- and 29 / 30) and at the last supported d."""
    lib = _lib()
    for nr, nq in cr.edge_shapes(lib.meld_knn16_tile_refs(), lib.meld_knn16_block_queries()):
        Xq, Yr = cr.edge_samples(d, nr, nq)
        K = cr.cross_block_reference(Xq, Yr, cr.KNN, cr.DECAY, cr.THRESH)[0]
        _both_routes("d=%d nr=%d nq=%d" % (d, nr, nq), Xq, Yr, cr.KNN, cr.DECAY, K)


@pytest.mark.parametrize("d", cr.FAR_DIMS)
def test_certification_does_not_depend_on_the_unit_of_length(d):
    """d. far_samples times a power of two: every operand of the search, every distance and every allowance scales exactly, so
    the block is bit-identical, the bandwidths scale by t, and the SAME rows are flagged and searched again."""
    from meld_amd.graph import HipOps

    A, B = cr.far_samples(d, cr.SEED)
    out = {}
    for t in cr.UNIT_SCALES:
        Xq_d, Yr_d = torch.from_numpy(A * t).cuda(), torch.from_numpy(B * t).cuda()
        _, _, _, bw, info, (keys, vals) = _block_direct(HipOps(), Xq_d, Yr_d, cr.KNN, cr.DECAY)
        order = torch.argsort(keys)  # (keys are unique: the stream as a set of (key, value) pairs)
        out[t] = (keys[order], vals[order], bw, info["n_flagged_rows"], info["n_researched_rows"])
        print("d=%d t=%g: %d entries, %d rows flagged, %d searched again" % (d, t, keys.shape[0] // 2, out[t][3], out[t][4]))
    k1, v1, bw1, flagged1, researched1 = out[1.0]
    for t in cr.UNIT_SCALES:
        k, v, bw, flagged, researched = out[t]
        assert torch.equal(k, k1) and torch.equal(v, v1), t
        assert torch.equal(bw, bw1 * t), t
        assert flagged == flagged1 and researched == researched1, (t, flagged, flagged1, researched, researched1)


@pytest.mark.parametrize("d", cr.FAR_DIMS)
def test_mnn_graph_far_from_the_centre_matches_the_oracle(d):
    """e. The MNN graph of the two samples, interleaved: same entries, weights (1e-9 of the largest) and degrees (1e-9) as the
    oracle -- the bounds of test_mnn_graph_matches_the_oracle."""
    import meld_amd
    from oracle import meld_oracle as mo

    X, batch = cr.mnn_cells(d)
    op = meld_amd.MELD(knn=cr.KNN, verbose=0).fit(X, sample_idx=batch)
    assert op.graph.info["graph"] == "mnn" and op.graph.info["n_samples"] == 2
    G = mo.build_graph(X, knn=cr.KNN, sample_idx=batch, algorithm="brute")
    W = op.graph.W
    print("d=%d: nnz %d (oracle %d), max |W - oracle| / max |W| = %.3e" % (d, W.nnz, G.W.nnz, abs(W - G.W).max() / abs(G.W).max()))
    assert W.nnz == G.W.nnz and abs(W - G.W).max() <= 1e-9 * abs(G.W).max()
    np.testing.assert_allclose(op.graph.dw, G.dw, rtol=1e-9)
