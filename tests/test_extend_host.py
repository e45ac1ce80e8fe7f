"""Out-of-sample extension, host side (no GPU): the shape check and its messages, the refusals, a NumPy restatement of the apply
kernel against scipy.sparse on the fixture, and the fixture's own well-definedness (tests/golden/make_golden_extend.py)."""
import os

import numpy as np
import pytest
import torch
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {"a": dict(knn=5, decay=40, thresh=1e-4), "b": dict(knn=5, decay=None, thresh=1e-4), "w": dict(knn=20, decay=2, thresh=1e-4)}


@pytest.fixture(scope="module")
def g9():
    return np.load(os.path.join(ROOT, "tests", "golden", "g9_extend.npz"))


def _kernel(z, tag, q, n=600):
    ip = z["K_{}_{}_indptr".format(tag, q)]
    return sparse.csr_matrix((z["K_{}_{}_data".format(tag, q)], z["K_{}_{}_indices".format(tag, q)].astype(np.int32), ip), shape=(len(ip) - 1, n))


def _stub_graph(n=6):
    from meld_amd.graph import DeviceGraph

    return DeviceGraph(torch.zeros(n + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.float64),
                       torch.zeros(n, dtype=torch.float64))


def _with_state(G, **kw):
    from meld_amd.extend import attach_extension_state

    args = dict(X=torch.zeros(G.N, 3, dtype=torch.float64), n_features_in=3, project=None, row_fn=None, knn=2, decay=40.0, thresh=1e-4)
    args.update(kw)
    return attach_extension_state(G, **args)


def test_shape_check_and_messages():
    """[UPSTREAM, unpinned graphtools ``Data._check_extension_shape``]"""
    from meld_amd.extend import check_extension_shape

    assert check_extension_shape((5, 40), 40, 8) == "raw"
    assert check_extension_shape((5, 8), 40, 8) == "reduced"
    assert check_extension_shape((1, 8), 8, 8) == "raw"
    with pytest.raises(ValueError, match=r"Y must be of shape either \(n, 40\) or \(n, 8\)"):
        check_extension_shape((5, 9), 40, 8)
    with pytest.raises(ValueError, match=r"Y must be of shape \(n, 8\)$"):
        check_extension_shape((5, 9), 8, 8)
    with pytest.raises(ValueError, match=r"Expected a 2D matrix. Y has shape \(8,\)"):
        check_extension_shape((8,), 8, 8)
    # ... and through the graph's methods, before anything touches a device
    G = _with_state(_stub_graph())
    assert G.n_features_in == 3
    with pytest.raises(ValueError, match=r"Y must be of shape \(n, 3\)"):
        G.build_kernel_to_data(np.zeros((2, 4)))
    with pytest.raises(ValueError, match="Expected a 2D matrix"):
        G.extend_to_data(np.zeros(3))


def test_interpolate_needs_transitions_or_cells():
    G = _stub_graph()
    with pytest.raises(ValueError, match="Either transitions or Y must be provided."):
        G.interpolate(np.zeros((G.N, 2)))
    # a scipy matrix of transitions is multiplied on the host, whatever the graph
    T = sparse.random(4, G.N, density=0.5, random_state=0, format="csr")
    F = np.arange(2.0 * G.N).reshape(G.N, 2)
    np.testing.assert_allclose(G.interpolate(F, transitions=T), T @ F)


def test_refusals_name_their_case():
    from meld_amd import MELD

    Y = np.zeros((2, 3))
    cases = []
    G = _stub_graph()
    cases.append((G, "from_scipy"))
    G = _stub_graph()
    G.info["adopted_from"] = "kNNGraph"
    cases.append((G, "adopted from kNNGraph"))
    G = _stub_graph()
    G.info["graph"] = "mnn"
    cases.append((G, "MNN graph"))
    G = _stub_graph()
    G.info.update(route="metric_knn", metric="manhattan")
    cases.append((G, "L1 / L-inf"))
    G = _stub_graph()
    G.info["dense"] = True
    cases.append((G, "dense graph"))
    G = _with_state(_stub_graph())
    G.N = 12  # (a shard: six of twelve rows)
    cases.append((G, "row-sharded"))
    cases.append((_with_state(_stub_graph(), knn_max=9), "knn_max"))
    cases.append((_with_state(_stub_graph(), bandwidth=lambda d: d), "callable bandwidth"))
    cases.append((_with_state(_stub_graph(), bandwidth=np.ones(6)), "per-cell bandwidth"))
    for G, what in cases:
        for call in (lambda: G.build_kernel_to_data(Y), lambda: G.extend_to_data(Y), lambda: G.interpolate(np.zeros((G.N, 1)), Y=Y),
                     lambda: G.kernel_to_data_device(Y)):
            with pytest.raises(NotImplementedError, match=what):
                call()
    with pytest.raises(NotImplementedError, match="callable bandwidth"):
        _with_state(_stub_graph()).build_kernel_to_data(Y, bandwidth=lambda d: d)
    # MELD.transform_new: the reference-style error without densities, the graph's refusals unchanged
    op = MELD()
    with pytest.raises(ValueError, match="sample_densities must be set prior to running transform_new"):
        op.transform_new(Y)
    op._graph = cases[2][0]
    op.sample_densities = __import__("pandas").DataFrame(np.zeros((6, 2)), columns=["ctrl", "expt"])
    with pytest.raises(NotImplementedError, match="MNN graph"):
        op.transform_new(Y)


def apply_restated(rowptr, col, val, rowsum, F, colmap=None):
    """``meld_extend_apply`` (csrc/extend.hip) in NumPy, addition for addition: CG = the power of two >= p (at most 64) lanes per
    entry, 64 / CG entry slots, two accumulators per lane over alternate trips, the slots' sums met by xor exchanges from
    offset 32 down to CG, one division by the row sum."""
    M, p = len(rowsum), F.shape[1]
    log_cg = 0
    while (1 << log_cg) < p and log_cg < 6:
        log_cg += 1
    cg, eg = 1 << log_cg, 64 >> log_cg
    out = np.zeros((M, p))
    for r in range(M):
        rs, re = int(rowptr[r]), int(rowptr[r + 1])
        for c0 in range(0, p, cg):
            width = min(cg, p - c0)
            acc = np.zeros((2, eg, width))
            for es in range(eg):
                for t, e in enumerate(range(rs + es, re, eg)):
                    j = int(col[e]) if colmap is None else int(colmap[col[e]])
                    acc[t % 2, es] += val[e] * F[j, c0:c0 + width]
            lanes = acc[0] + acc[1]
            off = eg // 2
            while off >= 1:  # (lane offset 32 ... CG = slot offset eg / 2 ... 1)
                lanes = lanes + lanes[np.arange(eg) ^ off]
                off //= 2
            out[r, c0:c0 + width] = lanes[0] / rowsum[r] if rowsum[r] > 0 else 0.0
    return out


@pytest.mark.parametrize("tag", ["a", "b", "w"])
def test_apply_restatement_matches_scipy_on_the_fixture(g9, tag):
    F = g9["F"].astype(np.float64)
    for q in ("q150", "q63", "q1"):
        K = _kernel(g9, tag, q)
        rowsum = np.asarray(K.sum(1)).ravel()
        T = sparse.diags(1.0 / rowsum) @ K
        for p in (1, 3, 7):
            got = apply_restated(K.indptr, K.indices, K.data, rowsum, F[:, :p])
            np.testing.assert_allclose(got, T @ F[:, :p], rtol=1e-12, atol=1e-14)
            # (the fixture keeps the products as float32: half a unit in the last of its 24 bits, relative to the column)
            np.testing.assert_allclose(got, g9["TF_{}_{}".format(tag, q)][:, :p], rtol=2.0 ** -24, atol=2.0 ** -24 * np.abs(got).max())
    # F in another order, the columns translated: the same numbers
    K = _kernel(g9, tag, "q63")
    perm = np.random.default_rng(0).permutation(600)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(600)
    rowsum = np.asarray(K.sum(1)).ravel()
    np.testing.assert_array_equal(apply_restated(K.indptr, K.indices, K.data, rowsum, F[perm][:, :3], colmap=inv),
                                  apply_restated(K.indptr, K.indices, K.data, rowsum, F[:, :3]))


def test_fixture_pattern_is_well_defined(g9):
    """The generator's assertions on the committed file: no row beyond the 128-entry candidate list, a wide row beyond 64 entries,
    no stored value within 1e-6 (relative) above thresh, no excluded pair within 1e-9 (relative) of the radius."""
    from tests.golden import make_golden_extend as gen

    ref = g9["ref"].astype(np.float64)
    assert ref.shape == (600, 8) and g9["q150"].shape == (150, 8) and g9["q63"].shape == (63, 8) and g9["q1"].shape == (1, 8)
    for q in ("q150", "q63", "q1"):
        Q = g9[q].astype(np.float64)
        for tag, par in PARAMS.items():
            gen.check_pattern(_kernel(g9, tag, q), Q, ref, **par)
    assert np.diff(g9["K_w_q150_indptr"]).max() > 64
    # the copies of fitted cells and the far outliers are where the generator put them
    q150 = g9["q150"].astype(np.float64)
    np.testing.assert_array_equal(q150[g9["copy_rows"]], ref[g9["copies"]])
    d = gen.pairwise(q150, ref)
    nearest = d.min(1)
    assert (nearest[-int(g9["n_outliers"]):] > 20 * np.median(nearest)).all()
    Ka = _kernel(g9, "a", "q150")
    for r, c in zip(g9["copy_rows"], g9["copies"]):
        assert Ka[r, c] == 1.0
    # well under the size of g6_c2mini_5000x50.npz: the generator's bound, three quarters of it
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g9_extend.npz")) <= gen.size_bound()
    assert gen.size_bound() == os.path.getsize(os.path.join(ROOT, "tests", "golden", "g6_c2mini_5000x50.npz")) * 3 // 4
    assert gen.sha(gen.pca_cells()) == str(g9["pca_raw_sha"])
