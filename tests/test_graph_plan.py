"""Which graph ``MELD.fit`` builds (meld_amd.graph_plan) for each row of DESIGN.md section 4.0's table -- no GPU: the plan reads
shapes and parameters only.  The expectations restate the ``if`` chain ``MELD._build_graph`` held before the plan existed."""
import ast
import os

import pytest

from meld_amd.graph_plan import GraphPlan, plan_graph

BW_REFUSAL = ("bandwidth / bandwidth_scale / knn_max are implemented for the euclidean alpha-decay graphs only -- the sparse kNN "
              "graph, and (without knn_max) the dense graph of thresh=0 -- not with sample_idx or another distance")
CALLABLE_REFUSAL = "Callable bandwidth is only supported by the dense graph of thresh=0 (graphtools.graphs.TraditionalGraph)"
L1_REFUSAL = "distance='l1' is implemented for the plain alpha-decay / unweighted kNN graph only"
SAMPLES = [0] * 300 + [1] * 300


def plan(shape=(600, 10), sparse_input=False, knn=5, decay=40, thresh=1e-4, distance="euclidean", n_pca=None, **opts):
    return plan_graph(shape, sparse_input=sparse_input, knn=knn, decay=decay, thresh=thresh, distance=distance, n_pca=n_pca, opts=opts)


def halve(d):
    return d / 2


# (call, builder, keeps_cells, bw_opts)
ROUTES = [
    (dict(), "knn", True, {}),
    (dict(decay=None), "knn", True, {}),
    (dict(decay=None, thresh=0), "knn", True, {}),  # decay=None is decided before thresh
    (dict(thresh=0), "dense_exact", False, {}),
    (dict(thresh=0, bandwidth=2.0), "dense_exact", False, {"bandwidth": 2.0}),
    (dict(thresh=0, bandwidth=halve), "dense_exact", False, {"bandwidth": halve}),
    (dict(bandwidth=1.5, bandwidth_scale=0.8, knn_max=20), "knn", True, {"bandwidth": 1.5, "bandwidth_scale": 0.8, "knn_max": 20}),
    (dict(knn=127, shape=(300, 10)), "dense_knn", False, {}),
    (dict(knn=127, shape=(128, 10)), "knn", True, {}),  # clipped to N - 2 = 126
    (dict(knn=127, shape=(300, 10), bandwidth=1.0), "knn", True, {"bandwidth": 1.0}),
    (dict(distance="cosine", decay=None, bandwidth=1.0), "knn", True, {}),
    (dict(sample_idx=SAMPLES), "mnn", False, {}),
    (dict(sample_idx=SAMPLES, thresh=0), "dense_mnn", False, {}),
    (dict(sample_idx=SAMPLES, thresh=0, decay=None), "mnn", False, {}),
    (dict(distance="manhattan", shape=(16384, 10)), "dense_metric", True, {}),
    (dict(distance="manhattan", shape=(16385, 10)), "metric_knn", True, {}),
    (dict(distance="chebyshev", shape=(20000, 257)), "dense_metric", True, {}),
    (dict(distance="l1", thresh=0, decay=None), "dense_metric", True, {}),
    (dict(distance="precomputed_distance", shape=(200, 200), n_pca=20), "precomputed", False, {}),
]


@pytest.mark.parametrize("call,builder,keeps_cells,bw_opts", ROUTES)
def test_builder(call, builder, keeps_cells, bw_opts):
    p = plan(**call)
    assert isinstance(p, GraphPlan)
    assert (p.builder, p.keeps_cells, p.bw_opts) == (builder, keeps_cells, bw_opts)
    assert p.reduction is None and p.d == call.get("shape", (600, 10))[1]
    assert p.distance == call.get("distance", "euclidean") and p.symm == (0, 0.0)


# (call, exception, full message)
REFUSALS = [
    (dict(thresh=0, knn_max=10), NotImplementedError, BW_REFUSAL),
    (dict(bandwidth=halve), NotImplementedError, CALLABLE_REFUSAL),
    (dict(distance="cosine", bandwidth=1.0), NotImplementedError, BW_REFUSAL),
    (dict(sample_idx=SAMPLES, bandwidth=1.0), NotImplementedError, BW_REFUSAL),
    (dict(sample_idx=SAMPLES, bandwidth=1.0, decay=None), NotImplementedError, BW_REFUSAL),
    (dict(sample_idx=SAMPLES, kernel_symm="*"), NotImplementedError, "kernel_symm other than '+' with sample_idx (MNN graph) is not implemented"),
    (dict(distance="l1", thresh=0), NotImplementedError, L1_REFUSAL),
    (dict(distance="l1", sample_idx=SAMPLES), NotImplementedError, L1_REFUSAL),
    (dict(distance="precomputed", shape=(200, 150)), ValueError, "Precomputed matrix must be a square matrix. (200, 150) was given"),
    (dict(distance="precomputed_affinity", shape=(200, 150)), ValueError, "Precomputed affinity must be a square matrix. (200, 150) was given"),
    (dict(distance="precomputed", shape=(200, 200), bandwidth=1.0), NotImplementedError,
     "sample_idx / bandwidth options with a precomputed matrix are not implemented"),
    (dict(foo=1), NotImplementedError, "graph options ['foo'] are not implemented by the MI355X graph builder"),
    (dict(kernel_symm="mnn", theta=2.0), ValueError, "theta 2.0 not recognized. Expected a float between 0 and 1"),
    (dict(kernel_symm=None), NotImplementedError,
     "kernel_symm=None (a directed kernel) is not implemented: the filter needs a symmetric Laplacian"),
]


@pytest.mark.parametrize("call,exc,message", REFUSALS)
def test_refusal(call, exc, message):
    with pytest.raises(exc) as e:
        plan(**call)
    assert str(e.value) == message


def test_refusals_keep_their_order():
    # unknown options before kernel_symm, kernel_symm before the metric's own refusal, the bandwidth refusal before the callable one
    with pytest.raises(NotImplementedError, match="graph options"):
        plan(foo=1, kernel_symm="?")
    with pytest.raises(ValueError, match="kernel_symm '\\?' not recognized"):
        plan(distance="l1", thresh=0, kernel_symm="?")
    with pytest.raises(NotImplementedError, match="euclidean alpha-decay graphs only"):
        plan(distance="cosine", bandwidth=halve)
    # a precomputed matrix: its options before its shape
    with pytest.raises(NotImplementedError, match="precomputed matrix are not implemented"):
        plan(distance="precomputed", shape=(200, 150), knn_max=3)


@pytest.mark.parametrize("shape,sparse_input,n_pca,reduction,d", [
    ((600, 200), False, 100, "pca", 100),
    ((600, 200), False, 200, None, 200),
    ((400, 300), True, 20, "svd", 20),
    ((400, 300), True, None, None, 300),
])
def test_reduction(shape, sparse_input, n_pca, reduction, d):
    p = plan(shape=shape, sparse_input=sparse_input, n_pca=n_pca)
    assert (p.builder, p.reduction, p.d) == ("knn", reduction, d)


def test_the_metric_route_sees_the_reduced_width():
    # 300 columns are beyond the L1 search's 256; the 100 PCA scores the builder gets are not
    assert plan(distance="manhattan", shape=(20000, 300)).builder == "dense_metric"
    p = plan(distance="manhattan", shape=(20000, 300), n_pca=100)
    assert (p.builder, p.reduction, p.d, p.metric) == ("metric_knn", "pca", 100, 1)


def test_what_the_executor_reads():
    p = plan(distance="cosine", kernel_symm="mnn", theta=0.25, ksel=64)
    assert (p.front_end, p.transforms_rows, p.metric, p.symm) == (True, True, None, (2, 0.25))
    p = plan(distance="sqeuclidean")
    assert (p.front_end, p.transforms_rows) == (True, False)
    p = plan(distance="Chebyshev", thresh=0, decay=None)
    assert (p.distance, p.front_end, p.metric, p.keeps_cells) == ("chebyshev", False, 2, True)
    assert not plan(distance="manhattan", shape=(16384, 10), kernel_symm="*").front_end
    # plain "precomputed": distances or affinities is for the matrix's first entry to tell
    assert plan(distance="precomputed", shape=(200, 200)).precomputed_kind is None
    assert plan(distance="precomputed_affinity", shape=(200, 200)).precomputed_kind == "affinity"


def test_the_plan_needs_no_torch_to_be_imported():
    path = os.path.join(os.path.dirname(os.path.dirname(__file__)), "meld_amd", "graph_plan.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    names = {a.name for n in top if isinstance(n, ast.Import) for a in n.names} | {n.module for n in top if isinstance(n, ast.ImportFrom)}
    assert names == {"__future__", "dataclasses", "typing"}
