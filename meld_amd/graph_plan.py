"""Which graph ``MELD.fit`` builds, decided before any data is touched.

``plan_graph`` is a pure function of the input's shape and the estimator's parameters: which of the eight builders runs, on which
reduction of the data, with which options, and whether the graph keeps its cells for new ones (``meld_amd/extend.py``).  It raises
every refusal that depends on parameters and shapes alone.  ``MELD._build_graph`` follows the plan and
``distributed.fit_transform_sharded`` asks it which graphs the row-sharded builder builds itself; what depends on the data (NaN /
infinity, the first entry of a ``"precomputed"`` matrix, all-zero rows under the cosine distance, the clipping of
``resolve_graph_params``) is decided by them and by the builders.  DESIGN.md section 4.0 has the table.

No device and no tensor is needed here (``tests/test_graph_plan.py`` runs on the host); the modules that own the limits -- and
import torch -- are imported when the plan is made.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

OPTIONS = ("ksel", "profile", "sample_idx", "bandwidth", "bandwidth_scale", "knn_max", "kernel_symm", "theta")
_BW_OPTIONS = ("bandwidth", "bandwidth_scale", "knn_max")


@dataclass(frozen=True)
class GraphPlan:
    builder: str                # "precomputed" | "metric_knn" | "dense_metric" | "mnn" | "dense_mnn" | "dense_exact" | "dense_knn" | "knn"
    distance: str               # lower-cased
    reduction: Optional[str]    # None, "svd" (sparse input: uncentred truncated SVD) or "pca" (dense input)
    d: int                      # columns the builder sees: n_pca after a reduction
    symm: tuple                 # (mode, theta) of graph.symm_code
    bw_opts: dict               # bandwidth / bandwidth_scale / knn_max as the builder gets them
    keeps_cells: bool           # the graph gets an extension state
    front_end: bool = False     # graph.metric_front_end applies: the euclidean family, where the metric enters through the data
    transforms_rows: bool = False  # ... and changes the rows (cosine, correlation): new cells go through it as well
    metric: Optional[int] = None   # the library's code of an L1 / L-inf metric (metric_knn.METRICS)
    precomputed_kind: Optional[str] = None  # "distance" | "affinity"; None under plain "precomputed": the matrix's first entry tells


def check_options(opts):
    """The refusals that come before anything else, and ``(mode, theta)`` of ``kernel_symm`` / ``theta``
    ([UPSTREAM graphtools ``BaseGraph._check_symmetrization``]; "+" = (K + K^T) / 2 is what the reference runs with)."""
    from .graph import symm_code

    unsupported = [k for k in opts if k not in OPTIONS]
    if unsupported:
        raise NotImplementedError(
            "graph options {} are not implemented by the MI355X graph builder".format(sorted(unsupported))
        )
    symm = symm_code(opts.get("kernel_symm", "+"), opts.get("theta"))
    if symm[0] != 0 and opts.get("sample_idx") is not None:
        raise NotImplementedError("kernel_symm other than '+' with sample_idx (MNN graph) is not implemented")
    return symm


def plan_reduction(shape, sparse_input, distance, n_pca):
    """[UPSTREAM graphtools ``Data._reduce_data``]: the graph is built on ``n_pca`` components where that is fewer than the data
    has -- an uncentred truncated SVD of sparse input, a PCA of dense input; a precomputed matrix is never reduced."""
    if n_pca is None or n_pca >= min(shape) or str(distance).lower().startswith("precomputed"):
        return None
    return "svd" if sparse_input else "pca"


def plan_graph(shape, *, sparse_input, knn, decay, thresh, distance, n_pca, opts):
    """The ``GraphPlan`` of ``MELD(knn, decay, thresh, distance, n_pca, **opts).fit`` on an input of ``shape`` (N, n_features)."""
    from .metric_knn import MAX_KNN, METRICS, metric_route

    symm = check_options(opts)
    name = str(distance).lower()
    N, n_features = int(shape[0]), int(shape[-1])
    if name.startswith("precomputed"):
        # [UPSTREAM graphtools GraphEstimator._parse_input]: the input IS a square matrix of pairwise distances or affinities
        # ("precomputed": told apart by its first diagonal entry, 0 = distances); no reduction, a dense graph
        if any(opts.get(k) is not None for k in ("sample_idx",) + _BW_OPTIONS):
            raise NotImplementedError("sample_idx / bandwidth options with a precomputed matrix are not implemented")
        kind = name[len("precomputed"):].lstrip("_")
        if len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError("Precomputed {} must be a square matrix. {} was given".format(kind or "matrix", tuple(shape)))
        return GraphPlan("precomputed", name, None, n_features, symm, {}, False, precomputed_kind=kind or None)
    reduction = plan_reduction(shape, sparse_input, name, n_pca)
    d = int(n_pca) if reduction else n_features
    if name in METRICS:
        # no function of the euclidean distance of transformed rows, so the matrix pipe's search does not apply: the same kernel on
        # library pairwise distances, densely, up to DENSE_MAX_N cells, and beyond that the exact L1 / L-inf search of metric_knn
        try:
            route = metric_route(N, d, knn, decay, thresh, opts)
        except NotImplementedError:
            raise NotImplementedError("distance={!r} is implemented for the plain alpha-decay / unweighted kNN graph only".format(distance)) from None
        return GraphPlan("metric_knn" if route == "metric_knn" else "dense_metric", name, reduction, d, symm, {},
                         keeps_cells=thresh > 0 or decay is None, metric=METRICS[name])
    # the euclidean family (the metric enters through the data: cosine = the euclidean graph of the unit rows with the decay doubled)
    mnn = opts.get("sample_idx") is not None  # graphtools builds its MNN graph when sample_idx is forwarded (reference test/test_meld.py:34)
    # ([UPSTREAM graphtools api.Graph]: decay=None selects the kNN graph -- unweighted connectivity -- BEFORE thresh is looked at;
    # only an alpha-decay kernel with thresh = 0 is the dense "exact" graph)
    exact = thresh == 0 and decay is not None
    bw_opts = {k: opts[k] for k in _BW_OPTIONS if opts.get(k) is not None}
    if decay is None and not mnn:
        # [UPSTREAM graphtools kNNGraph.build_kernel_to_data]: without alpha decay the kernel is the connectivity of the knn + 1
        # nearest cells and the function returns before it looks at bandwidth, bandwidth_scale or knn_max: accepted, no effect
        bw_opts = {}
    if bw_opts and (mnn or (exact and "knn_max" in bw_opts) or name not in ("euclidean", "l2")):
        raise NotImplementedError("bandwidth / bandwidth_scale / knn_max are implemented for the euclidean alpha-decay graphs only -- the sparse kNN "
                                  "graph, and (without knn_max) the dense graph of thresh=0 -- not with sample_idx or another distance")
    if callable(bw_opts.get("bandwidth")) and not exact:
        # [UPSTREAM graphtools kNNGraph.__init__]: "Callable bandwidth is only supported by graphtools.graphs.TraditionalGraph."
        raise NotImplementedError("Callable bandwidth is only supported by the dense graph of thresh=0 (graphtools.graphs.TraditionalGraph)")
    if mnn:
        builder = "dense_mnn" if exact else "mnn"  # "exact" subgraphs: the dense route
    elif exact:
        builder = "dense_exact"
    elif min(int(knn), N - 2) > MAX_KNN and not bw_opts:
        builder = "dense_knn"  # beyond the candidate lists of the search kernel (128 entries): the same kernel evaluated densely, small N only
    else:
        builder = "knn"
    return GraphPlan(builder, name, reduction, d, symm, bw_opts, keeps_cells=builder == "knn", front_end=True,
                     transforms_rows=name in ("cosine", "correlation"))
