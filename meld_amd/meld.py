"""``MELD`` estimator -- MI355X drop-in for ``meld.MELD`` (reference ``meld/meld.py:13-274``).

Same constructor signature, defaults, validation messages, ``fit`` / ``transform`` /
``fit_transform`` / ``set_params`` behaviour, attributes (``graph``, ``samples``,
``sample_indicators``, ``sample_densities``, ``sample_labels_``) and output layout (DataFrame
``[N, p]``, index = labels' index, columns = sorted unique labels).  The two hot loops run on the
GPU: graph construction (``meld_amd.graph.build_knn_graph``) and the Chebyshev filter
(``meld_amd.filter.filter``).
"""
from __future__ import annotations

from ._options import is_set, opt

from functools import partial

import os

import numpy as np
import pandas as pd
import torch

from . import filter as _filter
from . import sparse as _sparse
from . import utils
from ._device_ops import stream
from .dense import build_dense_graph, build_dense_knn_graph, build_dense_mnn_graph, build_precomputed_graph
from .estimator import GraphEstimator, attribute, check_in, check_int, check_positive
from .extend import attach_extension_state
from .graph import HipOps, build_knn_graph, metric_front_end
from .graph_plan import check_options, plan_graph
from .metric_knn import build_metric_knn_graph
from .mnn import build_mnn_graph

__all__ = ["MELD"]

_FILTER_PARAMS = ("beta", "offset", "order", "solver", "chebyshev_order", "lap_type", "filter")


_LABEL_STREAMS = {}


def _label_stream(dev):
    key = (dev.type, dev.index)
    if key not in _LABEL_STREAMS:
        _LABEL_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _LABEL_STREAMS[key]


class MELD(GraphEstimator):
    """MELD operator for filtering signals over a graph.

    Parameters (reference ``meld/meld.py:16-40``)
    ----------
    beta : int, default 60 -- amount of smoothing
    offset : float, default 0 -- shift of the filter in the (normalised) spectrum, in [0, 1]
    order : int, default 1 -- falloff / squareness of the filter
    filter : {'heat', 'laplacian'}, default 'heat'
    solver : {'chebyshev', 'exact'}, default 'chebyshev'
    chebyshev_order : int, default 50
    lap_type : {'combinatorial', 'normalized'}, default 'combinatorial' (validated and stored;
        like the reference it is never forwarded, the Laplacian is always combinatorial)
    sample_normalize : bool, default True -- indicator columns are scaled to sum to 1
    anisotropy : default 1;  n_landmark : default None (recorded; the filter never uses graphtools' landmark operator,
        ``landmarks()`` builds it with that many landmarks)
    **kwargs : graph parameters -- knn=5, decay=40, n_pca=100, thresh=1e-4,
        distance='euclidean', n_jobs, random_state, verbose; ``ksel`` (candidate list length of the
        GPU search) and ``lmax`` are extensions: a number injects the Laplacian's spectral bound,
        ``"arpack"`` computes it exactly as the reference stack does (pygsp's ``eigsh`` call, on the
        host), default: a tightly converged Lanczos recurrence on the device.
    """

    # class-level defaults differ from the __init__ defaults exactly as in reference meld/meld.py:42-92
    beta = attribute("beta", default=40, on_set=check_positive, doc="Amount of smoothing to apply.")
    offset = attribute("offset", default=0, doc="Shift of the filter in the eigenvalue spectrum, in [0, 1].")
    order = attribute("order", default=1, doc="Falloff and smoothness of the filter.")
    filter = attribute("filter", default="heat", on_set=partial(check_in, ["heat", "laplacian"]),
                       doc="Filter type to use. Should be in ['heat', 'laplacian']")
    solver = attribute("solver", default="chebyshev", on_set=partial(check_in, ["chebyshev", "exact"]),
                       doc="'chebyshev' polynomial approximation or 'exact' eigen-solution.")
    chebyshev_order = attribute("chebyshev_order", default=30, on_set=[check_int, check_positive],
                                doc="Order of chebyshev approximation to use.")
    lap_type = attribute("lap_type", default="combinatorial",
                         on_set=partial(check_in, ["combinatorial", "normalized"]),
                         doc="The kind of Laplacian to calculate")
    sample_densities = attribute("sample_densities", doc="Density associated with each sample")

    def __init__(
        self,
        beta=60,
        offset=0,
        order=1,
        filter="heat",  # noqa: A002
        solver="chebyshev",
        chebyshev_order=50,
        lap_type="combinatorial",
        sample_normalize=True,
        anisotropy=1,
        n_landmark=None,
        **kwargs
    ):
        self.beta = beta
        self.offset = offset
        self.order = order
        self.solver = solver
        self.chebyshev_order = chebyshev_order
        self.lap_type = lap_type
        self.filter = filter
        self.sample_normalize = sample_normalize
        self._lmax_override = kwargs.pop("lmax", None)
        kwargs.pop("use_pygsp", None)  # the reference forces use_pygsp=True; nothing to choose here
        super().__init__(anisotropy=anisotropy, n_landmark=n_landmark, **kwargs)

    # -- state resets (reference meld/meld.py:120-141) -------------------------------------------
    def _reset_graph(self):
        self._reset_filter()

    def _reset_filter(self):
        self.filt = None
        self.sample_densities = None

    def set_params(self, **params):
        params = dict(params)
        for name in _FILTER_PARAMS:
            if name in params:
                value = params.pop(name)
                if value != getattr(self, name):
                    self._reset_filter()
                    setattr(self, name, value)
        if "lmax" in params:
            self._lmax_override = params.pop("lmax")
            self._reset_filter()
            if self.graph is not None and hasattr(self.graph, "lmax_info"):
                self.graph.lmax = None  # whatever bound the graph carries came from the previous setting
        return super().set_params(**params)

    # -- graph construction (replaces graphtools.Graph(...), reference meld/meld.py:117-118,273) ----
    @staticmethod
    def _finite_stats(X):
        """Rejects NaN / infinity in one pass (anywhere in a column, they make its sum non-finite; isfinite(X).all() is three).
        Where the pass can be the builder's own -- sums, minima, maxima of the columns, meld_col_stats_f64 -- returns
        (the HipOps that ran it, its results) for the builder, else (None, None)."""
        ops = col_stats = None
        if X.dim() == 2 and X.shape[1] <= 256 and X.shape[0] > 0 and X.is_contiguous():
            ops = HipOps(X.device)
            col_stats = ops.col_stats(X)
            finite = bool(torch.isfinite(col_stats[0]).all())
        else:
            finite = bool(torch.isfinite(X.sum(dim=0)).all())
        if not finite and not bool(torch.isfinite(X).all()):
            raise ValueError("Input data contains NaN or infinity")
        return ops, col_stats

    def _build_graph(self, data, **kwargs):
        """Follows ``graph_plan.plan_graph``: options, upload and finite check, plan, reduction, metric
        front end, the plan's builder, and one finishing stage for what every graph carries."""
        opts = dict(self.kwargs)
        opts.update(kwargs)
        check_options(opts)
        if not torch.cuda.is_available():
            raise RuntimeError("meld_amd needs a ROCm GPU (MI355X); there is no CPU fallback")
        sparse_input = _sparse.is_sparse_input(data)
        if sparse_input:
            # sparse input (meld_amd/sparse.py) stays CSR on the device up to its reduction; its values are checked on upload
            # and the matrix the builder sees -- scores, or densified where nothing reduces it -- below
            data = _sparse.DeviceCSR.from_input(data)
        elif isinstance(data, torch.Tensor):
            data = data.to(device="cuda", dtype=torch.float64)
        else:
            data = torch.from_numpy(data).to("cuda")
            if data.dtype != torch.float64:
                data = data.to(torch.float64)  # (float32 input: widened here, after the copy)
        ops0, col_stats = (None, None) if sparse_input else self._finite_stats(data)
        plan = plan_graph(tuple(data.shape), sparse_input=sparse_input, knn=self.knn, decay=self.decay, thresh=self.thresh,
                          distance=self.distance, n_pca=self.n_pca, opts=opts)
        red = _sparse.reduce_data(data, plan.reduction, self.n_pca, self.random_state, log=self._log)
        X_in = X = red.scores
        del data  # (a device CSR matrix has served its purpose)
        if sparse_input:
            ops0, col_stats = self._finite_stats(X)
        self.data_nu = X if plan.reduction else None
        decay_m, bw_to_metric = self.decay, None
        if plan.front_end:
            X, decay_m, bw_to_metric = metric_front_end(X, plan.distance, self.decay)
        decay_inf = float("inf") if decay_m is None else decay_m  # None: the unweighted kNN graph = a 0 / 1 kernel
        bw, ksel = plan.bw_opts, opts.get("ksel")
        if plan.builder == "precomputed":
            kind = plan.precomputed_kind or ("distance" if float(X[0, 0]) == 0.0 else "affinity")
            G = build_precomputed_graph(X, kind, knn=self.knn, decay=self.decay, thresh=self.thresh, anisotropy=self.anisotropy, symm=plan.symm)
        elif plan.builder == "metric_knn":
            G = build_metric_knn_graph(X, self.knn, self.decay, self.thresh, self.anisotropy, plan.distance,
                                       kernel_symm=opts.get("kernel_symm", "+"), theta=opts.get("theta"), ksel=ksel,
                                       profile=bool(opts.get("profile", False)), ops=ops0)
        elif plan.builder in ("dense_metric", "dense_knn"):
            G = build_dense_knn_graph(X, self.knn, decay_m, self.thresh, anisotropy=self.anisotropy, symm=plan.symm,
                                      metric=plan.distance if plan.metric else "euclidean")
        elif plan.builder == "dense_mnn":
            G = build_dense_mnn_graph(X, opts["sample_idx"], knn=self.knn, decay=decay_m, anisotropy=self.anisotropy)
        elif plan.builder == "mnn":
            G = build_mnn_graph(X, opts["sample_idx"], knn=self.knn, decay=decay_inf, thresh=self.thresh, anisotropy=self.anisotropy, ksel=ksel)
        elif plan.builder == "dense_exact":
            G = build_dense_graph(X, knn=self.knn, decay=decay_m, anisotropy=self.anisotropy, symm=plan.symm,
                                  bandwidth=bw.get("bandwidth"), bandwidth_scale=bw.get("bandwidth_scale", 1.0))
        else:
            G = build_knn_graph(
                X, knn=self.knn, decay=decay_inf, thresh=self.thresh, anisotropy=self.anisotropy,
                ksel=ksel, profile=bool(opts.get("profile", False)), **bw,
                # (the column statistics are those of the cells the graph is built on: not after a reduction / a metric front end)
                col_stats=col_stats if (plan.reduction is None and X is X_in) else None,
                kernel_symm=opts.get("kernel_symm", "+"), theta=opts.get("theta"), ops=ops0,
            )
        G.bandwidth_to_metric = bw_to_metric
        # n_landmark (reference meld/meld.py:105,118 forwards it to graphtools): a graphtools LandmarkGraph has the same kernel,
        # weights and Laplacian as the plain graph -- the landmark operator is a lazily built extra that MELD's filter never
        # touches -- so the parameter is recorded here and the operator is built on request (``landmarks()``, meld_amd/landmark.py)
        G.n_landmark = self.n_landmark
        if plan.keeps_cells:
            # what new cells need (meld_amd/extend.py): the matrix the search saw, in the caller's order (a reference: the graph
            # pins it), the model that maps a raw cell to it, the kernel's parameters in the units of the search
            row_fn = (lambda Q, m=plan.distance: metric_front_end(Q, m, None)[0]) if plan.transforms_rows else None
            attach_extension_state(G, X, red.n_features_in, red.project, row_fn, knn=int(self.knn), decay=decay_inf, thresh=self.thresh,
                                   bandwidth=bw.get("bandwidth"), bandwidth_scale=bw.get("bandwidth_scale"), knn_max=bw.get("knn_max"),
                                   ksel=None if plan.metric else ksel, metric=plan.metric, model=red.model)
        return G

    # -- indicators (reference meld/meld.py:143-191) ------------------------------------------------
    @staticmethod
    def _factorize(labels):
        """(codes, sorted uniques) of a 1-D label array, equal to ``np.unique(labels,
        return_inverse=True)`` but by hashing: O(N) instead of a sort of N strings (0.1-1 s at
        1M cells).  Fixed-width numpy strings are factorised as
        integer columns (exact, no string hashing)."""
        labels = np.asarray(labels)
        if labels.dtype.kind in "US" and labels.dtype.itemsize % 8 == 0 and labels.size:
            cols = np.ascontiguousarray(labels).view(np.uint64).reshape(labels.shape[0], -1)
            codes = np.zeros(labels.shape[0], dtype=np.int64)
            for c in range(cols.shape[1]):
                cc, cu = pd.factorize(cols[:, c], sort=False)
                codes, _ = pd.factorize(codes * len(cu) + cc, sort=False)
            first = np.full(int(codes.max()) + 1, -1, dtype=np.int64)
            first[codes[::-1]] = np.arange(labels.shape[0] - 1, -1, -1)  # first occurrence of each code
            uniques = labels[first]
        else:
            codes, uniques = pd.factorize(labels, sort=False)
            uniques = np.asarray(uniques)
        order = np.argsort(uniques, kind="stable")  # the p uniques, ordered as np.unique does
        rank = np.empty_like(order)
        rank[order] = np.arange(order.shape[0])
        return rank[codes], uniques[order]

    # labels below this many cells are factorised on the host (the device path costs a few launches)
    _DEVICE_FACTORIZE_MIN = 200_000

    @staticmethod
    def _factorize_device(labels, device):
        """``_factorize`` on the GPU for fixed-width string / integer labels: the raw label words go over PCIe once and
        ``meld_factorize_labels`` groups them (whole labels compared word by word: exact).  Returns (codes as an int64
        device tensor, sorted uniques, label counts), or None when the dtype is not eligible or there are more distinct
        labels than the device dictionary holds (the host path then factorises)."""
        return MELD._factorize_device_end(MELD._factorize_device_begin(labels, device))

    @staticmethod
    def _factorize_device_begin(labels, device):
        """The device half of ``_factorize_device``: everything up to the first value the host has to read, enqueued on
        the current stream (``meld_factorize_labels``, csrc/labels.hip: a dictionary of the distinct labels built in LDS,
        whole labels compared word by word).  ``fit_transform`` runs it on a side stream while the candidate search
        occupies the main one and reads the results (``_factorize_device_end``) after the graph is built."""
        from ._lib import check, get_lib, ptr

        lab = np.ascontiguousarray(labels)
        if lab.dtype.kind in "US" and lab.dtype.itemsize % 4 == 0 and lab.dtype.itemsize > 0:
            words = lab.view(np.int32).reshape(lab.shape[0], -1)
        elif lab.dtype.kind in "iu" and lab.dtype.itemsize == 8:
            words = lab.view(np.int32).reshape(lab.shape[0], -1)
        else:
            return None
        lib = get_lib()
        n, w = int(words.shape[0]), int(words.shape[1])
        if n == 0 or w > lib.meld_factorize_max_words():
            return None
        st = stream()
        t = torch.from_numpy(words).to(device)
        tb = lib.meld_factorize_temp_bytes(n)
        temp = torch.empty(tb, dtype=torch.uint8, device=device)
        G = lib.meld_factorize_max_groups()
        head = torch.empty(2 + 2 * G, dtype=torch.int64, device=device)
        check(lib.meld_factorize_labels(ptr(t), n, w, ptr(temp), tb, ptr(head), st), "meld_factorize_labels")
        head_h = torch.empty(2 + 2 * G, dtype=torch.int64, pin_memory=True)
        head_h.copy_(head, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        return dict(lab=lab, n=n, temp=temp, head=head, head_h=head_h, words=t, done=done, device=device, G=G)

    @staticmethod
    def _factorize_device_end(h):
        if h is None:
            return None
        from ._lib import check, get_lib, ptr

        h["done"].synchronize()
        cur = torch.cuda.current_stream()
        cur.wait_event(h["done"])
        for t in (h["temp"], h["head"], h["words"]):
            # allocated from the side stream's pool, consumed from here on by the current stream: without this the caching
            # allocator may hand their blocks to the next side-stream hook while kernels of this stream still read them
            t.record_stream(cur)
        lab, G, device, n = h["lab"], h["G"], h["device"], h["n"]
        head = h["head_h"].numpy()  # [status | groups | first row of every group | group sizes]
        if int(head[0]) != 0:
            return None  # more distinct labels than the device dictionary holds: the host factorises
        n_groups = int(head[1])
        uniques = lab[head[2 : 2 + n_groups]]
        order = np.argsort(uniques, kind="stable")  # the p uniques, ordered as np.unique does
        rank = np.empty(n_groups, dtype=np.int32)
        rank[order] = np.arange(n_groups, dtype=np.int32)
        codes = torch.empty(n, dtype=torch.int64, device=device)
        lib = get_lib()
        check(lib.meld_factorize_codes(ptr(h["temp"]), n, ptr(torch.from_numpy(rank).to(device)), ptr(codes), stream()), "meld_factorize_codes")
        counts = head[2 + G : 2 + G + n_groups][order].copy()
        return codes, uniques[order], counts

    @staticmethod
    def _flatten_labels(sample_labels):
        labels = np.asarray(getattr(sample_labels, "values", sample_labels))
        if labels.ndim > 1:
            if labels.shape[1] == 1:
                labels = labels.reshape(-1)
            else:
                raise ValueError("sample_labels must be a single column. Got" "shape={}".format(labels.shape))
        return labels

    def _create_sample_indicators(self, sample_labels, _factorized=None, _materialize=True):
        """One 0/1 column per sample label, columns sorted like ``np.unique``."""
        self.sample_labels_ = sample_labels
        labels = self._flatten_labels(sample_labels)
        codes, self.samples = _factorized if _factorized is not None else self._factorize(labels)
        self._codes = codes
        self._indicator_scale = None  # 0/1 indicators
        self._sample_indicators = None
        return self.sample_indicators if _materialize else None

    @property
    def sample_indicators(self):
        """DataFrame [N, p] of the (optionally column-normalised) sample indicators.  Built on
        first access from the label codes: the filter itself assembles the signal on the device."""
        if getattr(self, "_sample_indicators", None) is None and getattr(self, "_codes", None) is not None:
            codes = self._codes.cpu().numpy() if isinstance(self._codes, torch.Tensor) else self._codes
            n, p = codes.shape[0], self.samples.shape[0]
            if self._indicator_scale is None:
                arr = np.zeros((n, p), dtype=np.int64)
                arr[np.arange(n), codes] = 1
            else:
                arr = np.zeros((n, p), dtype=np.float64)
                arr[np.arange(n), codes] = self._indicator_scale[codes]
            self._sample_indicators = pd.DataFrame(arr, index=getattr(self, "_labels_index", None), columns=self.samples)
        return getattr(self, "_sample_indicators", None)

    @sample_indicators.setter
    def sample_indicators(self, value):
        self._sample_indicators = value

    # -- transform (reference meld/meld.py:193-250) -------------------------------------------------
    def transform(self, sample_labels):
        """Filters the sample indicators of ``sample_labels`` over the data graph and returns
        the ``[N, p]`` sample densities as a DataFrame."""
        self.graph = utils._check_pygsp_graph(self.graph)
        self._sample_labels = sample_labels

        if sample_labels.shape[0] != self.graph.N:
            raise ValueError(
                "Input data ({}) and input graph ({}) "
                "are not of the same size".format(sample_labels.shape, self.graph.N)
            )
        raw = np.asarray(getattr(sample_labels, "values", sample_labels))
        factorized = None
        self._label_counts = None
        if raw.ndim == 1 or (raw.ndim == 2 and raw.shape[1] == 1):
            flat = raw.reshape(-1)
            dev = getattr(getattr(self.graph, "val", None), "device", None)
            pre = getattr(self, "_prefactored", None)
            if pre is not None and pre[0] is sample_labels and dev is not None and pre[1][0].device == dev:
                on_device = pre[1]  # (fit_transform factorised them before the graph build)
                factorized = on_device[:2]
                self._label_counts = on_device[2]
            elif flat.shape[0] >= self._DEVICE_FACTORIZE_MIN and dev is not None and dev.type == "cuda":
                on_device = self._factorize_device(flat, dev)
                if on_device is not None:
                    factorized = on_device[:2]
                    self._label_counts = on_device[2]
            if factorized is None:
                factorized = self._factorize(flat)  # one pass serves both checks below
            n_unique = factorized[1].shape[0]
        else:
            n_unique = len(pd.unique(raw.ravel()))
        if n_unique == 1:
            raise ValueError(
                "Found only one unqiue sample label. Cannot estimate density " "of a single sample."
            )
        self._labels_index = sample_labels.index if hasattr(sample_labels, "index") else None

        # (the [N, p] DataFrame of indicators is only built if someone reads ``sample_indicators``)
        self._create_sample_indicators(sample_labels, _factorized=factorized, _materialize=False)
        if self.sample_normalize:
            # each indicator column divided by its sum (reference meld/meld.py:229-232): the column sums
            # are the label counts, so the normalised signal is 1/count at the cell's own label
            counts = self._label_counts if self._label_counts is not None else np.bincount(self._codes, minlength=self.samples.shape[0])
            counts = np.asarray(counts, dtype=np.float64)
            self._indicator_scale = 1.0 / counts
            self._sample_indicators = None

        if isinstance(self._lmax_override, str):
            # "arpack": the reference's own estimate on the host (pygsp's eigsh call); "lanczos": the default
            self.graph.estimate_lmax(method=self._lmax_override)
        elif self._lmax_override is not None:
            self.graph.lmax = self._lmax_override
        # the signal is a scaled one-hot: hand the filter the label codes (4 B per cell over PCIe instead
        # of 8p) and let it assemble the [N, p] matrix on the device
        signal = _filter.IndicatorSignal(self._codes, self.samples.shape[0], self._indicator_scale)
        densities = _filter.filter(
            signal=signal,
            graph=self.graph,
            filter=self.filter,
            beta=self.beta,
            offset=self.offset,
            order=self.order,
            solver=self.solver,
            chebyshev_order=self.chebyshev_order,
        )
        self.sample_densities = pd.DataFrame(densities, index=self._labels_index, columns=self.samples)
        return self.sample_densities

    def transform_sweep(self, sample_labels, betas):
        """``{beta: transform(sample_labels) with that beta}`` for a list of betas in ONE pass over the
        graph (the Chebyshev polynomials of L applied to the indicators do not depend on beta; only the
        coefficients do).  Parameter-sweep mode of SURVEY.md section 8f row 3; no reference counterpart
        beyond the loop of ``meld/benchmark.py:186-200``."""
        if self.solver != "chebyshev":
            raise NotImplementedError("transform_sweep supports solver='chebyshev' only")
        saved = self.beta
        first = self.transform(sample_labels)  # validation, indicators, lmax -- and the result for self.beta
        signal = _filter.IndicatorSignal(self._codes, self.samples.shape[0], self._indicator_scale)
        R = _filter.filter_sweep(signal, self.graph, self.filter, betas, offset=self.offset, order=self.order,
                                 chebyshev_order=self.chebyshev_order)
        out = {}
        for b, beta in enumerate(betas):
            out[beta] = pd.DataFrame(R[b], index=self._labels_index, columns=self.samples)
        self.beta = saved
        self.sample_densities = first
        return out

    def transform_new(self, Y):
        """The fitted sample densities interpolated to cells that were not in ``fit``: ``graph.interpolate(sample_densities,
        Y=Y)`` -- the kernel from the new cells to the fitted ones ([UPSTREAM graphtools ``kNNGraph.build_kernel_to_data``]),
        l1-normalised by row, applied to the densities on the device.  ``Y``: array, tensor or DataFrame with the columns of
        the data ``fit`` saw (or the reduced ones).  Returns a DataFrame ``[M, p]`` with the columns of ``sample_densities``
        and ``Y``'s index where it has one; ``meld.utils.normalize_densities`` applies to it as it is.  Call after
        ``transform`` / ``fit_transform``."""
        if self.sample_densities is None or self.graph is None:
            raise ValueError("sample_densities must be set prior to running transform_new(): call transform() or fit_transform() first.")
        G = self.graph
        if not hasattr(G, "interpolate"):
            raise NotImplementedError("the graph of this estimator cannot be extended to new cells")
        values = G.interpolate(np.ascontiguousarray(self.sample_densities.values, dtype=np.float64), Y=Y)
        index = Y.index if isinstance(Y, (pd.DataFrame, pd.Series)) else None
        return pd.DataFrame(values, index=index, columns=self.sample_densities.columns)

    def fit(self, X, **kwargs):
        """``GraphEstimator.fit``; where ``X`` is a DataFrame its column names and index are kept with the graph's model of the
        data (``impute`` labels its result with them)."""
        super().fit(X, **kwargs)
        st = getattr(self.graph, "_extend_state", None)
        if st is not None and not getattr(self, "_graph_precomputed", False):  # (a graph handed to fit keeps what it came with)
            frame = isinstance(X, pd.DataFrame)
            st.columns = X.columns if frame else None
            st.index = X.index if frame else None
            if isinstance(X, _sparse.DeviceCSR):  # (a preprocessed matrix carries the labels of the frame it was made from)
                st.columns = None if X.gene_names is None else pd.Index(X.gene_names)
                st.index = None if X.cell_index is None else pd.Index(X.cell_index)
        return self

    def impute(self, genes=None, t=3):
        """MAGIC's approximate solver on the fitted graph ([UPSTREAM magic-impute ``MAGIC.fit_transform(data, genes=...)``,
        unpinned: it cannot be imported next to this code]): the matrix the graph was searched on (the PCA or SVD scores, or the
        data where ``fit`` reduced nothing) is diffused ``t`` times with the graph's ``diff_op`` on the device and mapped back to
        the requested columns of the data ``fit`` saw -- ``X_t V[genes].T + mean[genes]`` (PCA), ``X_t V[genes].T`` (the uncentred
        SVD of sparse input), the columns themselves without a reduction -- by one GEMM.

        ``genes``: integers, a boolean mask over the columns, names (where ``fit`` received a DataFrame), or None for every
        column.  ``t``: an integer >= 0 (``"auto"`` is not implemented).  Returns a DataFrame ``[N, len(genes)]`` with the cells'
        index and the genes' names (the integers where ``fit`` saw no names).  NotImplementedError, naming the case, for a graph
        that keeps no cells (``fit(G)``, adopted graphs, precomputed matrices), for the metrics that transform the rows (cosine,
        correlation) and for a row-sharded graph.  For any other per-cell signal -- raw marker genes, densities -- call
        ``op.graph.diffuse(signal, t)``."""
        from . import diffuse

        if self.graph is None:
            raise ValueError("Estimator must be `fit` before running `impute`.")
        if not hasattr(self.graph, "diffuse_device"):
            raise NotImplementedError("the graph of this estimator cannot diffuse a signal")
        values, idx = diffuse.impute(self.graph, genes=genes, t=t)
        st = self.graph._extend_state
        columns = idx if getattr(st, "columns", None) is None else st.columns[idx]
        return pd.DataFrame(values.cpu().numpy(), index=getattr(st, "index", None), columns=columns)

    def geodesic(self, sources, distance=None):
        """Distances along the fitted graph from the cells ``sources`` (positions: integers or a boolean mask over the cells) to
        every cell ([UPSTREAM graphtools ``BaseGraph.shortest_path``]): a DataFrame ``[N, len(sources)]`` with the fitted cells'
        index, its columns labelled by the sources' index labels (their positions where ``fit`` saw no index); ``inf`` where there
        is no path.  ``distance``: ``"affinity"`` (``-log`` of the weights), ``"data"`` (euclidean distances of the cells the graph
        was searched on), ``"constant"`` (hops); None: ``"constant"`` for ``decay=None``, else ``"affinity"``.  See
        ``DeviceGraph.shortest_path_device``."""
        from . import geodesic

        if self.graph is None:
            raise ValueError("Estimator must be `fit` before running `geodesic`.")
        if not hasattr(self.graph, "shortest_path_device"):
            raise NotImplementedError("the graph of this estimator cannot compute shortest paths")
        values, idx = geodesic.geodesic(self.graph, sources, distance=distance)
        index = getattr(getattr(self.graph, "_extend_state", None), "index", None)
        return pd.DataFrame(values.cpu().numpy(), index=index, columns=idx if index is None else index[idx])

    def landmarks(self, **kwargs):
        """The landmark record of the fitted graph ([UPSTREAM graphtools ``LandmarkGraph``], what ``n_landmark`` yields there):
        ``DeviceGraph.landmarks(**kwargs)`` -- ``n_landmark`` defaults to the estimator's, ``clusters`` passes labels in."""
        if self.graph is None:
            raise ValueError("Estimator must be `fit` before running `landmarks`.")
        if not hasattr(self.graph, "landmarks"):
            raise NotImplementedError("the graph of this estimator cannot build landmarks")
        return self.graph.landmarks(**kwargs)

    def phate(self, **kwargs):
        """The PHATE embedding of the fitted cells ([UPSTREAM phate ``PHATE.fit_transform``], what the reference's notebooks plot
        the densities over): ``DeviceGraph.phate(**kwargs).embedding`` as a DataFrame ``[N, n_components]`` with the fitted cells'
        index and the columns ``PHATE1``, ``PHATE2``, ...; the record itself (stress, ``t``, ``transform`` for new cells) is
        ``op.graph.phate(**kwargs)``, kept on the graph."""
        if self.graph is None:
            raise ValueError("Estimator must be `fit` before running `phate`.")
        if not hasattr(self.graph, "phate"):
            raise NotImplementedError("the graph of this estimator cannot build a PHATE embedding")
        coords = self.graph.phate(**kwargs).embedding
        index = getattr(getattr(self.graph, "_extend_state", None), "index", None)
        return pd.DataFrame(coords, index=index, columns=["PHATE{}".format(c + 1) for c in range(coords.shape[1])])

    def louvain(self, **kwargs):
        """Louvain communities of the fitted cells (what the reference's comparison takes from ``sc.tl.louvain``):
        ``DeviceGraph.louvain(**kwargs).labels`` as a Series named ``"louvain"`` on the fitted cells' index; the record itself
        (modularity, levels, the dendrogram) is ``op.graph.louvain(**kwargs)``, kept on the graph."""
        if self.graph is None:
            raise ValueError("Estimator must be `fit` before running `louvain`.")
        if not hasattr(self.graph, "louvain"):
            raise NotImplementedError("the graph of this estimator cannot find communities")
        labels = self.graph.louvain(**kwargs).labels
        index = getattr(getattr(self.graph, "_extend_state", None), "index", None)
        return pd.Series(labels, index=index, name="louvain")

    def leiden(self, **kwargs):
        """Leiden communities of the fitted cells (what the reference's comparison takes from ``sc.tl.leiden``):
        ``DeviceGraph.leiden(**kwargs).labels`` as a Series named ``"leiden"`` on the fitted cells' index; the record itself
        (modularity, levels, the dendrogram) is ``op.graph.leiden(**kwargs)``, kept on the graph."""
        if self.graph is None:
            raise ValueError("Estimator must be `fit` before running `leiden`.")
        if not hasattr(self.graph, "leiden"):
            raise NotImplementedError("the graph of this estimator cannot find communities")
        labels = self.graph.leiden(**kwargs).labels
        index = getattr(getattr(self.graph, "_extend_state", None), "index", None)
        return pd.Series(labels, index=index, name="leiden")

    def rank_sum_test(self, data, groups=None, group=None, reference=None, gene_names=None):
        """Which genes differ between groups of cells: the Wilcoxon rank-sum test per gene on the device
        (``meld_amd.diffexp.rank_sum_test``; the reference's notebooks end with ``de.test.two_sample(..., test='rank')``).
        ``groups``: one label per cell -- clusters, thresholded likelihoods, ...; omitted after ``transform``, the cells' sample
        labels are used.  ``data`` (cells x genes) is always passed: ``fit`` keeps the graph, not the expression matrix -- the
        device CSR matrix is dropped once it is reduced -- so hold a ``DeviceCSR`` yourself to test it more than once without
        another upload and transpose."""
        from .diffexp import rank_sum_test

        if groups is None:
            groups = getattr(self, "_sample_labels", None)
            if groups is None:
                raise ValueError("rank_sum_test: pass `groups`, or run `transform` first to test between the sample labels")
        return rank_sum_test(data, groups, group=group, reference=reference, gene_names=gene_names)

    def fit_transform(self, X, sample_labels, **kwargs):
        """Builds the graph on ``X`` and estimates the density of each sample in
        ``sample_labels`` (reference ``meld/meld.py:252-274``)."""
        finish = self._prefactor_under_search(sample_labels, eligible=not isinstance(X, str))
        try:
            try:
                self.fit(X, **kwargs)
            except BaseException:
                finish(publish=False)  # (the hook is withdrawn, its device work dropped: a failed fit leaves no factorisation behind)
                raise
            finish()
            return self.transform(sample_labels)
        finally:
            self._prefactored = None

    def _prefactor_under_search(self, sample_labels, eligible=True):
        """The label factorisation of ``transform`` (fixed-width labels of large inputs: a host-blocking copy, a sort, a few
        gathers, two read-backs -- 1.2 ms at 1M cells) is independent of the graph: it is started by the graph build right
        after the candidate search has been launched (``graph._WHILE_SEARCHING``), on a side stream, while the host would
        otherwise wait for the search.  Returns ``finish()``: call it after the build; it reads the results and leaves them
        in ``self._prefactored`` for the ``transform`` that follows (or leaves nothing, and ``transform`` factorises as usual)."""
        self._prefactored = None
        pending, hook = {}, None
        try:
            raw = np.asarray(getattr(sample_labels, "values", sample_labels))
            if eligible and (raw.ndim == 1 or (raw.ndim == 2 and raw.shape[1] == 1)) and raw.shape[0] >= self._DEVICE_FACTORIZE_MIN \
                    and torch.cuda.is_available() and opt("MELD_LABEL_OVERLAP", "1") != "0":
                from . import graph as _graph

                dev = torch.device("cuda", torch.cuda.current_device())
                flat = raw.reshape(-1)

                def hook():
                    # runs inside the graph build, right after the candidate search has been launched: the copy of the
                    # labels blocks a host that would otherwise wait for the search, and the launches share the GPU with it
                    try:
                        side = _label_stream(dev)
                        with torch.cuda.stream(side):
                            pending["h"] = self._factorize_device_begin(flat, dev)
                    except Exception:  # (anything unusual about the labels is reported by transform's own checks)
                        pending["h"] = None

                _graph._WHILE_SEARCHING.append(hook)
        except Exception:
            hook = None

        def finish(publish=True):
            if hook is not None:
                from . import graph as _graph

                if hook in _graph._WHILE_SEARCHING:  # (no search was launched: small N, a precomputed graph, ...)
                    _graph._WHILE_SEARCHING.remove(hook)
            if not publish:
                pending.pop("h", None)
                return
            if pending.get("h") is not None:
                try:
                    fz = self._factorize_device_end(pending["h"])
                except Exception:
                    fz = None
                if fz is not None:
                    self._prefactored = (sample_labels, fz)

        return finish
