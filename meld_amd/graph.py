"""Device-resident alpha-decay kNN graph: the MI355X replacement of ``graphtools.Graph``.

The reference builds its graph with ``graphtools.Graph(X, knn, decay, thresh, anisotropy=1,
use_pygsp=True, ...)`` (reference ``meld/meld.py:117-118,273``) and hands a PyGSP graph to
``meld/filter.py``.  ``DeviceGraph`` offers the attributes that path touches -- ``N``
(``meld/meld.py:209``), ``estimate_lmax()`` / ``lmax`` (``meld/filter.py:39,45``) -- plus host
exports (``W``, ``K``, ``L``, ``dw``) for inspection and tests.  All arithmetic is done by the HIP
kernels of ``libmeld_hip.so``; torch only owns the device memory and the stream.
"""
from __future__ import annotations

from ._options import opt

import math
import time

from types import SimpleNamespace

import numpy as np
import torch

from ._device_ops import coo_merge, csr_from_keys, scan_i32, sort_pairs, stream
from ._device_ops import stream as _stream  # (the name the contract tests import from here)
from ._lib import check, get_lib, ptr
from .knn_plan import SearchOptions, bucket_route, plan_knn_search, search_nprod, sphere_layout

__all__ = ["DeviceGraph", "build_knn_graph", "default_ksel", "EVENTS", "record_events"]

# Optional HIP-event timing of the hot kernels (bench.py turns it on).  Events are recorded on
# the stream the kernels are launched on (torch's current stream).
EVENTS = {"enabled": False, "pairs": []}


def record_events(enabled=True):
    EVENTS["enabled"] = bool(enabled)
    EVENTS["pairs"] = []


class _EventSpan:
    def __init__(self, name, **meta):
        self.name, self.meta = name, meta

    def __enter__(self):
        if EVENTS["enabled"]:
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            self.a.record()
        return self

    def __exit__(self, *exc):
        if EVENTS["enabled"]:
            self.b.record()
            EVENTS["pairs"].append((self.name, self.a, self.b, self.meta))
        return False


def event_times_ms():
    """name -> list of elapsed ms (call after a device sync)."""
    out = {}
    for name, a, b, meta in EVENTS["pairs"]:
        out.setdefault(name, []).append(a.elapsed_time(b))
    return out


def default_ksel(knn):
    """Candidate-list length of the search kernel: ~4x the (knn+1) nearest, in [32, 128].
    (graphtools searches 6*(knn+1) first [UPSTREAM search_multiplier]; rows that need more go
    through the exact radius sweep exactly as graphtools re-searches them.)"""
    k = 4 * (knn + 1)
    k = ((k + 31) // 32) * 32
    return int(min(128, max(32, k)))


class _Timer:
    """Per-stage wall times (host clock around a device sync); only active when asked for."""

    def __init__(self, enabled):
        self.enabled = enabled
        self.t = {}
        self._t0 = None

    def start(self):
        if self.enabled:
            torch.cuda.synchronize()
            self._t0 = time.perf_counter()

    def stop(self, name):
        if self.enabled:
            torch.cuda.synchronize()
            self.t[name] = self.t.get(name, 0.0) + time.perf_counter() - self._t0
            self._t0 = time.perf_counter()


class _HookList(list):
    """Callables run once by the next directed_kernel_coo OF THIS THREAD right after it has launched the candidate search
    (fit_transform's label factorisation).  Per thread: two builds running concurrently must not run each other's hooks."""


class _PerThreadHooks:
    def __init__(self):
        import threading

        self._tls = threading.local()

    def _lst(self):
        lst = getattr(self._tls, "hooks", None)
        if lst is None:
            lst = self._tls.hooks = _HookList()
        return lst

    def append(self, h):
        self._lst().append(h)

    def remove(self, h):
        self._lst().remove(h)

    def pop(self):
        return self._lst().pop()

    def __contains__(self, h):
        return h in self._lst()

    def __bool__(self):
        return bool(self._lst())

    def __len__(self):
        return len(self._lst())


_WHILE_SEARCHING = _PerThreadHooks()


class DeviceGraph:
    """Symmetric weight matrix W (CSR, fp64 values, int32 columns, no diagonal) and degrees
    ``dw = W 1`` resident in HBM; ``L = diag(dw) - W`` is applied on the fly, never stored.

    Attributes mirror what callers of the PyGSP graph use: ``N``, ``lmax``, ``estimate_lmax()``,
    and (host-side, lazily copied) ``W``, ``K``, ``L``, ``dw``.
    """

    def __init__(self, rowptr, col, val, dw, ksum=None, anisotropy=1.0, row_begin=0, n_total=None, info=None):
        self.rowptr = rowptr  # int64 [n_rows + 1]
        self.col = col  # int32 [nnz]
        self.val = val  # fp64  [nnz]
        self.dw_dev = dw  # fp64  [n_rows]
        self.ksum = ksum  # fp64  [N] row sums of the symmetrised kernel (diag included)
        self.anisotropy = float(anisotropy)
        self.n_rows = int(rowptr.shape[0] - 1)
        self.row_begin = int(row_begin)
        self.N = int(n_total if n_total is not None else self.n_rows)
        self.nnz = int(col.shape[0])
        self.info = info or {}
        self._lmax = None
        self.lmax_info = {}
        # sharding: a single-GPU graph is one shard that owns every row
        self.rows_pad = self.n_rows  # local rows incl. padding (equal on every rank)
        self.n_pad = self.N  # global rows incl. padding
        self.comm = None
        self.ops = None
        # cache-locality permutation (device int64, new -> old index) or None: the device arrays are
        # in the permuted order, every host-facing export and the filter input/output use the
        # caller's original order
        self.perm = None
        self.bandwidth = None
        self.n_landmark = None

    @classmethod
    def from_scipy(cls, W, device="cuda"):
        """Upload a symmetric, zero-diagonal scipy.sparse weight matrix (e.g. ``G.W`` of a graph
        built elsewhere) -- the counterpart of handing a prebuilt graph to ``MELD.fit``
        (reference ``meld/benchmark.py:194-195``)."""
        from scipy import sparse

        W = sparse.csr_matrix(W).astype(np.float64)
        W.sort_indices()
        if W.shape[0] != W.shape[1]:
            raise ValueError("W must be square")
        rowptr = torch.from_numpy(W.indptr.astype(np.int64)).to(device)
        col = torch.from_numpy(W.indices.astype(np.int32)).to(device)
        val = torch.from_numpy(W.data.astype(np.float64)).to(device)
        dw = torch.from_numpy(np.ravel(W.sum(1)).astype(np.float64)).to(device)
        return cls(rowptr, col, val, dw, ksum=None, anisotropy=0.0)

    @classmethod
    def from_foreign(cls, G, W=None, device="cuda"):
        """Adopt a graph object built elsewhere (graphtools / pygsp: anything with a square
        scipy-sparse ``.W``): upload its weights, keep the spectral bound it already carries
        (pygsp caches ``estimate_lmax`` in ``_lmax``; its ``estimate_lmax`` is then a no-op, and so
        is ours) and, when it exposes graphtools' kernel ``.K``, the kernel's diagonal (used by
        ``VertexFrequencyCluster``'s diffusion operator)."""
        from scipy import sparse

        if not torch.cuda.is_available():
            raise RuntimeError("meld_amd needs a ROCm GPU (MI355X); there is no CPU fallback")
        W = sparse.csr_matrix(G.W if W is None else W)
        if W.diagonal().any():
            W = (W - sparse.diags(W.diagonal(), 0)).tocsr()  # weights carry no self loops (pygsp's W)
            W.eliminate_zeros()
        out = cls.from_scipy(W, device=device)
        lm = getattr(G, "_lmax", None)
        if lm is None and isinstance(getattr(type(G), "lmax", None), property) is False:
            lm = getattr(G, "lmax", None)  # a plain attribute (not pygsp's computing property)
        if lm is not None and np.isfinite(lm) and lm > 0:
            out.lmax = float(lm)
        try:
            K = getattr(G, "K", None)
        except Exception:
            K = None
        if K is not None and sparse.issparse(K) and K.shape == W.shape:
            out._kdiag = torch.from_numpy(np.ascontiguousarray(K.diagonal(), dtype=np.float64)).to(device)
        out.info["adopted_from"] = type(G).__name__
        return out

    # -- pygsp-like surface -------------------------------------------------------------------
    @property
    def lmax(self):
        if self._lmax is None:
            self.estimate_lmax()
        return self._lmax

    @lmax.setter
    def lmax(self, value):
        self._lmax = None if value is None else float(value)
        self.lmax_info = {} if value is None else dict(method="injected")

    def estimate_lmax(self, recompute=False, tol=1e-3, max_iter=300, method=None):
        """Largest Laplacian eigenvalue x 1.01 (pygsp's safety factor, [UPSTREAM pygsp
        ``Graph.estimate_lmax``] at reference ``meld/filter.py:39``).  pygsp stops ARPACK at
        tol=5e-3, which makes its value run-to-run noisy at the 1e-4 level; here a Lanczos
        recurrence on the device SpMV is run to a relative Ritz residual ``tol``: measured on the 1M-cell
        benchmark graph the eigenvalue error is 1.2e-6 relative at the default 1e-3 (35 iterations), 9e-8 at 3e-4
        (40), 4e-9 at 1e-4 (45) -- the error goes with the square of the residual; 1.2e-6 is 1/40 of the spread of
        the reference's own estimate between two runs.  On the panel-tiled layout the SpMV streams an fp32 copy of
        the weights (vectors and sums fp64): that moves the eigenvalue by < 1e-7 relative.  No-op when a value is
        already set (same as pygsp), which is how parity tests inject a common lmax."""
        if self._lmax is not None and not recompute:
            # a value that is already there is kept (pygsp's no-op) -- unless it came from the OTHER estimator: asking for
            # the reference's ARPACK number after a Lanczos estimate (or the reverse) computes it
            have = self.lmax_info.get("method", "injected")
            if method is None or have == "injected" or have == method:
                return self._lmax
        method = method or "lanczos"
        if method == "arpack":
            return self._estimate_lmax_arpack()
        if method != "lanczos":
            raise ValueError("lmax method {!r} not recognized. Choose from ['lanczos', 'arpack']".format(method))
        from .filter import lanczos_lmax

        lam, info = lanczos_lmax(self, tol=tol, max_iter=max_iter)
        self._lmax = 1.01 * lam
        self.lmax_info = dict(info, method="lanczos")
        return self._lmax

    def _estimate_lmax_arpack(self):
        """The reference's own estimate, call for call ([UPSTREAM pygsp 0.5.1 ``Graph.estimate_lmax``] at
        reference ``meld/filter.py:39``): the Laplacian is copied to the host once and
        ``1.01 * scipy.sparse.linalg.eigsh(L, k=1, tol=5e-3, ncv=min(N, 10))`` is evaluated there
        (``2 max(dw)`` if ARPACK does not converge).  Opt-in (``MELD(lmax="arpack")``): slower than the
        device Lanczos and only converged to ARPACK's 5e-3, but it is the number the reference stack
        computes -- with it an un-injected ``fit_transform`` meets the reference within its own
        run-to-run spread (ARPACK's start vector comes from process-global state)."""
        from scipy.sparse.linalg import ArpackNoConvergence, eigsh

        if self.n_rows != self.N:
            raise NotImplementedError("lmax='arpack' needs an unsharded graph")
        L = self.L
        try:
            lam = eigsh(L, k=1, tol=5e-3, ncv=min(self.N, 10), return_eigenvectors=False)
            self._lmax = 1.01 * float(lam[0])
            self.lmax_info = dict(method="arpack", tol=5e-3)
        except ArpackNoConvergence:  # pragma: no cover
            self._lmax = 2.0 * float(np.max(self.dw))
            self.lmax_info = dict(method="arpack", converged=False)
        return self._lmax

    # -- host exports in the caller's cell order (tests / inspection; not used by the hot path) -----
    def _inv_perm_host(self):
        if self.perm is None:
            return None
        p = self.perm.cpu().numpy()
        inv = np.empty_like(p)
        inv[p] = np.arange(p.shape[0])
        return inv

    def _scipy(self, vals):
        from scipy import sparse

        M = sparse.csr_matrix((vals, self.col.cpu().numpy(), self.rowptr.cpu().numpy()[: self.n_rows + 1]), shape=(self.n_rows, self.N))
        inv = self._inv_perm_host()
        if inv is not None:
            if self.n_rows != self.N:
                raise ValueError("host export of a sharded, permuted graph is not supported")
            M = M[inv][:, inv].tocsr()
            M.sort_indices()
        return M

    def _vec_host(self, t):
        v = t.cpu().numpy()
        inv = self._inv_perm_host()
        return v if inv is None or v.shape[0] != inv.shape[0] else v[inv]

    @property
    def W(self):
        return self._scipy(self.val.cpu().numpy())

    @property
    def dw(self):
        return self._vec_host(self.dw_dev)

    @property
    def bandwidth_host(self):
        """bandwidths in the units of the graph's metric (``bandwidth`` itself is the euclidean one of the rows the search saw)"""
        if getattr(self, "bandwidth", None) is None:  # (a precomputed affinity has none)
            return None
        to_metric = getattr(self, "bandwidth_to_metric", None)
        return self._vec_host(self.bandwidth if to_metric is None else to_metric(self.bandwidth))

    @property
    def L(self):
        from scipy import sparse

        if self.n_rows != self.N:
            raise ValueError("L is only defined for an unsharded graph")
        return (sparse.diags(self.dw, 0) - self.W).tocsr()

    @property
    def K(self):
        """Symmetrised, anisotropy-normalised kernel including its diagonal (graphtools' ``G.K``)."""
        from scipy import sparse

        if self.n_rows != self.N:
            raise ValueError("K is only defined for an unsharded graph")
        if getattr(self, "_kdiag", None) is not None:  # dense graph: the diagonal was computed explicitly
            return (self.W + sparse.diags(self._vec_host(self._kdiag), 0)).tocsr()
        return (self.W + sparse.diags(self._vec_host(self.kernel_diagonal()), 0)).tocsr()

    # -- what the reference's side paths read from the graph: graphtools' ``knn`` / ``diff_op``
    # (reference meld/cluster.py:213, comparison/comparison.py:318-323), pygsp's Fourier basis (meld/cluster.py:235-236) --
    @property
    def knn(self):
        """The ``knn`` the graph was built with (graphtools' attribute; None for a weight matrix uploaded from elsewhere)."""
        return self.info.get("knn")

    @property
    def diff_op(self):
        """graphtools' diffusion operator: the kernel (diagonal included) with rows normalised to sum 1, as scipy CSR in
        the caller's cell order (built on first use, on the host: an inspection / side-path export like ``K``)."""
        if getattr(self, "_diff_op", None) is None:
            from scipy import sparse

            K = self.K
            self._diff_op = (sparse.diags(1.0 / np.ravel(K.sum(1)), 0) @ K).tocsr()
        return self._diff_op

    FOURIER_MAX_N = 16384

    def compute_fourier_basis(self, recompute=False, n_eigenvectors=None, tol=1e-6, max_iter=200, seed=0):
        """pygsp's ``compute_fourier_basis``: full eigendecomposition of the combinatorial Laplacian -- ``e`` ascending,
        ``U`` the eigenvectors (columns), both host arrays in the caller's cell order; also sets ``lmax = e[-1]`` like
        pygsp.  Dense O(N^3) on the device (rocSOLVER ``eigh``), offered up to FOURIER_MAX_N cells.

        ``n_eigenvectors=k`` ([UPSTREAM pygsp development line]; 1 <= k <= 48): computes and caches the ``k`` smallest
        eigenpairs only, at any graph size (``meld_amd/spectrum.py``); read them with ``fourier_basis(k)``.  ``U`` / ``e`` /
        ``lmax`` are not touched by it."""
        if n_eigenvectors is not None:
            self.fourier_basis_device(n_eigenvectors, recompute=recompute, tol=tol, max_iter=max_iter, seed=seed)
            return
        if getattr(self, "_U", None) is not None and not recompute:
            return
        self._e, self._U = self._dense_fourier()
        self.lmax = float(self._e[-1])

    def _dense_fourier(self):
        """``(e, U)`` of the full dense decomposition, host arrays in the caller's order; nothing is stored."""
        if self.n_rows != self.N:
            raise ValueError("the Fourier basis is only defined for an unsharded graph")
        if self.N > self.FOURIER_MAX_N:
            raise NotImplementedError("compute_fourier_basis is a dense O(N^3) eigendecomposition; N={} exceeds the {} cells "
                                      "it is offered for".format(self.N, self.FOURIER_MAX_N))
        n, dev = self.N, self.val.device
        row_of = torch.repeat_interleave(torch.arange(n, device=dev), self.rowptr[1:] - self.rowptr[:-1])
        L = torch.zeros(n, n, dtype=torch.float64, device=dev)
        L[row_of, self.col.to(torch.int64)] = -self.val
        L += torch.diag(self.dw_dev[:n])
        e, U = torch.linalg.eigh(L)
        e, U = e.cpu().numpy(), U.cpu().numpy()
        inv = self._inv_perm_host()
        if inv is not None:
            U = U[inv]
        return e, U

    def fourier_basis_device(self, k, recompute=False, tol=1e-6, max_iter=200, seed=0):
        """The ``k`` smallest eigenpairs of the combinatorial Laplacian as device tensors ``(e [k], U [N, k])``: ``e`` ascending,
        one row of ``U`` per cell in the caller's order, each column's entry of largest magnitude positive.  1 <= k <= 48;
        Chebyshev-filtered subspace iteration on the device (``meld_amd/spectrum.py``; up to 128 cells a slice of the dense
        decomposition), to residuals ``|L u - e u| <= tol * ub`` with ``ub`` a rigorous upper bound of the spectrum; RuntimeError
        when ``max_iter`` filter applications do not get there.  Computed on first use and kept per ``(k, tol, seed)``, apart
        from ``U`` / ``e``; ``lmax`` is neither set nor changed."""
        from . import spectrum

        key = (spectrum.check_k(k), float(tol), int(seed))
        if self.n_rows != self.N:
            raise ValueError("the Fourier basis is only defined for an unsharded graph")
        cache = self.__dict__.setdefault("_partial_fourier", {})
        if recompute or key not in cache:
            cache.pop(key, None)
            e, U, info = spectrum.partial_basis_device(self, key[0], tol=tol, max_iter=max_iter, seed=seed)
            cache[key] = dict(e=e, U=U, info=info, host=None)
        self.fourier_partial_info = cache[key]["info"]
        return cache[key]["e"], cache[key]["U"]

    def fourier_basis(self, k, recompute=False, tol=1e-6, max_iter=200, seed=0):
        """``fourier_basis_device`` as host fp64 arrays ``(e [k], U [N, k])``."""
        from . import spectrum

        self.fourier_basis_device(k, recompute=recompute, tol=tol, max_iter=max_iter, seed=seed)
        kept = self._partial_fourier[(spectrum.check_k(k), float(tol), int(seed))]
        if kept["host"] is None:
            kept["host"] = (kept["e"].cpu().numpy(), kept["U"].cpu().numpy())
        return kept["host"]

    @property
    def U(self):
        self.compute_fourier_basis()
        return self._U

    @property
    def e(self):
        self.compute_fourier_basis()
        return self._e

    @property
    def landmark_op(self):
        """graphtools' LandmarkGraph operator (reference ``meld/meld.py:105`` forwards ``n_landmark``): lazily built
        there, never used by MELD's filter; not implemented here."""
        raise NotImplementedError("the landmark operator (graphtools LandmarkGraph.landmark_op) is not implemented; "
                                  "MELD's density estimate does not use it")

    def landmarks(self, n_landmark=None, clusters=None, n_svd=100, random_state=None, recompute=False, kmeans="library"):
        """graphtools' ``LandmarkGraph`` for this graph as a ``landmark.Landmarks`` record (``meld_amd/landmark.py``,
        ``csrc/landmark.hip``): ``clusters`` / ``clusters_device``, ``transitions`` (``[N, L]``) / ``transitions_device``,
        ``landmark_op`` (``[L, L]``) / ``landmark_op_device``, ``landmark_sums``, ``extend_to_data(Y)`` and ``interpolate(T, Y=None)``
        with their ``_device`` forms.  The record is built on the device and kept per argument set (``recompute`` builds it anew).

        ``clusters``: one integer per cell in the caller's order (host or device), compacted to the labels present (landmark ``l``
        is the ``l``-th smallest label); otherwise the cells are clustered into at most ``n_landmark`` landmarks (default: the
        ``n_landmark`` the graph was fitted with) by k-means on ``diff_op @ V``, ``V`` the leading ``min(n_svd, n_landmark)`` singular
        vectors of the symmetric diffusion affinity from a seeded randomized range finder -- the same ``random_state`` gives the same labels.
        ``kmeans``: ``"library"`` (the default: k-means++ seeding, the LDS or library Lloyd step) or ``"device"`` (k-means|| seeding and
        the Lloyd step of ``csrc/kmeans_wide.hip``), both in ``meld_amd/kmeans.py``; part of the argument set, ValueError for any other value.
        ValueError without ``n_landmark`` and ``clusters``, for ``n_landmark >= N`` or above ``landmark.LANDMARK_MAX``, for bad
        ``clusters`` (TypeError for a dtype that is not integer) and on a row-sharded graph.  The ``landmark_op`` property of the
        graph itself stays unimplemented: the operator lives on the record."""
        from . import landmark

        return landmark.landmarks(self, n_landmark=n_landmark, clusters=clusters, n_svd=n_svd, random_state=random_state,
                                  recompute=recompute, kmeans=kmeans)

    def phate(self, n_components=2, t="auto", gamma=1, n_landmark=None, clusters=None, n_svd=100, mds="metric", max_iter=3000,
              eps=1e-6, t_max=100, random_state=None, recompute=False, kmeans="library"):
        """The PHATE embedding of this graph as a ``phate.PhateEmbedding`` record (``meld_amd/phate.py``, ``csrc/mds.hip``; [UPSTREAM
        phate ``PHATE.fit_transform``, unpinned: every stage is defined in ``meld_amd/phate.py``]): ``embedding`` (``[N,
        n_components]``, the caller's cell order) / ``embedding_device``, ``landmark_embedding``, ``t``, ``entropy``,
        ``potential_device``, ``distances_device``, ``stress``, ``normalized_stress``, ``iterations``, ``landmarks``, ``info``, and
        ``transform(Y)`` / ``transform_device(Y)`` for new cells.  Built on the device and kept per argument set (``recompute``
        builds it anew).

        The operator is ``landmarks(n_landmark, clusters=, n_svd=, random_state=).landmark_op_device`` (``n_landmark``: the graph's
        own, else 2000); a graph of at most ``n_landmark`` cells without ``clusters`` embeds its dense ``diff_op`` directly.  ``t``: a
        positive integer or ``"auto"`` (the knee of the von Neumann entropy of the operator's powers 1 .. ``t_max``); ``gamma`` in
        ``[-1, 1]`` selects the potential (1: ``-log``); ``mds``: ``"metric"`` (classical MDS, then SMACOF for at most ``max_iter``
        steps, to a relative stress decrease of ``eps``) or ``"classic"``.  ValueError, with the value, for ``n_components`` outside
        ``1 .. 8`` or not below the operator's rows, a ``t`` that is no positive integer, ``gamma`` outside ``[-1, 1]``, ``t_max <
        3``, an unknown ``mds``, and on a row-sharded graph; the refusals of ``landmarks()`` and of the extension to new cells
        pass through."""
        from . import phate

        return phate.phate(self, n_components=n_components, t=t, gamma=gamma, n_landmark=n_landmark, clusters=clusters, n_svd=n_svd,
                           mds=mds, max_iter=max_iter, eps=eps, t_max=t_max, random_state=random_state, recompute=recompute, kmeans=kmeans)

    def kernel_diagonal(self):
        """Diagonal of the kernel matrix K in the device order: K_ii = 1 / (ksum_i^2)^anisotropy for a
        graph built here (the alpha-decay kernel has 1 on its diagonal before the anisotropy
        normalisation); 1 for an uploaded weight matrix that came without its kernel
        (``from_scipy``: the kernel's own diagonal before any normalisation)."""
        if getattr(self, "_kdiag", None) is not None:
            return self._kdiag
        if self.ksum is None:
            return torch.ones(self.N, dtype=torch.float64, device=self.val.device)
        return 1.0 / (self.ksum * self.ksum) ** self.anisotropy

    # -- out-of-sample extension (meld_amd/extend.py, csrc/extend.hip): graphtools' names and semantics for cells that were not
    # in ``fit``.  Graphs without cells or without a comparable kernel raise NotImplementedError, naming the case. -------------
    @property
    def n_features_in(self):
        """Columns of the data ``fit`` received (None where the graph was not built from cells by ``MELD.fit``)."""
        st = getattr(self, "_extend_state", None)
        return None if st is None else st.n_features_in

    def kernel_to_data_device(self, Y, knn=None, bandwidth=None, bandwidth_scale=None, n_slices=0):
        """The kernel from the new cells ``Y`` to the fitted cells as device tensors ``(rowptr, col, val, rowsum)``: CSR
        ``[M, N]``, columns in the caller's cell order and sorted, with its row sums; nothing goes through the host.
        ``n_slices``: see ``extend.kernel_to_data_device`` (L1 / L-inf graphs; the result does not depend on it)."""
        from . import extend

        return extend.kernel_to_data_device(self, Y, knn=knn, bandwidth=bandwidth, bandwidth_scale=bandwidth_scale, n_slices=n_slices)

    def build_kernel_to_data(self, Y, knn=None, bandwidth=None, bandwidth_scale=None):
        """[UPSTREAM graphtools 1.5.x ``kNNGraph.build_kernel_to_data``]: scipy CSR ``[M, N]`` (a host export, like ``K``):
        ``exp(-(dist / bw)^decay)`` for every fitted cell with a value >= thresh, ``bw`` the distance to the knn-th nearest
        FITTED cell (or the graph's fixed numeric bandwidth) times ``bandwidth_scale``, floored at eps; ``decay=None``: the
        connectivity of the knn nearest fitted cells.  ``Y``: ``n_features_in`` columns (projected with the stored PCA / SVD
        model and the metric's front end) or the reduced number of columns."""
        from . import extend

        return extend.to_scipy(self.kernel_to_data_device(Y, knn=knn, bandwidth=bandwidth, bandwidth_scale=bandwidth_scale), self.N)

    def extend_to_data(self, Y):
        """[UPSTREAM graphtools ``BaseGraph.extend_to_data``]: the transitions ``[M, N]`` from new cells to fitted cells, the
        kernel of ``build_kernel_to_data`` l1-normalised by row (scipy CSR)."""
        from . import extend

        return extend.to_scipy(self.kernel_to_data_device(Y), self.N, normalise=True)

    def interpolate(self, transform, transitions=None, Y=None):
        """[UPSTREAM graphtools ``BaseGraph.interpolate``]: ``transitions @ transform`` for a ``transform`` with one row per
        fitted cell (caller's order).  With ``Y`` the product runs on the device and the transitions are never written;
        a scipy ``transitions`` is multiplied on the host."""
        from . import extend

        return extend.interpolate(self, transform, transitions=transitions, Y=Y)

    def interpolate_device(self, F, Y, device_order=False):
        """``interpolate(F, Y=Y)`` for a device tensor ``F [N, p]``, returning a device tensor ``[M, p]``.  ``device_order``:
        the rows of ``F`` are in the graph's device order (``perm``), the kernel's columns are translated on the fly."""
        from . import extend

        colmap = None
        if device_order and self.perm is not None:
            colmap = torch.empty_like(self.perm)
            colmap[self.perm] = torch.arange(self.perm.shape[0], device=self.perm.device, dtype=self.perm.dtype)
        extend.state_of(self)
        if F.dim() != 2 or int(F.shape[0]) != self.N:
            raise ValueError("transform must have one row per fitted cell ({}), got shape {}".format(self.N, tuple(F.shape)))
        return extend.apply_transitions(self.kernel_to_data_device(Y), F.to(torch.float64), colmap=colmap)

    # -- diffusion of cell signals (meld_amd/diffuse.py, csrc/diffuse.hip): ``diff_op`` applied on the device, never formed --------
    def diffuse_device(self, F, t=1, device_order=False):
        """``diff_op^t F`` as an fp64 device tensor ``[N, p]`` (``[N]`` for 1-D input): ``t`` steps of the random walk of the
        kernel matrix, ``y = (W x + kd .* x) / (dw + kd)``, on a device tensor, a host array or a DataFrame with one row per cell.
        Rows in the caller's order unless ``device_order`` (as in ``interpolate_device``: then neither the input nor the output is
        permuted).  ``t = 0`` returns a copy.  Signals wider than 128 columns go through the kernel panel by panel; a column's
        values do not depend on the other columns.  ValueError on a row-sharded graph and where a cell's kernel row sum is not
        positive (an adopted graph with an isolated vertex and a zero kernel diagonal); ``t="auto"`` is not implemented."""
        from . import diffuse

        return diffuse.diffuse_device(self, F, t=t, device_order=device_order)

    def diffuse(self, F, t=1):
        """``diffuse_device`` as a host ndarray; a DataFrame comes back as a DataFrame with its index and columns."""
        from . import diffuse

        return diffuse.diffuse(self, F, t=t)

    # -- geodesic distances (meld_amd/geodesic.py, csrc/geodesic.hip): [UPSTREAM graphtools ``BaseGraph.shortest_path``], many
    # sources per stream of the matrix; scipy's dijkstra bit for bit --------------------------------------------------------------
    def edge_lengths(self, distance=None):
        """The lengths the shortest paths add up, as scipy CSR in the caller's cell order with the pattern of ``W`` (a host
        export, like ``K``): ``"affinity"`` = ``-log W``, ``"data"`` = the euclidean distances of the cells the graph was
        searched on (exactly symmetric), ``"constant"`` = 1; None: ``"constant"`` for a ``decay=None`` graph, else ``"affinity"``."""
        from . import geodesic

        return self._scipy(geodesic.edge_lengths_device(self, distance).cpu().numpy())

    def shortest_path_device(self, sources, distance=None, min_only=False, device_order=False, max_rounds=None):
        """Distances along the graph from each of ``sources`` (integers or a boolean mask; duplicates allowed) as an fp64 device
        tensor ``[N, p]``, ``+inf`` where there is no path; ``min_only``: ``[N]``, the distance to the nearest source.  Synchronous
        Bellman-Ford rounds for up to 128 sources per stream of the matrix, until a round lowers nothing: the values are
        ``scipy.sparse.csgraph.dijkstra(self.edge_lengths(distance), indices=sources)`` bit for bit where all lengths are positive,
        and a column's values do not depend on the other sources.  Rows and sources in the caller's order unless
        ``device_order``.  ``geodesic_info`` is ``dict(rounds=[per panel], distance, p)``.  ValueError on a row-sharded graph, for
        sources out of range and for lengths that are not finite and >= 0 (an adopted graph with weights above 1 under
        ``"affinity"``); NotImplementedError where ``"data"`` has no cells to measure; RuntimeError after ``max_rounds`` rounds
        (default ``N``)."""
        from . import geodesic

        return geodesic.shortest_path_device(self, sources, distance=distance, min_only=min_only, device_order=device_order,
                                             max_rounds=max_rounds)

    def shortest_path(self, sources=None, distance=None, min_only=False, method="auto"):
        """``shortest_path_device`` as a host ndarray ``[N, p]``.  ``sources=None``: all cells, offered up to ``FOURIER_MAX_N``
        cells (the result is dense ``[N, N]``); beyond that ValueError asks for ``sources``.  ``method`` is accepted for
        graphtools' signature and ignored."""
        from . import geodesic

        return geodesic.shortest_path(self, sources=sources, distance=distance, min_only=min_only, method=method)

    # -- connectivity (meld_amd/components.py, csrc/components.hip): pygsp's ``is_connected`` / ``extract_components`` / ``subgraph``,
    # scipy's labels.  Single-GPU graphs; nothing goes through the host but the counts. ---------------------------------------------
    def connected_components_device(self, recompute=False, max_rounds=None):
        """``(n_components, labels)``: ``labels`` an int32 device tensor ``[N]`` in the caller's cell order, equal to
        ``scipy.sparse.csgraph.connected_components(G.W, directed=False)`` (components numbered by their smallest cell).
        Hook-and-compress rounds on the device until one writes nothing; RuntimeError, naming the rounds done, after ``max_rounds``
        (default ``4 ceil(log2 N) + 64``).  Kept on the graph; ``components_info`` is ``dict(rounds, n_components, largest)``."""
        from . import components

        return components.connected_components_device(self, recompute=recompute, max_rounds=max_rounds)

    def connected_components(self):
        """``connected_components_device`` with the labels as a host int32 array: scipy's return value."""
        n, labels = self.connected_components_device()
        return n, labels.cpu().numpy()

    @property
    def component_sizes(self):
        """Cells per component (host int64 ``[n_components]``, in label order)."""
        self.connected_components_device()
        return self._components["sizes"]

    def is_connected(self, recompute=False):
        """[UPSTREAM pygsp ``Graph.is_connected``]: one component."""
        return self.connected_components_device(recompute=recompute)[0] == 1

    def subgraph(self, ind):
        """[UPSTREAM pygsp ``Graph.subgraph``]: the graph induced by the cells ``ind`` -- an integer array or a boolean mask, on
        the host or the device.  Cell ``i`` of the result is ``ind[i]``; its device order is this graph's restricted to the kept
        cells, so it carries a ``perm`` of its own unless that is the identity.  Weights are copied bit for bit, degrees summed
        anew.  ValueError for duplicates, indices out of range and an empty selection, TypeError for other dtypes.  Carried over:
        ``info["orig_idx"]`` (host int64), the kept cells' kernel diagonal (``K`` / ``diff_op`` are this graph's kernel restricted
        to them), ``bandwidth``, ``info["knn"]``.  Not carried: ``lmax``, the Fourier caches, the tiled layout, the state of the
        out-of-sample extension."""
        from . import components

        return components.subgraph(self, ind)

    def extract_components(self):
        """[UPSTREAM pygsp ``Graph.extract_components``]: one subgraph per component, in label order, ``info["component"]`` set.
        A plain loop over ``subgraph``: one pass over this graph's CSR per component."""
        n, labels = self.connected_components_device()
        out = []
        for c in range(n):
            sub = self.subgraph(torch.nonzero(labels == c)[:, 0])
            sub.info["component"] = c
            out.append(sub)
        return out

    def largest_component(self):
        """The subgraph of the component with the most cells (the lowest label among equals), ``info["component"]`` set."""
        c = int(np.argmax(self.component_sizes))
        sub = self.subgraph(torch.nonzero(self._components["labels"] == c)[:, 0])
        sub.info["component"] = c
        return sub

    # -- communities (meld_amd/louvain.py, csrc/louvain.hip): the "Louvain clusters" the reference's comparison takes from scanpy
    # (comparison/comparison.py, find_n_clusters), by a deterministic synchronous rule.  Single-GPU graphs. ------------------------
    def louvain_device(self, resolution=1.0, n_clusters=None, tol=1e-7, max_rounds=None, max_levels=None, recompute=False):
        """``louvain`` (the same record; its ``labels_device`` and per-level labels never leave the GPU unless asked for)."""
        from . import louvain

        return louvain.louvain_device(self, resolution=resolution, n_clusters=n_clusters, tol=tol, max_rounds=max_rounds,
                                      max_levels=max_levels, recompute=recompute)

    def louvain(self, resolution=1.0, n_clusters=None, tol=1e-7, max_rounds=None, max_levels=None, recompute=False):
        """Louvain communities of the cells: a ``LouvainRecord`` with ``labels`` (int32 ``[N]``, caller's order, communities
        numbered by their smallest cell), ``labels_device``, ``n_communities``, ``sizes``, ``modularity``, ``resolution``,
        ``levels`` (per level ``dict(vertices, communities, rounds, Q)``) and ``level_labels(l)``, the dendrogram.  Synchronous,
        deterministic local moves (no random order, no floating-point atomics: the same bits every run, whatever ``perm``), then
        contraction, until a level merges nothing; a level ends when the modularity did not rise by more than ``tol``, when
        nothing moved, or after ``max_rounds`` (default 1000) rounds.  ``n_clusters=k`` bisects the resolution between 0.01 and 10
        like the reference's ``find_n_clusters`` and returns the first partition with exactly ``k`` communities (ValueError
        "r_start is too large" / "r_stop is too small" where the ends fail, and one naming the nearest counts when the interval
        closes below 0.001).  A graph without entries gives ``N`` singletons with modularity 0.0; isolated cells stay alone.
        ValueError on a row shard and for a resolution that is not finite and positive.  Kept on the graph per set of arguments."""
        return self.louvain_device(resolution=resolution, n_clusters=n_clusters, tol=tol, max_rounds=max_rounds, max_levels=max_levels,
                                   recompute=recompute)

    # -- Leiden communities (meld_amd/leiden.py, csrc/leiden.hip): the Louvain run with a refinement of every level's partition, so
    # that every community is connected (find_n_clusters(adata, k, "leiden") of the reference's comparison). -----------------------
    def leiden(self, resolution=1.0, n_clusters=None, tol=1e-7, max_rounds=None, max_levels=None, recompute=False):
        """Leiden communities of the cells: a ``LeidenRecord`` with the attributes of ``louvain``'s record (``labels``,
        ``labels_device``, ``n_communities``, ``sizes``, ``modularity``, ``resolution``, ``level_labels(l)``) and ``levels`` holding
        per level ``dict(vertices, communities, subcommunities, rounds, refine_rounds, Q)``.  The run is ``louvain``'s with a
        refinement between a level's moves and its contraction: inside every community the vertices merge again from singletons,
        a vertex joining only a sub-community it has an entry to and nobody leaving one of two or more, and the graph is
        contracted by those sub-communities.  Every community of a run that ends on its own induces a connected subgraph (a run
        cut by ``max_levels`` returns the last move partition, without that guarantee).  Synchronous and deterministic: the same
        bits every run, whatever ``perm``; upstream's randomised choice is not offered.  ``max_rounds`` bounds the rounds of a
        move phase and of a refinement alike.  ``n_clusters``, the graph without entries, row shards and the argument checks: as
        for ``louvain``.  Kept on the graph per set of arguments."""
        from . import leiden

        return leiden.leiden_device(self, resolution=resolution, n_clusters=n_clusters, tol=tol, max_rounds=max_rounds,
                                    max_levels=max_levels, recompute=recompute)

    def modularity(self, labels, resolution=1.0):
        """``Q(labels; resolution) = (sum_c in_c - resolution sum_c tot_c^2 / 2m) / 2m`` of any labelling of the cells (host or
        device integers, caller's order; the values need not be consecutive): ``networkx.community.modularity`` with
        ``weight="weight"`` on a graph without self-loops.  ValueError for a wrong length or negative labels."""
        from . import louvain

        return louvain.modularity(self, labels, resolution=resolution)


_BLAS_CTL = None


def _eigh_one_thread(a):
    """``np.linalg.eigh(a, UPLO="U")`` (row-major upper triangle) on one BLAS thread (threadpoolctl; plain numpy where it is absent)."""
    global _BLAS_CTL
    if a.shape[0] <= 64:  # (below OpenBLAS's threading threshold: 0.1 ms at 50 x 50 as it is)
        return np.linalg.eigh(a, UPLO="U")
    try:
        if _BLAS_CTL is None:
            from threadpoolctl import ThreadpoolController

            _BLAS_CTL = ThreadpoolController()
        with _BLAS_CTL.limit(limits=1, user_api="blas"):
            return np.linalg.eigh(a, UPLO="U")
    except ImportError:
        return np.linalg.eigh(a, UPLO="U")


def _radius_factor(decay, thresh):
    """Kernel radius in bandwidths: the distance at which the alpha-decay kernel falls to ``thresh``."""
    return 1.0 if math.isinf(decay) else float((-math.log(thresh)) ** (1.0 / decay))


class HipOps:
    """Local (per-GPU) stages of the path as calls into libmeld_hip.so.  The single-GPU builder
    and the row-sharded driver (``meld_amd.distributed``) compose the same stages; only the
    exchanges between them differ."""

    name = "hip"

    def __init__(self, device=None, search=None, prune=None, nprod=None, spmm=None):
        self.lib = get_lib()
        # recurrence kernel: "auto" (panel-tiled layout for graphs of at least PT_MIN_ROWS local rows),
        # "tiled" (always), "csr" (the CSR-stream kernel of spmm.hip)
        self.spmm = spmm
        # options of the kNN search (meld_amd.knn_plan.SearchOptions): attributes, so that a test can switch one off
        o = SearchOptions.from_env(search=search, prune=prune, nprod=nprod)
        self.search, self.nprod, self.prune, self.rotate, self.rotate_min_cells = o.search, o.nprod, o.prune, o.rotate, o.rotate_min_cells
        self.radius_cut, self.seed, self.seeded_bounds, self.block_order = o.radius_cut, o.seed, o.seeded_bounds, o.block_order
        if not torch.cuda.is_available():
            raise RuntimeError("meld_amd needs a ROCm GPU (MI355X); there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)

    def col_stats(self, X):
        """(sums, minima, maxima) of the columns of an fp64 [N, d <= 256] matrix in one pass (``meld_col_stats_f64``)."""
        N, d = int(X.shape[0]), int(X.shape[1])
        out = torch.empty(3, d, dtype=torch.float64, device=X.device)
        tb = self.lib.meld_col_stats_temp_bytes(d)
        tmp = torch.empty(tb, dtype=torch.uint8, device=X.device)
        check(self.lib.meld_col_stats_f64(ptr(X), N, d, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(tmp), tb, stream()), "meld_col_stats_f64")
        return out[0], out[1], out[2]

    def frame_axes_async(self, X, col_stats):
        """Start the frame of the search on ``X`` BEFORE the cells are brought into locality order: the covariance of evenly spaced
        rows does not depend on the order of the cells, so its scatter matrix and the read-back go out first, and the d x d
        eigenproblem is solved on the host while the GPU works through the ordering (the GPU used to idle ~0.35 ms at 1M cells
        while the host waited for the read-back, decomposed the matrix and sent the axes back).  Returns a function that finishes
        the job -- ``finish(lead)`` -> the axes as rows ``At`` (device, [d, meld_frame_max_dims()]) or None (frame declined) -- or
        None where the frame will not be asked for (options, size, width) or the column sums are not at hand."""
        lib = self.lib
        N, d = int(X.shape[0]), int(X.shape[1])
        if col_stats is None or d > int(lib.meld_frame_max_dims()) or not plan_knn_search(lib, N, d, 0, N, 1, 2, options=self).frame:
            return None
        st = stream()
        mean = col_stats[0] / N
        cov = torch.zeros(d, d, dtype=torch.float64, device=X.device)
        check(lib.meld_cov_sample_f64(ptr(X), N, d, ptr(mean), max(1, N // 32768), ptr(cov), st), "meld_cov_sample_f64")
        host = torch.empty(d, d, dtype=torch.float64, pin_memory=True)
        host.copy_(cov, non_blocking=True)
        done = torch.cuda.Event()
        done.record()

        def finish(lead):
            done.synchronize()
            evals, evecs = _eigh_one_thread(host.numpy())
            tot = float(evals.sum())
            if not np.isfinite(tot) or tot <= 0.0 or float(evals[-lead:].sum()) < 0.5 * tot:
                return False
            At = np.zeros((d, int(lib.meld_frame_max_dims())))
            At[:, :d] = evecs[:, ::-1].T
            return torch.from_numpy(At).to(X.device, non_blocking=True)

        return finish

    def principal_frame(self, X, mean, lead, comm=None, axes=None):
        """The cells in their principal frame, ``(X - mean) V`` with the eigenvectors of the covariance (of at most 32768 evenly
        spaced rows, ``meld_cov_sample_f64``) in descending order of variance (``meld_rotate_rows_f64``) -- or None when the
        ``lead`` leading coordinates would carry less than half of the variance (the search's partial test would seldom drop a
        block; any frame is valid, the graph is the same).  Distances are those of ``X`` to
        rounding (V is orthonormal to 1e-15): the search only nominates candidates, their distances are evaluated in fp64 on
        ``X`` itself.  The d x d eigenproblem is solved on the host (one read-back of d x d numbers)."""
        lib, st = self.lib, stream()
        N, d = int(X.shape[0]), int(X.shape[1])
        if axes is not None and (comm is None or getattr(comm, "world", 1) == 1):
            # (the axes were started before the ordering: frame_axes_async)
            At = axes(lead)
            if At is False:
                return None
            out = torch.empty_like(X)
            check(lib.meld_rotate_rows_f64(ptr(X), N, d, ptr(mean), ptr(At), ptr(out), st), "meld_rotate_rows_f64")
            return out
        wide = d > int(lib.meld_frame_max_dims())  # (beyond the frame kernels' row width: the same two products through the library)
        stride = max(1, N // 32768)
        if wide:
            Xs = X[::stride] - mean
            cov = torch.triu(Xs.T @ Xs)
            del Xs
        else:
            cov = torch.zeros(d, d, dtype=torch.float64, device=X.device)
            check(lib.meld_cov_sample_f64(ptr(X), N, d, ptr(mean), stride, ptr(cov), st), "meld_cov_sample_f64")
        if comm is not None and getattr(comm, "world", 1) > 1:
            # ranks of a row-sharded build hold the same cells but sum their scatter matrices in different orders (atomics): all
            # take rank 0's bits, so that the frame -- and the decision to use one -- is the same everywhere (the tile spheres
            # are shared between the ranks)
            if comm.rank != 0:
                cov.zero_()
            comm.all_reduce_sum(cov)
        # (ONE BLAS thread for the d x d eigenproblem: past ~64 x 64 OpenBLAS goes multi-threaded, and on a many-core host its
        # threads' start-up cost 60-370 ms for a 100 x 100 matrix that one thread decomposes in 1.1 ms -- found as a 62 ms idle gap
        # of the GPU in the d = 100 step)
        evals, evecs = _eigh_one_thread(cov.cpu().numpy())
        tot = float(evals.sum())
        if not np.isfinite(tot) or tot <= 0.0 or float(evals[-lead:].sum()) < 0.5 * tot:
            return None
        if wide:
            # d in (64, 141]: a plain N x d x d fp64 GEMM (rocBLAS) -- PCA scores, the reference's default input (n_pca = 100), are
            # already in their principal frame up to this rotation's rounding, so it is close to a permutation there
            V = torch.from_numpy(np.ascontiguousarray(evecs[:, ::-1])).to(X.device)
            return torch.addmm(-(mean @ V), X, V)
        At = np.zeros((d, int(lib.meld_frame_max_dims())))
        At[:, :d] = evecs[:, ::-1].T  # the axes as rows, by descending variance
        At = torch.from_numpy(At).to(X.device)
        out = torch.empty_like(X)
        check(lib.meld_rotate_rows_f64(ptr(X), N, d, ptr(mean), ptr(At), ptr(out), st), "meld_rotate_rows_f64")
        return out

    # ---- A2 + A3: directed alpha-decay kernel rows of [q_begin, q_begin + q_count) as COO -------
    def directed_kernel_coo(self, X, q_begin, q_count, knn, decay, thresh, ksel, tm=None, force_fallback=False, n_refs=None, assemble=False, comm=None,
                            bw_scale=1.0, bw_fixed=None, col_stats=None, knn_max=None, symm=(0, 0.0), count_rows_ge=None, frame_axes=None,
                            anisotropy=None):
        """Returns (keys[2M] int64, vals[2M] fp64, info): slot e < M holds (i, j, K_ij / 2) with
        key = i << 32 | j for the local row i; slot M + e holds the transposed (j, i, K_ij / 2).

        ``n_refs``: search BETWEEN two point sets (the cross blocks of the MNN kernel, ``meld_amd.mnn``): the references
        are the rows [0, n_refs) of X only, the queries lie behind them, there is no self among a row's candidates --
        the caller passes knn - 1 so that the bandwidth is the knn-th nearest reference.  No pruning table, no seeds
        (both rest on tile = query block).

        ``bw_scale`` / ``bw_fixed`` ([UPSTREAM graphtools kNNGraph ``bandwidth_scale`` / ``bandwidth``, forwarded by reference
        ``meld/meld.py:106,117-118``): the kernel uses ``max(bw * bw_scale, eps)``; ``bw_fixed`` (fp64 device tensor [N], in
        the order of ``X``) replaces the adaptive k-th-neighbour bandwidth -- the kernel radius of every row is then known
        before the search, which starts its thresholds there and cuts nothing on its own.  ``knn_max`` ([UPSTREAM kNNGraph
        ``knn_max``]): a row keeps its knn_max nearest cells (besides itself) at most.  ``count_rows_ge``: report the number of rows
        whose kernel radius holds at least that many cells, self counted (``info["rows_with_at_least"]``: what graphtools'
        re-search loop branches on, see ``build_knn_graph``).

        ``anisotropy`` (with ``assemble``): the rows leave their buckets with the anisotropy applied and their degrees summed
        (``info["assembled"]`` then ends with the kernel row sums and the degrees).

        The route (search back end, frame, seeds, pruning, lists, slices, filter pass) is ``meld_amd.knn_plan.plan_knn_search``'s;
        the stages run in this order: search operands, start thresholds, step lists, candidate search, refinement (+ the
        full-precision re-search), exact sweep, emit."""
        N = int(X.shape[0])
        NR = int(n_refs) if n_refs is not None else N  # references of the search
        if n_refs is not None and not (0 < NR <= q_begin and q_begin + q_count <= N):
            raise ValueError("cross search: the queries must lie behind the n_refs references")
        a = SimpleNamespace(X=X, N=N, d=int(X.shape[1]), NR=NR, cross=n_refs is not None, q_begin=q_begin, q_count=q_count, knn=knn, decay=decay,
                            thresh=thresh, bw_scale=bw_scale, bw_fixed=bw_fixed, knn_max=knn_max, force_fallback=force_fallback,
                            col_stats=col_stats, frame_axes=frame_axes, tm=tm or _Timer(False), assemble=bool(assemble), rows_fused=True)
        out = self._directed_kernel(a, ksel, comm, assemble, symm, count_rows_ge, anisotropy)
        if out is None:
            # The fused row pass (plan.fused_rows) sent the rows to buckets that cannot be finished -- a hub cell with more entries
            # than a bucket holds, or a column three times in a row -- and kept no kernel values for the sort-based assembly: the
            # graph is built again with the three row kernels.  Rare; the same graph as if the fused pass had never been planned.
            a.rows_fused = False
            out = self._directed_kernel(a, ksel, comm, assemble, symm, count_rows_ge, anisotropy)
            out[3]["fused_rows_recovered"] = True
        return out

    def _directed_kernel(self, a, ksel, comm, assemble, symm, count_rows_ge, anisotropy):
        """The stages of ``directed_kernel_coo``; None where the fused row pass ended in buckets that cannot be finished."""
        q_count, force_fallback = a.q_count, a.force_fallback
        r = self._search_and_refine(a, ksel, comm)
        retry_from = None
        if r.n_flag > max(1024, q_count // 100) and ksel < 128 and r.plan.search == "f16x3" and not force_fallback:
            # Many uncertified rows with a short candidate list (dense low-dimensional data: more than ksel cells inside the radius
            # inflated by the search-error allowance): search once more with the longest list instead of sweeping them one by one
            # (1M cells in the plane, knn = 15: 292k rows through the sweep at ksel = 64, 0.63 s; none at ksel = 128, 32 ms).  Same
            # graph either way.  (comm is NOT forwarded on purpose: only the ranks that need the retry take it, so it must not issue
            # collectives -- the shared-spheres all-gather of the first try is skipped, every rank computes all spheres itself.)
            retry_from, ksel = (ksel, r.n_flag), 128
            r = self._search_and_refine(a, ksel, None)
        s = self._exact_sweep(a, r, count_rows_ge)
        keys, vals, assembled = self._emit(a, r, s, ksel, assemble, symm, anisotropy)
        if r.buckets is not None and assembled is None and r.m_main + s.fb_total > 0:
            return None
        p, c = r.plan, r.cands
        info = dict(ksel=int(ksel), KP=int(c.KP), search=p.search, nprod=p.nprod, n_flagged_rows=r.n_flag,
                    fused_rows=p.fused_rows if p.fused_rows != "sort+emit" or getattr(c, "raw", None) is not None else "emit",
                    # the route the search took (meld_amd.knn_plan.KnnPlan)
                    prune=p.prune, radius_cut=p.radius_cut, seed=p.seed != "none", seeded_bounds=p.seeded_bounds, block_order=p.block_order != "none",
                    step_lists=p.lists != "none", principal_frame=p.frame, two_phase=p.two_pass, n_rows_bandwidth_recomputed=s.n_rebandwidth,
                    n_researched_rows=r.n_flag_stage1 if p.stage2 else 0, nnz_directed=r.m_main + s.fb_total,
                    # (wave, tile) pairs the first search pass computed (all of them without pruning)
                    wave_tiles_done=r.tiles_done_h, blocks_past_partial_test=r.blocks_on_h, pairs_past_filter=r.pairs_kept_h)
        if s.rows_at_least is not None:
            info["rows_with_at_least"] = s.rows_at_least
        if assembled is not None:
            info["assembled"] = assembled  # (rowptr, col, val) of the symmetrised rows: the caller skips assemble_rows
        if retry_from is not None:
            info["ksel_retry_from"], info["n_flagged_rows_first_try"] = int(retry_from[0]), int(retry_from[1])
        return keys, vals, r.bw, info

    def _search_and_refine(self, a, ksel, comm):
        """One pass of candidate search + exact refinement at candidate-list length ``ksel``: the plan, the candidates and the refined
        rows, with the one read-back of the scalars the host needs next."""
        lib, dev = self.lib, a.X.device
        nprod = search_nprod(self.nprod, a.d)
        resident = lib.meld_knn16_resident_blocks(a.d, nprod) if lib.meld_knn16_kblocks(a.d) > 0 and nprod in (1, 3) else 0
        plan = plan_knn_search(lib, a.N, a.d, a.q_begin, a.q_count, a.knn, ksel, options=self, cross=a.cross, bandwidth=a.bw_fixed is not None,
                               world=getattr(comm, "world", 1) if comm is not None else 1, resident=resident,
                               assemble=a.assemble and a.rows_fused, free_bytes=torch.cuda.mem_get_info(dev)[0] if a.assemble and a.rows_fused else 0,
                               x_aligned=a.X.data_ptr() % 16 == 0)
        a.tm.start()
        col_min = col_max = None
        if a.col_stats is not None:  # (the front end's pass over X -- its NaN / infinity check -- already has them)
            sums, col_min, col_max = a.col_stats
            mean = sums / a.N
        elif a.d <= 256:
            # one pass: the mean and the columns' extremes (from which the operand scale follows without another pass over X)
            sums, col_min, col_max = self.col_stats(a.X)
            mean = sums / a.N
        else:  # beyond the column-sum kernel's width (only the library search path handles such data)
            mean = a.X.mean(dim=0)
        norm2 = torch.empty(a.N, dtype=torch.float32, device=dev)
        nmax = torch.zeros(1, dtype=torch.float32, device=dev)
        if plan.search == "wide":
            c = self._candidates_wide(a, plan, ksel, mean, norm2, nmax)
        elif plan.search == "f32":
            c = self._candidates_f32(a, plan, ksel, mean, norm2, nmax)
        else:
            c = self._candidates_f16x3(a, plan, ksel, comm, mean, col_min, col_max, norm2, nmax)
        a.tm.stop("knn_topk")
        return self._refine(a, c, ksel)

    def _candidates_wide(self, a, plan, ksel, mean, norm2, nmax):
        """Library path for wide data that was not reduced by PCA: chunked fp64 GEMMs (rocBLAS) for |q|^2 + |r|^2 - 2 q.r and
        torch.topk merges, feeding the same exact refinement.  No hand-written kernel: the reference's default (n_pca = 100) never
        gets here, and the distance GEMM at d >> 100 is a plain library GEMM."""
        dev, N, q_begin, q_count = a.X.device, a.N, a.q_begin, a.q_count
        cap = int(ksel)
        Xc = a.X - mean
        n2 = (Xc * Xc).sum(dim=1)
        norm2.copy_(n2.to(torch.float32))
        nmax.copy_(n2.max().to(torch.float32).reshape(1))
        a.tm.stop("prepare")
        kk = min(int(ksel), N)
        cand_idx = torch.zeros(q_count * cap, dtype=torch.int32, device=dev)
        cand_d2 = torch.full((q_count * cap,), float("inf"), dtype=torch.float32, device=dev)
        cand_cnt = torch.full((q_count,), kk, dtype=torch.int32, device=dev)
        QC, RC = 4096, 32768
        with _EventSpan("knn_topk", N=N, d=a.d, q=q_count):
            for q0 in range(0, q_count, QC):
                q1 = min(q_count, q0 + QC)
                Xq = Xc[q_begin + q0 : q_begin + q1]
                nq = n2[q_begin + q0 : q_begin + q1]
                best_d = torch.full((q1 - q0, 0), 0.0, dtype=torch.float64, device=dev)
                best_i = torch.zeros((q1 - q0, 0), dtype=torch.int64, device=dev)
                for r0 in range(0, N, RC):
                    r1 = min(N, r0 + RC)
                    D = nq[:, None] + n2[None, r0:r1] - 2.0 * (Xq @ Xc[r0:r1].T)
                    ids = torch.arange(r0, r1, device=dev, dtype=torch.int64)[None, :].expand(q1 - q0, -1)
                    D = torch.cat([best_d, D], dim=1)
                    ids = torch.cat([best_i, ids], dim=1)
                    best_d, sel = torch.topk(D, min(kk, D.shape[1]), dim=1, largest=False, sorted=True)
                    best_i = torch.gather(ids, 1, sel)
                rows = torch.arange(q0, q1, device=dev, dtype=torch.int64)[:, None] * cap + torch.arange(kk, device=dev)[None, :]
                cand_d2[rows.reshape(-1)] = best_d.clamp_(min=0.0).to(torch.float32).reshape(-1)
                cand_idx[rows.reshape(-1)] = best_i.to(torch.int32).reshape(-1)
        # (fp64 GEMM form + fp32 storage of d2: << 1e-6 max|x~|^2)
        return SimpleNamespace(plan=plan, idx=cand_idx, d2=cand_d2, cnt=cand_cnt, thr=None, cap=cap, err_coef=1e-6, err_lin=0.0, KP=a.d,
                               norm2=norm2, nmax=nmax, tiles_done=None, research=None)

    def _candidates_f32(self, a, plan, ksel, mean, norm2, nmax):
        """fp32 operands on v_mfma_f32_32x32x2_f32 (knn.hip)."""
        lib, st, dev, X, N, d = self.lib, stream(), a.X.device, a.X, a.N, a.d
        KP = lib.meld_knn_padded_dim(d)
        if KP < 0:
            check(KP, "meld_knn_padded_dim")
        TS, BQ = lib.meld_knn_tile_refs(), lib.meld_knn_block_queries()
        cap = lib.meld_knn_row_capacity(ksel)
        if cap < 0:
            check(cap, "meld_knn_row_capacity")
        n_tiles = (N + TS - 1) // TS
        Rt = torch.empty(n_tiles * KP * TS, dtype=torch.float32, device=dev)
        check(lib.meld_knn_prepare_refs(ptr(X), N, d, ptr(mean), KP, ptr(Rt), ptr(norm2), ptr(nmax), st), "meld_knn_prepare_refs")
        q_pad = ((a.q_count + BQ - 1) // BQ) * BQ
        Q = torch.empty(q_pad * KP, dtype=torch.float32, device=dev)
        check(lib.meld_knn_prepare_queries(ptr(X), N, d, ptr(mean), KP, a.q_begin, a.q_count, ptr(Q), st), "meld_knn_prepare_queries")
        a.tm.stop("prepare")
        cand_idx = torch.empty(q_pad * cap, dtype=torch.int32, device=dev)
        cand_d2 = torch.empty(q_pad * cap, dtype=torch.float32, device=dev)
        cand_cnt = torch.empty(q_pad, dtype=torch.int32, device=dev)
        with _EventSpan("knn_topk", N=N, d=d, q=a.q_count):
            check(lib.meld_knn_topk(ptr(Q), ptr(Rt), N, KP, a.q_count, ksel, ptr(cand_idx), ptr(cand_d2), ptr(cand_cnt), st), "meld_knn_topk")
        return SimpleNamespace(plan=plan, idx=cand_idx, d2=cand_d2, cnt=cand_cnt, thr=None, cap=cap, err_coef=lib.meld_knn_error_coef(d), err_lin=0.0,
                               KP=KP, norm2=norm2, nmax=nmax, tiles_done=None, research=None)

    def _candidates_f16x3(self, a, plan, ksel, comm, mean, col_min, col_max, norm2, nmax):
        """Split-fp16 operands on v_mfma_f32_32x32x16_f16 (knn16.hip): operands, start thresholds, step lists, the search."""
        lib, dev = self.lib, a.X.device
        cap = lib.meld_knn16_row_capacity(ksel)
        if cap < 0:
            check(cap, "meld_knn16_row_capacity")
        plan, o, nmax = self._operands16(a, plan, comm, mean, col_min, col_max, norm2, nmax)
        c = SimpleNamespace(plan=plan, cap=cap, err_coef=lib.meld_knn16_error_coef_const(plan.nprod, a.d), err_lin=lib.meld_knn16_error_coef_lin(plan.nprod),
                            KP=16 * o.KB, norm2=norm2, nmax=nmax, research=o if plan.stage2 else None)
        c.idx = torch.empty(o.q_pad * cap, dtype=torch.int32, device=dev)
        c.d2 = torch.empty(o.q_pad * cap, dtype=torch.float32, device=dev)
        c.cnt = torch.empty(o.q_pad, dtype=torch.int32, device=dev)
        c.thr, rfac = None, 1.0
        if plan.radius_cut:
            # rows are cut at the kernel radius their (knn+1)-th neighbour so far implies; the search publishes each row's final
            # threshold for refine's completeness test (the cut keeps everything within max(rf * bandwidth_scale, 1) bandwidths)
            c.thr = torch.full((o.q_pad,), float("inf"), dtype=torch.float32, device=dev)
            rfac = max(_radius_factor(a.decay, a.thresh) * float(a.bw_scale), 1.0)
        # [(wave, tile) pairs looked at, blocks of 32 references past the partial test (two-pass route: pairs the search computed,
        # then its blocks)]
        c.tiles_done = torch.zeros(4, dtype=torch.int64, device=dev)
        seeds = self._start_thresholds(a, plan, o, c, rfac)
        lists = self._step_lists(a, plan, o, seeds, nmax, comm)
        self._search16(a, plan, o, c, ksel, seeds, rfac, lists)
        return c

    def _operands16(self, a, plan, comm, mean, col_min, col_max, norm2, nmax):
        """The split-fp16 operands, in the cells' principal frame where the plan asks for it and the data carry one: everything up
        to the candidate lists works on X_s, refinement and the exact sweeps on X.  Returns the plan as it stands after the frame's
        test, the operands and the largest norm the error bounds speak of."""
        lib, st, dev, X, N, d = self.lib, stream(), a.X.device, a.X, a.N, a.d
        KB, TS, BQ = lib.meld_knn16_kblocks(d), lib.meld_knn16_tile_refs(), lib.meld_knn16_block_queries()
        o = SimpleNamespace(X_s=X, mean_s=mean, KB=KB, BQ=BQ, n_tiles=(a.NR + TS - 1) // TS, q_pad=((a.q_count + BQ - 1) // BQ) * BQ)
        if plan.frame:
            X_s = self.principal_frame(X, mean, int(lib.meld_knn16_split_dims(d)), comm, axes=a.frame_axes)
            if X_s is None:
                plan = plan.without_frame()
            else:
                sums_s, col_min, col_max = self.col_stats(X_s)
                o.X_s, o.mean_s = X_s, sums_s / N
        o.Rt = torch.empty(o.n_tiles * lib.meld_knn16_tile_bytes(d), dtype=torch.uint8, device=dev)
        o.Q = torch.empty(o.q_pad * lib.meld_knn16_query_bytes(d), dtype=torch.uint8, device=dev)
        o.Qn = torch.empty(o.q_pad, dtype=torch.float32, device=dev)
        o.scale_info = torch.empty(4, dtype=torch.float32, device=dev)
        tail = (a.q_begin, a.q_count, ptr(o.Rt), ptr(o.Q), ptr(o.Qn), ptr(norm2), ptr(nmax), ptr(o.scale_info), st)
        if a.cross:
            # (norm2 / nmax come back covering the queries too, in input units: the error bounds speak of the largest norm among ALL
            # points of the search, and refine reads the query's own norm at its row)
            check(lib.meld_knn16_prepare_cross(ptr(X), a.NR, N, d, ptr(mean), *tail), "meld_knn16_prepare_cross")
        elif plan.fused_operands:
            # queries = all the references: both layouts and the tile spheres (for _step_lists) from one read of every tile
            o.spheres = torch.empty(lib.meld_knn16_bounds_temp_bytes(N, d, a.q_count), dtype=torch.uint8, device=dev)
            check(lib.meld_knn16_prepare_fused(ptr(o.X_s), N, d, ptr(o.mean_s), ptr(col_min), ptr(col_max), ptr(o.Rt), ptr(o.Q), ptr(o.Qn), ptr(norm2),
                                               ptr(nmax), ptr(o.scale_info), ptr(o.spheres), st), "meld_knn16_prepare_fused")
        elif col_min is not None:
            check(lib.meld_knn16_prepare_scaled(ptr(o.X_s), N, d, ptr(o.mean_s), ptr(col_min), ptr(col_max), *tail), "meld_knn16_prepare_scaled")
        else:
            check(lib.meld_knn16_prepare(ptr(o.X_s), N, d, ptr(o.mean_s), *tail), "meld_knn16_prepare")
        a.tm.stop("prepare")
        return plan, o, nmax

    def _start_thresholds(self, a, plan, o, c, rfac):
        """Start thresholds of the first pass (scaled units) instead of +inf, or None."""
        lib, st, dev = self.lib, stream(), a.X.device
        if plan.seed == "bandwidth":
            # every row's radius is known: the thresholds start there, with the row's search-error allowance on top
            rad = (a.bw_fixed[a.q_begin : a.q_begin + a.q_count] * float(a.bw_scale)).clamp_(min=float(np.finfo(float).eps)) * _radius_factor(a.decay, a.thresh)
            nmx = c.nmax.to(torch.float64)
            e_row = float(c.err_coef) * nmx + float(c.err_lin) * torch.sqrt(c.norm2[a.q_begin : a.q_begin + a.q_count].to(torch.float64) * nmx)
            seeds = torch.full((o.q_pad,), float("inf"), dtype=torch.float32, device=dev)
            seeds[: a.q_count] = ((rad * rad + 1.01 * e_row) * o.scale_info[0].to(torch.float64) ** 2 * (1.0 + 1e-5)).to(torch.float32)
            if o.q_pad > a.q_count:
                seeds[a.q_count :] = seeds[a.q_count - 1]
            return seeds
        if plan.seed == "mfma":
            # every row starts at the kernel radius its own block of BQ cells (and its neighbour tiles) implies
            seeds = torch.empty(o.q_pad, dtype=torch.float32, device=dev)
            check(lib.meld_knn16_seed_thresholds_mfma(ptr(o.Q), ptr(o.Qn), ptr(o.Rt), ptr(o.scale_info), ptr(c.nmax), a.N, a.d, a.q_begin, a.q_count, a.knn,
                                                      rfac, plan.nprod, 0, ptr(seeds), st), "meld_knn16_seed_thresholds_mfma")
            a.tm.stop("seed")
            return seeds
        return None

    def _step_lists(self, a, plan, o, seeds, nmax, comm):
        """Exact tile pruning (after the seeds: with them the table also drops the tiles no query of a wave can reach from its own
        start threshold, see meld_knn16_bounds).  Returns (bounds table, step lists, their lengths, dispatch order); all None
        without pruning."""
        if not plan.prune:
            return None, None, None, None
        lib, st, dev, N, d = self.lib, stream(), a.X.device, a.N, a.d
        X_s, mean_s, n_tiles, n_blocks = o.X_s, o.mean_s, o.n_tiles, o.q_pad // o.BQ
        spheres_ready = getattr(o, "spheres", None) is not None  # (meld_knn16_prepare_fused left them there)
        tmpb = o.spheres if spheres_ready else torch.empty(lib.meld_knn16_bounds_temp_bytes(N, d, a.q_count), dtype=torch.uint8, device=dev)
        if plan.bounds == "bounds_from_spheres":
            # row-sharded build: the spheres of the reference tiles are the same on every rank (0.7 ms at 1M cells): every rank
            # computes 1 / world of them and the three arrays are all-gathered (4 MB in all)
            rows_c, row_b = sphere_layout(lib, N, d)
            per = rows_c // comm.world
            t0s = min(comm.rank * per, n_tiles)
            t1s = min(t0s + per, n_tiles)
            tmpb.zero_()
            check(lib.meld_knn16_tile_spheres(ptr(X_s), N, d, ptr(mean_s), ptr(o.scale_info), ptr(tmpb), t0s, max(t1s - t0s, 0), st), "meld_knn16_tile_spheres")
            parts = (tmpb[: rows_c * row_b], tmpb[rows_c * row_b : rows_c * (row_b + 4)], tmpb[rows_c * (row_b + 4) : rows_c * (row_b + 8)])
            for arr, width in zip(parts, (row_b, 4, 4)):
                mine = arr[comm.rank * per * width : (comm.rank + 1) * per * width].clone()
                comm.all_gather_rows(arr, mine)
        lb2 = step_list = step_cnt = None
        if plan.lists == "direct":
            # queries = all the cells: the lists come straight from the cells (bounds as two bits per (wave, tile); the fp16 table,
            # its symmetrisation pass and the list builder's pass over it never exist)
            step_list = torch.empty(n_blocks * n_tiles, dtype=torch.int32, device=dev)
            step_cnt = torch.empty(n_blocks, dtype=torch.int32, device=dev)
            scratch = torch.empty(lib.meld_knn16_list_scratch_bytes(N), dtype=torch.uint8, device=dev)
            check((lib.meld_knn16_step_lists_direct_spheres if spheres_ready else lib.meld_knn16_step_lists_direct_lead)(ptr(X_s), N, d, ptr(mean_s), ptr(o.scale_info), ptr(nmax), ptr(o.Rt), ptr(seeds), ptr(o.Qn), plan.nprod,
                ptr(tmpb), ptr(scratch), ptr(step_list), n_tiles, ptr(step_cnt), int(plan.lead_bounds), st),
                  "meld_knn16_step_lists_direct")
            del scratch
        else:
            sb = plan.seeded_bounds
            lb2 = torch.empty(lib.meld_knn16_bounds_bytes(N, a.q_count), dtype=torch.uint8, device=dev)
            check((lib.meld_knn16_bounds_from_spheres if plan.bounds == "bounds_from_spheres" or spheres_ready else lib.meld_knn16_bounds)(
                ptr(X_s), N, d, ptr(mean_s), ptr(o.scale_info), ptr(nmax), ptr(o.Rt), a.q_begin, a.q_count, ptr(seeds) if sb else None,
                ptr(o.Qn) if sb else None, plan.nprod, ptr(tmpb), ptr(lb2), st), "meld_knn16_bounds")
            if plan.lists == "table":
                # the tiles a block can rule out at its start thresholds, written down once (the count is the block's work)
                step_list = torch.empty(n_blocks * n_tiles, dtype=torch.int32, device=dev)
                step_cnt = torch.empty(n_blocks, dtype=torch.int32, device=dev)
                check(lib.meld_knn16_step_lists(ptr(lb2), ptr(seeds), N, d, a.q_count, plan.nprod, ptr(nmax), ptr(o.scale_info), a.q_begin,
                                                ptr(step_list), n_tiles, ptr(step_cnt), st), "meld_knn16_step_lists")
        work = step_cnt
        if plan.block_order == "work":
            # longest query blocks first (the dispatch follows the block index): see meld_knn16_block_work
            work = torch.empty(n_blocks, dtype=torch.int32, device=dev)
            check(lib.meld_knn16_block_work(ptr(lb2), ptr(seeds), N, d, a.q_count, plan.nprod, ptr(nmax), ptr(o.scale_info), ptr(work), st), "meld_knn16_block_work")
        block_order = torch.argsort(work, descending=True, stable=True).to(torch.int32) if plan.block_order != "none" else None
        a.tm.stop("bounds")
        return lb2, step_list, step_cnt, block_order

    def _search16(self, a, plan, o, c, ksel, seeds, rfac, lists):
        """The first pass: the partial filter where the plan has one (the search then stages whole tiles for the quarter of the
        pairs that survive), then the search itself, over ``plan.main_slices`` slices of the references."""
        lib, st, dev, d, q_count, q_pad, cap = self.lib, stream(), a.X.device, a.d, a.q_count, o.q_pad, c.cap
        lb2, step_list, step_cnt, block_order = lists
        q0 = 0 if a.cross else a.q_begin
        tiles_b = c.tiles_done
        if plan.two_pass:
            with _EventSpan("knn_filter", N=a.N, d=d, q=q_count):
                check(lib.meld_knn16_partial_filter(ptr(o.Q), ptr(o.Qn), ptr(o.Rt), ptr(o.scale_info), ptr(c.nmax), d, q_count, ptr(seeds), ptr(step_list),
                                                    ptr(step_cnt), o.n_tiles, ptr(step_cnt), ptr(c.tiles_done), ptr(block_order), st), "meld_knn16_partial_filter")
                if block_order is not None:  # (longest blocks first, by what is left of them)
                    block_order = torch.argsort(step_cnt, descending=True, stable=True).to(torch.int32)
            tiles_b = c.tiles_done[1:]  # (the search counts the pairs it computes, and its blocks, behind the filter's)
            a.tm.stop("knn_filter")
        S = plan.main_slices
        with _EventSpan("knn_topk", N=a.N, d=d, q=q_count):
            if S > 1:  # every slice with its own candidate rows, merged afterwards
                out = (torch.empty(S * q_pad * cap, dtype=torch.int32, device=dev), torch.empty(S * q_pad * cap, dtype=torch.float32, device=dev),
                       torch.empty(S * q_pad, dtype=torch.int32, device=dev), torch.full((S, q_pad), float("inf"), dtype=torch.float32, device=dev))
            else:
                out = (c.idx, c.d2, c.cnt, c.thr)
            c.raw = None
            if step_list is not None and plan.fused_rows == "sort+emit" and S == 1:
                # the rows stay as the search leaves them: the refinement ranks them in registers (meld_knn_refine_sort_emit)
                check(lib.meld_knn16_topk_listed_raw(ptr(o.Q), ptr(o.Qn), ptr(o.Rt), ptr(o.scale_info), a.NR, d, q_count, ksel, ptr(step_list), ptr(step_cnt),
                                                     o.n_tiles, ptr(c.nmax), q0, ptr(seeds), plan.knn_cut, rfac, *map(ptr, out), ptr(tiles_b), ptr(block_order),
                                                     int(plan.partial_in_search), st), "meld_knn16_topk_listed_raw")
                c.raw = (o.Qn, o.scale_info)
            elif step_list is not None:
                check(lib.meld_knn16_topk_listed_partial(ptr(o.Q), ptr(o.Qn), ptr(o.Rt), ptr(o.scale_info), a.NR, d, q_count, ksel, ptr(step_list), ptr(step_cnt),
                                                         o.n_tiles, ptr(c.nmax), q0, ptr(seeds), plan.knn_cut, rfac, *map(ptr, out), ptr(tiles_b), ptr(block_order),
                                                         S, int(plan.partial_in_search), st), "meld_knn16_topk_listed")
            else:
                check(lib.meld_knn16_topk(ptr(o.Q), ptr(o.Qn), ptr(o.Rt), ptr(o.scale_info), a.NR, d, q_count, ksel, plan.nprod, S, ptr(lb2), ptr(c.nmax), q0,
                                          ptr(seeds), plan.knn_cut, rfac, *map(ptr, out), ptr(c.tiles_done), ptr(block_order), st), "meld_knn16_topk")
            if S > 1:
                check(lib.meld_knn16_merge_slices(*map(ptr, out[:3]), q_count, ksel, S, ptr(c.idx), ptr(c.d2), ptr(c.cnt), st), "meld_knn16_merge_slices")
                c.thr.copy_(out[3].amin(0))  # the merged row holds every reference below the smallest slice threshold
            del out
            # the search is the one long launch of the build (26 of 45 ms at 1M cells) and the host has nothing to do until its
            # results are refined: work that does not depend on the graph (fit_transform's label factorisation: a host-blocking
            # copy + a few small launches on a side stream) is started here
            while _WHILE_SEARCHING:
                _WHILE_SEARCHING.pop()()
        del o.Q

    def _refine(self, a, c, ksel):
        """Exact refinement + alpha-decay kernel of every candidate row; rows the first pass could not certify searched again with
        the full hi/lo split (a few % of the rows) where the plan has that stage; then ONE read-back of the scalars the host
        wants here (each one is an idle gap of the GPU of ~50 us: nothing is queued behind it): rows still flagged, kept
        entries, (wave, tile) pairs the first pass computed."""
        lib, st, dev, q_count = self.lib, stream(), a.X.device, a.q_count
        r = SimpleNamespace(plan=c.plan, cands=c)
        max_rank = 0 if a.knn_max is None else int(a.knn_max) + 1  # (self counted, as graphtools counts it)
        r.bw = torch.empty(q_count, dtype=torch.float64, device=dev)
        r.keep_cnt = torch.empty(q_count, dtype=torch.int32, device=dev)
        r.flag_rows = torch.empty(q_count, dtype=torch.int32, device=dev)
        n_flag = torch.zeros(1, dtype=torch.int32, device=dev)
        nmax_used = c.nmax
        if a.force_fallback:  # test hook: an infinite error bound flags every row
            nmax_used = torch.full((1,), float("inf"), dtype=torch.float32, device=dev)
        r.buckets = r.cand_val = r.rows2 = None
        if c.plan.fused_rows != "off":
            # the kept entries of the complete rows go straight into the row buckets (cursor, tcol, tval); kernel values are stored
            # for the rows of the second stage only (_stage2), which _emit sends behind them with the swept entries
            B = int(lib.meld_csr_bucket_slots())
            r.buckets = (torch.empty(q_count, dtype=torch.int32, device=dev), torch.empty(q_count * B, dtype=torch.int32, device=dev),
                         torch.empty(q_count * B, dtype=torch.float64, device=dev))
            raw = getattr(c, "raw", None)  # (the search left the rows raw: ranked inside the refinement)
            tail = (ksel, c.cap, a.knn, float(a.decay), float(a.thresh), ptr(nmax_used), float(c.err_coef), ptr(c.norm2), float(c.err_lin), ptr(r.bw),
                    ptr(r.keep_cnt), ptr(r.flag_rows), ptr(n_flag), float(a.bw_scale), ptr(a.bw_fixed), max_rank, *map(ptr, r.buckets), st)
            if raw is not None:
                check(lib.meld_knn_refine_sort_emit(ptr(a.X), a.N, a.d, ptr(c.idx), ptr(c.d2), ptr(c.cnt), ptr(raw[0]), ptr(raw[1]), ptr(c.thr), *tail),
                      "meld_knn_refine_sort_emit")
            else:
                check(lib.meld_knn_refine_emit(ptr(a.X), a.N, a.d, ptr(c.idx), ptr(c.d2), ptr(c.cnt), ptr(c.thr), *tail), "meld_knn_refine_emit")
        else:
            r.cand_val = torch.empty(q_count * ksel, dtype=torch.float64, device=dev)
            check(
                lib.meld_knn_refine(
                    ptr(a.X), a.N, a.d, a.q_begin, q_count, ptr(c.idx), ptr(c.d2), ptr(c.cnt), ptr(c.thr), ksel, c.cap, a.knn, float(a.decay),
                    float(a.thresh), ptr(nmax_used), float(c.err_coef), ptr(c.norm2), float(c.err_lin), ptr(r.bw), ptr(r.cand_val), ptr(r.keep_cnt),
                    ptr(r.flag_rows), ptr(n_flag), None, 0, None, float(a.bw_scale), ptr(a.bw_fixed), max_rank, st,
                ),
                "meld_knn_refine",
            )
        r.n_flag = r.n_flag_stage1 = int(n_flag.item())
        a.tm.stop("refine")
        stage2 = c.research is not None and r.n_flag > 0 and not a.force_fallback
        if stage2:
            self._stage2(a, c, r, ksel, n_flag, max_rank)
        c.research = None
        r.keep_off = scan_i32(r.keep_cnt)
        td, p = c.tiles_done, c.plan
        heads = [n_flag[0].to(torch.int64), r.keep_off[q_count]] + ([td[0], td[2] if p.two_pass else td[1], td[1]] if td is not None else [])
        heads_h = torch.stack(heads).tolist()
        if stage2:
            r.n_flag = int(heads_h[0])
        r.m_main = int(heads_h[1])
        r.tiles_done_h = int(heads_h[2]) if td is not None else None
        r.blocks_on_h = int(heads_h[3]) if td is not None and p.frame else None
        r.pairs_kept_h = int(heads_h[4]) if td is not None and p.two_pass else None  # (wave, tile) pairs the filter pass left to the search
        if r.pairs_kept_h is not None and lib.meld_knn16_kblocks(a.d) > 7:
            r.blocks_on_h = 2 * r.pairs_kept_h  # (beyond seven K blocks the search behind the filter has no test of its own: both blocks of every pair it is handed)
        return r

    def _stage2(self, a, c, r, ksel, n_flag, max_rank):
        """The flagged rows searched again with the full hi/lo split; only what that cannot certify either goes to the exact sweep."""
        lib, st, dev, d, cap, o = self.lib, stream(), a.X.device, a.d, c.cap, c.research
        n_flag_h = r.n_flag
        rows2 = torch.sort(r.flag_rows[:n_flag_h]).values.contiguous()
        if r.buckets is not None:  # (fused row pass: the first stage stored no kernel values; these rows' are stored at their local row)
            r.cand_val = torch.empty(a.q_count * ksel, dtype=torch.float64, device=dev)
            r.rows2 = rows2
        q2_pad = ((n_flag_h + o.BQ - 1) // o.BQ) * o.BQ
        Q2 = torch.empty(q2_pad * lib.meld_knn16_query_bytes(d), dtype=torch.uint8, device=dev)
        Qn2 = torch.empty(q2_pad, dtype=torch.float32, device=dev)
        check(lib.meld_knn16_prepare_rows(ptr(o.X_s), a.N, d, ptr(o.mean_s), ptr(o.scale_info), a.q_begin, ptr(rows2), n_flag_h, ptr(Q2), ptr(Qn2), st), "meld_knn16_prepare_rows")
        # few queries: cut the references into slices so that the re-search fills the chip
        n_blocks2 = q2_pad // o.BQ
        resident = lib.meld_knn16_resident_blocks(d, 3)
        if resident < 0:
            check(resident, "meld_knn16_resident_blocks")
        n_slices = int(max(1, min(lib.meld_knn16_max_slices(ksel), 2 * resident // max(n_blocks2, 1), o.n_tiles)))
        # Start the thresholds of the re-search at a bound instead of +inf: the first pass found ksel references with approximate
        # d2 <= tau, so the true ksel-th distance is <= tau + E1 and its full-precision approximation <= tau + E1 + E3 -- nothing
        # above that can enter the list.  (Without it every slice selects from scratch: 19k appends per query at 1M cells.)
        thr2 = torch.empty(q2_pad, dtype=torch.float32, device=dev)
        check(lib.meld_knn16_research_thresholds(ptr(rows2), n_flag_h, a.q_begin, ptr(c.cnt), ptr(c.d2), cap, ksel, ptr(c.norm2), ptr(c.nmax),
                                                 float(c.err_coef), float(c.err_lin), float(lib.meld_knn16_error_coef(3, d)),
                                                 ptr(o.scale_info), ptr(thr2), st), "meld_knn16_research_thresholds")
        c2_idx = torch.empty(n_slices * q2_pad * cap, dtype=torch.int32, device=dev)
        c2_d2 = torch.empty(n_slices * q2_pad * cap, dtype=torch.float32, device=dev)
        c2_cnt = torch.empty(n_slices * q2_pad, dtype=torch.int32, device=dev)
        with _EventSpan("knn_topk_stage2", N=a.N, d=d, q=n_flag_h):
            check(lib.meld_knn16_topk(ptr(Q2), ptr(Qn2), ptr(o.Rt), ptr(o.scale_info), a.NR, d, n_flag_h, ksel, 3, n_slices, None, ptr(c.nmax), 0, ptr(thr2), 0, 1.0,
                                      ptr(c2_idx), ptr(c2_d2), ptr(c2_cnt), None, None, None, st), "meld_knn16_topk(stage 2)")
            if n_slices > 1:
                m_idx = torch.empty(q2_pad * cap, dtype=torch.int32, device=dev)
                m_d2 = torch.empty(q2_pad * cap, dtype=torch.float32, device=dev)
                m_cnt = torch.empty(q2_pad, dtype=torch.int32, device=dev)
                check(lib.meld_knn16_merge_slices(ptr(c2_idx), ptr(c2_d2), ptr(c2_cnt), n_flag_h, ksel, n_slices, ptr(m_idx), ptr(m_d2), ptr(m_cnt), st), "meld_knn16_merge_slices")
                c2_idx, c2_d2, c2_cnt = m_idx, m_d2, m_cnt
        n_flag.zero_()
        check(
            lib.meld_knn_refine(
                ptr(a.X), a.N, d, a.q_begin, n_flag_h, ptr(c2_idx), ptr(c2_d2), ptr(c2_cnt), None, ksel, cap, a.knn, float(a.decay),
                float(a.thresh), ptr(c.nmax), float(lib.meld_knn16_error_coef(3, d)), None, 0.0, ptr(r.bw), ptr(r.cand_val), ptr(r.keep_cnt),
                ptr(r.flag_rows), ptr(n_flag), ptr(rows2), cap, ptr(c.idx), float(a.bw_scale), ptr(a.bw_fixed), max_rank, st,
            ),
            "meld_knn_refine(stage 2)",
        )
        a.tm.stop("knn_stage2")

    def _exact_sweep(self, a, r, count_rows_ge):
        """Exact sweep of the rows the candidate lists could not certify (their bandwidth recomputed where a list missed one of
        the knn nearest cells, knn_max applied to the swept rows), and the count of rows with at least ``count_rows_ge`` cells."""
        lib, st, dev, q_count, n_flag_h = self.lib, stream(), a.X.device, a.q_count, r.n_flag
        knn_chk = a.knn if a.bw_fixed is None else 2**31 - 1  # (a given bandwidth is not verified against the neighbour count)
        s = SimpleNamespace(n_rebandwidth=0, fb_total=0, fb_off=None, fb_col=None, fb_val=None, fb_cnt=None, rows_at_least=None)
        if n_flag_h > 0:
            r.flag_rows = flag_rows = torch.sort(r.flag_rows[:n_flag_h]).values.contiguous()  # deterministic order
            fb_cnt = torch.empty(n_flag_h, dtype=torch.int32, device=dev)
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            cursor = torch.zeros(n_flag_h, dtype=torch.int32, device=dev)  # count pass: references closer than bw

            def sweep(fill, what, fb_cnt=None, fb_off=None, fb_col=None, fb_val=None, err=None):
                check(lib.meld_knn_radius_exact(ptr(a.X), a.NR, a.d, a.q_begin, ptr(flag_rows), n_flag_h, ptr(r.bw), knn_chk, float(a.decay), float(a.thresh), fill,
                                                ptr(fb_cnt), ptr(fb_off), ptr(cursor), ptr(fb_col), ptr(fb_val), ptr(err), float(a.bw_scale), st), what)

            sweep(0, "meld_knn_radius_exact(count)", fb_cnt=fb_cnt, err=err)
            if int(err.item()) != 0:
                # rows whose candidate list missed one of their knn nearest cells (marked fb_cnt = -1: more than knn references are
                # strictly closer than the bandwidth the list implied): their bandwidth is recomputed exactly over all references --
                # a rare library path (fp64 screen + direct differences) -- and the sweep is counted again (graphtools re-searches
                # such rows with more neighbours)
                bad = torch.nonzero(fb_cnt < 0).reshape(-1)
                rows_bad = flag_rows[bad].to(torch.int64)
                r.bw[rows_bad] = _exact_bandwidth(a.X, a.q_begin + rows_bad, a.knn, n_refs=a.NR)
                fb_cnt.zero_()
                cursor.zero_()
                err.zero_()
                sweep(0, "meld_knn_radius_exact(recount)", fb_cnt=fb_cnt, err=err)
                if int(err.item()) != 0:
                    raise NotImplementedError(
                        "degenerate neighbourhoods: the exact sweep could not settle the bandwidth of {} rows".format(int((fb_cnt < 0).sum())))
                s.n_rebandwidth = int(bad.shape[0])
            fb_off = scan_i32(fb_cnt)
            fb_total = int(fb_off[n_flag_h].item())
            # (a radius that covers most of the data -- small decay with a small thresh -- makes the graph effectively dense: say so
            # instead of failing inside an allocation; the reference's scipy matrices would be as large)
            need = 12 * fb_total + 32 * (r.m_main + fb_total)
            if need > torch.cuda.get_device_properties(dev).total_memory:
                raise MemoryError(
                    "the kernel radius covers {:.3g} neighbours per cell on average: the graph would hold {:.3g} entries ({:.0f} GB to "
                    "assemble) -- raise decay or thresh".format((r.m_main + fb_total) / max(q_count, 1), float(r.m_main + fb_total), need / 1e9))
            fb_col = torch.empty(max(fb_total, 1), dtype=torch.int32, device=dev)
            fb_val = torch.empty(max(fb_total, 1), dtype=torch.float64, device=dev)
            sweep(1, "meld_knn_radius_exact(fill)", fb_off=fb_off, fb_col=fb_col, fb_val=fb_val)  # (the count pass left the cursors at zero)
            if a.knn_max is not None and fb_total > 0 and int(fb_cnt.max()) > int(a.knn_max):
                # knn_max on the rows the sweep filled (everything inside the radius, unranked): keep the knn_max largest kernel
                # values of a row (= its nearest cells; ties by column) -- a rare path, a few library sorts over the swept entries
                rows_e = torch.repeat_interleave(torch.arange(n_flag_h, device=dev), fb_cnt.to(torch.int64))
                o = torch.argsort(fb_col[:fb_total].to(torch.int64), stable=True)
                o = o[torch.argsort(-fb_val[:fb_total][o], stable=True)]
                o = o[torch.argsort(rows_e[o], stable=True)]
                rank = torch.arange(fb_total, device=dev) - fb_off[:n_flag_h][rows_e[o]]
                keep = o[rank < int(a.knn_max)]
                keep = keep[torch.argsort(rows_e[keep], stable=True)]
                fb_col, fb_val = fb_col[keep].contiguous(), fb_val[keep].contiguous()
                fb_cnt = torch.clamp(fb_cnt, max=int(a.knn_max))
                fb_off = scan_i32(fb_cnt)
                fb_total = int(fb_off[n_flag_h].item())
            s.fb_total, s.fb_off, s.fb_col, s.fb_val, s.fb_cnt = fb_total, fb_off, fb_col, fb_val, fb_cnt
        a.tm.stop("radius_exact")
        if count_rows_ge is not None:
            tot = r.keep_cnt.to(torch.int64)
            if n_flag_h > 0 and s.fb_total > 0:
                tot = tot.clone()
                tot[r.flag_rows[:n_flag_h].to(torch.int64)] = s.fb_cnt.to(torch.int64)
            s.rows_at_least = int(((tot + 1) >= int(count_rows_ge)).sum())  # (+ 1: the cell itself, K_ii = 1 is carried analytically)
        return s

    def _emit(self, a, r, s, ksel, assemble, symm, anisotropy=None):
        """The kept entries as (keys, vals) COO pairs -- or, on a single GPU with every row local, straight into the row buckets of
        the symmetrisation (meld_coo_emit_scatter) instead of through 2 M (key, value) pairs (512 MB written and read back at 1M
        cells).  Returns (keys, vals, assembled): assembled = (rowptr, col, val[, row sums[, degrees]]) of the symmetrised rows, else
        None; with the degrees (``anisotropy`` given), val is the kernel with the anisotropy applied.  On the fused route
        (``plan.fused_rows``) the refinement has filled the buckets with the complete rows already: the rows of the second stage and
        the swept entries follow (meld_coo_emit_scatter_listed); buckets that cannot be finished then return (None, None, None)."""
        lib, st, dev, q_count, n_flag_h, c = self.lib, stream(), a.X.device, a.q_count, r.n_flag, r.cands
        M = r.m_main + s.fb_total
        assembled = None
        # (plan.fused_rows: the refinement filled the buckets with the complete rows; meld_amd.metric_knn hands in rows of its own)
        fused = getattr(r, "buckets", None) is not None
        if fused or (M > 0 and bucket_route(lib, a.NR, a.q_begin, q_count, ksel, cross=a.cross, assemble=assemble,
                                            free_bytes=torch.cuda.mem_get_info(dev)[0])):
            if fused and M == 0:
                r.buckets = None
            else:
                if fused:
                    cursor, tcol, tval = r.buckets
                    n2 = int(r.rows2.shape[0]) if r.rows2 is not None else 0
                    if n2 > 0 or (n_flag_h > 0 and s.fb_total > 0):  # the rows of the second stage, the entries of the sweep
                        check(lib.meld_coo_emit_scatter_listed(ptr(r.rows2), n2, ptr(c.idx), ptr(r.cand_val), ksel, c.cap, ptr(r.keep_cnt), ptr(r.flag_rows),
                                                               n_flag_h, ptr(s.fb_off), ptr(s.fb_col), ptr(s.fb_val), s.fb_total, ptr(cursor), ptr(tcol),
                                                               ptr(tval), st), "meld_coo_emit_scatter_listed")
                else:
                    B = int(lib.meld_csr_bucket_slots())
                    cursor = r.keep_cnt.clone()
                    if n_flag_h > 0 and s.fb_total > 0:
                        cursor[r.flag_rows[:n_flag_h].to(torch.int64)] = s.fb_cnt
                    tcol = torch.empty(q_count * B, dtype=torch.int32, device=dev)
                    tval = torch.empty(q_count * B, dtype=torch.float64, device=dev)
                    check(lib.meld_coo_emit_scatter(q_count, ptr(c.idx), ptr(r.cand_val), ksel, c.cap, ptr(r.keep_cnt), ptr(r.flag_rows), n_flag_h,
                                                    ptr(s.fb_off), ptr(s.fb_col), ptr(s.fb_val), s.fb_total, ptr(cursor), ptr(tcol), ptr(tval), st),
                          "meld_coo_emit_scatter")
                a.tm.stop("coo_emit")
                # MELD_ASSEMBLE_FUSED_ANISO=0: the anisotropy as a pass of its own over the finished CSR (same bits)
                aniso = anisotropy if opt("MELD_ASSEMBLE_FUSED_ANISO", "1") != "0" else None
                assembled = self._finish_buckets(cursor, tcol, tval, q_count, sums_diag=1.0, symm=symm, anisotropy=aniso)  # None: a bucket overflowed / a column thrice
                if assembled is not None and self.last_row_sums is not None:
                    assembled = assembled + (self.last_row_sums[1],)  # (kernel row sums incl. the unit diagonal)
                    if self.last_degrees is not None:
                        assembled = assembled + (self.last_degrees,)
                a.tm.stop("symmetrize")
                del cursor, tcol, tval
                if fused and assembled is None:
                    return None, None, None  # (no kernel values to fall back on: directed_kernel_coo builds the graph again)
        keys = vals = None
        if assembled is None:
            keys = torch.empty(2 * M, dtype=torch.int64, device=dev)
            vals = torch.empty(2 * M, dtype=torch.float64, device=dev)
            if M > 0:
                check(
                    lib.meld_coo_emit(
                        a.q_begin, q_count, ptr(c.idx), ptr(r.cand_val), ptr(c.cnt), ksel, c.cap, ptr(r.keep_off), ptr(r.flag_rows),
                        n_flag_h, ptr(s.fb_off), ptr(s.fb_col), ptr(s.fb_val), r.m_main, M, ptr(keys), ptr(vals), st,
                    ),
                    "meld_coo_emit",
                )
        a.tm.stop("coo_emit")
        return keys, vals, assembled

    # ---- A4: (K + K^T)/2 rows [row_begin, row_begin + n_rows) from unsorted COO ---------------------
    sort_pairs = staticmethod(sort_pairs)  # (part of the ops interface: distributed.py calls it on the object)

    def partition_remote(self, keys, vals, rows_per_rank, world, rank, cap):
        """Row-sharded build: the entries owed to the other ranks in a fixed-capacity send buffer [world, 2, cap] (keys |
        value bits, sentinel key ~0 in unused slots) and the per-owner counts, all on the device
        (``meld_coo_partition_remote``)."""
        dev = keys.device
        counts = torch.empty(world, dtype=torch.int32, device=dev)
        send = torch.empty(world * 2 * cap, dtype=torch.int64, device=dev)
        check(self.lib.meld_coo_partition_remote(ptr(keys), ptr(vals), int(keys.shape[0]), int(rows_per_rank), int(world), int(rank),
                                                 int(cap), ptr(counts), ptr(send), stream()), "meld_coo_partition_remote")
        return send, counts

    def _finish_buckets(self, cursor, tcol, tval, n_rows, sums_diag=None, symm=(0, 0.0), anisotropy=None):
        """Row buckets (meld_coo_scatter_rows / meld_coo_emit_scatter) -> CSR: every bucket sorted by column and its pairs
        of equal columns summed inside one wave, then compacted.  None when a bucket overflowed or a column occurs more
        than twice (the caller takes the sort-based path, whose summation order is defined).  ``anisotropy`` (with ``sums_diag``;
        the buckets hold ALL rows of the graph): the row sums come out of the merge, and the compaction writes
        K_ij / (ksum_i ksum_j)^a and sums the degrees (``last_degrees``) -- the CSR is written once, with the bits of
        ``meld_csr_compact_rows_sums`` + ``meld_csr_anisotropy_degrees``."""
        lib, st, dev = self.lib, stream(), cursor.device
        i32 = dict(dtype=torch.int32, device=dev)
        ucnt = torch.empty(n_rows, **i32)
        flags = torch.empty(1, **i32)
        fused = anisotropy is not None and sums_diag is not None
        if fused:
            sums = torch.empty(n_rows, dtype=torch.float64, device=dev)
            check(lib.meld_csr_rows_sort_merge_sums(ptr(cursor), n_rows, ptr(tcol), ptr(tval), ptr(ucnt), ptr(flags), int(symm[0]), float(symm[1]),
                                                    float(sums_diag), ptr(sums), st), "meld_csr_rows_sort_merge_sums")
        else:
            check(lib.meld_csr_rows_sort_merge(ptr(cursor), n_rows, ptr(tcol), ptr(tval), ptr(ucnt), ptr(flags), int(symm[0]), float(symm[1]), st), "meld_csr_rows_sort_merge")
        rowptr = scan_i32(ucnt)
        nnz, flag = (int(v) for v in torch.stack([rowptr[n_rows], flags[0].to(torch.int64)]).tolist())  # (one read-back)
        if flag != 0:
            return None
        col = torch.empty(nnz, **i32)
        val = torch.empty(nnz, dtype=torch.float64, device=dev)
        self.last_row_sums = self.last_degrees = None
        if nnz > 0 and fused:
            dw = torch.empty(n_rows, dtype=torch.float64, device=dev)
            check(lib.meld_csr_compact_rows_anisotropy(ptr(rowptr), n_rows, ptr(tcol), ptr(tval), ptr(col), ptr(val), ptr(sums), float(anisotropy), ptr(dw), st),
                  "meld_csr_compact_rows_anisotropy")
            self.last_row_sums, self.last_degrees = (sums_diag, sums), dw
        elif nnz > 0 and sums_diag is not None:
            # (the rows' sums on the way out of the buckets: meld_csr_row_sums' bits without its pass over the values)
            sums = torch.empty(n_rows, dtype=torch.float64, device=dev)
            check(lib.meld_csr_compact_rows_sums(ptr(rowptr), n_rows, ptr(tcol), ptr(tval), ptr(col), ptr(val), float(sums_diag), ptr(sums), st),
                  "meld_csr_compact_rows_sums")
            self.last_row_sums = (sums_diag, sums)
        elif nnz > 0:
            check(lib.meld_csr_compact_rows(ptr(rowptr), n_rows, ptr(tcol), ptr(tval), ptr(col), ptr(val), st), "meld_csr_compact_rows")
        self.last_assemble = "bucket"
        return rowptr, col, val

    def assemble_rows(self, keys, vals, row_begin, n_rows, N, foreign=False, symm=(0, 0.0)):
        """Sum duplicate keys, build the CSR (sorted rows) of the local rows: by row buckets sorted inside one wave
        each (include/meld_hip.h, meld_coo_row_counts ...), or -- for the inputs that path refuses, and with
        ``MELD_ASSEMBLE=sort`` -- by a global radix sort + reduce-by-key.  ``foreign``: the input may hold entries of
        rows outside the slice (the fixed-capacity exchange of the sharded build: other ranks' rows, sentinel keys);
        the bucket path ignores them, the sort path drops them first."""
        lib, st, dev = self.lib, stream(), keys.device
        n = int(keys.shape[0])
        B = int(lib.meld_csr_bucket_slots())
        # the buckets cost 12 B x B slots per row whatever the degree (3 KB per row: 3 GB at 1M rows): above a quarter of
        # the free memory -- very large or tightly sharded runs -- the sort path (32 B per entry) is taken instead
        bucket_bytes = n_rows * B * 12
        fits = bucket_bytes <= torch.cuda.mem_get_info(dev)[0] // 4 if n_rows > 0 else True
        if n > 0 and n_rows > 0 and fits and opt("MELD_ASSEMBLE", "bucket") != "sort":
            i32 = dict(dtype=torch.int32, device=dev)
            cursor = torch.empty(n_rows, **i32)
            tcol = torch.empty(n_rows * B, **i32)
            tval = torch.empty(n_rows * B, dtype=torch.float64, device=dev)
            check(lib.meld_coo_scatter_rows(ptr(keys), ptr(vals), n, row_begin, n_rows, ptr(cursor), ptr(tcol), ptr(tval), st), "meld_coo_scatter_rows")
            done = self._finish_buckets(cursor, tcol, tval, n_rows, symm=symm)
            if done is not None:
                return done
            del cursor, tcol, tval
        self.last_assemble = "sort" if n > 0 else "empty"
        if foreign and n > 0:
            rows = keys >> 32  # (the sentinel ~0 is -1 as int64: its row is negative)
            own = (rows >= row_begin) & (rows < row_begin + n_rows)
            keys, vals = keys[own].contiguous(), vals[own].contiguous()
            n = int(keys.shape[0])
        keys2, vals2 = self.sort_pairs(keys, vals, N)
        if symm[0] != 0 and n > 0:
            # kernel_symm "*" / "mnn" behind the global sort (overfull row buckets -- hub cells --, MELD_ASSEMBLE=sort): the two HALVES
            # of a key sit side by side; the rules of meld_csr_rows_sort_merge (csrc/assemble.hip) on them, as library segment
            # reductions -- a rare path.  Symmetric functions of the pair: (i, j) and (j, i) get the same bits.
            first = torch.ones(n, dtype=torch.bool, device=dev)
            first[1:] = keys2[1:] != keys2[:-1]
            seg = torch.cumsum(first, 0) - 1
            nseg = int(seg[-1].item()) + 1
            cnt = torch.bincount(seg, minlength=nseg)
            if int(cnt.max().item()) > 2:
                raise NotImplementedError("kernel_symm other than '+': an entry of the kernel occurs more than once per direction")
            hi = torch.zeros(nseg, dtype=torch.float64, device=dev).scatter_reduce_(0, seg, vals2, "amax", include_self=False)
            lo = torch.zeros(nseg, dtype=torch.float64, device=dev).scatter_reduce_(0, seg, vals2, "amin", include_self=False)
            lo = torch.where(cnt == 2, lo, torch.zeros_like(lo))  # (the missing direction counts as 0)
            if symm[0] == 1:
                v, keep = 4.0 * hi * lo, cnt == 2
            else:
                v = 2.0 * (float(symm[1]) * lo + (1.0 - float(symm[1])) * hi)
                keep = v != 0.0
            ukeys, uvals = keys2[first][keep].contiguous(), v[keep].contiguous()
            nnz = int(ukeys.shape[0])
        else:
            ukeys, uvals, nnz = coo_merge(keys2, vals2)
        rowptr, col = csr_from_keys(ukeys, nnz, row_begin, n_rows)
        return rowptr, col, uvals[:nnz].clone()

    def gather_rows(self, X, perm):
        """X[perm] for an fp64 [N, d] matrix (``meld_gather_rows_f64``)."""
        X = X.contiguous()
        perm = perm.to(torch.int64).contiguous()
        out = torch.empty((int(perm.shape[0]), int(X.shape[1])), dtype=torch.float64, device=X.device)
        check(self.lib.meld_gather_rows_f64(ptr(X), ptr(perm), int(perm.shape[0]), int(X.shape[1]), ptr(out), stream()), "meld_gather_rows_f64")
        return out

    def row_sums(self, rowptr, val, n_rows, diag):
        out = torch.empty(n_rows, dtype=torch.float64, device=rowptr.device)
        check(self.lib.meld_csr_row_sums(ptr(rowptr), ptr(val), n_rows, float(diag), ptr(out), stream()), "meld_csr_row_sums")
        return out

    def anisotropy(self, rowptr, col, val, n_rows, ksum_all, row_off, a):
        check(self.lib.meld_csr_anisotropy(ptr(rowptr), ptr(col), ptr(val), n_rows, ptr(ksum_all), row_off, float(a), stream()), "meld_csr_anisotropy")

    def anisotropy_degrees(self, rowptr, col, val, n_rows, ksum_all, row_off, a):
        """``anisotropy`` and the row sums of its result in one pass (``meld_csr_anisotropy_degrees``: the same bits as
        ``row_sums(..., 0.0)`` afterwards)."""
        dw = torch.empty(n_rows, dtype=torch.float64, device=val.device)
        check(self.lib.meld_csr_anisotropy_degrees(ptr(rowptr), ptr(col), ptr(val), n_rows, ptr(ksum_all), row_off, float(a), ptr(dw), stream()),
              "meld_csr_anisotropy_degrees")
        return dw

    # ---- A9 / A10: operator steps -----------------------------------------------------------------
    def dot_slots(self):
        return self.lib.meld_spmm_dot_slots()

    # ---- panel-tiled copy of W for the recurrence (csrc/spmm_tiled.hip) -----------------------------
    shards_spheres = True  # directed_kernel_coo(comm=...) splits the tile spheres of the pruning table over the ranks
    PT_MIN_ROWS = 65536  # below this the CSR-stream kernel is launch-bound anyway and the layout does not pay

    _pt_selfcheck = {}  # device index -> bool (once per device and process, i.e. per load of the library)

    @classmethod
    def _pt_self_check(cls):
        """Once per device and process, before the tiled recurrence kernel is trusted: steps on a small random symmetric
        matrix through both kernels, for every instantiation the product launches -- p = 2 and p = 1 on fp64 values (a 3-column
        step is one launch of each) and the p = 1 kernel on the fp32 copy of the values (the SpMV of the lmax estimate).  The
        tiled kernel keeps loads in flight in registers it names itself and counts its waits by hand; a toolchain that broke
        those assumptions would return stale data, not an error -- a mismatch here keeps every graph on the CSR-stream kernel
        (and says so).  (The assembly-level guard of the same assumption runs at build time: ``meld_amd.build``.)"""
        dev_i = int(torch.cuda.current_device())
        if dev_i in cls._pt_selfcheck:
            return cls._pt_selfcheck[dev_i]
        cls._pt_selfcheck[dev_i] = ok = True
        from scipy import sparse

        rng = np.random.default_rng(0)
        n = 6000
        A = sparse.random(n, n, density=20.0 / n, random_state=0, format="csr", dtype=np.float64)
        A.data = rng.random(A.nnz) + 0.1
        W = ((A + A.T) * 0.5).tocsr()
        W.setdiag(0)
        W.eliminate_zeros()
        W.sort_indices()
        x3 = torch.from_numpy(rng.random((n, 3))).cuda()
        x1 = x3[:, 0].contiguous()
        outs = {}
        for mode in ("tiled", "csr"):
            G = DeviceGraph.from_scipy(W)
            ops = HipOps(spmm=mode)
            if mode == "tiled" and ops.pt_layout(G, _checking=True) is None:
                ok = False
                break
            y3 = torch.empty_like(x3)
            ops.cheby_step(G, 3, x3, 0, x3, y3, None, 0.7, -0.2, -1.0, 0.0)  # one launch of the p = 2 and one of the p = 1 kernel
            # the SpMV of the device-resident Lanczos loops: scalars from device memory, fp32 values on the tiled layout
            state = torch.zeros(8, dtype=torch.float64, device="cuda")
            state[3], state[4] = 0.9, -0.3
            dots = torch.zeros(2 * ops.dot_slots(), dtype=torch.float64, device="cuda")
            y1 = torch.empty_like(x1)
            ops.lanczos_spmv(G, x1, x1.clone(), y1, state, dots)
            outs[mode] = (y3, y1, dots[: ops.dot_slots()].sum())
        if ok:
            t, c = outs["tiled"], outs["csr"]
            e3 = float((t[0] - c[0]).abs().max() / c[0].abs().max())
            e1 = float((t[1] - c[1]).abs().max() / c[1].abs().max())
            ed = float((t[2] - c[2]).abs() / c[2].abs())
            ok = e3 < 1e-12 and e1 < 1e-6 and ed < 1e-6  # (fp32 values: 6e-8 per weight)
        cls._pt_selfcheck[dev_i] = ok
        if not ok:
            import warnings

            warnings.warn("meld_amd: the panel-tiled recurrence kernel failed its self-check against the CSR-stream kernel; "
                          "every graph stays on the CSR-stream kernel", RuntimeWarning)
        return ok

    def pt_layout(self, G, _checking=False):
        """The panel-tiled layout of ``G``'s local rows, built on first use and kept on the graph
        (``G.pt``); None when the graph stays on the CSR-stream kernel (small graphs, ``spmm="csr"``, or a
        graph the builder cannot lay out -- recorded in ``G.info["spmm"]``)."""
        pt = getattr(G, "pt", None)
        if pt is not None:
            return pt if pt is not False else None
        mode = getattr(self, "spmm", None) or opt("MELD_SPMM", "auto")
        G.info["spmm"] = "csr"
        G.pt = False
        if mode == "csr" or G.n_rows == 0 or G.nnz == 0 or not G.val.is_cuda:
            return None
        if mode == "auto" and G.n_rows < self.PT_MIN_ROWS:
            return None
        if not _checking and not self._pt_self_check():
            G.info["spmm"] = "csr (tiled kernel failed its self-check)"
            return None
        from ._lib import PtLayout
        import ctypes as C

        lib, dev = self.lib, G.val.device
        nb = int(lib.meld_pt_num_blocks(G.n_rows))
        slen = int(lib.meld_pt_stream_len(G.nnz, nb))
        i32 = dict(dtype=torch.int32, device=dev)
        t = dict(
            blk_row=torch.empty(nb + 1, **i32), blk_ntile=torch.empty(nb, **i32), blk_ndist=torch.empty(nb, **i32),
            seg=torch.empty(int(lib.meld_pt_seg_len(nb)), **i32), list_cols=torch.empty(G.nnz, **i32),
            pval=torch.empty(slen, dtype=torch.float64, device=dev), pidx=torch.empty(slen, **i32),
            pval32=torch.empty(slen, dtype=torch.float32, device=dev),  # fp32 values for the lmax estimate's SpMV
            cdesc=torch.empty(int(lib.meld_pt_desc_len(nb)), dtype=torch.int16, device=dev),
        )
        status = torch.zeros(1, **i32)
        lay = PtLayout(*(t[k].data_ptr() for k in ("blk_row", "blk_ntile", "blk_ndist", "seg", "list_cols", "pval", "pidx")), nb,
                       t["pval32"].data_ptr(), slen, t["cdesc"].data_ptr())
        codes = torch.empty(G.nnz, **i32)  # scratch of the builder
        # in-block pairs are stored once (W symmetric); the builder verifies the symmetry of every block's own
        # square and reports status 5 otherwise (a weight matrix uploaded from elsewhere): built again unfolded
        fold = opt("MELD_SPMM_FOLD", "1") != "0"
        for symmetric in ((1, 0) if fold else (0,)):
            with _EventSpan("pt_build", N=G.N, nnz=G.nnz):
                check(lib.meld_pt_build(ptr(G.rowptr), ptr(G.col), ptr(G.val), G.n_rows, G.n_pad, G.row_begin, symmetric,
                                        C.byref(lay), ptr(codes), ptr(status), stream()), "meld_pt_build")
            st = int(status.item())
            if st != 5:
                break
        del codes
        G.info["spmm_fold"] = bool(symmetric) and st == 0
        if st != 0:  # cannot be laid out (see include/meld_hip.h): stay on the CSR-stream kernel
            G.info["spmm"] = "csr (tiled layout refused: status {})".format(st)
            return None
        G.pt = dict(struct=lay, tensors=t, nb=nb)
        G.info["spmm"] = "tiled"
        return G.pt

    def _operator(self, G, decide=True):
        """``G``'s ``meld_laplacian_t`` by reference, as every recurrence entry takes it: built once per graph and kept on it
        beside ``G.pt`` (and again when the layout is); ``layout`` is NULL where ``pt_layout`` keeps the graph on the
        CSR-stream kernel.  The record holds addresses only -- ``G`` keeps the tensors and the ``PtLayout`` alive.
        ``decide=False`` (an entry that reads the CSR arrays whatever the layout) does not have a layout built for its sake."""
        import ctypes as C

        pt = self.pt_layout(G) if decide or getattr(G, "pt", None) is not None else None
        kept = getattr(G, "operator", None)
        if kept is None or kept[0] is not pt:
            from ._lib import Laplacian

            rec = Laplacian(G.rowptr.data_ptr(), G.col.data_ptr(), G.val.data_ptr(), G.dw_dev.data_ptr(), G.n_rows, G.nnz,
                            C.pointer(pt["struct"]) if pt is not None else None)
            G.operator = kept = (pt, rec)
        return C.byref(kept[1])

    def cheby_step(self, G, p, x_full, x_row_off, z, y, r, alpha, beta, gamma, coef, dots=None):
        check(
            self.lib.meld_cheby_step(self._operator(G), p, ptr(x_full), x_row_off, ptr(z), ptr(y), ptr(r), float(alpha), float(beta),
                                     float(gamma), float(coef), ptr(dots), stream()),
            "meld_cheby_step",
        )

    def cheby_step_wide(self, G, p, x_full, x_row_off, z, y, alpha, beta, gamma):
        """One recurrence step on a wide row-major signal [rows, p], 1 <= p <= 64 (``meld_cheby_step_wide``: lanes = columns, the
        matrix streamed once for all columns)."""
        check(
            self.lib.meld_cheby_step_wide(self._operator(G, decide=False), int(p), ptr(x_full), int(x_row_off), ptr(z), ptr(y), float(alpha),
                                          float(beta), float(gamma), stream()),
            "meld_cheby_step_wide",
        )

    # tall-block algebra of the partial Fourier basis (csrc/subspace.hip): fp64 row-major blocks [n_rows, m], m <= 64, the
    # leading dimension taken from the tensor's row stride; per-workgroup partials added in workgroup order (no atomics)
    def block_n_blocks(self, n_rows):
        """Workgroups (= partial slots) of the two reductions for ``n_rows`` rows."""
        return int(min(self.lib.meld_block_max_blocks(), max(1, (int(n_rows) + 63) // 64)))

    def block_gram(self, A, B, n_rows, m, part, n_blocks, C):
        """``C[m, m] = A^T B`` (``meld_block_gram_f64``); ``part``: ``n_blocks * m * m`` doubles."""
        check(self.lib.meld_block_gram_f64(ptr(A), int(A.stride(0)), ptr(B), int(B.stride(0)), int(n_rows), int(m), ptr(part), int(n_blocks),
                                           ptr(C), stream()), "meld_block_gram_f64")

    def block_rotate(self, A, S, n_rows, m, out):
        """``out = A S`` for ``S [m, m]`` on the device (``meld_block_rotate_f64``); ``out`` may be ``A``."""
        check(self.lib.meld_block_rotate_f64(ptr(A), int(A.stride(0)), ptr(S), int(n_rows), int(m), ptr(out), int(out.stride(0)), stream()),
              "meld_block_rotate_f64")

    def block_residuals(self, LV, V, theta, n_rows, m, part, n_blocks, out):
        """``out[j] = sum_i (LV[i, j] - theta[j] V[i, j])^2`` (``meld_block_residuals_f64``); ``part``: ``n_blocks * m`` doubles."""
        assert LV.stride(0) == V.stride(0)
        check(self.lib.meld_block_residuals_f64(ptr(LV), ptr(V), int(V.stride(0)), ptr(theta), int(n_rows), int(m), ptr(part), int(n_blocks),
                                                ptr(out), stream()), "meld_block_residuals_f64")

    @staticmethod
    def _slice_begin(G, comm):
        """First row of this rank's slice of the full-length vectors: rank * rows_pad -- also for a rank beyond the last cell
        (``G.row_begin`` is clipped to N there; it owns no rows but still takes part in every collective)."""
        begin = int(comm.rank) * int(G.rows_pad)
        assert G.n_rows == 0 or begin == G.row_begin, (begin, G.row_begin)
        return begin

    def _cheby_run(self, G, handle, row_begin, p, t_prev2, t_prev1, r, coeffs, alpha2, beta2):
        """``meld_cheby_run``: steps 2 .. len(coeffs) - 1 enqueued from one C call, with the all-gather of every new slice on the
        RCCL communicator ``handle`` (None: a single GPU).  Returns 1 / 0: whether ``t_prev1`` / ``t_prev2`` holds the last T."""
        import ctypes as C

        c = np.ascontiguousarray(coeffs, dtype=np.float64)
        last = C.c_int(1)
        check(
            self.lib.meld_cheby_run(handle, self._operator(G), G.rows_pad, row_begin, p, ptr(t_prev2), ptr(t_prev1), ptr(r),
                                    c.ctypes.data_as(C.c_void_p), int(c.shape[0]), float(alpha2), float(beta2), C.byref(last), stream()),
            "meld_cheby_run",
        )
        return int(last.value)

    def cheby_run(self, G, p, t_prev2, t_prev1, r, coeffs, alpha2, beta2):
        """Steps 2 .. len(coeffs) - 1 of the Chebyshev recurrence on a single GPU in one call (on the tiled layout the
        accumulator is touched every other step; on the CSR-stream kernel the launches are those of stepping from Python).
        Returns False for a graph that is a row shard (the caller steps)."""
        if getattr(G, "comm", None) is not None or G.row_begin != 0:
            return False
        self._cheby_run(G, None, 0, p, t_prev2, t_prev1, r, coeffs, alpha2, beta2)
        return True

    def cheby_run_sharded(self, G, p, t_prev2, t_prev1, r, coeffs, alpha2, beta2):
        """The same on a row shard: the local rows' kernel and the all-gather of the new slice enqueued back to back from C on
        the library's own RCCL communicator.  Returns None when the graph's communicator offers no RCCL handle (gloo,
        host-staged test collectives: the caller steps from Python), else 1 / 0: whether ``t_prev1`` / ``t_prev2`` holds the
        last T."""
        comm = getattr(G, "comm", None)
        handle = comm.rccl() if comm is not None and hasattr(comm, "rccl") else None
        if handle is None:
            return None
        return self._cheby_run(G, handle, self._slice_begin(G, comm), p, t_prev2, t_prev1, r, coeffs, alpha2, beta2)

    def lanczos_steps_sharded(self, G, V, state, acc, alphas, betas, it_begin, n_iter):
        """Iterations of the one-reduction Lanczos recurrence on a row shard in one call (``meld_lanczos_steps_sharded``); False
        when the communicator offers no RCCL handle (the caller runs the phases from Python)."""
        comm = getattr(G, "comm", None)
        handle = comm.rccl() if comm is not None and hasattr(comm, "rccl") else None
        if handle is None:
            return False
        check(
            self.lib.meld_lanczos_steps_sharded(handle, self._operator(G), G.rows_pad, self._slice_begin(G, comm), ptr(V[0]), ptr(V[1]),
                                                ptr(V[2]), ptr(state), ptr(acc), ptr(alphas), ptr(betas), int(it_begin), int(n_iter),
                                                stream()),
            "meld_lanczos_steps_sharded",
        )
        return True

    def lanczos_steps(self, G, V, state, alphas, betas, it_begin, n_iter, scratch, stop=None):
        """Iterations [it_begin, it_begin + n_iter) of the device-resident Lanczos recurrence
        (``meld_lanczos_steps``): V is a [3, N] buffer of rotating vectors.  ``stop`` (int32 device tensor, optional): a launch
        that finds it nonzero does nothing (tiled layout only; the CSR kernels of small graphs run their batch out)."""
        check(
            self.lib.meld_lanczos_steps(self._operator(G), ptr(V[0]), ptr(V[1]), ptr(V[2]), ptr(state), ptr(alphas), ptr(betas),
                                        int(it_begin), int(n_iter), ptr(scratch), ptr(stop), stream()),
            "meld_lanczos_steps",
        )

    # the same iteration as four stream-ordered phases (row-sharded driver; see filter._lanczos_lmax_phases)
    def lanczos_spmv(self, G, x_full, z_local, y_local, state, dots):
        check(self.lib.meld_lanczos_spmv(self._operator(G), ptr(x_full), G.row_begin, ptr(z_local), ptr(y_local), ptr(state), ptr(dots),
                                         stream()), "meld_lanczos_spmv")

    def lanczos_alpha(self, state, dots, nrm2, alphas, it):
        check(self.lib.meld_lanczos_alpha(ptr(state), ptr(dots), ptr(nrm2), ptr(alphas), int(it), stream()), "meld_lanczos_alpha")

    def lanczos_axpy(self, x_local, y_local, state, nrm2):
        check(self.lib.meld_lanczos_axpy(ptr(x_local), ptr(y_local), int(x_local.shape[0]), ptr(state), ptr(nrm2), stream()), "meld_lanczos_axpy")

    def lanczos_beta(self, state, nrm2, dots, betas, it):
        check(self.lib.meld_lanczos_beta(ptr(state), ptr(nrm2), ptr(dots), ptr(betas), int(it), stream()), "meld_lanczos_beta")

    # one-reduction form of the sharded iteration (filter._lanczos_lmax_folded)
    def lanczos_fold(self, state, acc, alphas, betas, it):
        check(self.lib.meld_lanczos_fold(ptr(state), ptr(acc), ptr(alphas), ptr(betas), int(it), stream()), "meld_lanczos_fold")

    def lanczos_axpy3(self, y_local, u_local, u_prev_local, state, nrm2):
        check(self.lib.meld_lanczos_axpy3(ptr(y_local), ptr(u_local), ptr(u_prev_local), int(y_local.shape[0]), ptr(state), ptr(nrm2),
                                          stream()), "meld_lanczos_axpy3")

    def scale(self, x, a, r):
        check(self.lib.meld_scale_f64(ptr(x), float(a), ptr(r), x.numel(), stream()), "meld_scale_f64")

    def axpby(self, a, x, b, y, nrm2=None):
        check(self.lib.meld_axpby_f64(float(a), ptr(x), float(b), ptr(y), y.numel(), ptr(nrm2), stream()), "meld_axpby_f64")


def metric_front_end(X, distance, decay):
    """The graph builders are euclidean; other metrics come in through the data.  ``distance="cosine"`` ([UPSTREAM graphtools
    ``kNNGraph(distance=...)`` -> sklearn ``NearestNeighbors(metric="cosine")``]: d(x, y) = 1 - x.y / (|x| |y|)): on unit rows
    d_cos = |x^ - y^|^2 / 2, so the neighbours are those of the euclidean search on the normalised rows, and since the kernel sees
    distances only as the ratio d / bandwidth, d_cos / bw_cos = (d_euc / bw_euc)^2:  exp(-(d_cos / bw_cos)^decay) =
    exp(-(d_euc / bw_euc)^(2 decay)) -- the euclidean graph of the normalised rows with the decay doubled, entry for entry (the
    oracle, which hands the metric to sklearn, agrees to 1e-14: tests/test_oracle.py).  Returns (X', decay', to_metric) where
    to_metric maps a euclidean bandwidth of X' to the metric's own units.
    The same argument covers "sqeuclidean" (d = d_euc^2: the decay doubled, the rows as they are) and "correlation" (the cosine
    distance of the rows with their own means removed); "l2" is euclidean."""
    if distance in ("euclidean", "l2"):
        return X, decay, None
    decay2 = None if decay is None else 2 * decay
    if distance == "sqeuclidean":
        return X, decay2, (lambda bw: bw * bw)
    if distance not in ("cosine", "correlation"):
        raise NotImplementedError(
            "distance {!r} is not implemented by the MI355X graph builder (euclidean, l2, sqeuclidean, cosine, correlation)".format(distance))
    if distance == "correlation":
        X = X - X.mean(dim=1, keepdim=True)
    nrm = torch.linalg.vector_norm(X, dim=1, keepdim=True)
    if bool((nrm == 0).any()):
        raise ValueError("{} distance is undefined for {} rows".format(distance, "all-zero" if distance == "cosine" else "constant"))
    return (X / nrm).contiguous(), decay2, (lambda bw: 0.5 * bw * bw)


def _exact_bandwidth(X, rows, knn, n_refs=None):
    """Distance to the (knn+1)-th nearest cell (self included) of the given rows over ALL references (the first
    ``n_refs`` rows of X, by default all of them), exactly:
    an fp64 GEMM-form screen keeps the 4 (knn + 1) nearest, their distances are recomputed by direct differences.
    Library path for the handful of rows the exact sweep finds with an incomplete candidate list."""
    Xr = X if n_refs is None else X[: int(n_refs)]
    n2 = (Xr * Xr).sum(1)
    out = torch.empty(rows.shape[0], dtype=torch.float64, device=X.device)
    kk = min(int(Xr.shape[0]), 4 * (knn + 1))
    for lo in range(0, rows.shape[0], 256):
        r = rows[lo : lo + 256]
        Xq = X[r]
        d2 = (Xq * Xq).sum(1)[:, None] + n2[None, :] - 2.0 * (Xq @ Xr.T)
        cand = torch.topk(d2, kk, dim=1, largest=False).indices.contiguous()
        # the candidates' distances in the SWEEP's arithmetic (meld_knn_pair_distances: the summation order of csrc/refine.hip): the sweep counts
        # the references strictly closer than the bandwidth with its own summation order, and confirms a bandwidth ranked from
        # these by construction.  (A library norm, two ulps down, was flagged again at d = 52: "could not settle".)
        dist = torch.empty(cand.shape, dtype=torch.float64, device=X.device)
        r64 = r.to(torch.int64).contiguous()
        check(get_lib().meld_knn_pair_distances(ptr(X), int(X.shape[1]), ptr(r64), ptr(cand), int(r64.shape[0]), kk, ptr(dist), stream()),
              "meld_knn_pair_distances")
        out[lo : lo + 256] = torch.sort(dist, dim=1).values[:, min(knn, kk - 1)]
    return out.clamp_(min=float(np.finfo(np.float64).eps))


def resolve_graph_params(N, knn, thresh, ksel):
    """Parameter clipping shared by every builder ([UPSTREAM graphtools kNNGraph.__init__])."""
    if N < 3:
        raise ValueError("need at least 3 points to build a kNN graph, got {}".format(N))
    if knn > N - 2:  # graphtools clips (with a warning)
        knn = N - 2
    thresh = float(max(thresh, np.finfo(float).eps))  # graphtools' thresh floor
    if ksel is None:
        ksel = default_ksel(knn)
    if ksel < knn + 2:
        raise NotImplementedError(
            "knn={} needs a candidate list of at least knn+2 entries but the search kernel holds at most 128".format(knn)
        )
    return int(knn), thresh, int(ksel)


def symm_code(kernel_symm, theta):
    """(mode, theta) of ``meld_csr_rows_sort_merge`` for graphtools' ``kernel_symm`` / ``theta``
    [UPSTREAM ``BaseGraph._check_symmetrization``: "+" | "*" | "mnn" | None; theta in [0, 1], 1 when not given]."""
    if kernel_symm == "+":
        return (0, 0.0)
    if kernel_symm == "*":
        return (1, 0.0)
    if kernel_symm == "mnn":
        if theta is None:
            theta = 1.0
        if not isinstance(theta, (int, float)) or theta < 0 or theta > 1:
            raise ValueError("theta {} not recognized. Expected a float between 0 and 1".format(theta))
        return (2, float(theta))
    if kernel_symm is None:
        raise NotImplementedError("kernel_symm=None (a directed kernel) is not implemented: the filter needs a symmetric Laplacian")
    raise ValueError("kernel_symm '{}' not recognized. Choose from '+', '*', 'mnn', or 'none'.".format(kernel_symm))


def build_knn_graph(X, knn=5, decay=40, thresh=1e-4, anisotropy=1, ksel=None, profile=False, force_fallback=False,
                    reorder=True, bandwidth=None, bandwidth_scale=1.0, col_stats=None, knn_max=None, kernel_symm="+", theta=None, ops=None):
    """Data [N, d] -> DeviceGraph on one GPU.  Rows A2-A5 of SURVEY.md section 8(a).

    ``X`` is a CUDA fp64 tensor [N, d] (row-major).  Stages: centre + fp32 operands, MFMA
    distance GEMM with fused top-ksel, exact fp64 refinement + alpha-decay kernel, exact sweep for
    rows whose candidate list is provably incomplete, COO emit + radix sort + merge = (K + K^T)/2,
    anisotropy, degrees.
    """
    if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float64 and X.dim() == 2):
        raise TypeError("build_knn_graph expects a CUDA float64 tensor [N, d]")
    X = X.contiguous()
    N, d = int(X.shape[0]), int(X.shape[1])
    ops = ops if ops is not None else HipOps(X.device)
    tm = _Timer(profile)
    knn, thresh, ksel = resolve_graph_params(N, knn, thresh, ksel)
    # [UPSTREAM graphtools kNNGraph(bandwidth=, bandwidth_scale=)]: a given bandwidth (one number or one per cell) replaces the
    # distance to the knn-th neighbour; either way it is multiplied by bandwidth_scale and floored at eps
    bw_scale = float(bandwidth_scale)
    if not (bw_scale > 0 and math.isfinite(bw_scale)):
        raise ValueError("bandwidth_scale must be positive and finite, got {!r}".format(bandwidth_scale))
    symm = symm_code(kernel_symm, theta)
    if knn_max is not None:
        knn_max = int(knn_max)
        if knn_max < knn:  # [UPSTREAM kNNGraph.__init__]
            raise ValueError("`knn_max` must be greater than or equal to `knn`")
        if knn_max + 2 > ksel:  # (the candidate list has to hold them)
            ksel = min(128, ((knn_max + 2 + 31) // 32) * 32)
            if knn_max + 2 > ksel:
                raise NotImplementedError("knn_max={} needs a candidate list beyond the 128 entries the search kernel holds".format(knn_max))
    bw_fixed = None
    if bandwidth is not None:
        if callable(bandwidth):
            raise NotImplementedError("a callable bandwidth is not implemented by the MI355X graph builder")
        b = torch.as_tensor(np.asarray(bandwidth, dtype=np.float64)).to(X.device)
        if b.dim() == 0:
            b = b.expand(N)
        if tuple(b.shape) != (N,):
            raise ValueError("bandwidth must be a number or have one entry per cell ({}), got shape {}".format(N, tuple(b.shape)))
        if not bool(torch.isfinite(b).all()) or bool((b < 0).any()):
            raise ValueError("bandwidth must be finite and non-negative")
        bw_fixed = b.contiguous().clone()

    # (the frame of the search does not depend on the order of the cells: its scatter matrix and read-back go out in front of
    # the ordering, the host decomposes it while the GPU orders: frame_axes_async)
    frame_axes = ops.frame_axes_async(X, col_stats) if (bw_fixed is None and hasattr(ops, "frame_axes_async")) else None
    perm = None
    if reorder:
        from .reorder import locality_permutation

        tm.start()
        perm = locality_permutation(X)
        if perm is not None:
            X = ops.gather_rows(X, perm)
            if bw_fixed is not None:
                bw_fixed = bw_fixed.index_select(0, perm).contiguous()
        tm.stop("reorder")

    # [UPSTREAM graphtools build_kernel_to_data] caps a row at knn_max + 1 cells only where its re-search ends at
    # ``search_knn == knn_max``; the search sizes go (knn + 1) x 6, x 36, then knn_max + 1 (x 216 always exceeds the 127 this builder
    # accepts), and a row that leaves the re-search earlier holds everything inside its radius anyway.  So the result IS the hard cap
    # -- except where 36 (knn + 1) < knn_max + 1 (knn <= 2 here) and the loop never runs because no more than N // 10 rows have
    # 6 (knn + 1) cells inside their radius (or 36 (knn + 1) >= N / 2): upstream then finishes those rows with an UNCAPPED radius
    # search, and the graph is the one without knn_max.  That is decided by a count over the uncapped rows, so this corner builds
    # the uncapped kernel first.
    k1 = knn + 1
    info = None
    if knn_max is not None and decay is not None and math.isfinite(decay) and 36 * k1 < min(knn_max + 1, N):
        trial = ops.directed_kernel_coo(X, 0, N, knn, decay, thresh, ksel, tm=tm, force_fallback=force_fallback, assemble=True,
                                        bw_scale=bw_scale, bw_fixed=bw_fixed, col_stats=col_stats, knn_max=None, symm=symm, count_rows_ge=6 * k1,
                                        frame_axes=frame_axes, anisotropy=anisotropy)
        if trial[3]["rows_with_at_least"] <= N // 10 or 36 * k1 >= N / 2:
            keys, vals, bw, info = trial
            info["knn_max_uncapped_as_upstream"] = True
            knn_max = None
        del trial
    if info is None:
        keys, vals, bw, info = ops.directed_kernel_coo(X, 0, N, knn, decay, thresh, ksel, tm=tm, force_fallback=force_fallback, assemble=True,
                                                       bw_scale=bw_scale, bw_fixed=bw_fixed, col_stats=col_stats, knn_max=knn_max, symm=symm,
                                                       frame_axes=frame_axes, anisotropy=anisotropy)
    if bw_scale != 1.0:  # (the stages record the unscaled bandwidth; the graph reports the one the kernel used)
        bw = (bw * bw_scale).clamp_(min=float(np.finfo(float).eps))
    if info.get("nnz_directed", 0) == 0:
        raise ValueError("the kernel has no off-diagonal entries; cannot build a graph")
    tm.start()
    ksum = dw = None
    if info.get("assembled") is not None:  # (the kept candidates went straight into the row buckets)
        asm = info.pop("assembled")
        rowptr, col, val = asm[:3]
        ksum = asm[3] if len(asm) > 3 else None  # (the row sums came out of the buckets with the rows)
        dw = asm[4] if len(asm) > 4 else None  # (... and the anisotropy was applied, the degrees summed, on the way out)
    else:
        rowptr, col, val = ops.assemble_rows(keys, vals, 0, N, N, symm=symm)
    del keys, vals
    tm.stop("symmetrize")
    if ksum is None:
        ksum = ops.row_sums(rowptr, val, N, 1.0)
    if dw is None:
        dw = ops.anisotropy_degrees(rowptr, col, val, N, ksum, 0, anisotropy)
    tm.stop("anisotropy_degree")

    nnz = int(col.shape[0])
    info.update(N=N, d=d, knn=knn, nnz=nnz, mean_degree=nnz / N, stage_seconds=dict(tm.t), assemble=getattr(ops, "last_assemble", None))
    G = DeviceGraph(rowptr, col, val, dw, ksum=ksum, anisotropy=anisotropy, info=info)
    G.bandwidth = bw
    G.perm = perm
    G.ops = ops
    return G
