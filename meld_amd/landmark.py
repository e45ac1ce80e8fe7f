"""Landmarks of a fitted graph: graphtools' ``LandmarkGraph`` operator, transitions and interpolation, on the device.

The reference forwards ``n_landmark`` to graphtools (``meld/meld.py:105,118``), where it yields a ``LandmarkGraph``: the cells are
coarse-grained into a few thousand landmarks, dense ``[L, L]`` algebra on ``landmark_op`` stands in for ``[N, N]`` (PHATE's diffusion
potential, any dense spectral method), and ``interpolate`` carries the result back to cells.  This module restates [UPSTREAM
graphtools 1.5.x ``LandmarkGraph.build_landmark_op`` / ``_landmarks_to_data`` / ``extend_to_data``, unpinned: it cannot be imported
next to this code].  With ``K = W + diag(kd)`` the symmetric kernel (``G.K``), ``c[i]`` in ``[0, L)`` the landmark of cell ``i`` and
``C`` the ``[N, L]`` one-hot of ``c``::

    A           = K C                            A[j, l] = sum_{i: c[i] = l} K[j, i]        (upstream's pmn.T before normalisation)
    transitions = pnm = diag(1 / r) A            r = A 1, the row sums of K
    pmn         = diag(1 / s) A^T                s = A^T 1
    landmark_op = pmn @ pnm                      dense [L, L], row-stochastic, non-negative
    extend_to_data(Y)  = normalize(build_kernel_to_data(Y) C, "l1")                         [M, L]
    interpolate(T, Y)  = extend_to_data(Y) @ T;  interpolate(T) = transitions @ T           T [L, p]

``csrc/landmark.hip`` merges the rows of a CSR matrix by the label of their columns (``meld_landmark_merge_count`` /
``meld_landmark_merge_fill``) and builds the operator from ``A`` and its transpose (``meld_landmark_gram``); the transpose comes from
the existing transpose-keys, sort and csr-from-keys entries (``sparse.DeviceCSR.T``), the products with ``T`` from
``meld_extend_apply``.

Upstream's clusters come from a randomized SVD and ``MiniBatchKMeans``, whose random numbers cannot be reproduced: the default
clustering here (``default_clusters``) follows the same recipe with a seeded range finder and the seeded k-means of ``cluster.py``,
and labels can be passed in (``clusters=``) -- the operator is a function of the labels.

``check_n_landmark``, ``compact_labels`` and ``check_clusters`` are pure helpers (no device).
"""
from __future__ import annotations

import hashlib
import numbers

import numpy as np

from ._graph_steps import require_unsharded

__all__ = ["LANDMARK_MAX", "Landmarks", "check_n_landmark", "compact_labels", "check_clusters", "merge_by_label", "spectral_features",
           "default_clusters", "check_kmeans", "landmarks"]

LANDMARK_MAX = 4096  # ``meld_landmark_max()``: the Gram's LDS accumulator (tests/test_landmark_host.py holds the two together)
OVERSAMPLE = 10  # columns of the range finder beyond n_svd
POWER_ITERATIONS = 4  # power iterations of the range finder that always run (each a product with diff_aff; one more follows)
MAX_PASSES = 32  # products with diff_aff at most
RANGE_TOL = 3e-3  # residual |diff_aff v - theta v| / max |theta| of the leading Ritz pairs at which the passes end
KMEANS_MAX_ITER = 100


def check_n_landmark(n_landmark, N):
    """``n_landmark`` as an int in ``[1, min(N - 1, LANDMARK_MAX)]``; ValueError otherwise (graphtools refuses ``n_landmark >= N``
    too)."""
    if isinstance(n_landmark, (bool, np.bool_)) or not isinstance(n_landmark, (numbers.Integral, np.integer)):
        raise ValueError("n_landmark must be a positive integer, got {!r}".format(n_landmark))
    n_landmark = int(n_landmark)
    if n_landmark < 1:
        raise ValueError("n_landmark must be a positive integer, got {}".format(n_landmark))
    if n_landmark >= int(N):
        raise ValueError("n_landmark ({}) must be less than the number of cells ({})".format(n_landmark, int(N)))
    if n_landmark > LANDMARK_MAX:
        raise ValueError("n_landmark={} is above the {} landmarks the device operator is built for".format(n_landmark, LANDMARK_MAX))
    return n_landmark


def compact_labels(labels):
    """``(compact int32 [N], values)``: landmark ``l`` is the ``l``-th smallest label present (``np.unique`` semantics)."""
    values, inverse = np.unique(np.asarray(labels), return_inverse=True)
    return inverse.reshape(-1).astype(np.int32), values


def check_clusters(clusters, N):
    """``clusters`` -- one integer per cell in the caller's order, host or device -- as compact host int32 labels and their
    number.  TypeError for a dtype that is not integer, ValueError for a wrong length, more than one dimension, negative values,
    fewer than one cell and more distinct labels than ``LANDMARK_MAX``."""
    if hasattr(clusters, "detach") and hasattr(clusters, "cpu"):  # (a torch tensor, host or device)
        clusters = clusters.detach().cpu().numpy()
    c = np.asarray(getattr(clusters, "values", clusters))
    if c.dtype == np.bool_ or c.dtype.kind not in "iu":
        raise TypeError("clusters must be integers, got dtype {}".format(c.dtype))
    if c.ndim != 1:
        raise ValueError("clusters must be one-dimensional, got shape {}".format(c.shape))
    if c.shape[0] != int(N):
        raise ValueError("clusters must have one entry per cell ({}), got {}".format(int(N), c.shape[0]))
    if c.size and int(c.min()) < 0:
        raise ValueError("clusters must not be negative, got {}".format(int(c.min())))
    compact, values = compact_labels(c)
    if values.shape[0] > LANDMARK_MAX:
        raise ValueError("clusters hold {} distinct labels, above the {} landmarks the device operator is built for".format(
            values.shape[0], LANDMARK_MAX))
    return compact, int(values.shape[0])


# -- device side ---------------------------------------------------------------------------------------------------------------
def merge_by_label(rowptr, col, val, n_cols, label, n_landmark, kd=None, colmap=None):
    """``(rowptr, col, val, rowsum)`` of the CSR ``[n_rows, n_landmark]`` whose row ``i`` is row ``i`` of the input with its entries
    merged by ``label`` of their column -- every present label once, ascending; values added in storage order, the diagonal
    ``kd[i]`` (square matrices) last; ``rowsum`` the raw sums.  ``label``: int32 device ``[n_cols]`` in ``[0, n_landmark)``;
    ``colmap``: int64 device ``[n_cols]`` or None, ``label[colmap[c]]`` is the label of column ``c``."""
    import torch

    from ._device_ops import scan_i32, stream
    from ._lib import check, get_lib, ptr

    lib, dev = get_lib(), rowptr.device
    n_rows, nnz = int(rowptr.shape[0]) - 1, int(col.shape[0])
    counts = torch.empty(max(n_rows, 1), dtype=torch.int32, device=dev)
    marked = torch.empty(max(nnz + (n_rows if kd is not None else 0), 1), dtype=torch.int32, device=dev)
    if nnz == 0:  # (any address serves, none is read)
        col, val = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    st = stream()
    check(lib.meld_landmark_merge_count(ptr(rowptr), ptr(col), n_rows, int(n_cols), ptr(label), int(n_landmark), ptr(colmap),
                                        0 if kd is None else 1, ptr(marked), ptr(counts), st), "meld_landmark_merge_count")
    out_rowptr = scan_i32(counts[:n_rows])
    n_out = int(out_rowptr[-1])  # (the one word the host reads)
    out_col = torch.empty(max(n_out, 1), dtype=torch.int32, device=dev)
    out_val = torch.empty(max(n_out, 1), dtype=torch.float64, device=dev)
    rowsum = torch.empty(n_rows, dtype=torch.float64, device=dev)
    check(lib.meld_landmark_merge_fill(ptr(rowptr), ptr(val), ptr(kd), n_rows, ptr(marked), ptr(out_rowptr), ptr(out_col), ptr(out_val),
                                       ptr(rowsum), st), "meld_landmark_merge_fill")
    return out_rowptr, out_col[:n_out], out_val[:n_out], rowsum


def _gram(A, N, L):
    """``(landmark_op [L, L], s [L])`` from the merged CSR ``A = (rowptr, col, val, rowsum)`` of ``N`` cells."""
    import torch

    from ._device_ops import stream
    from ._lib import check, get_lib, ptr
    from .sparse import DeviceCSR

    rowptr, col, val, rowsum = A
    dev = rowptr.device
    T = DeviceCSR(rowptr, col, val, (N, L)).T  # (transpose keys, radix sort, CSR assembly: cells ascending inside a landmark)
    op = torch.empty(L, L, dtype=torch.float64, device=dev)
    s = torch.empty(L, dtype=torch.float64, device=dev)
    one_i = torch.zeros(1, dtype=torch.int32, device=dev)
    one_d = torch.zeros(1, dtype=torch.float64, device=dev)
    has = int(col.shape[0]) > 0
    check(get_lib().meld_landmark_gram(ptr(rowptr), ptr(col if has else one_i), ptr(val if has else one_d), N, ptr(T.rowptr),
                                       ptr(T.col if has else one_i), ptr(T.val if has else one_d), L, ptr(rowsum), ptr(op), ptr(s),
                                       stream()), "meld_landmark_gram")
    return op, s


def _orthonormal(Z):
    """An orthonormal basis of the columns of tall ``Z``: the tall Gram and a small ``eigh`` (directions below 1e-12 of the largest
    are dropped)."""
    import torch

    from ._device_ops import tall_gram

    w, U = torch.linalg.eigh(tall_gram(Z, Z))
    keep = w > 1e-12 * w[-1].clamp(min=1e-300)
    return Z @ (U[:, keep] / torch.sqrt(w[keep])[None, :])


def spectral_features(G, n_landmark, n_svd=100, random_state=None, info=None):
    """The features the default clustering runs k-means on, an fp64 device tensor ``[N, min(n_svd, n_landmark, N - 1)]`` in the
    graph's device order: ``diff_op @ V``, ``V`` the leading singular vectors of ``diff_aff = D^-1/2 K D^-1/2`` (see
    ``default_clusters``)."""
    import torch

    from ._device_ops import tall_gram
    from .diffuse import diffuse_device, walk_vectors

    N, dev = G.N, G.val.device
    seed = 0 if random_state is None else int(random_state)
    n_svd = int(max(1, min(int(n_svd), N - 1, int(n_landmark))))
    width = int(min(n_svd + OVERSAMPLE, N))
    _, s = walk_vectors(G)
    root = torch.sqrt(s)[:, None]

    def diff_aff(X):
        return root * diffuse_device(G, X / root, t=1, device_order=True)

    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    Q = _orthonormal(torch.randn(N, width, dtype=torch.float64, device=dev, generator=gen))
    for passes in range(1, MAX_PASSES + 1):
        Z = diff_aff(Q)
        # Rayleigh-Ritz on the current basis: the residuals of the leading n_svd Ritz pairs say when the range is found
        T = tall_gram(Q, Z)
        theta, Y = torch.linalg.eigh(0.5 * (T + T.T))
        lead = torch.argsort(theta.abs(), descending=True)[:n_svd]
        R = Z @ Y[:, lead] - (Q @ Y[:, lead]) * theta[lead][None, :]
        residual = float(torch.linalg.vector_norm(R, dim=0).max() / theta.abs().max().clamp(min=1e-300))  # (the pass's one read-back)
        if (passes > POWER_ITERATIONS and residual <= RANGE_TOL) or passes == MAX_PASSES:
            break
        Q = _orthonormal(Z)
    w, U = torch.linalg.eigh(tall_gram(Z, Z))
    order = torch.argsort(w, descending=True)[:n_svd]
    order = order[w[order] > 1e-24 * w.max().clamp(min=1e-300)]
    V = Z @ (U[:, order] / torch.sqrt(w[order])[None, :])
    if info is not None:
        info.update(n_svd=int(order.shape[0]), range_finder_columns=width, range_finder_passes=passes, range_finder_residual=residual,
                    random_state=seed)
    return diffuse_device(G, V.contiguous(), t=1, device_order=True)


def default_clusters(G, n_landmark, n_svd=100, random_state=None, info=None, kmeans="library"):
    """Labels of the default clustering, an int64 device tensor ``[N]`` in the caller's order (not compacted): graphtools' recipe
    -- k-means on ``diff_op @ V``, ``V`` the leading ``n_svd`` singular vectors of ``diff_aff = D^-1/2 K D^-1/2`` -- from existing
    kernels and library calls: ``diff_aff x = sqrt(r) * diffuse_step(x / sqrt(r))``; a seeded Gaussian ``[N, n_svd + 10]``, power
    iterations orthonormalised in between (tall Gram + small ``eigh``); ``Z = diff_aff Q``, ``Z^T Z = U S^2 U^T``, ``V = Z U S^-1``;
    ``kmeans.kmeans_device(diff_op V, n_landmark, n_init=1)``.  The seed is ``random_state`` (None: 0).

    The power iterations run until the leading ``n_svd`` Ritz pairs of the basis have residuals below ``RANGE_TOL`` (4 iterations
    at least, ``MAX_PASSES`` products with ``diff_aff`` at most; one small ``eigh`` and one word read back per pass): a fixed 4 is
    not enough where the spectrum of ``diff_aff`` decays slowly.  Measured on four disconnected blobs of 200 cells (eigenvalues 1, 1,
    1, 1, 0.903, 0.902, ...): after 4 passes the cosines of the principal angles between the features and those of the exact vectors
    are 0.67 - 0.85 and k-means mixes the blobs; after 8, 0.91 - 0.96, still mixed; after 16, above 0.99, and the blobs are recovered.

    ``n_svd`` is clipped to ``N - 1`` and to ``n_landmark``: k-means into k clusters has no use for more than k spectral
    directions, and the surplus hides them -- on four disconnected blobs of 200 cells the 96 further columns of ``n_svd = 100``
    carry 20 times the variance of the four that tell the blobs apart (within-blob inertia 60.96 of 63.96 in total: the blobs
    are the best partition by 1.5 %, and neither this k-means nor sklearn's finds it from a k-means++ start), while on four
    columns every start does.  Upstream's default (2,000 landmarks, 100 vectors) is not touched by the clip.

    ``kmeans="library"`` seeds with k-means++ and prefers the LDS Lloyd step (``csrc/kmeans.hip``; the library step beyond what it
    stages); ``"device"`` clusters the same features with k-means|| seeding and the Lloyd step of ``csrc/kmeans_wide.hip`` under the
    same seed and iteration cap."""
    import torch

    from .kmeans import kmeans_device

    features = spectral_features(G, n_landmark, n_svd=n_svd, random_state=random_state, info=info)
    km = {}
    seed = 0 if random_state is None else int(random_state)
    route = dict(seeding="k-means||", prefer="wide") if kmeans == "device" else dict(seeding="k-means++", prefer="lds")
    lab = kmeans_device(features, int(n_landmark), n_init=1, max_iter=KMEANS_MAX_ITER, seed=seed, info=km, **route)["labels"].to(torch.int64)
    if G.perm is not None:  # (device row v is the caller's cell perm[v])
        out = torch.empty_like(lab)
        out[G.perm] = lab
        lab = out
    if info is not None:
        info.update(kmeans_iterations=km.get("iterations"))
        if kmeans == "device":
            info.update(kmeans="device")
    return lab


class Landmarks:
    """The landmark record of a graph for one set of labels (``DeviceGraph.landmarks``).

    ``n_landmark``; ``clusters`` (host int32 ``[N]``, caller's order, compact) and ``clusters_device``; ``landmark_op_device``
    (fp64 ``[L, L]``) and ``landmark_op`` (its host copy); ``landmark_sums`` (``s``, device ``[L]``); ``transitions_device`` =
    ``(rowptr, col, val, rowsum)``: the merged matrix ``A = K C`` with raw sums, rows in the graph's device order (the convention of
    ``kernel_to_data_device``: divide by ``rowsum`` for the transitions); ``transitions``: scipy CSR ``[N, L]``, rows in the caller's
    order and l1-normalised (a host export, like ``K``); ``info``: ``n_svd``, k-means iterations, entries of ``A`` and the like."""

    def __init__(self, G, clusters, n_landmark, transitions_device, landmark_op_device, landmark_sums, info):
        import torch

        self._graph = G
        self.clusters = clusters
        self.clusters_device = torch.from_numpy(clusters).to(G.val.device)
        self.n_landmark = int(n_landmark)
        self.transitions_device = transitions_device
        self.landmark_op_device = landmark_op_device
        self.landmark_sums = landmark_sums
        self.info = info
        self._landmark_op = None
        self._transitions = None

    @property
    def landmark_op(self):
        if self._landmark_op is None:
            self._landmark_op = self.landmark_op_device.cpu().numpy()
        return self._landmark_op

    @property
    def transitions(self):
        if self._transitions is None:
            from .extend import to_scipy

            T = to_scipy(self.transitions_device, self.n_landmark, normalise=True)
            inv = self._graph._inv_perm_host()
            self._transitions = T if inv is None else T[inv].tocsr()
        return self._transitions

    # -- new cells ----------------------------------------------------------------------------------------------------------------
    def extend_to_data_device(self, Y):
        """``(rowptr, col, val, rowsum)``: the kernel rows of the new cells ``Y`` merged by landmark, CSR ``[M, L]`` with raw sums
        (``kernel_to_data_device`` through the merge kernel).  NotImplementedError, naming the case, for a graph that cannot be
        extended to new cells."""
        G = self._graph
        rowptr, col, val, _ = G.kernel_to_data_device(Y)  # (refuses what extend.refusal names; columns in the caller's order)
        return merge_by_label(rowptr, col, val, G.N, self.clusters_device, self.n_landmark)

    def extend_to_data(self, Y):
        """[UPSTREAM graphtools ``LandmarkGraph.extend_to_data``]: the transitions ``[M, L]`` from new cells to landmarks, scipy
        CSR (a host export)."""
        from .extend import to_scipy

        return to_scipy(self.extend_to_data_device(Y), self.n_landmark, normalise=True)

    def interpolate_device(self, T, Y=None, device_order=False):
        """``extend_to_data(Y) @ T`` (``[M, p]``) or, without ``Y``, ``transitions @ T`` (``[N, p]``, rows in the caller's order
        unless ``device_order``) for ``T [L, p]`` (device tensor, host array or DataFrame; ``[L]`` gives a vector): an fp64 device
        tensor.  The product is ``meld_extend_apply``: the normalised transitions are never written."""
        import torch

        from . import filter as _filter
        from .extend import _to_device, apply_transitions

        G = self._graph
        F = _to_device(T, G.val.device)
        flat = F.dim() == 1
        if flat:
            F = F[:, None]
        if F.dim() != 2 or int(F.shape[0]) != self.n_landmark:
            raise ValueError("transform must have one row per landmark ({}), got shape {}".format(self.n_landmark, tuple(F.shape)))
        if Y is None:
            out = apply_transitions(self.transitions_device, F)
            if G.perm is not None and not device_order and int(out.shape[1]):
                out = _filter._to_caller_order(out, G)
        else:
            out = apply_transitions(self.extend_to_data_device(Y), F)
        return out[:, 0] if flat else out

    def interpolate(self, T, Y=None):
        """``interpolate_device`` as a host ndarray."""
        return self.interpolate_device(T, Y=Y).cpu().numpy()


def _build(G, compact, L, info):
    import torch

    from .diffuse import walk_vectors

    dev = G.val.device
    label = torch.from_numpy(np.ascontiguousarray(compact, dtype=np.int32)).to(dev)
    kd, _ = walk_vectors(G)  # (ValueError where a cell has no positive kernel row sum)
    rowptr = G.rowptr[: G.N + 1]
    A = merge_by_label(rowptr, G.col, G.val, G.N, label, L, kd=kd, colmap=G.perm)
    op, s = _gram(A, G.N, L)
    info = dict(info, entries=int(A[1].shape[0]), n_landmark=L)
    return Landmarks(G, compact, L, A, op, s, info)


def check_kmeans(kmeans):
    """``kmeans`` as one of the two routes of ``kmeans.kmeans_device``, ``"library"`` (k-means++, the LDS or library step) and
    ``"device"`` (k-means||, the wide step); ValueError otherwise."""
    if not isinstance(kmeans, str) or kmeans not in ("library", "device"):
        raise ValueError("kmeans must be 'library' or 'device', got {!r}".format(kmeans))
    return kmeans


def landmarks(G, n_landmark=None, clusters=None, n_svd=100, random_state=None, recompute=False, kmeans="library"):
    """``DeviceGraph.landmarks``: the ``Landmarks`` record for the given labels, or for the default clustering into ``n_landmark``
    (default: the ``n_landmark`` the graph was fitted with); kept on the graph per argument set.  ``kmeans``: which k-means the
    default clustering runs, ``"library"`` (the default) or ``"device"``; part of the argument set."""
    check_kmeans(kmeans)
    if n_landmark is None and clusters is None:
        n_landmark = getattr(G, "n_landmark", None)
        if n_landmark is None:
            raise ValueError("neither n_landmark nor clusters given, and the graph was fitted without n_landmark")
    require_unsharded(G, "landmarks are")
    if clusters is not None:
        compact, L = check_clusters(clusters, G.N)
        key = ("clusters", hashlib.sha1(compact.tobytes()).hexdigest())
        info = dict(clustering="given")
    else:
        n_landmark = check_n_landmark(n_landmark, G.N)
        if isinstance(n_svd, (bool, np.bool_)) or not isinstance(n_svd, (numbers.Integral, np.integer)) or int(n_svd) < 1:
            raise ValueError("n_svd must be a positive integer, got {!r}".format(n_svd))
        key = ("default", n_landmark, int(n_svd), None if random_state is None else int(random_state))
        if kmeans != "library":  # (the default route keeps the key it always had)
            key = key + (kmeans,)
    cache = G.__dict__.setdefault("_landmarks", {})
    if recompute:
        cache.pop(key, None)
    if key not in cache:
        if clusters is None:
            info = dict(clustering="default")
            lab = default_clusters(G, n_landmark, n_svd=n_svd, random_state=random_state, info=info, kmeans=kmeans)
            compact, values = compact_labels(lab.cpu().numpy())
            L = int(values.shape[0])
        cache[key] = _build(G, compact, L, info)
    return cache[key]
