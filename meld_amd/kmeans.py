"""k-means on the device, all of it: ``meld_amd.KMeans``, the clustering of ``VertexFrequencyCluster.predict`` and both ``kmeans=``
routes of ``landmarks()`` are ``kmeans_device`` with a seeder and a preferred Lloyd step.

The reference compares MELD against k-means on the cells (``comparison/comparison.py::run_geometry_clustering`` calls [UPSTREAM
``sklearn.cluster.KMeans(n_clusters).fit_predict``]), and graphtools' landmark clustering is a k-means into thousands of clusters.

* ``assign``: nearest centre and squared distance of every point (``meld_kmeans_wide_assign``, any ``k`` in chunks of 4096 centres);
* ``segment_sums``: the sums of every cluster's rows in an order that is a function of the labels alone (a stable ``torch.sort`` of the
  labels, ``bincount`` / ``cumsum`` -- library calls, as ``louvain.py`` does for its contraction -- and ``meld_kmeans_wide_sums``);
* three Lloyd steps ``(Y, C) -> (new centres, inertia, labels int32)``, device tensors, no sync; new centres are ``sums / count``,
  an empty cluster keeps its centre (``_new_centres``).  ``lloyd_step`` ("wide"): ``assign`` + ``segment_sums``, the same bits on
  every run.  ``lds_step(Y, k)`` ("lds") makes the step of ``csrc/kmeans.hip`` (``meld_kmeans_assign``: at most 64 centres of at
  most 32 dimensions staged in LDS, per-workgroup partial sums added in workgroup order) around its buffers.  ``library_step``
  ("library"): chunked distance GEMMs, ``argmin``, ``index_add_``; any shape.  The last two accumulate with float atomics and are
  not reproducible bit for bit.  ``pick_backend(d, k, prefer)`` names the one a run takes;
* ``lloyd``: steps from given centres; the stopping rule is squared centre shift <= ``tol`` x mean column variance, looked at once
  per ``CHECK_EVERY`` steps; the inertia of every step stays on the device until the end;
* ``seed_parallel``: k-means|| (Bahmani, Moseley, Vattani, Kumar, Vassilvitskii, "Scalable k-means++", VLDB 2012): one uniformly
  drawn centre, ``SEED_ROUNDS`` rounds that draw every point independently with probability ``min(1, 2 k d2_i / sum d2)`` and update
  ``d2`` with the assign kernel against the new candidates only, the candidates weighted by the number of points nearest to them,
  and a weighted k-means++ over the few thousand candidates that never reads a word back;
* ``seed_plusplus``: sequential k-means++, one word read back per centre;
* ``kmeans_device``: a seeding and ``lloyd`` per run, the run of lowest inertia of ``n_init``.

There is no CPU fallback.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from ._device_ops import stream
from ._lib import check, get_lib, ptr

__all__ = ["KMeans", "MAX_D", "MAX_K", "assign", "segment_sums", "lloyd_step", "lloyd", "seed_parallel", "kmeans_device"]

MAX_D = 128  # ``meld_kmeans_wide_max_d()``
MAX_K = 4096  # ``meld_kmeans_wide_max_k()``: centres per launch (tests/test_kmeans_host.py holds these and the library's together)
LDS_MAX_D, LDS_MAX_K = 32, 64  # what ``csrc/kmeans.hip`` stages in LDS
LIBRARY_ROWS = 1 << 18  # rows per distance GEMM of the library step
SEED_ROUNDS = 5
CHECK_EVERY = 8  # Lloyd steps between two looks of the host at the centre shift


def assign(Y, C, want_d2=True):
    """``(labels int32 [n], best_d2 fp64 [n] or None)``: the centre of ``C [k, d]`` nearest to every row of ``Y [n, d]`` (fp64 device
    tensors, unit stride inside a row, ``d <= MAX_D``), ties to the lowest index.  More than ``MAX_K`` centres go through the kernel
    in chunks, the label offset added and the minima combined (a later chunk wins only with a strictly smaller distance)."""
    lib = get_lib()
    n, d = int(Y.shape[0]), int(Y.shape[1])
    k = int(C.shape[0])
    if Y.dim() != 2 or C.dim() != 2 or int(C.shape[1]) != d or Y.dtype != torch.float64 or C.dtype != torch.float64:
        raise ValueError("assign takes fp64 points [n, d] and centres [k, d], got {} {} and {} {}".format(
            tuple(Y.shape), Y.dtype, tuple(C.shape), C.dtype))
    if n > 1 and Y.stride(1) != 1 and d > 1:
        Y = Y.contiguous()
    ldy = int(Y.stride(0)) if n > 1 else d
    if ldy < d:
        Y, ldy = Y.contiguous(), d
    C = C.contiguous()
    chunked = k > MAX_K
    lab = torch.empty(n, dtype=torch.int32, device=Y.device)
    d2 = torch.empty(n, dtype=torch.float64, device=Y.device) if (want_d2 or chunked) else None
    norms = torch.empty(min(k, MAX_K), dtype=torch.float64, device=Y.device)
    st = stream()
    for lo in range(0, k, MAX_K):
        Cc = C[lo : lo + MAX_K]
        first = lo == 0
        lab_c = lab if first else torch.empty_like(lab)
        d2_c = d2 if first else torch.empty_like(d2)
        check(lib.meld_kmeans_wide_assign(ptr(Y), ldy, n, d, ptr(Cc), int(Cc.shape[0]), ptr(norms), ptr(lab_c), ptr(d2_c), st),
              "meld_kmeans_wide_assign")
        if not first:
            better = d2_c < d2
            lab = torch.where(better, lab_c + lo, lab)
            d2 = torch.minimum(d2, d2_c)
    return lab, (d2 if want_d2 else None)


def segment_sums(Y, labels, k):
    """``(sums fp64 [k, d], counts int64 [k])`` of the rows of ``Y`` by ``labels`` (int32 device, in ``[0, k)``): the same bits on every
    run -- the rows of a cluster are added in the order the stable sort of the labels puts them in, through fixed slots."""
    n, d = int(Y.shape[0]), int(Y.shape[1])
    order = torch.sort(labels, stable=True).indices
    counts = torch.bincount(labels, minlength=k)
    seg = torch.zeros(k + 1, dtype=torch.int64, device=Y.device)
    seg[1:] = torch.cumsum(counts, 0)
    sums = torch.zeros(k, d, dtype=torch.float64, device=Y.device)
    ldy = int(Y.stride(0)) if n > 1 else d
    check(get_lib().meld_kmeans_wide_sums(ptr(Y), ldy, n, d, ptr(order), ptr(seg), int(k), ptr(sums), stream()), "meld_kmeans_wide_sums")
    return sums, counts


def _sq_dists(Y, C, y2=None, c2=None):
    """The expanded squared distances ``|y|^2 + |c|^2 - 2 y.c`` ``[n, k]`` on a library GEMM (not clamped: rounding can leave a
    small negative); ``y2``, ``c2``: the squared norms where the caller has them."""
    y2 = (Y * Y).sum(1) if y2 is None else y2
    c2 = (C * C).sum(1) if c2 is None else c2
    return y2[:, None] + c2[None, :] - 2.0 * (Y @ C.T)


def _library_chunks(Y, C, rows):
    """``(lo, Y[lo : lo + rows], best, idx)`` per chunk of ``rows`` points: the smallest expanded distance of every point of the
    chunk (not clamped) and the centre it belongs to, ties to the lowest index.  The chunk is the caller's: rocBLAS may pick its
    kernel by the number of rows."""
    c2 = (C * C).sum(1)
    for lo in range(0, int(Y.shape[0]), rows):
        Yc = Y[lo : lo + rows]
        best, idx = torch.min(_sq_dists(Yc, C, c2=c2), dim=1)
        yield lo, Yc, best, idx


def _new_centres(sums, cnt, C):
    """``sums / cnt``; an empty cluster keeps its centre."""
    return torch.where(cnt[:, None] > 0, sums / cnt.clamp(min=1).to(torch.float64)[:, None], C)


def lloyd_step(Y, C):
    """The "wide" Lloyd step: ``(new centres, inertia, labels)`` -- assign, sort, sums; no sync."""
    lab, d2 = assign(Y, C)
    sums, cnt = segment_sums(Y, lab, int(C.shape[0]))
    return _new_centres(sums, cnt, C), d2.sum(), lab


def lds_step(Y, k):
    """The "lds" Lloyd step for the contiguous points ``Y [n, d]`` and ``k`` centres (``meld_kmeans_assign``, ``d <= LDS_MAX_D``,
    ``k <= LDS_MAX_K``): the per-workgroup partials and the labels are allocated here, once, and every call of the step returned
    writes them -- the labels it returns are that one buffer."""
    lib = get_lib()
    n, d, k = int(Y.shape[0]), int(Y.shape[1]), int(k)
    nb = int(min(lib.meld_kmeans_max_blocks(), max(1, (n + 255) // 256)))
    f64 = dict(dtype=torch.float64, device=Y.device)
    part_sum, part_cnt, part_in = torch.empty(nb * k * d, **f64), torch.empty(nb * k, **f64), torch.empty(nb, **f64)
    lab = torch.empty(n, dtype=torch.int32, device=Y.device)

    def step(Y, C):
        if tuple(Y.shape) != (n, d) or tuple(C.shape) != (k, d) or not (Y.is_contiguous() and C.is_contiguous()):
            raise ValueError("this step was made for contiguous points {} and centres {}, got {} and {}".format(
                (n, d), (k, d), tuple(Y.shape), tuple(C.shape)))
        check(lib.meld_kmeans_assign(ptr(Y), n, d, ptr(C), k, ptr(lab), ptr(part_sum), ptr(part_cnt), ptr(part_in), nb, stream()),
              "meld_kmeans_assign")
        sums = part_sum.view(nb, k, d).sum(0)  # fixed-order reduction of the per-workgroup partials
        return _new_centres(sums, part_cnt.view(nb, k).sum(0), C), part_in.sum(), lab

    return step


def library_step(Y, C):
    """The "library" Lloyd step, any ``d`` and ``k``: chunked distance GEMMs, argmin, ``index_add_`` for the sums."""
    k = int(C.shape[0])
    lab = torch.empty(Y.shape[0], dtype=torch.int32, device=Y.device)
    sums = torch.zeros(k, int(Y.shape[1]), dtype=Y.dtype, device=Y.device)
    cnt = torch.zeros(k, dtype=Y.dtype, device=Y.device)
    inertia = torch.zeros((), dtype=Y.dtype, device=Y.device)
    for lo, Yc, best, idx in _library_chunks(Y, C, LIBRARY_ROWS):
        lab[lo : lo + Yc.shape[0]] = idx.to(lab.dtype)
        sums.index_add_(0, idx, Yc)
        cnt.index_add_(0, idx, torch.ones_like(best))
        inertia = inertia + best.clamp_(min=0.0).sum()
    return _new_centres(sums, cnt, C), inertia, lab


def pick_backend(d, k, prefer):
    """The Lloyd step a run on ``d`` features into ``k`` clusters takes: ``prefer="lds"`` (VertexFrequencyCluster,
    ``landmarks(kmeans="library")``) is ``"lds"`` where ``csrc/kmeans.hip`` stages the centres, ``prefer="wide"`` (``KMeans``,
    ``landmarks(kmeans="device")``) is ``"wide"`` up to ``MAX_D`` features; ``"library"`` beyond either."""
    if prefer not in ("lds", "wide"):
        raise ValueError("prefer must be 'lds' or 'wide', got {!r}".format(prefer))
    if prefer == "lds":
        return "lds" if d <= LDS_MAX_D and k <= LDS_MAX_K else "library"
    return "wide" if d <= MAX_D else "library"


def lloyd(Y, C, step, max_iter=300, tol=1e-4):
    """Lloyd iterations of ``step`` from the centres ``C``: a dict with ``centres``, ``labels`` (int32 device, the assignment to the
    final centres; ``lds_step``'s buffer where that is the step), ``inertia`` (of that assignment), ``iterations`` and ``history``
    (fp64 device: the inertia of every step).  ``max_iter=0`` takes no step, only that assignment."""
    Y = Y.contiguous()
    var_tol = tol * float(Y.var(dim=0, unbiased=False).mean())
    C = C.contiguous()
    history = []
    steps = 0
    for it in range(int(max_iter)):
        newC, inertia, _ = step(Y, C)
        history.append(inertia)
        shift = ((newC - C) ** 2).sum()
        C = newC.contiguous()
        steps = it + 1
        if it % CHECK_EVERY == CHECK_EVERY - 1 and float(shift) <= var_tol:  # (the host looks once per 8 steps)
            break
    if step is lloyd_step:  # (the assignment alone: nobody asks for the centres after these)
        lab, d2 = assign(Y, C)
        inertia = d2.sum()
    else:
        _, inertia, lab = step(Y, C)
    hist = torch.stack(history) if history else torch.zeros(0, dtype=torch.float64, device=Y.device)
    return dict(centres=C, labels=lab, inertia=float(inertia), iterations=steps, history=hist)


def _nearest(Y, C):
    """``(labels, d2)`` against any number of centres of any width (the library route for ``d > MAX_D``)."""
    if int(Y.shape[1]) <= MAX_D:
        return assign(Y, C)
    lab = torch.empty(Y.shape[0], dtype=torch.int64, device=Y.device)
    d2 = torch.empty(Y.shape[0], dtype=torch.float64, device=Y.device)
    rows = max(1, (1 << 26) // max(1, int(C.shape[0])))
    for lo, _, best, idx in _library_chunks(Y, C, rows):
        lab[lo : lo + rows], d2[lo : lo + rows] = idx, best.clamp_(min=0.0)
    return lab.to(torch.int32), d2


def seed_plusplus(Y, k, gen, info=None):
    """Sequential k-means++ seeding: ``k`` rows of ``Y`` as centres ``[k, d]``, one ``randint`` and then one ``multinomial`` per
    further centre from ``gen``, each read back (``info`` is ``seed_parallel``'s argument and stays as it is)."""
    n = int(Y.shape[0])
    first = int(torch.randint(0, n, (1,), device=Y.device, generator=gen))
    C = [Y[first]]
    d2 = ((Y - C[0]) ** 2).sum(1)
    for _c in range(1, k):
        tot = d2.sum()
        probs = d2 / tot if float(tot) > 0 else torch.full_like(d2, 1.0 / n)
        nxt = int(torch.multinomial(probs, 1, generator=gen))
        C.append(Y[nxt])
        d2 = torch.minimum(d2, ((Y - C[-1]) ** 2).sum(1))
    return torch.stack(C).contiguous()


def seed_parallel(Y, k, gen, info=None):
    """k-means|| seeding (module docstring): ``k`` centres ``[k, d]`` for the rows of ``Y``; every draw comes from ``gen``.  The host
    reads one word per round (the number of new candidates); the weighted k-means++ over the candidates reads none."""
    n = int(Y.shape[0])
    dev = Y.device
    cand = torch.randint(0, n, (1,), device=dev, generator=gen)
    lab, d2 = _nearest(Y, Y[cand])
    lab = lab.to(torch.int64)
    for _ in range(SEED_ROUNDS):
        tot = d2.sum()
        p = torch.where(tot > 0, (2.0 * k) * d2 / tot.clamp(min=1e-300), torch.zeros_like(d2)).clamp_(max=1.0)
        new = torch.nonzero(torch.rand(n, dtype=torch.float64, device=dev, generator=gen) < p).flatten()
        if int(new.shape[0]) == 0:
            continue
        lab_n, d2_n = _nearest(Y, Y[new])  # (against the new candidates only)
        better = d2_n < d2
        lab = torch.where(better, lab_n.to(torch.int64) + int(cand.shape[0]), lab)
        d2 = torch.minimum(d2, d2_n)
        cand = torch.cat([cand, new])
    m = int(cand.shape[0])
    P = Y[cand].contiguous()
    w = torch.bincount(lab, minlength=m).to(torch.float64)  # points nearest to every candidate
    # weighted k-means++ over the candidates, greedy as sklearn's: 2 + log k draws per centre, the one that lowers the weighted
    # potential most is kept.  Indices stay tensors, nothing is read back.
    trials = 2 + int(np.log(k))
    p2 = (P * P).sum(1)
    chosen = torch.empty(k, dtype=torch.int64, device=dev)
    last = torch.multinomial(w, 1, generator=gen)
    chosen[0:1] = last
    dd = ((P - P[last]) ** 2).sum(1)
    for c in range(1, k):
        pr = w * dd
        ok = pr.sum() > 0  # (false once every distinct candidate is taken: the missing centres repeat the last one)
        idx = torch.multinomial(torch.where(ok, pr, w), trials, replacement=True, generator=gen)
        dist = _sq_dists(P, P[idx], p2, p2[idx]).clamp_(min=0.0)  # [m, trials]
        dist.scatter_(0, idx[None, :], 0.0)  # (a candidate is at distance 0 from itself, whatever the expanded form rounds to)
        dist = torch.minimum(dist, dd[:, None])
        pick = torch.argmin((w[:, None] * dist).sum(0))
        nxt = torch.where(ok, idx[pick].reshape(1), last)  # (indexed by the tensor: no int() of it, no sync)
        chosen[c : c + 1] = nxt
        dd = torch.where(ok, dist[:, pick], dd)
        last = nxt
    if info is not None:
        info.update(seed_candidates=m)
    return P[chosen].contiguous()


def kmeans_device(Y, k, n_init=1, max_iter=300, tol=1e-4, seed=None, init=None, info=None, seeding="k-means||", prefer="wide"):
    """A seeding (``"k-means||"``: ``seed_parallel``, ``"k-means++"``: ``seed_plusplus``; or the centres ``init``) + ``lloyd`` on the
    step ``pick_backend`` names for ``prefer``, on the fp64 device tensor ``Y [n, d]``; the run of lowest inertia of ``n_init``, all
    of them drawing from one generator.  Returns ``lloyd``'s dict with ``lloyd`` (``"device"`` for the wide step, ``"lds"`` or
    ``"library"``) and the seeder's ``seed_candidates``; ``info`` receives ``iterations``, ``inertia`` and ``lloyd``."""
    if not Y.is_cuda:
        raise RuntimeError("meld_amd needs a ROCm GPU (MI355X); there is no CPU fallback")
    if seeding not in ("k-means||", "k-means++"):
        raise ValueError("seeding must be 'k-means||' or 'k-means++', got {!r}".format(seeding))
    Y, k, inits = Y.contiguous(), int(k), max(1, int(n_init))
    backend = pick_backend(int(Y.shape[1]), k, prefer)
    step = {"wide": lloyd_step, "library": library_step}.get(backend) or lds_step(Y, k)
    seeder = seed_parallel if seeding == "k-means||" else seed_plusplus
    gen = torch.Generator(device=Y.device)
    gen.manual_seed(0 if seed is None else int(seed))
    best = None
    for i in range(inits):
        extra = {}
        C0 = init if init is not None else seeder(Y, k, gen, info=extra)
        run = lloyd(Y, C0, step, max_iter=max_iter, tol=tol)
        run.update(extra, lloyd="device" if backend == "wide" else backend)
        if best is None or run["inertia"] < best["inertia"]:
            best = run
            if backend == "lds" and i + 1 < inits:  # (the next run writes the label buffer of ``lds_step``)
                best["labels"] = best["labels"].clone()
    if info is not None:
        info.update(iterations=best["iterations"], inertia=best["inertia"], lloyd=best["lloyd"])
    return best


def _positive_int(name, v, least=1):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (numbers.Integral, np.integer)) or int(v) < least:
        raise ValueError("{} must be an integer >= {}, got {!r}".format(name, least, v))
    return int(v)


class KMeans:
    """k-means on the device ([UPSTREAM ``sklearn.cluster.KMeans``]'s role in the reference's comparison): k-means|| seeding and
    Lloyd iterations in HIP for up to 128 features, any number of clusters.

    ``init``: ``"k-means||"`` or an array ``[n_clusters, d]`` of starting centres (then ``n_init`` must be 1).  ``fit(X)`` takes a
    numpy array, a DataFrame or a device tensor ``[n, d]`` (converted to fp64 on the device) and sets ``cluster_centers_`` (host
    ``[k, d]``), ``labels_`` (host int32), ``labels_device_``, ``inertia_``, ``n_iter_``, ``inertia_history_`` (the inertia of every
    Lloyd step) and ``info_`` (``"lloyd"``: ``"device"``, or ``"library"`` for more than 128 features).  The same ``random_state``
    (None: 0) gives the same bits."""

    def __init__(self, n_clusters=8, init="k-means||", n_init=1, max_iter=300, tol=1e-4, random_state=None):
        self.n_clusters = _positive_int("n_clusters", n_clusters)
        self.n_init = _positive_int("n_init", n_init)
        self.max_iter = _positive_int("max_iter", max_iter, least=0)
        if isinstance(tol, (bool, np.bool_)) or not isinstance(tol, (numbers.Real, np.floating, np.integer)) or not float(tol) >= 0.0:
            raise ValueError("tol must be a non-negative number, got {!r}".format(tol))
        self.tol = float(tol)
        if random_state is not None and (isinstance(random_state, (bool, np.bool_)) or not isinstance(random_state, (numbers.Integral, np.integer))):
            raise ValueError("random_state must be None or an integer, got {!r}".format(random_state))
        self.random_state = random_state
        if isinstance(init, str):
            if init != "k-means||":
                raise ValueError("init must be 'k-means||' or an array [n_clusters, d], got {!r}".format(init))
        else:
            shape = tuple(getattr(init, "shape", ()))
            if len(shape) != 2 or int(shape[0]) != self.n_clusters:
                raise ValueError("init must be 'k-means||' or an array [n_clusters={}, d], got shape {}".format(self.n_clusters, shape))
            if self.n_init != 1:
                raise ValueError("n_init must be 1 with an array init, got {}".format(self.n_init))
        self.init = init
        self.cluster_centers_ = None
        self._centres_device = None

    @staticmethod
    def _to_device(X, name="X"):
        shape = tuple(getattr(X, "shape", ()))
        if len(shape) != 2 or int(shape[0]) < 1 or int(shape[1]) < 1:
            raise ValueError("{} must be two-dimensional [n, d] with at least one row and one column, got shape {}".format(name, shape))
        if not torch.cuda.is_available():
            raise RuntimeError("meld_amd needs a ROCm GPU (MI355X); there is no CPU fallback")
        if isinstance(X, torch.Tensor):
            return X.detach().to(device="cuda", dtype=torch.float64).contiguous()
        return torch.from_numpy(np.ascontiguousarray(getattr(X, "values", X), dtype=np.float64)).to("cuda")

    def fit(self, X):
        Y = self._to_device(X)
        n, d = int(Y.shape[0]), int(Y.shape[1])
        if n < self.n_clusters:
            raise ValueError("X has {} rows, fewer than n_clusters={}".format(n, self.n_clusters))
        init = None
        if not isinstance(self.init, str):
            init = self._to_device(self.init, "init")
            if int(init.shape[1]) != d:
                raise ValueError("init has {} columns, X has {}".format(int(init.shape[1]), d))
        run = kmeans_device(Y, self.n_clusters, n_init=self.n_init, max_iter=self.max_iter, tol=self.tol, seed=self.random_state, init=init)
        self._centres_device = run["centres"]
        self.cluster_centers_ = run["centres"].cpu().numpy()
        self.labels_device_ = run["labels"]
        self.labels_ = run["labels"].cpu().numpy()
        self.inertia_ = run["inertia"]
        self.n_iter_ = run["iterations"]
        self.inertia_history_ = run["history"].cpu().numpy()
        self.info_ = dict(lloyd=run["lloyd"], seed_candidates=run.get("seed_candidates"))
        return self

    def fit_predict(self, X):
        return self.fit(X).labels_

    def _fitted(self, X):
        if self._centres_device is None:
            raise ValueError("Estimator must be `fit` before this call.")
        Y = self._to_device(X)
        if int(Y.shape[1]) != int(self._centres_device.shape[1]):
            raise ValueError("X has {} columns, the estimator was fitted on {}".format(int(Y.shape[1]), int(self._centres_device.shape[1])))
        return Y

    def predict(self, X):
        """The nearest centre of every row of ``X`` (host int32): one assign launch (beyond ``MAX_D`` features the library's)."""
        Y, C = self._fitted(X), self._centres_device
        if int(Y.shape[1]) <= MAX_D:
            return assign(Y, C, want_d2=False)[0].cpu().numpy()
        return torch.cat([idx for _, _, _, idx in _library_chunks(Y, C, LIBRARY_ROWS)]).to(torch.int32).cpu().numpy()

    def transform(self, X):
        """The distances ``[n, k]`` of the rows of ``X`` to the centres (host fp64; a library GEMM)."""
        return torch.sqrt(_sq_dists(self._fitted(X), self._centres_device).clamp_(min=0.0)).cpu().numpy()
