"""A plain host reference of the exact re-evaluation (``meld_knn_refine``) and of the exact sweep (``meld_knn_radius_exact``).

NumPy only, every distance in ``np.longdouble`` (64-bit mantissa on x86: about 2000 times finer than the kernels' fp64).  It restates
the contract of include/meld_hip.h ("exact re-evaluation + alpha-decay kernel") and of DESIGN.md section 4.2, row by row, with none of
the kernels' shortcuts: no prefix gate on the approximate distances, no fast ranking, one summation order (NumPy's).

The contract, per candidate row q (local row ``orow = rows[q]`` or q, cell ``gi = q_begin + orow``):
  * the list is the first ``n = min(cnt[q], ksel)`` entries of the row; anything behind them is ignored;
  * entries are ranked by (exact distance, index); the bandwidth is the distance of rank ``knn`` (self counted), or the given
    ``bw_fixed[gi]``; what is RECORDED is that value floored at eps, what the kernel USES is max(recorded * bw_scale, eps);
  * radius = used bandwidth * (-ln thresh)^(1 / decay) (decay = inf: 1); reach = radius, and with an adaptive bandwidth
    max(radius, recorded bandwidth);
  * E = err_coef * norm2_max + err_coef_lin * sqrt(norm2[gi] * norm2_max);
  * tau = approximate d2 of slot ksel - 1 if cnt[q] >= ksel, else +inf; lowered to thr[q] when thresholds are given;
  * complete  <=>  reach^2 + E <= tau,
                   or (max_rank > 0, the entry of rank max_rank - 1 exists, its d^2 + E <= tau and it is not closer than the
                   recorded bandwidth);
    never with n <= knn and no given bandwidth (the list cannot even define the bandwidth);
  * a complete row holds K = exp(-(d / used bandwidth)^decay) (decay = inf: d <= used bandwidth) per slot, 0 where K < thresh, on
    the row's own index and at ranks >= max_rank; an incomplete row holds zeros and keep_cnt 0.
"""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)  # DBL_EPSILON


def exact_d2(X, i, cols=None):
    """|X[i] - X[cols]|^2 in long double (cols = None: every row of X)."""
    Y = X if cols is None else X[np.asarray(cols, dtype=np.int64)]
    t = Y.astype(LD) - X[i].astype(LD)
    return np.sum(t * t, axis=1, dtype=LD)


def radius_factor(decay, thresh):
    if np.isinf(decay):
        return LD(1)
    return np.power(-np.log(LD(thresh)), LD(1) / LD(decay))


def kernel_values(dist, bw_used, decay):
    """exp(-(dist / bw)^decay) in long double (decay = inf: the connectivity of dist <= bw); NaN -> 1."""
    dist = np.asarray(dist, dtype=LD)
    if np.isinf(decay):
        return (dist <= bw_used).astype(LD)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        v = np.exp(-np.power(dist / LD(bw_used), LD(decay)))
    return np.where(np.isnan(v), LD(1), v)


def refine_ref(X, q_begin, idx, d2, cnt, thr, ksel, cap, knn, decay, thresh, norm2_max, err_coef, norm2=None, err_coef_lin=0.0,
               bw_scale=1.0, bw_fixed=None, max_rank=0, rows=None):
    """One entry per CANDIDATE row q (the caller places it at local row rows[q]).  Returns a dict of arrays:
    bw (long double, recorded), val [q][ksel] (long double), keep_cnt, complete, margin = (tau - (reach^2 + E)) / tau (+inf where
    tau is), margin_rank = the same for the entry of rank max_rank - 1 (nan where the clause does not apply), dist [q][ksel] and
    rank [q][ksel] (inf / -1 behind the list), reach2, E, tau."""
    idx = np.asarray(idx).reshape(-1, cap)
    d2 = np.asarray(d2).reshape(-1, cap)
    nq = idx.shape[0]
    rf = radius_factor(decay, thresh)
    out = dict(bw=np.zeros(nq, LD), val=np.zeros((nq, ksel), LD), keep_cnt=np.zeros(nq, np.int64), complete=np.zeros(nq, bool),
               margin=np.zeros(nq, LD), margin_rank=np.full(nq, np.nan, LD), dist=np.full((nq, ksel), np.inf, LD),
               rank=np.full((nq, ksel), -1, np.int64), reach2=np.zeros(nq, LD), E=np.zeros(nq, LD), tau=np.zeros(nq, LD))
    for q in range(nq):
        orow = int(rows[q]) if rows is not None else q
        gi = q_begin + orow
        n = min(int(cnt[q]), ksel)
        cols = idx[q, :n].astype(np.int64)
        dist = np.sqrt(exact_d2(X, gi, cols)) if n else np.zeros(0, LD)
        order = np.lexsort((cols, dist))  # by (distance, index)
        rank = np.empty(n, np.int64)
        rank[order] = np.arange(n)
        if bw_fixed is not None:
            bw_raw = LD(bw_fixed[gi])
        else:
            bw_raw = dist[order[knn]] if n > knn else LD(0)
        bw_raw = max(bw_raw, LD(EPS))
        bw_used = max(bw_raw * LD(bw_scale), LD(EPS))
        radius = bw_used * rf
        reach = radius if bw_fixed is not None else max(radius, bw_raw)
        E = LD(err_coef) * LD(norm2_max)
        if norm2 is not None and err_coef_lin > 0:
            E = E + LD(err_coef_lin) * np.sqrt(LD(norm2[gi]) * LD(norm2_max))
        tau = LD(d2[q, ksel - 1]) if int(cnt[q]) >= ksel else LD(np.inf)
        if thr is not None:
            tau = min(tau, LD(thr[q]))
        complete = bool(reach * reach + E <= tau)
        margin = LD(np.inf) if np.isinf(tau) else (tau - (reach * reach + E)) / tau
        if max_rank > 0 and n >= max_rank:
            d_m = dist[order[max_rank - 1]]
            out["margin_rank"][q] = LD(np.inf) if np.isinf(tau) else (tau - (d_m * d_m + E)) / tau
            if d_m * d_m + E <= tau and d_m >= bw_raw:
                complete = True
        if bw_fixed is None and n <= knn:
            complete = False
        if complete and n:
            v = kernel_values(dist, bw_used, decay)
            v = np.where(v < LD(thresh), LD(0), v)
            v = np.where(cols == gi, LD(0), v)
            if max_rank > 0:
                v = np.where(rank >= max_rank, LD(0), v)
            out["val"][q, :n] = v
            out["keep_cnt"][q] = int(np.count_nonzero(v > 0))
        out["bw"][q], out["complete"][q], out["margin"][q] = bw_raw, complete, margin
        out["dist"][q, :n], out["rank"][q, :n] = dist, rank
        out["reach2"][q], out["E"][q], out["tau"][q] = reach * reach, E, tau
    return out


def sweep_ref(X, q_begin, rows, bw, knn, decay, thresh, bw_scale=1.0):
    """Brute force over all N references for the local rows ``rows``; ``bw``: the recorded (unscaled) bandwidth per local row
    (indexed by local row, any float type).  Returns a list of dicts, one per row: cols (sorted), vals (long double, same order),
    n_closer (references strictly closer than the recorded bandwidth, the row itself among them), confirmed (n_closer <= knn, or a
    bandwidth at eps), dist (long double, all N), v (all N, the row's own entry included)."""
    res = []
    for r in rows:
        r = int(r)
        gi = q_begin + r
        dist = np.sqrt(exact_d2(X, gi))
        b = LD(bw[r])
        bw_used = max(b * LD(bw_scale), LD(EPS))
        v = kernel_values(dist, bw_used, decay)
        keep = v >= LD(thresh)
        keep[gi] = False
        cols = np.nonzero(keep)[0]
        n_closer = int(np.count_nonzero(dist < b))
        res.append(dict(cols=cols, vals=v[cols], n_closer=n_closer, confirmed=bool(n_closer <= knn or b <= LD(EPS)), dist=dist, v=v))
    return res


def true_lists(X, q_begin, q_count, kk, rows=None):
    """The kk nearest cells (self included) of every row by long-double brute force, ranked by (distance, index):
    (idx [q][kk], d2 [q][kk] long double)."""
    idx = np.zeros((q_count, kk), np.int64)
    d2 = np.zeros((q_count, kk), LD)
    for q in range(q_count):
        gi = q_begin + (int(rows[q]) if rows is not None else q)
        e = exact_d2(X, gi)
        o = np.lexsort((np.arange(e.shape[0]), e))[:kk]
        idx[q], d2[q] = o, e[o]
    return idx, d2
