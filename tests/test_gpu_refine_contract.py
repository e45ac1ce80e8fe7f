"""Contract tests of ``meld_knn_refine`` and ``meld_knn_radius_exact`` (csrc/refine.hip), called directly with candidate lists made
on the host, against tests/refine_reference.py (long double, tied to the oracle by tests/test_refine_reference.py).

The rest of the suite reaches these kernels only through the graph builder, with lists the search kernels produced -- lists that are
already complete on the data the suite uses, so the certification decision (``reach^2 + E <= tau``) is never seen on a list that is
wrong.  Here the lists are built so that every branch of the decision, of the ranking and of both distance code paths is observed.

Inputs
    Cells are ``normal * uniform(0.2, 2) + offset``; for d >= 100 they live in 6 intrinsic dimensions, mapped into d by a random
    orthonormal map, plus 1e-3 noise (isotropic cells in hundreds of dimensions put the kernel radius beyond any list).  A list holds
    the true nearest cells (long-double brute force); the approximate d2 is the exact one moved by at most 0.9 E (E = the row's
    search-error allowance as handed to the kernel, or a smaller one), rounded to fp32 and sorted, so the exact order deviates from
    the list order inside the allowance -- on every second row in the worst direction for the kernel's prefix gate (the knn + 1
    nearest moved down, everything else up).  The slots behind ``cnt`` up to ``cap`` hold poison that is IN RANGE: the row's own
    index or its nearest cell's, approximate d2 0.  No index in this file is out of range.

Conditions asserted on the host before anything is launched (``_conditions``): no two candidate distances of a row closer than
1e-10 relative except exact copies of a cell; no reference kernel value within 1e-6 relative of ``thresh`` (decay = inf: no distance
within 1e-10 of the bandwidth except the bandwidth entry itself); every certification margin at least 1e-6 in magnitude.  Every slot
of every row is therefore decided and every slot is compared.

Tolerances (derived, not tuned), u = 2^-53
    The kernel's d2 is a sum of FMA chains of squared differences, none longer than ceil(d / 2): the difference carries one rounding,
    its square enters the chain exactly (FMA), every chain step rounds once, and at most three more additions join the chains --
    relative error at most (d / 2 + 8) u, all terms being non-negative.  The square root halves it (and adds u / 2, inside the 8):
        |bw - bw_ref| <= (d / 2 + 8) u / 2 * bw_ref.
    A kernel value v = exp(-(dist / bw)^decay) has d ln v = -decay (dist / bw)^decay d ln(dist / bw); a kept value has
    (dist / bw)^decay <= -ln thresh, and dist / bw carries two such distance errors and a division, at most (d + 16) u / 2 together
    -- doubled here -- plus a few ulps of pow and exp:
        |v - v_ref| <= (decay * (-ln thresh) * (d + 16) + 64) u * v_ref.
    decay = inf gives 0 or 1: compared exactly.  A bandwidth at DBL_EPSILON and a given bandwidth are compared exactly.
    keep_cnt, n_flag, the set of flagged rows (a set: the order of the atomic appends is not fixed), cand_idx_out and every zero /
    non-zero pattern are compared exactly.
    The certification boundary is placed 20 fp32 ulps from ``reach^2 + E``: 1.2e-6 .. 2.4e-6 relative, the fewest ulps that keep the
    1e-6 margin above, and ten orders of magnitude beyond the fp64 rounding of either side of the comparison.

Largest deviations seen on the MI355X are recorded in DESIGN.md section 4.2 next to these bounds; each test prints its own.
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from tests import refine_reference as rr

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
EPS = rr.EPS
THRESH = 1e-4


def bw_tol(d):
    return (d / 2 + 8) * U / 2


def val_tol(d, decay, thresh=THRESH):
    return 0.0 if math.isinf(decay) else (decay * (-math.log(thresh)) * (d + 16) + 64) * U


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def make_cells(rng, N, d):
    if d < 100:
        return rng.normal(size=(N, d)) * rng.uniform(0.2, 2.0, size=d) + rng.normal(size=d)
    Z = rng.normal(size=(N, 6)) * rng.uniform(0.2, 2.0, size=6)
    Q, _ = np.linalg.qr(rng.normal(size=(d, 6)))
    return np.ascontiguousarray(Z @ Q.T + rng.normal(size=d) + 1e-3 * rng.normal(size=(N, d)))


def make_lists(X, gis, true_idx, true_d2, cnt, cap, e_pert, rng, knn, adversarial_every=2):
    """Candidate lists from the true neighbours: cnt[q] entries each, approximate d2 within 0.9 e_pert[q] of the exact one, fp32,
    sorted; in-range poison behind them."""
    nq = len(gis)
    idx = np.zeros((nq, cap), np.int32)
    d2 = np.zeros((nq, cap), np.float32)
    for q in range(nq):
        n = int(cnt[q])
        e = true_d2[q, :n]
        shift = rng.uniform(-0.9, 0.9, size=n)
        if adversarial_every and q % adversarial_every == 0:
            shift = np.where(np.arange(n) <= knn, -0.9, 0.9)
        a = np.maximum(e + LD(e_pert[q]) * shift, 0).astype(np.float32)
        assert np.all(np.abs(a.astype(LD) - e) <= LD(e_pert[q]) + LD(2.0 ** -23) * e)
        o = np.argsort(a, kind="stable")
        idx[q, :n], d2[q, :n] = true_idx[q, :n][o], a[o]
        poison = [int(gis[q]), int(true_idx[q, 1])]
        for c in range(n, cap):
            idx[q, c] = poison[c & 1]
    return idx, d2


def allowance(X, gis, e_target, form):
    """(norm2_max, err_coef, norm2 or None, err_coef_lin, E per row) with a typical E of e_target: constant only, or half of it
    constant and half through the row's own norm."""
    n2 = np.sum(X * X, axis=1).astype(np.float32)
    nmax = np.float32(n2.max())
    if form == "const":
        c = float(e_target) / float(nmax)
        return nmax, c, None, 0.0, np.full(len(gis), LD(c) * LD(nmax))
    c = 0.5 * float(e_target) / float(nmax)
    lin = 0.5 * float(e_target) / math.sqrt(float(np.median(n2)) * float(nmax))
    E = LD(c) * LD(nmax) + LD(lin) * np.sqrt(n2[gis].astype(LD) * LD(nmax))
    return nmax, c, n2, lin, E


def make_case(X, q_begin, q_count, ksel, knn, decay, idx, d2, cnt, nmax, err_coef, norm2=None, err_lin=0.0, thr=None, bw_scale=1.0,
              bw_fixed=None, max_rank=0, rows=None, out_cap=0, n_local=None, thresh=THRESH):
    return SimpleNamespace(X=X, N=X.shape[0], d=X.shape[1], q_begin=q_begin, q_count=q_count, ksel=ksel, cap=idx.shape[1], knn=knn, decay=decay,
                           thresh=thresh, idx=idx, d2=d2, cnt=np.asarray(cnt, np.int32), nmax=np.float32(nmax), err_coef=float(err_coef),
                           norm2=norm2, err_lin=float(err_lin), thr=thr, bw_scale=bw_scale, bw_fixed=bw_fixed, max_rank=max_rank, rows=rows,
                           out_cap=out_cap, n_local=n_local if n_local is not None else q_count)


def reference(c):
    return rr.refine_ref(c.X, c.q_begin, c.idx, c.d2, c.cnt, c.thr, c.ksel, c.cap, c.knn, c.decay, c.thresh, c.nmax, c.err_coef, c.norm2,
                         c.err_lin, c.bw_scale, c.bw_fixed, c.max_rank, c.rows)


def _conditions(c, ref):
    """What keeps a comparison from excusing a failure; asserted before the launch."""
    X = c.X
    for q in range(c.q_count):
        n = min(int(c.cnt[q]), c.ksel)
        dist, cols = ref["dist"][q, :n], c.idx[q, :n]
        o = np.lexsort((cols, dist))
        ds, cs = dist[o], cols[o]
        for k in range(1, n):
            if ds[k] == ds[k - 1]:
                assert np.array_equal(X[cs[k]], X[cs[k - 1]]), ("two cells at one distance that are no copies", q, k)
            else:
                assert (ds[k] - ds[k - 1]) / ds[k] > 1e-10, ("near tie", q, k, float((ds[k] - ds[k - 1]) / ds[k]))
        bw_used = max(ref["bw"][q] * LD(c.bw_scale), LD(EPS))
        if math.isinf(c.decay):
            off = np.abs(dist / bw_used - 1)
            assert np.all((off > 1e-10) | (dist == bw_used)), ("distance on the bandwidth", q)
        else:
            v = rr.kernel_values(dist, bw_used, c.decay)
            assert float(np.min(np.abs(v / LD(c.thresh) - 1))) > 1e-6, ("value on the threshold", q)
        if np.isfinite(ref["margin"][q]):
            assert abs(ref["margin"][q]) >= 1e-6, ("certification margin", q, float(ref["margin"][q]))
        if c.max_rank > 0 and np.isfinite(ref["margin_rank"][q]) and ref["margin"][q] < 0:
            assert abs(ref["margin_rank"][q]) >= 1e-6, ("rank margin", q, float(ref["margin_rank"][q]))


# ---------------------------------------------------------------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------------------------------------------------------------
SENT_BW, SENT_VAL, SENT_CNT, SENT_IDX = -7.0, -3.0, -5, -9


def run_refine(c):
    """meld_knn_refine on the case; every output as a host array (pre-filled with sentinels)."""
    import torch

    from meld_amd._lib import check, get_lib, ptr
    from meld_amd.graph import _stream

    dev = "cuda"
    t = lambda a, dt: None if a is None else torch.from_numpy(np.array(a, dtype=dt, order="C")).to(dev)
    X, idx, d2, cnt = t(c.X, np.float64), t(c.idx, np.int32), t(c.d2, np.float32), t(c.cnt, np.int32)
    thr, norm2, bwf, rows = t(c.thr, np.float32), t(c.norm2, np.float32), t(c.bw_fixed, np.float64), t(c.rows, np.int32)
    nmax = t(np.array([c.nmax]), np.float32)
    L = c.n_local
    bw = torch.full((L,), SENT_BW, dtype=torch.float64, device=dev)
    val = torch.full((L, c.ksel), SENT_VAL, dtype=torch.float64, device=dev)
    keep = torch.full((L,), SENT_CNT, dtype=torch.int32, device=dev)
    flag_rows = torch.full((max(L, c.q_count),), -1, dtype=torch.int32, device=dev)
    n_flag = torch.zeros(1, dtype=torch.int32, device=dev)
    idx_out = torch.full((L, c.out_cap), SENT_IDX, dtype=torch.int32, device=dev) if c.rows is not None else None
    check(get_lib().meld_knn_refine(ptr(X), c.N, c.d, c.q_begin, c.q_count, ptr(idx), ptr(d2), ptr(cnt), ptr(thr), c.ksel, c.cap, c.knn,
                                    float(c.decay), float(c.thresh), ptr(nmax), c.err_coef, ptr(norm2), c.err_lin, ptr(bw), ptr(val), ptr(keep),
                                    ptr(flag_rows), ptr(n_flag), ptr(rows), c.out_cap, ptr(idx_out), float(c.bw_scale), ptr(bwf), c.max_rank,
                                    _stream()), "meld_knn_refine")
    torch.cuda.synchronize()
    nf = int(n_flag.item())
    return SimpleNamespace(bw=bw.cpu().numpy(), val=val.cpu().numpy(), keep_cnt=keep.cpu().numpy(), n_flag=nf,
                           flag_rows=flag_rows.cpu().numpy(), idx_out=None if idx_out is None else idx_out.cpu().numpy())


def compare(c, out, ref, label=""):
    """Every row and every slot of the outputs against the reference; returns the largest deviations (bandwidth, value) in units
    of their bounds' u."""
    where = np.arange(c.q_count) if c.rows is None else np.asarray(c.rows, np.int64)
    bw, val, keep = out.bw[where], out.val[where], out.keep_cnt[where]
    # flags: exactly the rows the contract cannot certify, each once
    assert 0 <= out.n_flag <= c.q_count
    flagged = out.flag_rows[: out.n_flag]
    assert len(set(flagged.tolist())) == out.n_flag
    assert set(flagged.tolist()) == set(where[~ref["complete"]].tolist()), (
        label, sorted(set(flagged.tolist()) ^ set(where[~ref["complete"]].tolist()))[:10])
    assert out.n_flag == int((~ref["complete"]).sum())
    # bandwidths
    rbw = ref["bw"].astype(np.float64)
    exact = (ref["bw"] <= LD(EPS)) | (c.bw_fixed is not None)
    assert np.array_equal(bw[exact], rbw[exact]), label
    dev_bw = np.abs(bw.astype(LD) - ref["bw"]) / ref["bw"]
    assert float(dev_bw.max()) <= bw_tol(c.d), (label, float(dev_bw.max()) / U, bw_tol(c.d) / U)
    # kernel values: pattern exactly, values within the bound, every slot
    rv = ref["val"]
    assert np.array_equal(val > 0, rv > 0), (label, np.argwhere((val > 0) != (rv > 0))[:10].tolist())
    assert np.all(val[rv == 0] == 0)
    nz = rv > 0
    dev_v = np.zeros(1, LD)
    if nz.any():
        dev_v = np.abs(val[nz].astype(LD) - rv[nz]) / rv[nz]
        assert float(dev_v.max()) <= val_tol(c.d, c.decay, c.thresh), (label, float(dev_v.max()) / U, val_tol(c.d, c.decay, c.thresh) / U)
    assert np.array_equal(keep, ref["keep_cnt"]), label
    assert np.all(keep[~ref["complete"]] == 0) and np.all(val[~ref["complete"]] == 0)
    print("DEVIATION {} d={} decay={} rows={} certified={} bw {:.2f}u (bound {:.1f}u) val {:.1f}u (bound {:.0f}u)".format(
        label, c.d, c.decay, c.q_count, int(ref["complete"].sum()), float(dev_bw.max()) / U, bw_tol(c.d) / U, float(dev_v.max()) / U,
        val_tol(c.d, c.decay, c.thresh) / U))
    return float(dev_bw.max()) / U, float(dev_v.max()) / U


def check_case(c, label="", min_certified=0, min_flagged=0):
    ref = reference(c)
    _conditions(c, ref)
    assert int(ref["complete"].sum()) >= min_certified, (label, int(ref["complete"].sum()))
    assert int((~ref["complete"]).sum()) >= min_flagged, (label, int((~ref["complete"]).sum()))
    out = run_refine(c)
    compare(c, out, ref, label)
    return out, ref


_TRUE = {}


def cells_and_truth(seed, N, d, q_begin, q_count, kk, edit=None):
    """Cells and the true kk nearest of the query rows, computed once per configuration and never modified."""
    key = (seed, N, d, q_begin, q_count, kk, edit.__name__ if edit else None)
    if key not in _TRUE:
        X = make_cells(np.random.default_rng(seed), N, d)
        if edit is not None:
            X = edit(X)
        ti, td = rr.true_lists(X, q_begin, q_count, kk)
        for a in (X, ti, td):
            a.setflags(write=False)
        _TRUE[key] = (X, ti, td)
    return _TRUE[key]


def true_bw2(td, knn):
    return td[:, knn]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. values on certified rows
# ---------------------------------------------------------------------------------------------------------------------------------
# every d, ksel, knn, decay and error form of the contract occurs, and every d with more than one list length; not the full product
# (504 cases, each with a long-double brute force).  d: 2, 50, 52, 256 take the four-lane gather (50: one full round of seven
# 64-byte pieces minus three, 52 and 256: partial / several rounds), 1, 7 the odd tail, 302 the lane-per-candidate loop with a
# remainder (151 = 30 * 5 + 1).  ksel 12 / 64: the `<`-only ranking and its boundary, 65 / 128: two entries per lane.
VALUE_CASES = [
    # d, ksel, knn, decay, form, allowance as a fraction of the median bandwidth^2, q_begin
    (1, 12, 1, 2.0, "const", 0.2, 0),
    (1, 128, 30, math.inf, "lin", 0.05, 0),
    (2, 64, 1, 2.0, "lin", 0.2, 0),
    (2, 128, 30, 40.0, "const", 0.05, 1001),
    (7, 64, 7, 40.0, "const", 0.2, 0),
    (7, 65, 7, math.inf, "lin", 0.1, 333),
    (7, 12, 1, 40.0, "lin", 0.2, 0),
    (50, 64, 7, 40.0, "lin", 0.01, 0),
    (50, 12, 1, 40.0, "const", 0.01, 0),
    (52, 128, 30, 40.0, "const", 0.005, 0),
    (52, 65, 1, math.inf, "lin", 0.02, 0),
    (256, 128, 7, 40.0, "lin", 0.1, 0),
    (256, 64, 30, 40.0, "const", 0.02, 1200),
    (302, 65, 7, math.inf, "const", 0.1, 0),
    (302, 12, 1, 40.0, "lin", 0.1, 77),
    (302, 128, 30, 40.0, "const", 0.05, 0),
]


@pytest.mark.parametrize("d,ksel,knn,decay,form,efrac,q_begin", VALUE_CASES)
def test_values_bandwidths_and_flags_on_perturbed_complete_lists(d, ksel, knn, decay, form, efrac, q_begin):
    N, q_count, cap = 1500, 101, ksel + 7
    X, ti, td = cells_and_truth(100 + d, N, d, q_begin, q_count, cap)
    gis = q_begin + np.arange(q_count)
    rng = np.random.default_rng(1000 * d + ksel)
    nmax, c0, norm2, lin, E = allowance(X, gis, efrac * float(np.median(true_bw2(td, knn))), form)
    cnt = np.full(q_count, ksel, np.int32)
    cnt[3] = ksel + 5  # a row that holds more than ksel entries: only the first ksel are the list, slot ksel - 1 is still tau
    cnt[6] = max(knn + 2, ksel // 2)  # a short row with no published threshold: tau = inf, certified
    idx, d2 = make_lists(X, gis, ti, td, cnt, cap, E, rng, knn)
    c = make_case(X, q_begin, q_count, ksel, knn, decay, idx, d2, cnt, nmax, c0, norm2, lin)
    check_case(c, "values", min_certified=q_count // 4)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the certification boundary
# ---------------------------------------------------------------------------------------------------------------------------------
def _ulps(x, k):
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return x


@pytest.mark.parametrize("variant,d,ksel,knn,bw_scale", [("last_slot", 50, 64, 7, 1.0), ("last_slot", 7, 128, 7, 1.0), ("cand_thr", 7, 64, 7, 1.0),
                                                         ("last_slot_scale_below_1_over_rf", 52, 12, 7, 0.6), ("cand_thr", 302, 65, 3, 0.6)])
def test_certification_boundary(variant, d, ksel, knn, bw_scale):
    """tau 20 fp32 ulps above ``reach^2 + E`` certifies the row with the reference's values, 20 ulps below flags it (keep_cnt 0, a row
    of zeros) -- with tau the last slot of a full list or the published threshold of a short one, and with a bandwidth scale below
    1 / rf, where ``reach`` is the bandwidth entry and not the radius.  E is about 0.3 reach^2."""
    N, q_count, q_begin, decay, cap = 1500, 102, 8, 40.0, ksel + 7
    X, ti, td = cells_and_truth(200 + d, N, d, q_begin, q_count, cap)
    gis = q_begin + np.arange(q_count)
    rng = np.random.default_rng(d + ksel)
    rf = float(rr.radius_factor(decay, THRESH))
    bw2 = true_bw2(td, knn)
    reach2 = bw2 * LD(max(rf * bw_scale, 1.0)) ** 2
    nmax, c0, norm2, lin, E = allowance(X, gis, 0.3 * float(np.median(reach2)), "const")
    B = reach2 + E
    short = variant == "cand_thr"
    if short:  # a list cut at the threshold: everything below it, nothing else
        cnt = np.array([int(np.count_nonzero(td[q] <= B[q])) for q in range(q_count)], np.int32)
        assert np.all(cnt > knn) and np.all(cnt < ksel), (int(cnt.min()), int(cnt.max()))
    else:
        cnt = np.full(q_count, ksel, np.int32)
    idx, d2 = make_lists(X, gis, ti, td, cnt, cap, 0.1 * E, rng, knn)
    thr = np.zeros(q_count, np.float32) if short else None
    for q in range(q_count):
        t = _ulps(B[q], 20 if q % 2 == 0 else -20)
        n = int(cnt[q])
        if short:
            thr[q] = t
            d2[q, :n] = np.minimum(d2[q, :n], t)
        else:
            d2[q, :n] = np.minimum(d2[q, :n], t)  # (keeps the list sorted: its last slot IS the bound)
            d2[q, n - 1] = t
    c = make_case(X, q_begin, q_count, ksel, knn, decay, idx, d2, cnt, nmax, c0, norm2, lin, thr=thr, bw_scale=bw_scale)
    out, ref = check_case(c, variant)
    # which way each row falls is the reference's verdict, not the construction's -- and it must be the one constructed
    assert np.array_equal(ref["complete"], np.arange(q_count) % 2 == 0)
    assert np.all(np.abs(ref["margin"]) < 1e-5)
    assert np.all(out.keep_cnt[1::2] == 0) and np.all(out.val[1::2] == 0)
    if bw_scale == 1.0:  # (the bandwidth entry itself is kept: exp(-1))
        assert np.all(out.keep_cnt[0::2] >= knn)
    if bw_scale < 1.0 / rf:
        assert np.allclose((ref["reach2"] / (ref["bw"] * ref["bw"])).astype(np.float64), 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. lists that are wrong
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,ksel", [(7, 64), (50, 65)])
def test_incomplete_and_short_lists(d, ksel):
    """Row q % 3 == 0: a full list from which a true neighbour inside the radius was taken out, its last slot inside
    ``reach^2 + E`` -- flagged.  q % 3 == 1: a short list (n > knn) without a published threshold -- certified, tau is +inf.
    q % 3 == 2: n <= knn -- flagged, whatever tau.  With a given bandwidth the short lists of both kinds are certified."""
    N, q_count, q_begin, knn, decay, cap = 1500, 99, 0, 7, 40.0, ksel + 7
    X, ti, td = cells_and_truth(300 + d, N, d, q_begin, q_count, cap)
    gis = q_begin + np.arange(q_count)
    rng = np.random.default_rng(d)
    kind = np.arange(q_count) % 3
    # the allowance: the typical gap between the radius and the end of a full list, and half as much again
    rf2 = float(rr.radius_factor(decay, THRESH)) ** 2
    bw2 = true_bw2(td, knn)
    nmax, c0, norm2, lin, E = allowance(X, gis, 1.5 * max(float(np.median(td[:, ksel] - rf2 * bw2)), 0.05 * float(np.median(bw2))), "const")
    cnt = np.where(kind == 0, ksel, np.where(kind == 1, knn + 1 + (np.arange(q_count) % 9), np.arange(q_count) % knn + 1)).astype(np.int32)
    ti2, td2 = ti.copy(), td.copy()
    for q in np.nonzero(kind == 0)[0]:
        r = 1 + (q // 3) % knn  # the true neighbour of this rank goes missing (ranks 1 .. knn: inside the bandwidth)
        ti2[q, r:-1], td2[q, r:-1] = ti[q, r + 1:], td[q, r + 1:]
    idx, d2 = make_lists(X, gis, ti2, td2, cnt, cap, 0.05 * E, rng, knn)
    c = make_case(X, q_begin, q_count, ksel, knn, decay, idx, d2, cnt, nmax, c0, norm2, lin)
    out, ref = check_case(c, "wrong lists")
    want = kind == 1
    flagged_full = ~ref["complete"][kind == 0]
    assert flagged_full.sum() >= 20 and np.all(ref["margin"][kind == 0][flagged_full] <= -1e-6)
    assert np.array_equal(ref["complete"][kind != 0], want[kind != 0])
    # the same lists under a given bandwidth: nothing to read from the list, a short one is certified
    bwf = np.ones(N)
    bwf[gis] = np.sqrt(true_bw2(td, knn)).astype(np.float64) * rng.uniform(0.8, 1.2, size=q_count)
    c2 = make_case(X, q_begin, q_count, ksel, knn, decay, idx, d2, cnt, nmax, c0, norm2, lin, bw_fixed=bwf)
    out2, ref2 = check_case(c2, "wrong lists, given bandwidth")
    assert ref2["complete"][kind != 0].all()
    assert np.array_equal(out2.bw, bwf[gis])


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. ties
# ---------------------------------------------------------------------------------------------------------------------------------
TIE_KNN = 7


def _tie_edit(X):
    """Exact copies: (row, rank of the neighbour that gets a twin).  Row 23 gets nine copies of ITSELF (more than knn)."""
    X = X.copy()
    free = iter(range(1400, 1500))
    for row, rank in [(5, TIE_KNN - 1), (11, TIE_KNN), (17, 3), (29, 20), (41, TIE_KNN - 1), (53, 1)]:
        e = rr.exact_d2(X, row)
        j = np.lexsort((np.arange(X.shape[0]), e))[rank]
        X[next(free)] = X[j]
    for _ in range(TIE_KNN + 2):
        X[next(free)] = X[23]
    return X


@pytest.mark.parametrize("ksel", [64, 128])
@pytest.mark.parametrize("max_rank", [0, TIE_KNN + 1, TIE_KNN + 2])
def test_ties_are_ranked_by_index(ksel, max_rank):
    """Exact copies of cells inside a list: the twins share one distance and are ranked by index -- with the twin pair at ranks
    (knn - 1, knn), where a ranking by `<` alone leaves rank knn empty, at (knn, knn + 1), where a knn_max tells them apart, and
    elsewhere; in a list of 64 (the `<`-only ranking must notice the tie and hand over) and of 128.  A cell with more than knn
    copies of itself records DBL_EPSILON exactly: the copies get 1, the row itself and everything else 0."""
    N, d, q_count, q_begin, knn, decay, cap = 1500, 7, 63, 0, TIE_KNN, 40.0, ksel + 7
    X, ti, td = cells_and_truth(400, N, d, q_begin, q_count, cap, edit=_tie_edit)
    gis = q_begin + np.arange(q_count)
    rng = np.random.default_rng(ksel + max_rank)
    # the twins really sit where the test says
    for row, lo in [(5, knn - 1), (11, knn), (41, knn - 1), (17, 3)]:
        assert td[row, lo] == td[row, lo + 1] and ti[row, lo] < ti[row, lo + 1] and np.array_equal(X[ti[row, lo]], X[ti[row, lo + 1]])
    assert np.all(td[23, :knn + 3] == 0) and td[23, knn + 3] > 0
    nmax, c0, norm2, lin, E = allowance(X, gis, 0.05 * float(np.median(true_bw2(td, knn))), "const")
    cnt = np.full(q_count, ksel, np.int32)
    idx, d2 = make_lists(X, gis, ti, td, cnt, cap, E, rng, knn)
    c = make_case(X, q_begin, q_count, ksel, knn, decay, idx, d2, cnt, nmax, c0, norm2, lin, max_rank=max_rank)
    out, ref = check_case(c, "ties")
    assert ref["complete"][[5, 11, 17, 23, 41]].all()
    assert out.bw[23] == EPS
    copies = X[idx[23, :ksel]] == X[23]
    copies = copies.all(axis=1) & (idx[23, :ksel] != 23)
    assert copies.sum() == knn + 2
    want = np.where(copies, 1.0, 0.0)
    if max_rank:
        want[ref["rank"][23] >= max_rank] = 0.0
    assert np.array_equal(out.val[23], want)
    if max_rank == knn + 1:  # of the twins at ranks (knn, knn + 1) the lower index stays, the higher goes
        s_lo, s_hi = [int(np.nonzero(idx[11, :ksel] == ti[11, k])[0][0]) for k in (knn, knn + 1)]
        assert out.val[11, s_lo] > 0 and out.val[11, s_hi] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. max_rank, 6. a given bandwidth
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", [False, True])
def test_max_rank_certifies_what_it_keeps_and_no_more(given):
    """decay 2: the radius (3 bandwidths) lies far beyond a list of 16.  Row q % 2 == 0: the entry of rank max_rank - 1 is certified
    (d_m^2 + E <= tau) -- complete, ranks >= max_rank zero.  q % 2 == 1: the same construction with an allowance that puts that
    entry inside tau - E -- flagged.  With a GIVEN bandwidth the entry must also be no closer than the bandwidth: rows q % 4 == 2
    are handed a bandwidth beyond it and are flagged although the entry is certified."""
    N, d, q_count, q_begin, knn, decay, ksel, max_rank = 1500, 7, 98, 500, 7, 2.0, 16, 10
    cap = ksel + 7
    X, ti, td = cells_and_truth(500, N, d, q_begin, q_count, cap)
    gis = q_begin + np.arange(q_count)
    rng = np.random.default_rng(5 + given)
    # per-row allowance through the linear term alone: E_i = sqrt(norm2[i]) with norm2_max = 1, err_coef_lin = 1
    gap = td[:, ksel - 1] - td[:, max_rank - 1]  # room between the certified entry and the end of the list
    assert np.all(gap > 0)
    E = np.where(np.arange(q_count) % 2 == 0, 0.3 * gap, 1.7 * gap)
    norm2 = np.ones(N, np.float32)
    norm2[gis] = (E.astype(np.float64) ** 2).astype(np.float32)
    E = np.sqrt(norm2[gis].astype(LD))
    cnt = np.full(q_count, ksel, np.int32)
    idx, d2 = make_lists(X, gis, ti, td, cnt, cap, 0.2 * E, rng, knn)
    bwf = None
    if given:
        bwf = np.ones(N)
        d_m = np.sqrt(td[:, max_rank - 1]).astype(np.float64)
        bwf[gis] = np.where(np.arange(q_count) % 4 == 2, 1.1 * d_m, 0.9 * d_m)
    c = make_case(X, q_begin, q_count, ksel, knn, decay, idx, d2, cnt, np.float32(1.0), 0.0, norm2, 1.0, max_rank=max_rank, bw_fixed=bwf)
    out, ref = check_case(c, "max_rank")
    assert np.all(ref["margin"] < 0)  # no list reaches its radius: whatever is complete is so by the rank clause
    want = np.arange(q_count) % 2 == 0
    if given:
        want &= np.arange(q_count) % 4 != 2
    assert np.array_equal(ref["complete"], want)
    ok = ref["complete"]
    assert np.all(out.val[ok][ref["rank"][ok] >= max_rank] == 0) and np.all(out.keep_cnt[ok] == max_rank - 1)


@pytest.mark.parametrize("bw_scale", [0.6, 1.3])
@pytest.mark.parametrize("d", [7, 50])
def test_given_bandwidth_per_cell(d, bw_scale):
    """bw_fixed: the kernel uses max(given * scale, eps), records the given value unscaled, bit for bit."""
    N, q_count, q_begin, knn, decay, ksel = 1500, 97, 1403, 7, 40.0, 64
    cap = ksel + 7
    X, ti, td = cells_and_truth(600 + d, N, d, q_begin, q_count, cap)
    gis = q_begin + np.arange(q_count)
    rng = np.random.default_rng(d)
    nmax, c0, norm2, lin, E = allowance(X, gis, 0.02 * float(np.median(true_bw2(td, knn))), "lin")
    bwf = rng.uniform(0.5, 1.5, size=N)
    bwf[gis] = np.sqrt(true_bw2(td, knn)).astype(np.float64) * rng.uniform(0.8, 1.2, size=q_count)
    cnt = np.full(q_count, ksel, np.int32)
    idx, d2 = make_lists(X, gis, ti, td, cnt, cap, E, rng, knn)
    c = make_case(X, q_begin, q_count, ksel, knn, decay, idx, d2, cnt, nmax, c0, norm2, lin, bw_scale=bw_scale, bw_fixed=bwf)
    # (a radius of 1.3 * 1.057 bandwidths lies beyond most lists of 64 in 50 dimensions: those rows are compared as flagged ones)
    out, ref = check_case(c, "given bandwidth", min_certified=10 if bw_scale < 1 else 1, min_flagged=0 if bw_scale < 1 else 1)
    assert np.array_equal(out.bw, bwf[gis])


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. second-stage form
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,ksel", [(50, 64), (7, 128)])
def test_second_stage_form_writes_at_rows_only(d, ksel):
    """``rows``: candidate row q belongs to local row rows[q] (scattered, in no order).  bw / cand_val / keep_cnt change at those
    rows only, cand_idx_out (row stride out_cap > ksel) receives the list in list order and zeros behind n, its columns beyond ksel
    stay, and flag_rows holds LOCAL rows."""
    N, n_local, q_count, q_begin, knn, decay = 1500, 157, 37, 40, 7, 40.0
    cap, out_cap = ksel + 7, ksel + 9
    rows = np.random.default_rng(9).permutation(n_local)[:q_count].astype(np.int32)
    key = ("stage2", d, ksel)
    if key not in _TRUE:
        X = make_cells(np.random.default_rng(700 + d), N, d)
        _TRUE[key] = (X,) + rr.true_lists(X, q_begin, q_count, cap, rows=rows)
    X, ti, td = _TRUE[key]
    gis = q_begin + rows.astype(np.int64)
    rng = np.random.default_rng(d)
    nmax, c0, norm2, lin, E = allowance(X, gis, 0.01 * float(np.median(true_bw2(td, knn))), "lin")
    cnt = np.full(q_count, ksel, np.int32)
    cnt[::5] = np.arange(len(cnt[::5])) + knn - 2  # short rows on both sides of n = knn + 1
    idx, d2 = make_lists(X, gis, ti, td, cnt, cap, E, rng, knn)
    c = make_case(X, q_begin, q_count, ksel, knn, decay, idx, d2, cnt, nmax, c0, norm2, lin, rows=rows, out_cap=out_cap, n_local=n_local)
    out, ref = check_case(c, "second stage", min_certified=8, min_flagged=3)
    untouched = np.setdiff1d(np.arange(n_local), rows)
    assert np.all(out.bw[untouched] == SENT_BW) and np.all(out.val[untouched] == SENT_VAL) and np.all(out.keep_cnt[untouched] == SENT_CNT)
    assert np.all(out.idx_out[untouched] == SENT_IDX) and np.all(out.idx_out[:, ksel:] == SENT_IDX)
    for q, r in enumerate(rows):
        n = min(int(cnt[q]), ksel)
        assert np.array_equal(out.idx_out[r, :n], idx[q, :n]) and np.all(out.idx_out[r, n:ksel] == 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the exact sweep
# ---------------------------------------------------------------------------------------------------------------------------------
SWEEP_KNN = 7


def _sweep_edit(X):
    X = X.copy()
    X[2400:2410] = X[1237]  # ten copies of one of the swept rows: its bandwidth is eps
    return X


def run_sweep(X, q_begin, flag_rows, bw, knn, decay, thresh, bw_scale):
    """Count pass, then fill pass: (fb_cnt, err_flag, cursors after the count pass, per-row (cols, vals) or None)."""
    import torch

    from meld_amd._lib import check, get_lib, ptr
    from meld_amd.graph import _stream

    lib, dev, st = get_lib(), "cuda", _stream()
    N, d = X.shape
    Xd = torch.from_numpy(np.array(X, dtype=np.float64, order="C")).to(dev)
    fr = torch.from_numpy(np.asarray(flag_rows, np.int32)).to(dev)
    bwd = torch.from_numpy(np.ascontiguousarray(bw, dtype=np.float64)).to(dev)
    nf = len(flag_rows)
    fb_cnt = torch.full((nf,), 99, dtype=torch.int32, device=dev)  # (zeroed inside)
    cursor = torch.full((nf,), 99, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib.meld_knn_radius_exact(ptr(Xd), N, d, q_begin, ptr(fr), nf, ptr(bwd), knn, float(decay), float(thresh), 0, ptr(fb_cnt), None,
                                    ptr(cursor), None, None, ptr(err), float(bw_scale), st), "meld_knn_radius_exact(count)")
    torch.cuda.synchronize()
    cnt_h, cur_h, err_h = fb_cnt.cpu().numpy(), cursor.cpu().numpy(), int(err.item())
    filled = None
    if err_h == 0:
        off = np.concatenate([[0], np.cumsum(cnt_h)]).astype(np.int64)
        offd = torch.from_numpy(off).to(dev)
        col = torch.full((int(off[-1]) + 1,), -1, dtype=torch.int32, device=dev)
        val = torch.full((int(off[-1]) + 1,), -1.0, dtype=torch.float64, device=dev)
        check(lib.meld_knn_radius_exact(ptr(Xd), N, d, q_begin, ptr(fr), nf, ptr(bwd), knn, float(decay), float(thresh), 1, None, ptr(offd),
                                        ptr(cursor), ptr(col), ptr(val), None, float(bw_scale), st), "meld_knn_radius_exact(fill)")
        torch.cuda.synchronize()
        assert np.array_equal(cursor.cpu().numpy(), cnt_h)  # the fill pass found what the count pass counted
        assert int(col[-1]) == -1 and float(val[-1]) == -1.0  # and wrote nothing behind it
        col, val = col.cpu().numpy(), val.cpu().numpy()
        filled = []
        for f in range(nf):
            cc, vv = col[off[f]:off[f + 1]], val[off[f]:off[f + 1]]
            o = np.argsort(cc)
            filled.append((cc[o], vv[o]))
    return cnt_h, err_h, cur_h, filled


def _swept_rows_bandwidths(X, q_begin, rows, n_local, knn, decay):
    """The refinement's OWN bandwidths of the rows (complete lists, second-stage form), checked against the reference: what the
    sweep must confirm -- it counts the cells strictly closer in the same arithmetic, so the bandwidth entry itself never counts."""
    ksel = 64
    ti, td = rr.true_lists(X, q_begin, len(rows), ksel, rows=rows)
    cnt = np.full(len(rows), ksel, np.int32)
    c = make_case(X, q_begin, len(rows), ksel, knn, decay, ti.astype(np.int32), td.astype(np.float32), cnt, np.float32(1.0), 0.0,
                  rows=np.asarray(rows, np.int32), out_cap=ksel, n_local=n_local)
    ref = reference(c)
    out = run_refine(c)
    dev = np.abs(out.bw[rows].astype(LD) - ref["bw"]) / ref["bw"]
    assert float(dev.max()) <= bw_tol(X.shape[1])
    bw_ref = np.ones(n_local, LD)
    bw_ref[rows] = ref["bw"]
    bw_gpu = np.where(out.bw == SENT_BW, 1.0, out.bw)
    return bw_gpu, bw_ref


def _check_sweep(X, q_begin, rows, bw_gpu, bw_ref, knn, decay, bw_scale, label):
    d = X.shape[1]
    sw = rr.sweep_ref(X, q_begin, rows, bw_ref, knn, decay, THRESH, bw_scale)
    for r, s in zip(rows, sw):  # every one of the N references is decided
        used = max(bw_ref[r] * LD(bw_scale), LD(EPS))
        if math.isinf(decay):
            off = np.abs(s["dist"] / used - 1)
            assert np.all((off > 1e-10) | (s["dist"] == used)), r
        else:
            assert float(np.min(np.abs(s["v"] / LD(THRESH) - 1))) > 1e-6, r
        assert s["confirmed"] and (s["n_closer"] == knn or bw_ref[r] == LD(EPS))
    cnt, err, cur, filled = run_sweep(X, q_begin, rows, bw_gpu, knn, decay, THRESH, bw_scale)
    assert err == 0 and np.all(cur == 0)
    assert np.array_equal(cnt, [len(s["cols"]) for s in sw]), label
    worst = 0.0
    for f, (r, s) in enumerate(zip(rows, sw)):
        cols, vals = filled[f]
        assert np.array_equal(cols, s["cols"]) and (q_begin + r) not in cols, (label, r)
        if len(cols):
            dv = np.abs(vals.astype(LD) - s["vals"]) / s["vals"]
            worst = max(worst, float(dv.max()))
    assert worst <= val_tol(d, decay), (label, worst / U, val_tol(d, decay) / U)
    print("DEVIATION sweep {} d={} decay={} scale={} val {:.1f}u (bound {:.0f}u)".format(label, d, decay, bw_scale, worst / U, val_tol(d, decay) / U))
    return sw, cnt


@pytest.mark.parametrize("decay,bw_scale", [(40.0, 1.0), (math.inf, 1.0), (40.0, 0.6), (math.inf, 0.6)])
@pytest.mark.parametrize("d", [7, 50, 302])
def test_exact_sweep_counts_fills_and_verifies_the_bandwidth(d, decay, bw_scale):
    """13 rows (two workgroups, the second with five), 2500 references (three chunks of 1024, the last partial), q_begin > 0.
    Count pass: fb_cnt equals the reference's count under the refinement's own bandwidth, err_flag 0, cursors zero; a row at
    DBL_EPSILON with ten copies is accepted.  Fill pass: the (column, value) set of every row, the row itself absent.  Rows handed a
    bandwidth 1 % too large have more than knn cells strictly closer: fb_cnt -1, err_flag 1, the other rows unchanged."""
    N, q_begin, n_local, knn = 2500, 1000, 1200, SWEEP_KNN
    key = ("sweep", d)
    if key not in _TRUE:
        X = _sweep_edit(make_cells(np.random.default_rng(800 + d), N, d))
        X.setflags(write=False)
        _TRUE[key] = X
    X = _TRUE[key]
    others = np.setdiff1d(np.arange(1, 1100), [1237 - q_begin])
    rows = np.sort(np.concatenate([[1237 - q_begin, 0, n_local - 1], np.random.default_rng(d).permutation(others)[:10]])).astype(np.int32)
    assert len(rows) == 13 and len(set(rows.tolist())) == 13
    bw_gpu, bw_ref = _swept_rows_bandwidths(X, q_begin, rows, n_local, knn, 40.0)
    assert bw_gpu[1237 - q_begin] == EPS
    sw, cnt = _check_sweep(X, q_begin, rows, bw_gpu, bw_ref, knn, decay, bw_scale, "own bandwidth")
    # a bandwidth 1 % too large: the true bandwidth entry is now strictly closer
    big = bw_gpu.copy()
    bad = rows[rows != 1237 - q_begin][[1, 4, 8, 11]]
    assert 1237 - q_begin not in bad
    big[bad] *= 1.01
    ref_big = rr.sweep_ref(X, q_begin, bad, bw_ref * LD(1.01), knn, decay, THRESH, bw_scale)
    assert all(not s["confirmed"] and s["n_closer"] > knn for s in ref_big)
    cnt2, err2, cur2, _ = run_sweep(X, q_begin, rows, big, knn, decay, THRESH, bw_scale)
    assert err2 == 1 and np.all(cur2 == 0)
    isbad = np.isin(rows, bad)
    assert np.all(cnt2[isbad] == -1) and np.array_equal(cnt2[~isbad], cnt[~isbad])


def test_exact_sweep_of_wide_rows_raises_its_lds_limit():
    """d = 1100: eight rows of 1100 doubles are 70 400 bytes of dynamic LDS, beyond the 64 KB a launch gets without asking; the entry
    point raises the kernel's limit (gfx950 has 160 KB per workgroup) and the sweep is the reference's."""
    N, d, q_begin, n_local, knn = 1500, 1100, 100, 900, SWEEP_KNN
    X = make_cells(np.random.default_rng(1100), N, d)
    rows = np.array([0, 13, 444, 800, 899], np.int32)
    bw_gpu, bw_ref = _swept_rows_bandwidths(X, q_begin, rows, n_local, knn, 40.0)
    _check_sweep(X, q_begin, rows, bw_gpu, bw_ref, knn, 40.0, 1.0, "wide")


def test_exact_sweep_refuses_rows_beyond_the_lds_of_a_workgroup():
    """d = 2560: eight rows no longer fit the 160 KB of a workgroup.  Refused by the argument check, before anything is launched."""
    import torch

    from meld_amd._lib import get_lib, ptr

    lib = get_lib()
    one = torch.zeros(8, dtype=torch.float64, device="cuda")
    i32 = torch.zeros(8, dtype=torch.int32, device="cuda")
    rc = lib.meld_knn_radius_exact(ptr(one), 1, 2560, 0, ptr(i32), 1, ptr(one), 5, 40.0, 1e-4, 0, ptr(i32), None, ptr(i32), None, None, ptr(i32), 1.0, None)
    assert rc != 0 and b"meld_knn_radius_exact: d=2560" in lib.meld_last_error() and b"LDS" in lib.meld_last_error()
    torch.cuda.synchronize()
    assert lib.meld_knn_radius_exact(ptr(one), 1, 2559, 0, None, 1, ptr(one), 5, 40.0, 1e-4, 0, ptr(i32), None, ptr(i32), None, None, ptr(i32), 1.0, None) != 0
    assert b"bad arguments" in lib.meld_last_error()  # (d = 2559 passes the size check and stops at the next one)
