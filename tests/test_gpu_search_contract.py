"""Contract tests of the split-fp16 search stages (csrc/knn16.hip), every stage called directly and judged by the fp64 brute force of
tests/search_reference.py (tied to the oracle by tests/test_search_reference.py) -- never by another variant of itself.

The rest of the suite compares these stages with one another (pruned against unpruned, listed against table-driven, ...) and end to
end through the graph; an error all variants share -- an allowance that is too small, a bound that is no lower bound, a published
threshold that promises more than the row holds -- passes all of that.  Here every output is held against what it promises:

  operands   norm2, norm2_max, scale_info and Qn are the reference's to fp32 rounding (bounds: search_reference.check_operands)
  seeds      >= s^2 x the exact kernel radius^2 of the row; +inf for knn + 1 > 64
  table      every finite lb2[wave][tile] <= the exact minimum scaled d2 of the pair; +inf only on a pair that is not needed
  lists      no needed (wave, tile) pair lacks its bit, from any builder and after the partial filter; cnt >= 1; distinct tiles in
             scan order from the block's own position; work[b] = the list length
  rows       count in [1, ksel]; indices in range, distinct; sorted by (d2, index); |d2 - exact| <= E_row; every reference with exact
             d2 < tau - E_row present (tau = min(last entry of a full row, the threshold the row was searched under)); without
             seeds and cut every reference below (exact ksel-th) - 2 E_row; with the cut, on rows that are not full, every
             reference inside the exact kernel radius and cand_thr >= radius^2
  re-search  thr >= (tau + E1 + E3) s^2 in fp64, hence >= s^2 (exact ksel-th + E3); +inf on short lists; and not above it by more
             than RESEARCH_UPPER(d)

A pair is *needed* when some query p of the wave and reference r of the tile have s^2 d2(p, r) <= seed_p + s^2 E_p, with E_p the
per-row allowance c_const n_max + c_lin sqrt(n_p n_max) from the library's own coefficients.  None of the lower-bound and superset
contracts has any slack: the kernels document them as conservative.

RESEARCH_UPPER: knn16_research_thr_kernel forms (tau + e1 + e3) * (s * s) * (1.0 + 1e-5) in fp64 from fp32 inputs and rounds ONCE to
fp32.  Against the reference's exact n_i, n_max and s that is: the explicit factor 1e-5; one fp32 rounding of the result; two in
s^2 (s is the fp32 reciprocal of absmax, itself a cast: 2 x 2 u with the cast); (d + 12) u in each norm the allowances are made of
(search_reference.check_operands).  u = 2^-24: 1e-5 + (d + 12 + 4 + 1) u.

Found by these tests: the rows left knn16_finish_rows_kernel sorted by their RAW value; on the integer grid (three products) two raw
values that round to one stored d2 left with their indices descending.  The kernel now ranks by the stored value.

Cases and what each is the smallest shape for: search_reference.CASES.  Largest deviations seen on the MI355X: DESIGN.md section
4.2.1; each test prints its own (lines starting with SEARCH-CONTRACT).
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from tests import search_reference as sr

pytestmark = pytest.mark.gpu

LD = np.longdouble
RF = sr.RF
SKIP_CAP = 0.01  # share of (row, reference) decisions a check may leave undecided


def RESEARCH_UPPER(d):
    return 1e-5 + (d + 17) * 2.0 ** -24


def _accept(v, label):
    print("SEARCH-CONTRACT {}: margin {:.4g} skipped {:.3%}".format(label, v.margin, v.skipped))
    assert v.ok, (label, v)
    assert v.skipped <= SKIP_CAP, (label, v.skipped)
    return v


# ---------------------------------------------------------------------------------------------------------------------------------
# device side: one record per case, filled stage by stage and shared by the tests (nothing in it is modified after it is made)
# ---------------------------------------------------------------------------------------------------------------------------------
_DEV = {}


def _env():
    import torch

    from meld_amd._lib import check, get_lib, ptr
    from meld_amd.graph import _stream

    return torch, get_lib(), check, ptr, _stream()


def device_case(name):
    if name in _DEV:
        return _DEV[name]
    torch, lib, check, ptr, st = _env()
    c, X, mean, ref = sr.case_setup(name)
    g = SimpleNamespace(name=name, c=c, ref=ref, N=ref.N, d=ref.d, q_begin=ref.q_begin, q_count=ref.q_count, knn=c["knn"], ksel=c["ksel"])
    BQ, TS = lib.meld_knn16_block_queries(), lib.meld_knn16_tile_refs()
    assert (BQ, TS) == (sr.BLOCK, sr.WAVE)
    g.q_pad, g.n_tiles, g.n_blocks = -(-g.q_count // BQ) * BQ, -(-g.N // TS), -(-g.q_count // BQ)
    g.cap = lib.meld_knn16_row_capacity(g.ksel)
    assert g.cap > 0
    g.Xd = torch.from_numpy(X).cuda()
    g.mean = torch.from_numpy(np.ascontiguousarray(mean)).cuda()
    g.o = prepare(g, "plain")
    g.E = {p: ref.allowance(lib.meld_knn16_error_coef_const(p, g.d), lib.meld_knn16_error_coef_lin(p)) for p in (1, 3)}
    g.split = lib.meld_knn16_split_dims(g.d) > 0 and lib.meld_knn16_kblocks(g.d) >= 2
    g.full = g.q_begin == 0 and g.q_count == g.N
    g.cache = {}
    _DEV[name] = g
    return g


def prepare(g, how):
    torch, lib, check, ptr, st = _env()
    dev, d = "cuda", g.d
    o = SimpleNamespace()
    o.Rt = torch.empty(g.n_tiles * lib.meld_knn16_tile_bytes(d), dtype=torch.uint8, device=dev)
    o.Q = torch.empty(g.q_pad * lib.meld_knn16_query_bytes(d), dtype=torch.uint8, device=dev)
    o.Qn = torch.full((g.q_pad,), -1.0, dtype=torch.float32, device=dev)
    o.norm2 = torch.full((g.N,), -1.0, dtype=torch.float32, device=dev)
    o.nmax = torch.zeros(1, dtype=torch.float32, device=dev)
    o.sinfo = torch.empty(4, dtype=torch.float32, device=dev)
    o.spheres = None
    tail = (g.q_begin, g.q_count, ptr(o.Rt), ptr(o.Q), ptr(o.Qn), ptr(o.norm2), ptr(o.nmax), ptr(o.sinfo), st)
    if how == "plain":
        check(lib.meld_knn16_prepare(ptr(g.Xd), g.N, d, ptr(g.mean), *tail), "prepare")
    elif how == "scaled":
        lo, hi = g.Xd.min(dim=0).values.contiguous(), g.Xd.max(dim=0).values.contiguous()
        check(lib.meld_knn16_prepare_scaled(ptr(g.Xd), g.N, d, ptr(g.mean), ptr(lo), ptr(hi), *tail), "prepare_scaled")
    else:
        assert g.q_begin == 0 and g.q_count == g.N
        o.spheres = torch.empty(lib.meld_knn16_bounds_temp_bytes(g.N, d, g.N), dtype=torch.uint8, device=dev)
        check(lib.meld_knn16_prepare_fused(ptr(g.Xd), g.N, d, ptr(g.mean), None, None, ptr(o.Rt), ptr(o.Q), ptr(o.Qn), ptr(o.norm2), ptr(o.nmax),
                                           ptr(o.sinfo), ptr(o.spheres), st), "prepare_fused")
    torch.cuda.synchronize()
    return o


def seeds_of(g, knn, side=0):
    key = ("seeds", knn, side)
    if key not in g.cache:
        torch, lib, check, ptr, st = _env()
        o = g.o
        s = torch.full((g.q_pad,), -1.0, dtype=torch.float32, device="cuda")
        check(lib.meld_knn16_seed_thresholds_mfma(ptr(o.Q), ptr(o.Qn), ptr(o.Rt), ptr(o.sinfo), ptr(o.nmax), g.N, g.d, g.q_begin, g.q_count, knn, RF, 1,
                                                  side, ptr(s), st), "seeds")
        torch.cuda.synchronize()
        g.cache[key] = s
    return g.cache[key]


def needed_of(g, seeds, nprod):
    key = ("needed", id(seeds), nprod)
    if key not in g.cache:
        g.cache[key] = g.ref.needed(seeds.cpu().numpy().astype(np.float64), g.E[nprod]) if seeds is not None else (
            np.ones((g.ref.n_waves, g.n_tiles), bool), np.zeros((g.ref.n_waves, g.n_tiles), bool))
    return g.cache[key]


def table_of(g, seeds, nprod, how="bounds"):
    """lb2 [4 n_blocks][n_tiles] fp16 of meld_knn16_bounds, or of meld_knn16_tile_spheres (in two halves) +
    meld_knn16_bounds_from_spheres."""
    key = ("table", id(seeds), nprod, how)
    if key not in g.cache:
        torch, lib, check, ptr, st = _env()
        o = g.o
        tmp = torch.full((lib.meld_knn16_bounds_temp_bytes(g.N, g.d, g.q_count),), 0x5A, dtype=torch.uint8, device="cuda")
        lb2 = torch.full((lib.meld_knn16_bounds_bytes(g.N, g.q_count) // 2,), -1.0, dtype=torch.float16, device="cuda")
        assert lb2.numel() == 4 * g.n_blocks * g.n_tiles
        args = (ptr(g.Xd), g.N, g.d, ptr(g.mean), ptr(o.sinfo), ptr(o.nmax), ptr(o.Rt), g.q_begin, g.q_count, ptr(seeds),
                ptr(o.Qn) if seeds is not None else None, nprod)
        if how == "bounds":
            check(lib.meld_knn16_bounds(*args, ptr(tmp), ptr(lb2), st), "bounds")
        else:
            tmp.zero_()
            half = g.n_tiles // 2
            for t0, n in ((half, g.n_tiles - half), (0, half)):
                check(lib.meld_knn16_tile_spheres(ptr(g.Xd), g.N, g.d, ptr(g.mean), ptr(o.sinfo), ptr(tmp), t0, n, st), "tile_spheres")
            check(lib.meld_knn16_bounds_from_spheres(*args, ptr(tmp), ptr(lb2), st), "bounds_from_spheres")
        torch.cuda.synchronize()
        g.cache[key] = lb2
    return g.cache[key]


def lists_of(g, seeds, nprod, how):
    """(list [n_blocks][n_tiles] int32, cnt [n_blocks]) from: "table" (meld_knn16_bounds + meld_knn16_step_lists), "direct",
    "lead0", "lead1" (meld_knn16_step_lists_direct[_lead]), "spheres0", "spheres1" (meld_knn16_prepare_fused +
    meld_knn16_step_lists_direct_spheres); + "+filter": thinned by meld_knn16_partial_filter."""
    key = ("lists", id(seeds), nprod, how)
    if key in g.cache:
        return g.cache[key]
    torch, lib, check, ptr, st = _env()
    o = g.o
    if how.endswith("+filter"):
        lst, cnt = lists_of(g, seeds, nprod, how[:-7])
        lst, cnt = lst.clone(), cnt.clone()
        tested = torch.zeros(4, dtype=torch.int64, device="cuda")
        check(lib.meld_knn16_partial_filter(ptr(o.Q), ptr(o.Qn), ptr(o.Rt), ptr(o.sinfo), ptr(o.nmax), g.d, g.q_count, ptr(seeds), ptr(lst), ptr(cnt),
                                            g.n_tiles, ptr(cnt), ptr(tested), None, st), "partial_filter")
    else:
        lst = torch.full((g.n_blocks * g.n_tiles,), -1, dtype=torch.int32, device="cuda")
        cnt = torch.full((g.n_blocks,), -1, dtype=torch.int32, device="cuda")
        if how == "table":
            lb2 = table_of(g, seeds, nprod)
            check(lib.meld_knn16_step_lists(ptr(lb2), ptr(seeds), g.N, g.d, g.q_count, nprod, ptr(o.nmax), ptr(o.sinfo), g.q_begin, ptr(lst), g.n_tiles,
                                            ptr(cnt), st), "step_lists")
        else:
            assert g.full
            scratch = torch.empty(lib.meld_knn16_list_scratch_bytes(g.N), dtype=torch.uint8, device="cuda")
            src = o
            if how.startswith("spheres"):
                key_f = ("fused",)
                if key_f not in g.cache:
                    g.cache[key_f] = prepare(g, "fused")
                src = g.cache[key_f]
                tmp = src.spheres
            else:
                tmp = torch.full((lib.meld_knn16_bounds_temp_bytes(g.N, g.d, g.N),), 0x5A, dtype=torch.uint8, device="cuda")
            head = (ptr(g.Xd), g.N, g.d, ptr(g.mean), ptr(src.sinfo), ptr(src.nmax), ptr(src.Rt), ptr(seeds), ptr(src.Qn), nprod, ptr(tmp), ptr(scratch),
                    ptr(lst), g.n_tiles, ptr(cnt))
            if how == "direct":
                check(lib.meld_knn16_step_lists_direct(*head, st), how)
            elif how.startswith("lead"):
                check(lib.meld_knn16_step_lists_direct_lead(*head, int(how[-1]), st), how)
            else:
                check(lib.meld_knn16_step_lists_direct_spheres(*head, int(how[-1]), st), how)
    torch.cuda.synchronize()
    g.cache[key] = (lst, cnt)
    return g.cache[key]


def block_order_of(g, permuted):
    if not permuted:
        return None
    key = ("order",)
    if key not in g.cache:
        import torch

        g.cache[key] = torch.from_numpy(np.random.default_rng(5).permutation(g.n_blocks).astype(np.int32)).cuda()
    return g.cache[key]


def run_search(g, entry, nprod=1, lb2=None, seeds=None, cut=False, publish=False, slices=1, lists=None, partial=0, order=None):
    """One search launch (+ merge of slices, + meld_knn16_finish_rows behind the raw entry point): (idx, d2, cnt, thr or None) on the
    host, rows [q_pad][cap].  The buffers start as poison: index -7, d2 NaN, count -3."""
    torch, lib, check, ptr, st = _env()
    o, S, q_pad, cap = g.o, slices, g.q_pad, g.cap
    idx = torch.full((S * q_pad * cap,), -7, dtype=torch.int32, device="cuda")
    d2 = torch.full((S * q_pad * cap,), float("nan"), dtype=torch.float32, device="cuda")
    cnt = torch.full((S * q_pad,), -3, dtype=torch.int32, device="cuda")
    thr = torch.full((S, q_pad), float("inf"), dtype=torch.float32, device="cuda") if (cut or publish) else None
    done = torch.zeros(4, dtype=torch.int64, device="cuda")
    knn = g.knn if cut else 0
    head = (ptr(o.Q), ptr(o.Qn), ptr(o.Rt), ptr(o.sinfo), g.N, g.d, g.q_count, g.ksel)
    mid = (ptr(o.nmax), g.q_begin, ptr(seeds), knn, RF, ptr(idx), ptr(d2), ptr(cnt), ptr(thr), ptr(done), ptr(order))
    if entry == "topk":
        check(lib.meld_knn16_topk(*head, nprod, S, ptr(lb2), *mid, st), entry)
    else:
        lst, lcnt = lists
        lhead = head + (ptr(lst), ptr(lcnt), g.n_tiles)
        if entry == "listed":
            check(lib.meld_knn16_topk_listed(*lhead, *mid, S, st), entry)
        elif entry == "partial":
            check(lib.meld_knn16_topk_listed_partial(*lhead, *mid, S, partial, st), entry)
        else:
            assert S == 1
            check(lib.meld_knn16_topk_listed_raw(*lhead, *mid, partial, st), entry)
            check(lib.meld_knn16_finish_rows(ptr(d2), ptr(idx), ptr(cnt), ptr(o.Qn), ptr(o.sinfo), q_pad, g.ksel, st), "finish_rows")
    if S > 1:
        mi = torch.full((q_pad * cap,), -7, dtype=torch.int32, device="cuda")
        md = torch.full((q_pad * cap,), float("nan"), dtype=torch.float32, device="cuda")
        mc = torch.full((q_pad,), -3, dtype=torch.int32, device="cuda")
        check(lib.meld_knn16_merge_slices(ptr(idx), ptr(d2), ptr(cnt), g.q_count, g.ksel, S, ptr(mi), ptr(md), ptr(mc), st), "merge_slices")
        idx, d2, cnt = mi, md, mc
    torch.cuda.synchronize()  # (padding rows beyond q_count are searched like any other: the call must come back clean)
    thr_h = None if thr is None else thr.amin(0).cpu().numpy()
    return idx.view(q_pad, cap).cpu().numpy(), d2.view(q_pad, cap).cpu().numpy(), cnt.cpu().numpy(), thr_h


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. operands and seeds
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sr.CASES))
def test_operands_and_seeds(name):
    torch, lib, check, ptr, st = _env()
    g = device_case(name)
    ref = g.ref
    for how in ("plain", "scaled") + (("fused",) if g.full else ()):
        o = g.o if how == "plain" else prepare(g, how)
        _accept(sr.check_operands(ref, o.norm2.cpu().numpy(), float(o.nmax.item()), o.sinfo.cpu().numpy(), o.Qn.cpu().numpy()), name + " operands " + how)
        # padding queries repeat the last one
        assert bool((o.Qn[g.q_count:] == o.Qn[g.q_count - 1]).all())
    # the row-list form: local rows in no order, one of them twice
    rows = np.random.default_rng(1).permutation(g.q_count)[:min(70, g.q_count)].astype(np.int32)
    rows[-1] = rows[0]
    rd = torch.from_numpy(rows).cuda()
    rp = -(-len(rows) // sr.BLOCK) * sr.BLOCK
    Q2 = torch.empty(rp * lib.meld_knn16_query_bytes(g.d), dtype=torch.uint8, device="cuda")
    Qn2 = torch.full((rp,), -1.0, dtype=torch.float32, device="cuda")
    check(lib.meld_knn16_prepare_rows(ptr(g.Xd), g.N, g.d, ptr(g.mean), ptr(g.o.sinfo), g.q_begin, ptr(rd), len(rows), ptr(Q2), ptr(Qn2), st), "prepare_rows")
    torch.cuda.synchronize()
    assert torch.equal(Qn2[:len(rows)], g.o.Qn[rd.long()])  # the same chain on the same values: the same bits
    # seeds: the case's knn with the automatic neighbourhood and with one wider than the data; knn + 1 = 63, 64 and 65
    for knn, side in ((g.knn, 0), (g.knn, 64), (min(62, g.N - 2), 2), (min(63, g.N - 2), 64)):
        s = seeds_of(g, knn, side).cpu().numpy()
        assert not np.isnan(s).any() and bool((s[g.q_count:] >= 0).all())
        v = _accept(sr.check_seeds(ref, s, knn, RF), "{} seeds knn={} side={}".format(name, knn, side))
    s = seeds_of(g, 64, 0).cpu().numpy()
    assert np.isposinf(s).all() and len(s) == g.q_pad


def test_cross_operands():
    """meld_knn16_prepare_cross: references [0, n_refs), queries the rows behind them, scale and norms over all rows -- norm2 and
    norm2_max in input units for both sets, Qn in scaled units."""
    torch, lib, check, ptr, st = _env()
    n_refs, n_total, d = 300, 453, 23
    X = sr.make_data("noise", n_total, d, 21)
    X[n_refs + 7] *= 3.0  # the largest norm is a query's
    mean = X.mean(axis=0)
    ref = sr.Setup(X, mean, n_refs, n_total - n_refs)
    assert int(np.argmax(ref.n)) == n_refs + 7
    Xd, md = torch.from_numpy(X).cuda(), torch.from_numpy(mean).cuda()
    q_pad, n_tiles = -(-ref.q_count // sr.BLOCK) * sr.BLOCK, -(-n_refs // sr.WAVE)
    Rt = torch.empty(n_tiles * lib.meld_knn16_tile_bytes(d), dtype=torch.uint8, device="cuda")
    Q = torch.empty(q_pad * lib.meld_knn16_query_bytes(d), dtype=torch.uint8, device="cuda")
    Qn = torch.full((q_pad,), -1.0, dtype=torch.float32, device="cuda")
    norm2 = torch.full((n_total,), -1.0, dtype=torch.float32, device="cuda")
    nmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    sinfo = torch.empty(4, dtype=torch.float32, device="cuda")
    check(lib.meld_knn16_prepare_cross(ptr(Xd), n_refs, n_total, d, ptr(md), n_refs, ref.q_count, ptr(Rt), ptr(Q), ptr(Qn), ptr(norm2), ptr(nmax),
                                       ptr(sinfo), st), "prepare_cross")
    torch.cuda.synchronize()
    _accept(sr.check_operands(ref, norm2.cpu().numpy(), float(nmax.item()), sinfo.cpu().numpy(), Qn.cpu().numpy()), "cross operands")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. bounds and lists
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sr.CASES))
def test_bounds_table(name):
    torch, lib, check, ptr, st = _env()
    g = device_case(name)
    ref = g.ref
    rows, row_bytes = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib.meld_knn16_sphere_layout(g.N, g.d, ctypes.byref(rows), ctypes.byref(row_bytes)), "sphere_layout")
    assert rows.value >= g.n_tiles and rows.value * (row_bytes.value + 8) + 256 == lib.meld_knn16_bounds_temp_bytes(g.N, g.d, g.q_count)
    assert row_bytes.value == lib.meld_knn16_query_bytes(g.d)
    seeds = seeds_of(g, g.knn)
    for nprod in (1, 3):
        need, und = needed_of(g, seeds, nprod)
        for how in ("bounds", "spheres"):
            lb = table_of(g, seeds, nprod, how).view(4 * g.n_blocks, g.n_tiles).float().cpu().numpy()
            v = _accept(sr.check_bounds(ref, lb, need, und), "{} table {} nprod={} seeded".format(name, how, nprod))
            if g.c["kind"] == "clusters":
                assert np.isposinf(lb[:ref.n_waves]).mean() >= 0.30  # the table really rules pairs out
    for how in ("bounds", "spheres"):
        lb = table_of(g, None, 1, how).view(4 * g.n_blocks, g.n_tiles).float().cpu().numpy()
        _accept(sr.check_bounds(ref, lb), "{} table {} unseeded".format(name, how))
        assert np.isfinite(lb[:ref.n_waves]).all()


@pytest.mark.parametrize("name", list(sr.CASES))
def test_step_lists_hold_every_needed_pair(name):
    torch, lib, check, ptr, st = _env()
    g = device_case(name)
    ref = g.ref
    seeds = seeds_of(g, g.knn)
    hows = ["table"] + (["direct", "lead0", "lead1", "spheres0", "spheres1"] if g.full else [])
    for nprod in (1, 3):
        need, und = needed_of(g, seeds, nprod)
        if g.c["kind"] == "clusters":
            assert (~need).mean() >= 0.30, (~need).mean()
        lb2 = table_of(g, seeds, nprod)
        work = torch.full((g.n_blocks,), -1, dtype=torch.int32, device="cuda")
        check(lib.meld_knn16_block_work(ptr(lb2), ptr(seeds), g.N, g.d, g.q_count, nprod, ptr(g.o.nmax), ptr(g.o.sinfo), ptr(work), st), "block_work")
        torch.cuda.synchronize()
        for how in hows:
            lst, cnt = lists_of(g, seeds, nprod, how)
            v = _accept(sr.check_lists(ref, lst.cpu().numpy(), cnt.cpu().numpy(), g.n_tiles, need, und, work=work.cpu().numpy() if how == "table" else None),
                        "{} lists {} nprod={} (margin: share of pairs left out)".format(name, how, nprod))
            if g.c["kind"] == "clusters":
                assert v.margin > 0.30, (how, v.margin)  # the lists really drop pairs
            if g.split and nprod == 1:
                lst, cnt = lists_of(g, seeds, nprod, how + "+filter")
                v2 = _accept(sr.check_lists(ref, lst.cpu().numpy(), cnt.cpu().numpy(), g.n_tiles, need, und, thinned=True),
                             "{} lists {} after the partial filter".format(name, how))
                assert v2.margin >= v.margin
    # without seeds every pair is needed: the table-driven lists hold every tile for every wave that has a cell
    need, und = needed_of(g, None, 1)
    lb2 = table_of(g, None, 1)
    lst = torch.full((g.n_blocks * g.n_tiles,), -1, dtype=torch.int32, device="cuda")
    cnt = torch.full((g.n_blocks,), -1, dtype=torch.int32, device="cuda")
    work = torch.full((g.n_blocks,), -1, dtype=torch.int32, device="cuda")
    check(lib.meld_knn16_step_lists(ptr(lb2), None, g.N, g.d, g.q_count, 1, ptr(g.o.nmax), ptr(g.o.sinfo), g.q_begin, ptr(lst), g.n_tiles, ptr(cnt), st), "step_lists")
    check(lib.meld_knn16_block_work(ptr(lb2), None, g.N, g.d, g.q_count, 1, ptr(g.o.nmax), ptr(g.o.sinfo), ptr(work), st), "block_work")
    torch.cuda.synchronize()
    _accept(sr.check_lists(ref, lst.cpu().numpy(), cnt.cpu().numpy(), g.n_tiles, need, und, work=work.cpu().numpy()), name + " lists table unseeded")
    assert bool((cnt == g.n_tiles).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the search
# ---------------------------------------------------------------------------------------------------------------------------------
# variant: entry point, nprod, table, seeds, cut, publish, slices, lists, partial
SEARCHES = {
    "topk1": ("topk", 1, None, False, False, False, 1, None, 0),
    "topk3": ("topk", 3, None, False, False, False, 1, None, 0),
    "topk3_table": ("topk", 3, "unseeded", False, False, False, 1, None, 0),
    "topk1_seeds": ("topk", 1, None, True, False, False, 1, None, 0),
    "topk1_seeds_published": ("topk", 1, None, True, False, True, 1, None, 0),
    "topk1_table_seeds_cut": ("topk", 1, "seeded", True, True, False, 1, None, 0),
    "topk3_table_seeds_cut": ("topk", 3, "seeded", True, True, False, 1, None, 0),
    "topk3_seeds_cut_slices": ("topk", 3, None, True, True, False, 3, None, 0),
    "topk1_table_cut_slices": ("topk", 1, "seeded", True, True, False, 3, None, 0),
    "listed_cut": ("listed", 1, None, True, True, False, 1, "table", 0),
    "listed_slices": ("listed", 1, None, True, False, True, 3, "table", 0),
    "partial0_cut": ("partial", 1, None, True, True, False, 1, "direct", 0),
    "partial1_cut": ("partial", 1, None, True, True, False, 1, "lead1", 1),
    "partial1_cut_slices": ("partial", 1, None, True, True, False, 3, "table", 1),
    "raw0_cut": ("raw", 1, None, True, True, False, 1, "spheres0", 0),
    "raw1_filtered_cut": ("raw", 1, None, True, True, False, 1, "table+filter", 1),
}


@pytest.mark.parametrize("variant", list(SEARCHES))
@pytest.mark.parametrize("name", list(sr.CASES))
def test_search_rows(name, variant):
    entry, nprod, table, seeded, cut, publish, slices, lists, partial = SEARCHES[variant]
    g = device_case(name)
    ref = g.ref
    seeds = seeds_of(g, g.knn) if seeded else None
    lb2 = None if table is None else table_of(g, seeds if table == "seeded" else None, nprod)
    if lists is not None:
        if not g.full and lists.split("+")[0] != "table":
            lists = "table"  # (the direct builders take all the cells as queries)
        if lists.endswith("+filter") and not g.split:
            lists = lists[:-7]
        lists = lists_of(g, seeds, 1, lists)
    S = min(slices, g.n_tiles)
    E = g.E[nprod]
    s2 = LD(ref.s) * LD(ref.s)
    for permuted in (False, True):
        idx, d2, cnt, thr = run_search(g, entry, nprod, lb2, seeds, cut, publish, S, lists, partial, block_order_of(g, permuted))
        if thr is None and seeds is not None:  # searched under its start threshold, nothing published
            thr = (seeds.cpu().numpy()[:g.q_count].astype(LD) / s2)
        v = sr.check_rows(ref, idx, d2, cnt, g.ksel, E, thr=thr, exact_rule=not seeded and not cut,
                          radius2=ref.radius2(g.knn, RF) if cut else None)
        _accept(v, "{} {}{} (margin: |d2 - exact| / E_row; rows short of ksel: {:.1%})".format(
            name, variant, " permuted" if permuted else "", float((cnt[:g.q_count] < g.ksel).mean())))
        if cut and S == 1 and (name == "duplicates" or (name == "clusters" and nprod == 3)):
            # the cut engaged, so the radius clause above was not vacuous.  The host condition (test_search_reference.py) has
            # 97 % of the clusters' rows with fewer than ksel references inside rf^2 (A + E) + 2 E; the kernel cuts at
            # rf^2 (A~ + E) + E with A~ <= A + E, which lies (rf^2 - 1) E = 0.12 E beyond that: most rows, not all of the 97 %
            assert (cnt[:g.q_count] < g.ksel).mean() >= 0.50


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. start thresholds of the re-search
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sr.CASES))
def test_research_thresholds(name):
    torch, lib, check, ptr, st = _env()
    g = device_case(name)
    ref, o = g.ref, g.o
    e3 = lib.meld_knn16_error_coef(3, g.d)
    rows = np.random.default_rng(2).permutation(g.q_count)[:min(g.q_count, 300)].astype(np.int32)
    rd = torch.from_numpy(rows).cuda()
    rp = -(-len(rows) // sr.BLOCK) * sr.BLOCK
    passes = [("plain", run_search(g, "topk", 1))]
    seeds = seeds_of(g, g.knn)
    passes.append(("cut", run_search(g, "topk", 1, None, seeds, True)))
    n_inf = 0
    for label, (idx, d2, cnt, _) in passes:
        thr = torch.full((rp,), -1.0, dtype=torch.float32, device="cuda")
        d2d, cntd = torch.from_numpy(d2).cuda(), torch.from_numpy(cnt).cuda()
        check(lib.meld_knn16_research_thresholds(ptr(rd), len(rows), g.q_begin, ptr(cntd), ptr(d2d), g.cap, g.ksel, ptr(o.norm2), ptr(o.nmax),
                                                 lib.meld_knn16_error_coef_const(1, g.d), lib.meld_knn16_error_coef_lin(1), e3, ptr(o.sinfo), ptr(thr), st),
              "research_thresholds")
        torch.cuda.synchronize()
        t = thr.cpu().numpy()
        assert np.all(t[len(rows):] == t[len(rows) - 1])  # padding rows copy the last row's value
        _accept(sr.check_research(ref, rows, t, d2, cnt, g.ksel, g.E[1], e3, RESEARCH_UPPER(g.d)),
                "{} re-search thresholds after the {} pass (margin: thr / documented - 1)".format(name, label))
        n_inf += int(np.isposinf(t[:len(rows)]).sum())
        if label == "plain":
            assert np.all(cnt[:g.q_count] == g.ksel) and np.isfinite(t).all()
    if g.c["kind"] in ("duplicates", "grid"):
        assert n_inf > 0  # short first lists occurred
