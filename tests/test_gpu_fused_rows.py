"""The fused row pass behind the search (``KnnPlan.fused_rows``: ``meld_knn_refine_emit`` on finished rows, ``meld_knn_refine_sort_emit``
on the raw rows of ``meld_knn16_topk_listed_raw``, ``meld_coo_emit_scatter_listed`` for what they leave out) against the three kernels
it replaces on the single-GPU route (finish -> refinement -> ``meld_coo_emit_scatter``): only the order of the entries inside a row
bucket differs, which ``meld_csr_rows_sort_merge`` does not depend on, so everything behind the buckets is compared BIT FOR BIT -- no
tolerance anywhere in this file.  The routes are forced through the development switch ``MELD_ROWS_FUSED`` = 0 | a | b
(tests/conftest.py sets ``MELD_DEV=1``)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import meld_oracle as mo
from tests import test_gpu_refine_contract as rc

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. kernel contract: candidate rows made on the host, handed straight to the entry points
# ---------------------------------------------------------------------------------------------------------------------------------
def _merge(lib, cursor, tcol, tval, n, symm):
    """meld_csr_rows_sort_merge_sums on the buckets; (ucnt, row sums, flags, merged heads of every bucket)."""
    from meld_amd._lib import check, ptr
    from meld_amd.graph import _stream

    B = int(lib.meld_csr_bucket_slots())
    ucnt = torch.empty(n, dtype=torch.int32, device="cuda")
    flags = torch.empty(1, dtype=torch.int32, device="cuda")
    sums = torch.empty(n, dtype=torch.float64, device="cuda")
    check(lib.meld_csr_rows_sort_merge_sums(ptr(cursor), n, ptr(tcol), ptr(tval), ptr(ucnt), ptr(flags), symm, 0.7, 1.0, ptr(sums), _stream()), "merge")
    torch.cuda.synchronize()
    u = ucnt.cpu().numpy()
    live = np.arange(B)[None, :] < u[:, None]
    return u, sums.cpu().numpy(), int(flags.item()), tcol.cpu().numpy().reshape(n, B)[live], tval.cpu().numpy().reshape(n, B)[live]


def _raw_rows(c, rng):
    """The case's finished lists as the RAW rows the search leaves: two half-rows of n0 and n1 unsorted entries, values
    v = d2 / s - |q|^2 (fp32), cnt = n0 | n1 << 16.  Rows take turns at an even split, an empty first and an empty second half-row
    (where the list fits one); every 7th row gets three equal values (ties, broken by index) and every 11th a -0.0 next to a +0.0."""
    n, cap, half = c.q_count, c.cap, c.cap // 2
    s1 = np.float32(0.25)
    Qn = rng.uniform(0.5, 4.0, size=n).astype(np.float32)
    idx, v, cnt = np.zeros((n, cap), np.int32), np.zeros((n, cap), np.float32), np.zeros(n, np.int32)
    split = []
    for q in range(n):
        L = int(c.cnt[q])
        vals = (c.d2[q, :L] / s1 - Qn[q]).astype(np.float32)
        if q % 7 == 0 and L >= 6:
            vals[3:6] = vals[3]
        if q % 11 == 0 and L >= 3:
            vals[1], vals[2] = np.float32(-0.0), np.float32(0.0)
        o = rng.permutation(L)
        n0 = {0: (L + 1) // 2, 1: 0 if L <= half else L - half, 2: L if L <= half else half}[q % 3]
        split.append((n0, L - n0))
        idx[q, :n0], v[q, :n0] = c.idx[q, :L][o[:n0]], vals[o[:n0]]
        idx[q, half:half + L - n0], v[q, half:half + L - n0] = c.idx[q, :L][o[n0:]], vals[o[n0:]]
        cnt[q] = n0 | ((L - n0) << 16)
    return idx, v, cnt, Qn, np.array([1.0, s1], np.float32), split


def _three_routes(c, raw, symm):
    """The raw rows through finish -> refinement -> emit + scatter -> merge ("legacy"), finish -> emitting refinement -> merge
    ("emit") and the ranking + emitting refinement -> merge ("sort+emit")."""
    from meld_amd._lib import check, get_lib, ptr
    from meld_amd.graph import _stream

    lib, dev, n = get_lib(), "cuda", c.q_count
    B = int(lib.meld_csr_bucket_slots())
    t = lambda a, dt: None if a is None else torch.from_numpy(np.array(a, dtype=dt, order="C")).to(dev)
    X, norm2, nmax = t(c.X, np.float64), t(c.norm2, np.float32), t(np.array([c.nmax]), np.float32)
    Qn, sinfo = t(raw[3], np.float32), t(raw[4], np.float32)
    out = {}
    for route in ("legacy", "emit", "sort+emit"):
        idx, d2, cnt = t(raw[0], np.int32), t(raw[1], np.float32), t(raw[2], np.int32)
        bw = torch.full((n,), rc.SENT_BW, dtype=torch.float64, device=dev)
        keep = torch.full((n,), rc.SENT_CNT, dtype=torch.int32, device=dev)
        flag_rows = torch.full((n,), -1, dtype=torch.int32, device=dev)
        n_flag = torch.zeros(1, dtype=torch.int32, device=dev)
        tcol = torch.full((n * B,), -1, dtype=torch.int32, device=dev)
        tval = torch.full((n * B,), -1.0, dtype=torch.float64, device=dev)
        cursor = torch.full((n,), 77, dtype=torch.int32, device=dev)  # (the emitting entry points clear it)
        tail = (c.ksel, c.cap, c.knn, float(c.decay), float(c.thresh), ptr(nmax), c.err_coef, ptr(norm2), c.err_lin, ptr(bw), ptr(keep), ptr(flag_rows),
                ptr(n_flag), float(c.bw_scale), None, c.max_rank, ptr(cursor), ptr(tcol), ptr(tval), _stream())
        if route != "sort+emit":
            check(lib.meld_knn16_finish_rows(ptr(d2), ptr(idx), ptr(cnt), ptr(Qn), ptr(sinfo), n, c.ksel, _stream()), "meld_knn16_finish_rows")
        if route == "legacy":
            val = torch.full((n, c.ksel), rc.SENT_VAL, dtype=torch.float64, device=dev)
            check(lib.meld_knn_refine(ptr(X), n, c.d, 0, n, ptr(idx), ptr(d2), ptr(cnt), None, c.ksel, c.cap, c.knn, float(c.decay), float(c.thresh),
                                      ptr(nmax), c.err_coef, ptr(norm2), c.err_lin, ptr(bw), ptr(val), ptr(keep), ptr(flag_rows), ptr(n_flag), None, 0, None,
                                      float(c.bw_scale), None, c.max_rank, _stream()), "meld_knn_refine")
            cursor = keep.clone()
            check(lib.meld_coo_emit_scatter(n, ptr(idx), ptr(val), c.ksel, c.cap, ptr(keep), ptr(flag_rows), 0, None, None, None, 0, ptr(cursor), ptr(tcol),
                                            ptr(tval), _stream()), "meld_coo_emit_scatter")
        elif route == "emit":
            check(lib.meld_knn_refine_emit(ptr(X), n, c.d, ptr(idx), ptr(d2), ptr(cnt), None, *tail), "meld_knn_refine_emit")
        else:
            check(lib.meld_knn_refine_sort_emit(ptr(X), n, c.d, ptr(idx), ptr(d2), ptr(cnt), ptr(Qn), ptr(sinfo), None, *tail), "meld_knn_refine_sort_emit")
        torch.cuda.synchronize()
        nf = int(n_flag.item())
        out[route] = SimpleNamespace(bw=bw.cpu().numpy(), keep=keep.cpu().numpy(), flagged=set(flag_rows[:nf].cpu().tolist()), n_flag=nf,
                                     cursor=cursor.cpu().numpy(), merged=_merge(lib, cursor, tcol, tval, n, symm),
                                     idx=idx.cpu().numpy().reshape(n, c.cap), d2=d2.cpu().numpy().reshape(n, c.cap), cnt=cnt.cpu().numpy())
    return out


LENGTHS = lambda knn, cap: [0, 1, knn, knn + 1, 63, 64, 65, 127, 128, 129, cap - 1]


@pytest.mark.parametrize("d", [2, 10, 50])
@pytest.mark.parametrize("knn", [5, 15])
def test_fused_row_passes_fill_the_buckets_of_the_three_kernels(d, knn):
    """Raw candidate rows of every length around the places where the kernels change their path (an empty row, one without a
    bandwidth entry, the three widths of the sorting network, one and two entries per lane, more entries than ksel; half-rows even
    and one-sided; ties; -0.0 against +0.0) on a few hundred cells: the buckets after the merge, their lengths, the row sums, the
    bandwidths and keep_cnt bit for bit, the flagged rows as a set, and the rows written back for the flagged ones equal to the
    finish kernel's."""
    from meld_amd._lib import get_lib

    ksel = 128
    cap = int(get_lib().meld_knn16_row_capacity(ksel))
    N = 384
    assert cap - 1 < N and cap % 2 == 0
    X, ti, td = rc.cells_and_truth(41, N, d, 0, N, cap - 1)
    rng = np.random.default_rng(7)
    lens = LENGTHS(knn, cap)
    cnt = np.array([lens[(q // 3) % len(lens)] for q in range(N)], np.int32)  # (every length with every split of the half-rows)
    assert (cnt <= 64).any() and ((cnt > 64) & (cnt <= 128)).any() and (cnt > 128).any()  # all three sort widths run
    bw2 = np.median(rc.true_bw2(td, knn).astype(np.float64))
    nmax, coef, norm2, lin, E = rc.allowance(X, np.arange(N), 0.02 * bw2, "lin")
    idx, d2 = rc.make_lists(X, np.arange(N), ti, td, cnt, cap, E, rng, knn)
    c = rc.make_case(X, 0, N, ksel, knn, 40.0, idx, d2, cnt, nmax, coef, norm2, lin)
    raw = _raw_rows(c, rng)
    assert any(a == 0 and b > 0 for a, b in raw[5]) and any(b == 0 and a > 0 for a, b in raw[5])
    for symm in (0, 1, 2):
        out = _three_routes(c, raw, symm)
        L0 = out["legacy"]
        assert 0 < L0.n_flag < N and int((L0.keep > 0).sum()) > N // 4, (L0.n_flag, int((L0.keep > 0).sum()))
        assert L0.merged[2] == 0
        for route in ("emit", "sort+emit"):
            R = out[route]
            assert np.array_equal(L0.bw, R.bw) and np.array_equal(L0.keep, R.keep), route
            assert L0.n_flag == R.n_flag and L0.flagged == R.flagged and len(R.flagged) == R.n_flag, route
            assert np.array_equal(L0.cursor, R.cursor), route  # what every bucket was sent, whatever the order
            assert L0.merged[2] == R.merged[2]
            for a, b in zip(L0.merged, R.merged):
                assert np.array_equal(a, b), route
            assert all(R.keep[r] == 0 for r in R.flagged)
        # the flagged rows leave the ranking kernel as the finish kernel leaves them
        R = out["sort+emit"]
        for r in R.flagged:
            n = int(L0.cnt[r])
            assert R.cnt[r] == n == min(int(cnt[r]), ksel), r
            assert np.array_equal(R.idx[r, :n], L0.idx[r, :n]) and np.array_equal(R.d2[r, :n].view(np.uint32), L0.d2[r, :n].view(np.uint32)), r
        for L in lens:  # a list that ends before ksel holds every reference: certified as soon as it has a bandwidth entry
            rows = np.nonzero(cnt == L)[0]
            assert len(rows) >= 3
            if L < ksel:
                assert all((r in R.flagged) == (L <= knn) for r in rows), L


def test_listed_emit_sends_second_stage_rows_and_swept_entries_behind_the_claims():
    """meld_coo_emit_scatter_listed: rows of a second-stage refinement (through the row list) and entries of the exact sweep go into
    buckets that already hold entries, each own entry behind an atomic claim -- against meld_coo_emit_scatter on the same inputs with
    its cursor preset, after the merge."""
    from meld_amd._lib import check, get_lib, ptr
    from meld_amd.graph import _stream

    lib, dev = get_lib(), "cuda"
    B = int(lib.meld_csr_bucket_slots())
    rng = np.random.default_rng(3)
    n, ksel, cap = 700, 64, 128
    idx = np.stack([rng.permutation(n)[:cap] for _ in range(n)]).astype(np.int32)
    for q in range(n):  # (no diagonal entries: the refinement never keeps one)
        idx[q][idx[q] == q] = (q + 1) % n
    val = np.where(rng.random((n, ksel)) < 0.4, rng.random((n, ksel)), 0.0)
    swept = np.sort(rng.choice(n, 40, replace=False)).astype(np.int32)
    listed = np.sort(rng.choice(np.setdiff1d(np.arange(n), swept), 90, replace=False)).astype(np.int32)
    val[swept] = 0.0
    keep = (val > 0).sum(1).astype(np.int32)
    fb_cnt = rng.integers(0, 30, size=len(swept)).astype(np.int32)
    fb_cnt[3] = 0
    fb_off = np.concatenate([[0], np.cumsum(fb_cnt)]).astype(np.int64)
    fb_col = np.concatenate([np.setdiff1d(rng.permutation(n)[: k + 1], [r])[:k] for r, k in zip(swept, fb_cnt)]).astype(np.int32)
    fb_val = rng.random(int(fb_off[-1]))
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    idx_d, val_d, keep_d, swept_d, listed_d, off_d, col_d, fval_d = map(g, (idx, val, keep, swept, listed, fb_off, fb_col, fb_val))
    res = []
    for fused in (False, True):
        tcol = torch.full((n * B,), -1, dtype=torch.int32, device=dev)
        tval = torch.full((n * B,), -1.0, dtype=torch.float64, device=dev)
        if fused:
            # the first stage's share: every row that is neither listed nor swept, by the legacy kernel on a list of those rows'
            # values alone, then the rest behind the claims
            first = np.setdiff1d(np.arange(n), listed).astype(np.int32)
            cursor = torch.zeros(n, dtype=torch.int32, device=dev)
            check(lib.meld_coo_emit_scatter_listed(ptr(g(first)), len(first), ptr(idx_d), ptr(val_d), ksel, cap, ptr(keep_d), None, 0, None, None, None, 0,
                                                   ptr(cursor), ptr(tcol), ptr(tval), _stream()), "listed(first)")
            check(lib.meld_coo_emit_scatter_listed(ptr(listed_d), len(listed), ptr(idx_d), ptr(val_d), ksel, cap, ptr(keep_d), ptr(swept_d), len(swept),
                                                   ptr(off_d), ptr(col_d), ptr(fval_d), int(fb_off[-1]), ptr(cursor), ptr(tcol), ptr(tval), _stream()),
                  "listed(rest)")
        else:
            cur = keep.copy()
            cur[swept] = fb_cnt
            cursor = g(cur)
            check(lib.meld_coo_emit_scatter(n, ptr(idx_d), ptr(val_d), ksel, cap, ptr(keep_d), ptr(swept_d), len(swept), ptr(off_d), ptr(col_d), ptr(fval_d),
                                            int(fb_off[-1]), ptr(cursor), ptr(tcol), ptr(tval), _stream()), "meld_coo_emit_scatter")
        torch.cuda.synchronize()
        res.append((cursor.cpu().numpy(), _merge(lib, cursor, tcol, tval, n, 0)))
    (c0, m0), (c1, m1) = res
    assert np.array_equal(c0, c1) and c0.max() <= B
    assert m0[2] == m1[2]
    for a, b in zip(m0, m1):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. whole builds, both routes forced
# ---------------------------------------------------------------------------------------------------------------------------------
def _build(X, route, monkeypatch, **kw):
    import meld_amd

    monkeypatch.setenv("MELD_ROWS_FUSED", route)
    G = meld_amd.build_knn_graph(X, **kw)
    if route == "0" or G.info.get("fused_rows_recovered"):
        assert G.info["fused_rows"] == "off", (route, G.info["fused_rows"])
    elif route == "a":
        assert G.info["fused_rows"] == "emit", (route, G.info["fused_rows"])
    else:  # ("b": the rows stay raw where the search is list-driven and in one slice)
        assert G.info["fused_rows"] in ("emit", "sort+emit"), (route, G.info["fused_rows"])
    return G


def _assert_same_graph(A, B):
    assert torch.equal(A.rowptr, B.rowptr) and torch.equal(A.col, B.col) and torch.equal(A.val, B.val)
    assert torch.equal(A.dw_dev, B.dw_dev) and torch.equal(A.ksum, B.ksum) and torch.equal(A.bandwidth, B.bandwidth)
    for k in ("n_flagged_rows", "n_researched_rows", "nnz", "nnz_directed", "ksel", "n_rows_bandwidth_recomputed"):
        assert A.info[k] == B.info[k], (k, A.info[k], B.info[k])


_CELLS = {}


def _cells(N, d, seed=0):
    if (N, d, seed) not in _CELLS:
        _CELLS[(N, d, seed)] = torch.from_numpy(mo.synthetic_cells(N, n_dims=d, seed=seed)[0]).cuda()
    return _CELLS[(N, d, seed)]


@pytest.mark.parametrize("N", [1000, 4099])
@pytest.mark.parametrize("d", [2, 10, 50])
@pytest.mark.parametrize("knn", [5, 15])
def test_whole_build_is_the_same_graph(N, d, knn, monkeypatch):
    X = _cells(N, d)
    for aniso in (0, 1):
        for symm, theta in (("+", None), ("*", None), ("mnn", 0.7)):
            kw = dict(knn=knn, anisotropy=aniso, kernel_symm=symm, theta=theta)
            B = _build(X, "0", monkeypatch, **kw)
            for route in ("a", "b"):
                A = _build(X, route, monkeypatch, **kw)
                assert "fused_rows_recovered" not in A.info
                _assert_same_graph(A, B)


def test_every_row_through_the_sweep(monkeypatch):
    X = _cells(1500, 10)
    A, A2, B = (_build(X, r, monkeypatch, knn=7, force_fallback=True) for r in ("a", "b", "0"))
    assert A.info["n_flagged_rows"] == 1500
    _assert_same_graph(A, B)
    _assert_same_graph(A2, B)


def test_knn_max(monkeypatch):
    X = _cells(4099, 10)
    A, A2, B = (_build(X, r, monkeypatch, knn=5, knn_max=9) for r in ("a", "b", "0"))
    _assert_same_graph(A, B)
    _assert_same_graph(A2, B)
    assert int((A.rowptr[1:] - A.rowptr[:-1]).max()) > 0


@pytest.mark.parametrize("route", ["a", "b"])
def test_second_stage_rows_go_through_the_row_list(route, monkeypatch):
    """Cells whose fp16-hi first pass leaves rows for the full-precision re-search, which certifies some of them (asserted): their
    entries reach the buckets through meld_coo_emit_scatter_listed's row list."""
    Xh = np.random.default_rng(2).normal(size=(3000, 8))
    Xh[:, 0] += np.where(np.arange(3000) % 2, 50.0, -50.0)  # (two far groups: the allowance of the fp16-hi pass scales with |x|^2, the margins do not)
    X = torch.from_numpy(Xh).cuda()
    A, B = (_build(X, r, monkeypatch, knn=8) for r in (route, "0"))
    print("searched again: {}, still flagged: {}".format(A.info["n_researched_rows"], A.info["n_flagged_rows"]))
    assert A.info["n_researched_rows"] > A.info["n_flagged_rows"], A.info
    _assert_same_graph(A, B)


def test_sliced_search_takes_the_emit_stage(monkeypatch):
    from meld_amd.graph import HipOps
    from meld_amd.knn_plan import plan_knn_search, search_nprod

    N, d = 20000, 10
    ops = HipOps()
    p = plan_knn_search(ops.lib, N, d, 0, N, 5, 64, options=ops, resident=ops.lib.meld_knn16_resident_blocks(d, search_nprod(ops.nprod, d)),
                        assemble=True, free_bytes=1 << 40)
    assert p.main_slices > 1 and p.fused_rows == "emit"
    X = _cells(N, d)
    A, A2, B = (_build(X, r, monkeypatch, knn=5, ksel=64) for r in ("a", "b", "0"))
    assert A2.info["fused_rows"] == "emit"  # (finished rows out of the merge of the slices: stage "emit" alone)
    _assert_same_graph(A, B)
    _assert_same_graph(A2, B)


@pytest.mark.parametrize("kind", ["plain", "swept", "researched"])
def test_raw_rows_through_a_whole_build(kind, monkeypatch):
    """The list-driven search in ONE slice: the rows reach the refinement raw.  "plain": the fewest cells at which the plan asks for
    one slice on this device.  "swept" / "researched": every row flagged / most rows searched again at full precision -- all of them
    written back finished -- on fewer cells (the sweep is quadratic), the slices switched off instead."""
    from meld_amd.graph import HipOps
    from meld_amd.knn_plan import plan_knn_search, search_nprod

    d = 10 if kind != "researched" else 8
    ops = HipOps()
    resident = ops.lib.meld_knn16_resident_blocks(d, search_nprod(ops.nprod, d))
    N = 2 * resident * ops.lib.meld_knn16_block_queries() + 77
    if kind != "plain":
        N = 20001
        monkeypatch.setattr(ops.lib, "meld_knn16_max_slices", lambda ksel: 1, raising=False)
    p = plan_knn_search(ops.lib, N, d, 0, N, 5, 64, options=ops, resident=resident, assemble=True, free_bytes=1 << 40)
    assert p.main_slices == 1 and p.fused_rows == "sort+emit", p
    if kind == "researched":
        Xh = np.random.default_rng(2).normal(size=(N, d))
        Xh[:, 0] += np.where(np.arange(N) % 2, 50.0, -50.0)
        X = torch.from_numpy(Xh).cuda()
    else:
        X = _cells(N, d, seed=3)
    kw = dict(knn=5, ksel=64, force_fallback=kind == "swept", ops=ops)
    A = _build(X, "b", monkeypatch, **kw)
    assert A.info["fused_rows"] == "sort+emit"
    B = _build(X, "0", monkeypatch, **kw)
    print(kind, "flagged", A.info["n_flagged_rows"], "searched again", A.info["n_researched_rows"])
    if kind == "swept":
        assert A.info["n_flagged_rows"] == N
    if kind == "researched":
        assert A.info["n_researched_rows"] > A.info["n_flagged_rows"]
    _assert_same_graph(A, B)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. a hub cell: more entries than a bucket holds
# ---------------------------------------------------------------------------------------------------------------------------------
def _sphere_with_centre(n=600, d=20, seed=4, max_cos=0.49):
    """n points on (a thin shell at) the unit sphere, no two closer than the centre is to either (cos of their angle < max_cos < 1/2, by rejection),
    and the centre as cell 0: the centre is every point's NEAREST cell."""
    rng = np.random.default_rng(seed)
    pts = np.zeros((0, d))
    while len(pts) < n:
        c = rng.normal(size=(20000, d))
        c /= np.linalg.norm(c, axis=1, keepdims=True)
        if len(pts):
            c = c[(c @ pts.T).max(axis=1) < max_cos]
        for v in c:
            if len(pts) == n:
                break
            if len(pts) == 0 or float((pts @ v).max()) < max_cos:
                pts = np.vstack([pts, v])
    # radii in [0.992, 1]: the points' distances to the centre all differ (the centre's own neighbours are ranked without ties), and two
    # points stay farther apart (d^2 >= 2 * 0.992^2 * (1 - max_cos) > 1) than the centre is from either
    pts *= rng.uniform(0.992, 1.0, size=(n, 1))
    return np.ascontiguousarray(np.vstack([np.zeros((1, d)), pts]) + 3.0)  # (off the origin: the search centres the cells itself)


def test_hub_cell_overflows_its_bucket_and_the_graph_is_rebuilt(monkeypatch):
    from meld_amd._lib import get_lib

    knn = 5
    Xh = _sphere_with_centre()
    n = Xh.shape[0]
    # on the CPU: the centre is among every point's knn nearest cells (it is the nearest), and the oracle's kernel has an entry
    # (point, centre) in every row -- an in-degree far above the bucket size
    D = np.linalg.norm(Xh[:, None, :] - Xh[None, :, :], axis=2)
    np.fill_diagonal(D, np.inf)
    assert np.all(np.argmin(D[1:], axis=1) == 0)
    K = mo.knn_kernel(Xh, knn=knn, decay=40, thresh=1e-4, algorithm="brute")
    indeg = int((K[1:, 0].toarray() > 0).sum())
    assert indeg == n - 1 > int(get_lib().meld_csr_bucket_slots())
    X = torch.from_numpy(Xh).cuda()
    A = _build(X, "b", monkeypatch, knn=knn)
    B = _build(X, "0", monkeypatch, knn=knn)
    assert A.info.get("fused_rows_recovered") is True and A.info["fused_rows"] == "off"
    assert "fused_rows_recovered" not in B.info
    _assert_same_graph(A, B)
    hub = int((A.rowptr[1:] - A.rowptr[:-1]).max())
    assert hub >= n - 1
