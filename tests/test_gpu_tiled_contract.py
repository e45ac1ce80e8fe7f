"""Contract tests of the panel-tiled layout (csrc/spmm_tiled.hip) at full blocks and at its limits, against tests/tiled_reference.py
(tests/test_tiled_reference.py shows on the host that every case sits exactly on its edge, that the checker reports mutated layouts and
that the step contract fails for a dropped entry, fp32 weights, a one-sided pair and an ignored coef_x).

Every limit of the layout is a packed field width, not a check in the step kernel: 12-bit row slots (blocks of up to 4,080 rows), 15-bit
positions in a (wave, tile) segment, 13-bit pair positions, KMAX = 512 chunk descriptors per wave, TMAX = 61 tiles per block, 384 bitmap
panels per builder pass (panel groups beyond), 4,096 panels in all.  For each: the largest instance the layout must still get right --
built with the block count the case is made for, decoded by ``check_layout`` (no violation) and stepped, element by element -- and the
smallest one it must refuse, with its status and the CSR-stream kernel's result.  A refused layout is never handed to a step.  (A
refused BUILD stores only inside its own arrays: positions are masked to their fields before they enter a code, ``place()`` of
``pt_fill_kernel`` stores at ``0 <= slot < span`` only, descriptors beyond KMAX are counted and not written, a block beyond TMAX
returns before its list chunk can pass lane 60 and is skipped by the fill (T < 0), status 3 returns before any kernel.)

Per element, for y = alpha (dw .* x - W x) + beta x + gamma z and r' = r + coef y + coef_x x (u = 2^-53, m_i entries in row i, g the
majorant of the reference module):
    |y_i - y_ref_i| <= (m_i + 8) u g_i,      |r'_i - r'_ref_i| <= |coef| (m_i + 8) u g_i + 3 u (|r_i| + |coef y_ref_i| + |coef_x x_i|),
the two dot sums of p = 1 within 4 tau <g, |x|> and 4 tau <g, g>; ``lanczos_spmv`` on the tiled layout against the weights rounded to fp32.
Derived in tests/tiled_reference.py, not measured, and not to be widened: a value beyond them is a finding.

Largest fraction of each bound used on the MI355X (each test prints its own ``TILED-CONTRACT`` lines; the same table is in DESIGN.md
section 4.2.2): cheby_step y / r / dot sums, lanczos_spmv y, and where run the steps of ``_cheby_run`` (y, r)
    case                 tiled layout                                           CSR-stream kernel
    FULL (+ unfolded)    0.24 / 0.22 / 4.0e-5, 0.15, run 0.19, 0.17             0.21 / 0.22 / 1.7e-6, 0.13, run 0.13, 0.34
    OFFSET               0.19 / 0.23 / 2.4e-5, 0.13                             0.16 / 0.23 / 2.1e-6, 0.15
    SEG                  0.26 / 0.31 / 4.9e-5, 0.18, run 0.20, 0.22             0.26 / 0.31 / 1.8e-5, 0.18, run 0.20, 0.42
    DESC                 0.31 / 0.29 / 1.8e-5, 0.21                             0.31 / 0.29 / 7.2e-6, 0.22
    PAIRS                0.29 / 0.28 / 4.6e-5, 0.20                             0.29 / 0.28 / 3.3e-6, 0.18
    TILES                0.014 / 0.013 / 1.9e-4, 0.008, run 0.018, 0.018        0.007 / 0.008 / 1.4e-4, 0.005, run 0.011, 0.011
    GROUPS384/385/769    0.046 / 0.038 / 2.9e-4, 0.033                          0.030 / 0.038 / 2.1e-4, 0.021
    COLS                 0.018 / 0.032 / 2.1e-3, 0.009                          0.015 / 0.019 / 2.1e-3, 0.010
    SPARSE-A / -B        0.27 / 0.29 / 1.5e-5, 0.22                             -
    PLAN-1M              0.34 / 0.32                                            -
    ADJACENT             0.20 / 0.27 / 3.8e-4                                   -
    refused (+1, DIAG)   -                                                      at most 0.23 / 0.31 / 2.1e-3
Nothing passes 0.42 of a bound; the short rows of FULL-like cases use the most (m_i + 8 is small), the 244-entry rows of TILES the least.

Found by these tests: a wave whose rows hold nothing but lower in-block entries has no stream, and ``pt_fill_kernel`` then skipped its
half of the block's symmetry sum -- status 5 for a bitwise symmetric matrix, which was laid out unfolded (PLAN-1M; ADJACENT below).
"""
import ctypes as C
import numpy as np
import pytest
import torch

from tests import tiled_reference as tr

pytestmark = pytest.mark.gpu

LD = tr.LD
WORST = {}  # (what, kernel) -> largest fraction of its bound seen in this process


def _note(what, kernel, f):
    if f is not None:
        WORST[(what, kernel)] = max(WORST.get((what, kernel), 0.0), float(f))


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    for (what, kernel), f in sorted(WORST.items()):
        print("\nTILED-CONTRACT worst %-14s %-5s %.2e" % (what, kernel, f), end="")
    print()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _graph(c, layout):
    from meld_amd.graph import DeviceGraph, HipOps

    G = DeviceGraph(_dev(c.rowptr), _dev(c.col), _dev(c.val), _dev(c.dw), row_begin=c.row_begin, n_total=c.n_total)
    G.rows_pad, G.n_pad = c.n_rows, c.n_cols
    G.ops = HipOps(spmm=layout)
    return G


def _geometry():
    from meld_amd._lib import get_lib

    v = [C.c_int() for _ in range(4)]
    get_lib().meld_pt_geometry(*(C.byref(x) for x in v))
    return tuple(x.value for x in v)


def _build(G, nb, fold=True):
    """A layout of ``G`` with ``nb`` blocks, built the way ``HipOps.pt_layout`` builds it: the same tensors, ``PtLayout``, and the
    1-then-0 symmetric retry on status 5.  Status 0: attached as ``G.pt``; otherwise nothing is attached and the graph is pinned to
    the CSR-stream kernel with the refusal in ``G.info`` -- a refused layout is never handed to a step.  Returns (status, tensors)."""
    from meld_amd._lib import PtLayout, check, ptr
    from meld_amd.graph import _stream

    lib, dev = G.ops.lib, G.val.device
    slen = int(lib.meld_pt_stream_len(G.nnz, nb))
    assert slen == tr.stream_len(G.nnz, nb)
    i32 = dict(dtype=torch.int32, device=dev)
    t = dict(
        blk_row=torch.empty(nb + 1, **i32), blk_ntile=torch.empty(nb, **i32), blk_ndist=torch.empty(nb, **i32),
        seg=torch.empty(int(lib.meld_pt_seg_len(nb)), **i32), list_cols=torch.empty(G.nnz, **i32),
        pval=torch.empty(slen, dtype=torch.float64, device=dev), pidx=torch.empty(slen, **i32),
        pval32=torch.empty(slen, dtype=torch.float32, device=dev),
        cdesc=torch.empty(int(lib.meld_pt_desc_len(nb)), dtype=torch.int16, device=dev),
    )
    status = torch.zeros(1, **i32)
    lay = PtLayout(*(t[k].data_ptr() for k in ("blk_row", "blk_ntile", "blk_ndist", "seg", "list_cols", "pval", "pidx")), nb,
                   t["pval32"].data_ptr(), slen, t["cdesc"].data_ptr())
    codes = torch.empty(G.nnz, **i32)
    for symmetric in ((1, 0) if fold else (0,)):
        check(lib.meld_pt_build(ptr(G.rowptr), ptr(G.col), ptr(G.val), G.n_rows, G.n_pad, G.row_begin, symmetric, C.byref(lay), ptr(codes),
                                ptr(status), _stream()), "meld_pt_build")
        st = int(status.item())
        if st != 5:
            break
    G.info["spmm_fold"] = bool(symmetric) and st == 0
    if st != 0:
        G.pt = False
        G.info["spmm"] = "csr (tiled layout refused: status {})".format(st)
        return st, None
    G.pt = dict(struct=lay, tensors=t, nb=nb)
    G.info["spmm"] = "tiled"
    return 0, t


def _host(t):
    return {k: v.cpu().numpy() for k, v in t.items()}


def _pair(c):
    """(tiled graph with the case's block count, CSR graph)."""
    Gt, Gc = _graph(c, "tiled"), _graph(c, "csr")
    st, t = _build(Gt, c.nb)
    assert st == 0 and Gt.info["spmm_fold"] is True, (c.name, st, Gt.info)
    return Gt, Gc, t


SCALARS = dict(alpha=0.7, beta=-0.3, gamma=-1.0, coef=0.25)


def _step(c, G, kernel, p, xd, z, r, alpha, beta, gamma, coef, ref, what):
    """One ``cheby_step`` held to the bound of ``ref`` (the reference of the same operands)."""
    label = "csr" if kernel.startswith("csr") else kernel
    zd = None if z is None else _dev(z)
    rd = None if r is None else _dev(r)
    yd = torch.full((c.n_rows + 1, p), 7.0, dtype=torch.float64, device="cuda")
    dots = torch.zeros(2 * G.ops.dot_slots(), dtype=torch.float64, device="cuda") if p == 1 else None
    G.ops.cheby_step(G, p, xd, c.row_begin, zd, yd[: c.n_rows], rd, alpha, beta, gamma, coef, dots)
    torch.cuda.synchronize()
    assert G.info["spmm"] == kernel, G.info
    y = yd.cpu().numpy()
    assert np.all(y[c.n_rows] == 7.0)  # nothing written past the local rows
    fy, fr = tr.step_fractions(ref, y[: c.n_rows], None if r is None else rd.cpu().numpy())
    fd = (None, None)
    if p == 1:
        s = G.ops.dot_slots()
        d = dots.cpu().numpy().astype(LD)
        fd = tr.dot_fractions(ref, d[:s].sum(), d[s:].sum())
    print("TILED-CONTRACT %-10s %-5s p=%d %-8s y %.2e  r %s  dots %s" % (
        c.name, label, p, what, fy, "-" if fr is None else "%.2e" % fr, "-" if p != 1 else "%.2e %.2e" % fd))
    _note("y", label, fy); _note("r", label, fr); _note("dot yx", label, fd[0]); _note("dot yy", label, fd[1])
    assert fy <= 1.0 and (fr is None or fr <= 1.0) and (p != 1 or max(fd) <= 1.0), (c.name, kernel, p, what, fy, fr, fd)


def _steps(c, graphs, ps=(1, 2, 3)):
    """``cheby_step`` for every p (3 is one launch of each instantiation), gamma zero without r and non-zero with r, on every
    (graph, kernel name) of ``graphs``; operands and references are made once per p."""
    Wref = tr.reference(c)
    for p in ps:
        x, z, r = tr.signals(c, p)
        xd = _dev(x)
        ref0 = tr.step_reference(Wref, c.dw, x, c.row_begin, None, None, 0.9, 0.4, 0.0, 0.0, 0.0)
        ref1 = tr.step_reference(Wref, c.dw, x, c.row_begin, z, r, coef_x=0.0, **SCALARS)
        for G, kernel in graphs:
            _step(c, G, kernel, p, xd, None, None, 0.9, 0.4, 0.0, 0.0, ref0, "gamma=0")
            _step(c, G, kernel, p, xd, z, r, ref=ref1, what="gamma,r", **SCALARS)


def _lanczos_spmv(c, G, kernel):
    """``meld_lanczos_spmv``: p = 1, the scalars read from device memory; the tiled layout streams the fp32 copy of the weights."""
    x, z, _ = tr.signals(c, 1, seed=1)
    state = torch.zeros(8, dtype=torch.float64, device="cuda")
    state[3], state[4] = 0.5, -0.25
    dots = torch.zeros(2 * G.ops.dot_slots(), dtype=torch.float64, device="cuda")
    yd = torch.empty(c.n_rows, dtype=torch.float64, device="cuda")
    G.ops.lanczos_spmv(G, _dev(x[:, 0]), _dev(z[:, 0]), yd, state, dots)
    torch.cuda.synchronize()
    ref = tr.step_reference(tr.reference(c, kernel == "tiled"), c.dw, x, c.row_begin, z, None, 0.5, 0.0, -0.25)
    fy, _ = tr.step_fractions(ref, yd.cpu().numpy())
    s = G.ops.dot_slots()
    d = dots.cpu().numpy().astype(LD)
    fd = tr.dot_fractions(ref, d[:s].sum(), d[s:].sum())
    print("TILED-CONTRACT %-10s %-5s lanczos_spmv  y %.2e  dots %.2e %.2e" % (c.name, kernel, fy, fd[0], fd[1]))
    _note("lanczos y", kernel, fy); _note("lanczos dots", kernel, max(fd))
    assert fy <= 1.0 and max(fd) <= 1.0, (c.name, kernel, fy, fd)


def _cheby_run(c, G, kernel, p):
    """``_cheby_run`` over 5 coefficients is one step that adds its own c_2 T_2, then a pair: a step that leaves r alone and one
    that adds c_4 T_4 + c_3 T_3 (the ``coef_x`` path of the tiled kernel; the CSR-stream kernel adds at every step).  Made as two calls
    -- 3 coefficients, then 4 on the buffers the first one left -- so that every step is judged from the device's own previous
    buffers: a single call overwrites T_2 with T_4."""
    rng = np.random.default_rng([5, p])
    co = rng.normal(size=5)
    alpha2, beta2 = 0.35, -0.6
    x0, _, r0 = tr.signals(c, p, seed=2)
    x1, _, _ = tr.signals(c, p, seed=3)
    Wref = tr.reference(c)
    a, b, r = _dev(x0), _dev(x1), _dev(r0)
    n = c.n_rows

    def judge(what, x_full, z, r_before, y_dev, r_after, coef, coef_x):
        ref = tr.step_reference(Wref, c.dw, x_full, 0, z, r_before, alpha2, beta2, -1.0, coef, coef_x)
        fy, fr = tr.step_fractions(ref, y_dev, r_after)
        print("TILED-CONTRACT %-10s %-5s p=%d run: %-22s y %.2e  r %s" % (c.name, kernel, p, what, fy, "-" if fr is None else "%.2e" % fr))
        _note("run y", kernel, fy); _note("run r", kernel, fr)
        assert fy <= 1.0 and (fr is None or fr <= 1.0), (c.name, kernel, p, what, fy, fr)

    last = G.ops._cheby_run(G, None, 0, p, a, b, r, co[:3], alpha2, beta2)
    torch.cuda.synchronize()
    assert last == 0 and G.info["spmm"] == kernel
    a1, r1 = a.cpu().numpy(), r.cpu().numpy()
    assert np.array_equal(a1[n:], x0[n:]) and np.array_equal(b.cpu().numpy(), x1)
    judge("T2, r += c2 T2", x1, x0[:n], r0, a1[:n], r1, co[2], 0.0)
    # the pair: t_prev2 = b (T_1), t_prev1 = a (T_2)
    last = G.ops._cheby_run(G, None, 0, p, b, a, r, np.array([0.0, 0.0, co[3], co[4]]), alpha2, beta2)
    torch.cuda.synchronize()
    assert last == 1
    b2, a2, r2 = b.cpu().numpy(), a.cpu().numpy(), r.cpu().numpy()
    if kernel == "tiled":  # the first step of the pair neither reads nor writes r
        judge("T3, r left alone", a1, x1[:n], None, b2[:n], None, 0.0, 0.0)
        judge("T4, r += c4 T4 + c3 T3", b2, a1[:n], r1, a2[:n], r2, co[4], co[3])
    else:  # the CSR-stream kernel adds c_3 T_3 at once; r between the two steps is not kept: the sum of both is judged on T_4's step
        ref3 = tr.step_reference(Wref, c.dw, a1, 0, x1[:n], r1, alpha2, beta2, -1.0, co[3], 0.0)
        fy, _ = tr.step_fractions(ref3, b2[:n])
        _note("run y", kernel, fy)
        assert fy <= 1.0
        r_mid = r1 + co[3] * b2[:n]  # (one rounded product and sum per element: inside the 3 u term of the bound below)
        judge("T4, r += c4 T4 (csr)", b2, a1[:n], r_mid, a2[:n], r2, co[4], 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# accepted cases
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tr.ACCEPTED)
def test_largest_accepted_instance(name):
    c = tr.case(name)
    Gt, Gc, t = _pair(c)
    h = _host(t)
    assert np.array_equal(h["blk_row"], tr.forced_blk_row(c))
    assert tr.check_layout(h, c.rowptr, c.col, c.val, c.row_begin, _geometry()) == []
    F = tr.case_facts(c)
    assert [int(x) for x in h["blk_ntile"]] == F.tiles and [int(x) for x in h["blk_ndist"]] == F.ndist
    _steps(c, ((Gt, "tiled"), (Gc, "csr")))
    for G, kernel in ((Gt, "tiled"), (Gc, "csr")):
        _lanczos_spmv(c, G, kernel)
        if c.row_begin == 0 and name in ("FULL", "SEG", "TILES"):
            for p in (1, 2):
                _cheby_run(c, G, kernel, p)
    assert Gt.pt["nb"] == c.nb and Gc.info["spmm"] == "csr"


def test_unfolded_layout_of_full_blocks():
    """``symmetric = 0``: no IN part; the in-block columns go through the tiles like any other."""
    c = tr.case("FULL")
    G = _graph(c, "tiled")
    st, t = _build(G, c.nb, fold=False)
    assert st == 0 and G.info["spmm_fold"] is False
    assert tr.check_layout(_host(t), c.rowptr, c.col, c.val, c.row_begin, _geometry(), folded=False) == []
    _steps(c, ((G, "tiled"),), ps=(2,))


def test_waves_that_own_nothing_but_lower_entries_keep_the_fold():
    """Adjacent pairs (2i, 2i + 1): the odd rows -- all the rows of the odd waves -- hold one lower in-block entry each and no stream.
    Their entries still owe their half of the block's symmetry sum: the builder used to skip a wave without a stream, found the sums
    unbalanced (status 5) and laid a perfectly symmetric matrix out unfolded (found by PLAN-1M, whose first half is made of such rows)."""
    n = 480
    i = np.arange(0, n, 2)
    c = tr._case("ADJACENT", n, n, 0, (i, i + 1), None, np.random.default_rng(480), nb=1)
    G = _graph(c, "tiled")
    st, t = _build(G, 1)
    assert st == 0 and G.info["spmm_fold"] is True
    h = _host(t)
    assert tr.check_layout(h, c.rowptr, c.col, c.val, 0, _geometry()) == []
    seg = h["seg"].reshape(1, tr.SEGROWS, tr.SEGW)[0]
    assert [int(seg[tr.NW + 1 + w, 62]) for w in range(tr.NW)] == [n // 12, 0] * 6  # pairs per wave
    _steps(c, ((G, "tiled"),), ps=(1, 2))


# ---------------------------------------------------------------------------------------------------------------------------------
# refused cases
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tr.REFUSED)
def test_smallest_refused_instance(name):
    """The expected status, exactly; nothing attached; the step is the CSR-stream kernel's and meets the bound.  Where the production
    block count reaches the case (TILES+1, COLS+1, DIAG) the public path is taken and must say the same."""
    c = tr.case(name)
    G = _graph(c, "tiled")
    st, t = _build(G, c.nb)
    assert st == c.status and t is None and G.pt is False
    assert G.info["spmm"] == "csr (tiled layout refused: status %d)" % c.status and G.info["spmm_fold"] is False
    _steps(c, ((G, G.info["spmm"]),), ps=(2,))
    if c.production:
        Gp = _graph(c, "tiled")
        _steps(c, ((Gp, "csr (tiled layout refused: status %d)" % c.status),), ps=(1,))
        assert Gp.pt is False


# ---------------------------------------------------------------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tr.PLANS)
def test_plans(name):
    c = tr.case(name)
    G = _graph(c, "tiled")
    if c.production:
        pt = G.ops.pt_layout(G)
        assert pt is not None and pt["nb"] == c.nb
        t = pt["tensors"]
    else:
        st, t = _build(G, c.nb)
        assert st == 0
    assert G.info["spmm"] == "tiled" and G.info["spmm_fold"] is True
    h = _host(t)
    by_entries = tr.plan_is_by_entries(c.n_rows, len(c.col), c.nb, int(G.ops.lib.meld_scan_temp_bytes(c.n_rows)))
    assert by_entries == name.startswith("SPARSE")
    plan = tr.plan_by_entries(c.rowptr, c.nb) if by_entries else tr.plan_by_time(c.rowptr, c.col, c.nb)
    assert np.array_equal(h["blk_row"], plan)
    assert np.diff(h["blk_row"]).max() == tr.RMAX
    assert tr.check_layout(h, c.rowptr, c.col, c.val, c.row_begin, _geometry()) == []
    if name == "SPARSE-B":
        assert h["blk_ntile"][1] == 0 and c.rowptr[tr.RMAX] == c.rowptr[2 * tr.RMAX]
    _steps(c, ((G, "tiled"),), ps=(2,) if name == "PLAN-1M" else (1, 2))
    if name != "PLAN-1M":
        _lanczos_spmv(c, G, "tiled")


# ---------------------------------------------------------------------------------------------------------------------------------
# the checker has teeth on the device's own layout
# ---------------------------------------------------------------------------------------------------------------------------------
def test_checker_reports_mutated_copies_of_the_device_layout():
    """Host copies only: nothing mutated goes back to the device."""
    c = tr.case("FULL")
    G = _graph(c, "tiled")
    st, t = _build(G, c.nb)
    assert st == 0
    h = _host(t)
    assert tr.check_layout(h, c.rowptr, c.col, c.val, c.row_begin, _geometry()) == []
    seen = []
    for what, m in tr.layout_mutants(c, h):
        v = tr.check_layout(m, c.rowptr, c.col, c.val, c.row_begin, _geometry())
        print("TILED-CONTRACT mutant %-42s -> %s" % (what, v[0] if v else "NOT REPORTED"))
        assert v, what
        seen.append(what)
    assert len(seen) == 7
    # the numpy model of the builder and the device agree on everything the layout defines
    m = tr.model_layout(c.rowptr, c.col, c.val, h["blk_row"], c.row_begin)
    for k in ("blk_ntile", "blk_ndist", "seg"):
        assert np.array_equal(m[k], h[k]), k
