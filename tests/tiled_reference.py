"""Host side of the contract of the panel-tiled recurrence kernel (csrc/spmm_tiled.hip): NumPy / SciPy only.

(a) ``check_layout``: a decoder and checker of a built layout (``pt_build_kernel`` + ``pt_fill_kernel``).  It returns a list of
    violations -- empty when the layout is right -- and never asserts, so that mutated copies can be fed to it.  ``model_layout`` is
    a plain numpy model of the builder written from its comments: it lets the checker be exercised where there is no device.

(b) ``step_reference`` / ``step_fractions``: one step in long double (tests/lanczos_reference.py: ``np.longdouble``, or exactly rounded
    fp64 sums where the platform's long double is no finer) with a per-element bound.  For fp64 operands
        y = alpha (dw .* x - W x) + beta x + gamma z,         r' = r + coef y + coef_x x,
        g_i = |alpha| (|dw_i x_i| + sum_j |w_ij x_j|) + |beta x_i| + |gamma z_i|            (majorant)
    and with u = 2^-53, m_i the number of entries of row i
        |y_i - y_ref_i|   <= (m_i + 8) u g_i
        |r'_i - r'_ref_i| <= |coef| (m_i + 8) u g_i + 3 u (|r_i| + |coef y_ref_i| + |coef_x x_i|).
    Derivation: m_i products and m_i - 1 additions in any order cost m_i u times the sum of their magnitudes; one product and one
    subtraction give (L x)_i; three products and two additions give y_i: (m_i + 6) u to first order, the remaining 2 cover the
    second-order terms.  r' takes two more products and two additions of three terms.  A kernel that contracts to FMAs only does
    better.  The instantiation that streams fp32 values is held to the same bound against the weights rounded to fp32 and widened
    (``lanczos_reference.reference_weights(W, True)``).  The two dot sums of p = 1 are held to the alpha bound of
    tests/lanczos_reference.py: 4 tau <g, |x|> and 4 tau <g, g> with tau = (rows + longest row + 16) u.
    Derived, not measured, and not to be widened: a value beyond them is a finding.

(c) The case matrices, one per limit of the layout (packed field widths set them, not checks in the step kernel), each with
    ``facts()``: the numbers the case exists for, computed from the CSR arrays and a given ``blk_row`` alone -- rows, distinct OUT
    columns, touched bitmap panels (and panel groups) per block, entries per (wave, tile), IN pairs per wave, chunk descriptors per
    wave -- and the status the builder must report.  ``plan_by_entries`` / ``plan_by_time`` are numpy transcriptions of the two plan
    kernels' arithmetic.
"""
import functools
from types import SimpleNamespace

import numpy as np
from scipy import sparse

from tests import lanczos_reference as lr

LD = lr.LD
U = lr.U

# geometry of csrc/spmm_tiled.hip (the first four are what meld_pt_geometry reports)
NW, RMAX, CP, TMAX = 12, 4080, 1024, 61
GEOMETRY = (NW, RMAX, CP, TMAX)
NB_RING = 4  # staged tiles in LDS
SEGW, SEGROWS = 64, 2 * (NW + 1)
QW = 8  # chunks per window of the IN part
PADCAP = 64
KMAX, KSLACK = 512, 32
D_FIRST, D_LAST = 0x80, 0x100
BP, BP_BITS = 2048, 11  # columns per bitmap panel
NPAN_MAX, TP_MAX = 4096, 384
SEG_MAX = 1 << 15  # entries of a (wave, tile) segment: positions are 15 bits
PAIR_MAX = 1 << 13  # IN pairs of a wave: positions are 13 bits
U_CHUNKS = 8  # chunks in flight per consumer wave (slack behind the streams)
W_ENTRY, W_FAR, W_ROW = 361, 754, 2840  # weights of the time-balanced plan


def stream_len(nnz, nb):
    """``meld_pt_stream_len``."""
    return int(nnz) + nb * NW * PADCAP + (U_CHUNKS + 1) * 64


def num_blocks(n_rows):
    """``meld_pt_num_blocks``."""
    if n_rows <= 0:
        return 0
    target = int(0.9576 * RMAX)
    if n_rows <= 64 * 256:
        return max(1, -(-n_rows // 256))
    k = -(-n_rows // (256 * target))
    nb = 256 * k
    if k == 1:
        nb = min(256, max(64, -(-n_rows // 256)))
    while nb * RMAX < n_rows:
        nb += 256
    return nb


# ---------------------------------------------------------------------------------------------------------------------------------
# the two plans
# ---------------------------------------------------------------------------------------------------------------------------------
def _plan(prefix, n_rows, nb):
    """Every block's cut by bisection of ``prefix`` (first row whose prefix reaches the block's share), then the caps in order: a
    block holds at most RMAX rows (``cut <= prev + RMAX``), what is left has to fit the remaining blocks (``must``)."""
    prefix = np.asarray(prefix, dtype=np.int64)
    tot = int(prefix[n_rows])
    b1 = np.arange(1, nb + 1, dtype=np.int64)
    target = (tot // nb) * b1 + ((tot % nb) * b1) // nb
    cut = np.searchsorted(prefix[:n_rows], target, side="left").astype(np.int64)
    cut[nb - 1] = n_rows
    blk = np.zeros(nb + 1, dtype=np.int64)
    prev = 0
    for b in range(nb):
        c = int(cut[b])
        must = n_rows - (nb - 1 - b) * RMAX
        c = max(c, must)
        c = min(c, prev + RMAX)
        c = min(max(c, prev), n_rows)
        blk[b + 1] = prev = c
    return blk


def plan_by_entries(rowptr, nb):
    """``pt_plan_kernel``: balanced nonzero counts."""
    return _plan(rowptr, len(rowptr) - 1, nb)


def row_weights(rowptr, col, nb, col_base=0):
    """``pt_row_weight_kernel``: estimated time of every row, 1e-6 us."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n_rows = len(rowptr) - 1
    win = max(1, n_rows // nb // 2)
    deg = np.diff(rowptr)
    rows = np.repeat(np.arange(n_rows, dtype=np.int64), deg)
    dlt = np.asarray(col, dtype=np.int64) - (col_base + rows)
    far = np.bincount(rows[(dlt > win) | (dlt < -win)], minlength=n_rows)
    return np.minimum(W_ENTRY * deg + W_FAR * far + W_ROW, 0x3FFFFFFF).astype(np.int64)


def plan_by_time(rowptr, col, nb, col_base=0):
    """``pt_row_weight_kernel`` + exclusive scan + ``pt_plan_weighted_kernel``."""
    w = row_weights(rowptr, col, nb, col_base)
    return _plan(np.concatenate([[0], np.cumsum(w)]), len(rowptr) - 1, nb)


def plan_is_by_entries(n_rows, nnz, nb, scan_bytes):
    """The builder's choice (``meld_pt_build``): the weights and their scan live in the not yet written value stream; where they
    do not fit -- or with one block -- the plan is by entries.  ``scan_bytes``: ``meld_scan_temp_bytes(n_rows)`` (>= 0)."""
    off_w = 8 * (n_rows + 1)
    off_t = (off_w + 4 * n_rows + 255) // 256 * 256
    return nb <= 1 or off_t + scan_bytes > 8 * stream_len(nnz, nb)


# ---------------------------------------------------------------------------------------------------------------------------------
# facts of a matrix under a plan
# ---------------------------------------------------------------------------------------------------------------------------------
def _block_entries(rowptr, col, blk_row, b, col_base, folded):
    r0, r1 = int(blk_row[b]), int(blk_row[b + 1])
    e0, e1 = int(rowptr[r0]), int(rowptr[r1])
    deg = np.diff(rowptr[r0 : r1 + 1])
    rl = np.repeat(np.arange(r1 - r0, dtype=np.int64), deg)
    k_in_row = np.arange(e1 - e0, dtype=np.int64) - np.repeat(rowptr[r0:r1] - e0, deg)
    c = np.asarray(col[e0:e1], dtype=np.int64)
    cg = c - (col_base + r0)
    inb = (cg >= 0) & (cg < r1 - r0) if folded else np.zeros(len(c), dtype=bool)
    return SimpleNamespace(r0=r0, nrows=r1 - r0, e0=e0, e1=e1, rl=rl, part=k_in_row >> 6, c=c, cg=cg, inb=inb, upper=inb & (cg > rl),
                           diag=inb & (cg == rl), out=~inb)


def facts(rowptr, col, blk_row, col_base=0, folded=True, n_cols=None):
    """What a layout of these CSR arrays under ``blk_row`` must hold, per block: ``rows``, ``ndist`` (distinct OUT columns),
    ``tiles``, ``panels`` (touched bitmap panels), ``groups`` (panel groups the builder loops over), ``seg`` ([NW, tiles] entries
    per (wave, tile)), ``pairs`` ([NW] IN pairs per wave), ``desc`` ([NW] chunk descriptors per wave), ``diag`` (diagonal entries);
    and ``status``: what the builder must report (0, 2, 3, 4 or 6; the symmetry of the values -- status 5 -- is not modelled)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    nb = len(blk_row) - 1
    F = SimpleNamespace(nb=nb, rows=np.diff(np.asarray(blk_row, dtype=np.int64)), ndist=[], tiles=[], panels=[], groups=[], seg=[],
                        pairs=[], desc=[], diag=[], status=0)
    for b in range(nb):
        E = _block_entries(rowptr, col, blk_row, b, col_base, folded)
        lst = np.unique(E.c[E.out])
        T = -(-len(lst) // CP)
        w = E.rl % NW
        seg = np.zeros((NW, max(T, 1)), dtype=np.int64)
        np.add.at(seg, (w[E.out], np.searchsorted(lst, E.c[E.out]) >> 10), 1)
        seg = seg[:, :T]
        pairs = np.bincount(w[E.upper], minlength=NW)
        desc = -(-pairs // 64) + np.maximum(1, -(-seg // 64)).sum(1) if E.e1 > E.e0 else np.zeros(NW, dtype=np.int64)
        panels = len(np.unique(lst >> BP_BITS))
        F.ndist.append(len(lst)); F.tiles.append(T); F.panels.append(panels); F.groups.append(max(1, -(-panels // TP_MAX)))
        F.seg.append(seg); F.pairs.append(pairs); F.desc.append(desc); F.diag.append(int(E.diag.sum()))
        if T > TMAX:
            F.status = max(F.status, 2)  # (the block gives up before it looks at anything else)
            continue
        if (seg.size and seg.max() > SEG_MAX) or pairs.max() > PAIR_MAX or desc.max() > KMAX:
            F.status = max(F.status, 4)
        if E.diag.any():
            F.status = max(F.status, 6)
    if n_cols is not None and -(-int(n_cols) // BP) > NPAN_MAX:
        F.status = 3  # (refused on the host, before any kernel)
    return F


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the layout: slots, a numpy model of the builder, the checker
# ---------------------------------------------------------------------------------------------------------------------------------
def row_slot(rl, nw=NW, slots=RMAX // NW):
    return (rl % nw) * slots + rl // nw


def row_of(slot, nw=NW, slots=RMAX // NW):
    """Inverse of the kernel's ``row_slot``."""
    return (slot % slots) * nw + slot // slots


def _in_slots(n_in):
    """For every slot of an IN part of ``n_in`` chunks: the position of its pair in the wave's (row, column) order.  Windows of QW
    chunks, transposed over the lanes: lane l owns qw consecutive pairs of a window of qw chunks, chunk c holds each lane's c-th."""
    s = np.arange(64 * n_in, dtype=np.int64)
    win, rem = s // (64 * QW), s % (64 * QW)
    c, l = rem // 64, rem % 64
    qw = np.minimum(QW, n_in - QW * win)
    return win * (64 * QW) + l * qw + c, c == qw - 1


def _out_slots(eoff_t):
    """For every slot of a wave's OUT part (``eoff_t``: offsets of its T + 1 tile bounds): processing index of its tile, position
    in the segment's order, whether it is its lane's last entry of the segment.  A segment of n = 64 q + r entries is transposed
    over the lanes: lane l owns q + 1 consecutive entries for l < r, else q; chunk c holds each lane's c-th."""
    tot = int(eoff_t[-1])
    s = np.arange(tot, dtype=np.int64)
    j = np.searchsorted(eoff_t[1:], s, side="right")
    within = s - eoff_t[j]
    n = (eoff_t[1:] - eoff_t[:-1])[j]
    q, r = n >> 6, n & 63
    c, l = within // 64, within % 64
    pos = np.where(l < r, l * (q + 1) + c, r * (q + 1) + (l - r) * q + c)
    mine = np.where(l < r, q + 1, q)
    return j, pos, c == mine - 1


def _descriptors(n_in, cnt):
    d = [64] * int(n_in)
    for n in cnt:
        nch = max(1, (int(n) + 63) >> 6)
        for c in range(nch):
            d.append(max(min(64, int(n) - 64 * c), 0) | (D_FIRST if c == 0 else 0) | (D_LAST if c == nch - 1 else 0))
    return d


def processing_order(tot):
    """Tiles in processing order: one of the heaviest left, then two of the lightest left (ties keep list order)."""
    srt = list(np.argsort(-np.asarray(tot, dtype=np.int64), kind="stable"))
    hi, lo, out = 0, len(srt) - 1, []
    while hi <= lo:
        out.append(srt[hi]); hi += 1
        for _ in range(2):
            if hi <= lo:
                out.append(srt[lo]); lo -= 1
    return np.array(out, dtype=np.int64)


def model_layout(rowptr, col, val, blk_row, col_base=0, folded=True):
    """A numpy model of ``pt_build_kernel`` + ``pt_fill_kernel`` for a matrix the builder accepts (``facts().status == 0``): the
    layout arrays as the device holds them.  What the device leaves unwritten (gaps between the streams, descriptors of blocks
    without entries) is filled with junk here."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    nnz, nb = int(rowptr[-1]), len(blk_row) - 1
    slen = stream_len(nnz, nb)
    t = dict(blk_row=np.asarray(blk_row, dtype=np.int32), blk_ntile=np.zeros(nb, dtype=np.int32), blk_ndist=np.zeros(nb, dtype=np.int32),
             seg=np.zeros(nb * SEGROWS * SEGW, dtype=np.int32), list_cols=np.full(nnz, -7, dtype=np.int32),
             pval=np.full(slen, np.nan), pidx=np.full(slen, 0xDEADBEEF, dtype=np.uint32).view(np.int32),
             cdesc=np.full(nb * NW * (KMAX + KSLACK), 0x7ABC, dtype=np.uint16).view(np.int16))
    seg = t["seg"].reshape(nb, SEGROWS, SEGW)
    cdesc = t["cdesc"].view(np.uint16).reshape(nb, NW, KMAX + KSLACK)
    pidx = t["pidx"].view(np.uint32)
    val = np.asarray(val, dtype=np.float64)
    for b in range(nb):
        E = _block_entries(rowptr, col, blk_row, b, col_base, folded)
        S = seg[b]
        S[SEGROWS - 1, 2:8] = [E.r0, E.nrows, 0, 0, np.uint32(E.e0 & 0xFFFFFFFF).astype(np.int32), E.e0 >> 32]
        if E.e1 == E.e0:
            continue
        v = val[E.e0 : E.e1]
        lst = np.unique(E.c[E.out])
        nd = len(lst)
        T = -(-nd // CP)
        t["list_cols"][E.e0 : E.e0 + nd] = lst
        t["blk_ntile"][b], t["blk_ndist"][b] = T, nd
        S[SEGROWS - 1, 4:6] = [T, nd]
        pan = np.unique(lst >> BP_BITS)
        grp = np.searchsorted(pan, E.c >> BP_BITS) // TP_MAX
        rank = np.searchsorted(lst, E.c)
        tile, local = rank >> 10, rank & (CP - 1)
        w = E.rl % NW
        cnt = np.zeros((NW, max(T, 1)), dtype=np.int64)
        np.add.at(cnt, (w[E.out], tile[E.out]), 1)
        order = processing_order(cnt[:, :T].sum(0)) if T else np.zeros(0, dtype=np.int64)
        inv = np.zeros(max(T, 1), dtype=np.int64)
        inv[order] = np.arange(T)
        S[NW, :T] = order
        run = 0
        for ow in range(NW):
            # IN pairs, in (row, column) order; flagged: the last upper entry of its 64-entry part of the row
            ii = np.nonzero(E.upper & (w == ow))[0]
            nin = len(ii)
            n_in = (nin + 63) >> 6
            key = E.rl[ii] * (1 << 20) + E.part[ii]
            ilast = np.append(key[1:] != key[:-1], True) if nin else np.zeros(0, dtype=bool)
            gpos, lane_last = _in_slots(n_in)
            slot_of = np.empty(64 * n_in, dtype=np.int64)
            slot_of[gpos] = np.arange(64 * n_in)
            lane_last_of = np.empty(64 * n_in, dtype=bool)
            lane_last_of[gpos] = lane_last
            cnt_w = cnt[ow, order] if T else np.zeros(0, dtype=np.int64)
            eoff_t = np.concatenate([[0], np.cumsum(cnt_w)]).astype(np.int64)
            length = 64 * n_in + int(eoff_t[-1])
            sb = E.e0 + b * NW * PADCAP + run
            t["pval"][sb : sb + length] = 0.0
            pidx[sb : sb + length] = 0
            sl = slot_of[:nin]
            t["pval"][sb + sl] = v[ii]
            pidx[sb + sl] = ((ilast | lane_last_of[:nin]).astype(np.uint32) | (row_slot(E.cg[ii]).astype(np.uint32) << 4)
                             | (row_slot(E.rl[ii]).astype(np.uint32) << 20))
            # OUT entries: per tile in (panel group, row, column) order; flagged: the last of its (row part, group) in the tile
            oo = np.nonzero(E.out & (w == ow))[0]
            if len(oo):
                j = inv[tile[oo]]
                srt = np.lexsort((E.c[oo], E.rl[oo], grp[oo], j))
                oo, j = oo[srt], j[srt]
                key = np.stack([j, grp[oo], E.rl[oo], E.part[oo]])
                last = np.append((key[:, 1:] != key[:, :-1]).any(0), True)
                sj, spos, slast = _out_slots(eoff_t)
                # slot of the entry at (tile j, position pos): invert the enumeration of the slots
                at = np.empty(len(oo), dtype=np.int64)
                at[eoff_t[sj] + spos] = np.arange(len(oo))
                lane_last_e = np.empty(len(oo), dtype=bool)
                lane_last_e[eoff_t[sj] + spos] = slast
                dst = sb + 64 * n_in + at
                t["pval"][dst] = v[oo]
                cs = ((j & (NB_RING - 1)) * CP + local[oo]).astype(np.uint32)
                pidx[dst] = (last | lane_last_e).astype(np.uint32) | (cs << 4) | (row_slot(E.rl[oo]).astype(np.uint32) << 20)
            d = _descriptors(n_in, cnt_w)
            cdesc[b, ow, :] = 0
            cdesc[b, ow, : len(d)] = d
            S[ow, 62] = n_in | (len(d) << 16)
            S[ow, 63] = run
            S[NW + 1 + ow, : T + 1] = eoff_t
            S[NW + 1 + ow, 62] = nin
            S[NW + 1 + ow, 63] = eoff_t[-1]
            run += length
    t["pval32"] = t["pval"].astype(np.float32)
    return t


def check_layout(t, rowptr, col, val, col_base, geometry=GEOMETRY, folded=True, limit=50):
    """Violations of the layout contract (strings; at most ``limit``) of the layout arrays ``t`` (numpy: ``blk_row, blk_ntile,
    blk_ndist, seg, list_cols, pval, pidx, pval32, cdesc``) of the CSR arrays ``rowptr, col, val`` whose row r is column
    ``col_base + r``.  ``folded``: built with the symmetric fold (in-block pairs stored once); an unfolded layout has no IN part."""
    out = []

    def bad(b, msg, *a):
        if len(out) < limit:
            out.append("block %s: %s" % (b, msg % a))

    nw, rmax, cp, tmax = geometry
    if (nw, rmax, cp, tmax) != GEOMETRY:
        return ["geometry %r is not the one this module decodes %r" % (geometry, GEOMETRY)]
    slots = rmax // nw
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    val = np.asarray(val, dtype=np.float64)
    n_rows, nnz = len(rowptr) - 1, int(rowptr[-1])
    blk_row = np.asarray(t["blk_row"], dtype=np.int64)
    nb = len(blk_row) - 1
    if blk_row[0] != 0 or blk_row[nb] != n_rows or np.any(np.diff(blk_row) < 0) or np.diff(blk_row).max() > rmax:
        return ["blk_row does not cut [0, %d) into non-decreasing steps of at most %d rows" % (n_rows, rmax)]
    seg = np.asarray(t["seg"]).reshape(nb, SEGROWS, SEGW)
    cdesc = np.asarray(t["cdesc"]).view(np.uint16).reshape(nb, nw, KMAX + KSLACK)
    pidx = np.asarray(t["pidx"]).view(np.uint32)
    pval = np.asarray(t["pval"])
    pval32 = np.asarray(t["pval32"])
    list_cols = np.asarray(t["list_cols"])
    if len(pval) < stream_len(nnz, nb) or len(pidx) != len(pval) or len(pval32) != len(pval):
        return ["the stream arrays hold %d entries, meld_pt_stream_len asks for %d" % (len(pval), stream_len(nnz, nb))]
    rows_d, cols_d, bits_d = [], [], []
    for b in range(nb):
        E = _block_entries(rowptr, col, blk_row, b, col_base, folded)
        S = seg[b]
        hdr = S[SEGROWS - 1]
        T, nd = int(t["blk_ntile"][b]), int(t["blk_ndist"][b])
        e0_hdr = int(np.uint32(hdr[6])) | (int(np.uint32(hdr[7])) << 32)
        if (int(hdr[2]), int(hdr[3]), int(hdr[4]), int(hdr[5]), e0_hdr) != (E.r0, E.nrows, T, nd, E.e0):
            bad(b, "header words (row0, nrows, T, ndist, entry base) %r, expected %r", (int(hdr[2]), int(hdr[3]), int(hdr[4]), int(hdr[5]), e0_hdr),
                (E.r0, E.nrows, T, nd, E.e0))
        if hdr[0] != 0 or hdr[1] != 0:
            bad(b, "symmetry sum is not zero")
        if hdr[8:].any():
            bad(b, "words behind the header are not zero")
        if E.e1 == E.e0:
            if T != 0 or nd != 0:
                bad(b, "a block without entries has T = %d, ndist = %d", T, nd)
            if S[: SEGROWS - 1].any():
                bad(b, "a block without entries has a schedule")
            continue
        exp = np.unique(E.c[E.out])
        if nd < 0 or nd > E.e1 - E.e0 or T != -(-nd // cp) or T > tmax:
            bad(b, "ndist = %d, T = %d (expected %d distinct OUT columns)", nd, T, len(exp))
            continue
        lst = list_cols[E.e0 : E.e0 + nd].astype(np.int64)
        if np.any(np.diff(lst) <= 0):
            bad(b, "list_cols is not sorted and distinct")
        if folded and np.any((lst >= col_base + E.r0) & (lst < col_base + E.r0 + E.nrows)):
            bad(b, "list_cols holds a column of the block's own row range")
        if nd != len(exp) or not np.array_equal(lst, exp):
            bad(b, "list_cols is not the set of the block's distinct OUT columns (%d listed, %d expected)", nd, len(exp))
        order = S[nw].astype(np.int64)
        if not np.array_equal(np.sort(order[:T]), np.arange(T)) or order[T:].any():
            bad(b, "the processing order is not a permutation of 0 .. T - 1 followed by zeros")
            continue
        pan = np.unique(lst >> BP_BITS)
        base_b, base_next = E.e0 + b * nw * PADCAP, E.e1 + (b + 1) * nw * PADCAP
        run = 0
        for w in range(nw):
            h = int(np.uint32(S[w, 62]))
            n_in, K, soff = h & 0xFFFF, h >> 16, int(S[w, 63])
            eoff = S[nw + 1 + w].astype(np.int64)
            nin, tot_out = int(eoff[62]), int(eoff[63])
            where = "wave %d" % w
            if S[w, :62].any():
                bad(b, "%s: words 0 .. 61 of its header row are not zero", where)
            if soff != run:
                bad(b, "%s: stream offset %d is not the running sum %d of the stream lengths", where, soff, run)
            eoff_t = eoff[: T + 1].copy()
            if eoff_t[0] != 0 or np.any(np.diff(eoff_t) < 0) or eoff_t[T] != tot_out or eoff[T + 1 : 62].any() or nin < 0 or \
                    n_in != (nin + 63) >> 6 or (not folded and nin != 0):
                bad(b, "%s: entry offsets / pair count are inconsistent (n_in_chunks %d, pairs %d, OUT entries %d)", where, n_in, nin, tot_out)
                run += 64 * n_in + tot_out
                continue
            length = 64 * n_in + tot_out
            sb = base_b + soff
            run += length
            if soff < 0 or sb + length > base_next or sb + length > len(pval):
                bad(b, "%s: stream [%d, %d) leaves the block's range [%d, %d)", where, sb, sb + length, base_b, base_next)
                continue
            # chunk descriptors
            d = _descriptors(n_in, np.diff(eoff_t))
            got = cdesc[b, w]
            if K != len(d):
                bad(b, "%s: %d chunk descriptors announced, the schedule has %d", where, K, len(d))
            if len(d) > KMAX:
                bad(b, "%s: %d chunk descriptors exceed KMAX", where, len(d))
            else:
                expd = np.zeros(KMAX + KSLACK, dtype=np.uint16)
                expd[: len(d)] = d
                if not np.array_equal(got, expd):
                    k = int(np.nonzero(got != expd)[0][0])
                    bad(b, "%s: chunk descriptor %d is 0x%x, expected 0x%x", where, k, int(got[k]), int(expd[k]))
            # ---- IN part
            gpos, lane_last = _in_slots(n_in)
            ix, v = pidx[sb : sb + 64 * n_in], pval[sb : sb + 64 * n_in]
            real = gpos < nin
            if np.any(ix[~real] != 0) or np.any(v[~real].view(np.int64) != 0):
                bad(b, "%s: padding of the IN part is not (value 0, word 0)", where)
            srt = np.argsort(gpos[real], kind="stable")
            ixr, vr, g, ll = ix[real][srt].astype(np.int64), v[real][srt], gpos[real][srt], lane_last[real][srt]
            if nin:
                si, sj = ixr >> 20, (ixr >> 4) & 0xFFF
                ri, rj = row_of(si, nw, slots), row_of(sj, nw, slots)
                if np.any(ixr & 0xE):
                    bad(b, "%s: bits 1 .. 3 of an IN index word are set", where)
                if np.any(si >= rmax) or np.any(sj >= rmax) or np.any(rj >= E.nrows) or not np.all(ri < rj):
                    bad(b, "%s: an IN pair is not (i < j) inside the block", where)
                if not np.all(ri % nw == w):
                    bad(b, "%s: an IN pair sits with a wave that does not own its row i", where)
                key = ri * rmax + rj
                if np.any(np.diff(key) <= 0):
                    bad(b, "%s: IN pairs are not in strictly increasing (row, column) order", where)
                need = np.append(ri[1:] != ri[:-1], True) | ll
                if np.any(need & ((ixr & 1) == 0)):
                    bad(b, "%s: an IN pair that ends its row, its lane's window or the part lacks the flush flag", where)
                rows_d += [E.r0 + ri, E.r0 + rj]
                cols_d += [col_base + E.r0 + rj, col_base + E.r0 + ri]
                bits_d += [vr.view(np.int64), vr.view(np.int64)]
            # ---- OUT part
            if tot_out:
                ix, v = pidx[sb + 64 * n_in : sb + length].astype(np.int64), pval[sb + 64 * n_in : sb + length]
                j, pos, lane_last = _out_slots(eoff_t)
                cs = (ix >> 4) & 0xFFF
                if np.any(ix & 0xE):
                    bad(b, "%s: bits 1 .. 3 of an OUT index word are set", where)
                if np.any((cs >> 10) != (j & (NB_RING - 1))):
                    bad(b, "%s: the tile-in-ring field of an OUT entry is not (j & 3)", where)
                sr = ix >> 20
                rl = row_of(sr, nw, slots)
                li = order[j] * cp + (cs & (cp - 1))
                if np.any(sr >= rmax) or np.any(rl >= E.nrows) or not np.all(rl % nw == w):
                    bad(b, "%s: an OUT entry names a row the wave does not own", where)
                if np.any(li >= nd):
                    bad(b, "%s: an OUT entry names a column slot beyond the block's distinct columns", where)
                cg = lst[np.minimum(li, nd - 1)] if nd else np.zeros(len(li), dtype=np.int64)
                srt = np.lexsort((pos, j))
                js, rs, cs_, fl, ll = j[srt], rl[srt], cg[srt], (ix[srt] & 1) != 0, lane_last[srt]
                grp = np.searchsorted(pan, cs_ >> BP_BITS) // TP_MAX
                same = js[1:] == js[:-1]
                k0, k1 = (grp[:-1] * rmax + rs[:-1]) * (1 << 24), (grp[1:] * rmax + rs[1:]) * (1 << 24)
                if np.any(same & ((k1 + cs_[1:]) <= (k0 + cs_[:-1]))):
                    bad(b, "%s: a segment is not in strictly increasing (panel group, row, column) order", where)
                need = np.append(~same | (rs[1:] != rs[:-1]), True) | ll
                if np.any(need & ~fl):
                    bad(b, "%s: an OUT entry that ends its row in the tile, its lane's run or the segment lacks the flush flag", where)
                rows_d.append(E.r0 + rl)
                cols_d.append(cg)
                bits_d.append(v.view(np.int64))
        if run and (pval32[base_b : base_b + run].view(np.int32) != pval[base_b : base_b + run].astype(np.float32).view(np.int32)).any():
            bad(b, "pval32 is not pval rounded to fp32 over the block's streams")
    # every nonzero exactly once, bit for bit
    rd = np.concatenate(rows_d) if rows_d else np.zeros(0, dtype=np.int64)
    cd = np.concatenate(cols_d) if cols_d else np.zeros(0, dtype=np.int64)
    bd = np.concatenate(bits_d) if bits_d else np.zeros(0, dtype=np.int64)
    rr = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(rowptr))
    if len(rd) != nnz:
        bad("*", "%d nonzeros decoded, the matrix has %d", len(rd), nnz)
    else:
        s1, s2 = np.lexsort((bd, cd, rd)), np.lexsort((val.view(np.int64), col, rr))
        miss = (rd[s1] != rr[s2]) | (cd[s1] != col[s2]) | (bd[s1] != val.view(np.int64)[s2])
        if miss.any():
            k = int(np.nonzero(miss)[0][0])
            bad("*", "%d decoded nonzeros differ from the matrix; first: decoded (%d, %d), matrix (%d, %d, %r)", int(miss.sum()), int(rd[s1][k]),
                int(cd[s1][k]), int(rr[s2][k]), int(col[s2][k]), float(val[s2][k]))
    return out


def layout_mutants(c, t):
    """(name, mutated copy) of a good layout of FULL: what the checker must report.  Host copies only: nothing mutated goes to a device."""
    def copy():
        return {k: np.array(v, copy=True) for k, v in t.items()}

    seg = np.asarray(t["seg"]).reshape(-1, SEGROWS, SEGW)
    b, w = 1, 4
    e0 = int(c.rowptr[int(t["blk_row"][b])])
    S = seg[b]
    n_in, soff = int(np.uint32(S[w, 62])) & 0xFFFF, int(S[w, 63])
    nin = int(S[NW + 1 + w, 62])
    sb = e0 + b * NW * PADCAP + soff
    gpos, _ = _in_slots(n_in)
    pad = sb + int(np.nonzero(gpos >= nin)[0][0])
    pair0, pair1 = sb + int(np.nonzero(gpos == 0)[0][0]), sb + int(np.nonzero(gpos == 5)[0][0])
    out0 = sb + 64 * n_in + 3
    m = copy(); m["pval"][out0] = 0.0; m["pidx"][out0] = 0; m["pval32"][out0] = 0.0
    yield "a dropped OUT entry", m
    m = copy()
    for k in ("pval", "pidx", "pval32"):
        m[k][pair1] = m[k][pair0]
    yield "a duplicated pair", m
    cd = np.asarray(t["cdesc"]).view(np.uint16).reshape(-1, NW, KMAX + KSLACK)
    K = int(np.uint32(S[w, 62])) >> 16
    k = next(k for k in range(n_in, K - 1) if cd[b, w, k] != cd[b, w, k + 1])
    m = copy(); v = m["cdesc"].view(np.uint16).reshape(cd.shape); v[b, w, k], v[b, w, k + 1] = cd[b, w, k + 1], cd[b, w, k]
    yield "a swapped pair of descriptors", m
    k = next(k for k in range(n_in, K) if cd[b, w, k] & D_LAST)
    m = copy(); v = m["cdesc"].view(np.uint16).reshape(cd.shape); v[b, w, k] &= ~np.uint16(D_LAST)
    yield "a cleared D_LAST", m
    m = copy(); m["list_cols"][e0 + 10], m["list_cols"][e0 + 11] = t["list_cols"][e0 + 11], t["list_cols"][e0 + 10]
    yield "a column list with two entries exchanged", m
    m = copy(); m["pval32"][out0] = np.nextafter(np.float32(t["pval32"][out0]), np.float32(4.0))
    yield "one pval32 value off by an ulp", m
    m = copy(); m["pidx"][pad] = 1 << 4
    yield "a non-zero padding word", m


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) one step in long double
# ---------------------------------------------------------------------------------------------------------------------------------
def step_reference(Wref, dw, x_full, row_begin, z=None, r=None, alpha=1.0, beta=0.0, gamma=0.0, coef=0.0, coef_x=0.0):
    """``Wref``: ``lanczos_reference.RefMatrix`` of the local rows (columns index ``x_full``); ``x_full`` [n_cols, p]; ``z``, ``r``
    [n_rows, p] or None.  Returns the record (y, r, g, m, x): reference y and r' (None without r), majorant g, row lengths, own x."""
    n = Wref.n
    xf = np.asarray(x_full, dtype=np.float64).reshape(len(x_full), -1)
    p = xf.shape[1]
    x = xf[row_begin : row_begin + n].astype(LD)
    dwl = np.asarray(dw, dtype=LD)[:, None]
    zz = np.zeros((n, p), dtype=LD) if z is None else np.asarray(z, dtype=LD).reshape(n, p)
    al, be, ga, co, cx = (LD(s) for s in (alpha, beta, gamma, coef, coef_x))
    xg = xf[Wref.indices].astype(LD)  # (only the entries' columns are widened: x_full may have millions of rows)
    Wx = np.stack([lr._row_sums(Wref.data * xg[:, c], Wref.indptr) for c in range(p)], axis=1)
    Wa = np.stack([lr._row_sums(Wref.absdata * np.abs(xg[:, c]), Wref.indptr) for c in range(p)], axis=1)
    y = al * (dwl * x - Wx) + be * x + ga * zz
    g = np.abs(al) * (np.abs(dwl * x) + Wa) + np.abs(be * x) + np.abs(ga * zz)
    rr = None if r is None else np.asarray(r, dtype=LD).reshape(n, p) + co * y + cx * x
    return SimpleNamespace(y=y, r=rr, g=g, m=np.diff(Wref.indptr)[:, None].astype(LD), x=x, r0=None if r is None else np.asarray(r, dtype=LD).reshape(n, p),
                           coef=co, coef_x=cx, tau=LD((n + Wref.longest + 16) * U))


def y_bound(ref):
    return (ref.m + 8) * U * ref.g


def r_bound(ref):
    return np.abs(ref.coef) * y_bound(ref) + 3 * U * (np.abs(ref.r0) + np.abs(ref.coef * ref.y) + np.abs(ref.coef_x * ref.x))


def step_fractions(ref, y_dev, r_dev=None):
    """Largest fraction of the y bound (and of the r bound) that a result uses: each must be <= 1."""
    fy = float(lr._fraction(np.asarray(y_dev, dtype=LD).reshape(ref.y.shape) - ref.y, y_bound(ref)).max())
    if r_dev is None:
        return fy, None
    return fy, float(lr._fraction(np.asarray(r_dev, dtype=LD).reshape(ref.y.shape) - ref.r, r_bound(ref)).max())


def dot_fractions(ref, yx_dev, yy_dev):
    """p = 1: the sums <y, x> and <y, y> over the local rows against the alpha bound of tests/lanczos_reference.py."""
    y, x, g = ref.y[:, 0], ref.x[:, 0], ref.g[:, 0]
    fx = float(lr._fraction(LD(yx_dev) - lr._dot(y, x), 4 * ref.tau * lr._dot(g, np.abs(x))))
    fy = float(lr._fraction(LD(yy_dev) - lr._dot(y, y), 4 * ref.tau * lr._dot(g, g)))
    return fx, fy


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) the cases
# ---------------------------------------------------------------------------------------------------------------------------------
def _weights(rng, n):
    """10^(-4 U) in [1e-4, 1], the range of the kernel weights: the smallest entries must count."""
    return 10.0 ** (-4.0 * rng.random(n))


def _uniq_pairs(i, j, n):
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    keep = lo != hi
    key = np.unique(lo[keep] * n + hi[keep])
    return key // n, key % n


def _case(name, n_rows, n_cols, row_begin, pairs, outs, rng, n_total=None, nb=None, status=0, dw=None, diag=None, what=""):
    """Local rows [row_begin, row_begin + n_rows) of a matrix with ``n_cols`` columns (padding included): ``pairs`` (i < j, local)
    give the shard's own square -- one value per pair, so it is bitwise symmetric --, ``outs`` (local row, global column) the rest."""
    pi, pj = _uniq_pairs(pairs[0], pairs[1], n_rows) if len(pairs[0]) else (np.zeros(0, dtype=np.int64),) * 2
    pv = _weights(rng, len(pi))
    if outs is not None and len(outs[0]):
        key = np.unique(np.asarray(outs[0], dtype=np.int64) * n_cols + np.asarray(outs[1], dtype=np.int64))
        orow, ocol = key // n_cols, key % n_cols
        assert not np.any((ocol >= row_begin) & (ocol < row_begin + n_rows))
    else:
        orow = ocol = np.zeros(0, dtype=np.int64)
    ov = _weights(rng, len(orow))
    rows, cols, vals = [pi, pj, orow], [row_begin + pj, row_begin + pi, ocol], [pv, pv, ov]
    if diag is not None:
        rows.append(np.array([diag])); cols.append(np.array([row_begin + diag])); vals.append(np.array([0.5]))
    W = sparse.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n_rows, n_cols))
    W.sort_indices()
    assert W.nnz == 2 * len(pi) + len(orow) + (diag is not None)
    forced = nb is not None
    nb = num_blocks(n_rows) if nb is None else nb
    return SimpleNamespace(name=name, W=W, rowptr=W.indptr.astype(np.int64), col=W.indices.astype(np.int32), val=W.data.astype(np.float64),
                           dw=np.ravel(W.sum(1)).astype(np.float64) if dw is None else dw, n_rows=n_rows, n_cols=n_cols, row_begin=row_begin,
                           n_total=n_cols if n_total is None else n_total, nb=nb, production=not forced or nb == num_blocks(n_rows),
                           status=status, what=what)


def _full_pairs(rng):
    n = 2 * RMAX
    i = np.arange(n)
    pi = [i[: n - d] for d in (1, 2, 3)] + [rng.integers(0, n, 3 * n)]
    pj = [i[d:] for d in (1, 2, 3)] + [rng.integers(0, n, 3 * n)]
    pi, pj = np.concatenate(pi), np.concatenate(pj)
    empty = np.array([5, RMAX + 5, 8000])
    keep = ~np.isin(pi, empty) & ~np.isin(pj, empty)
    pi, pj = pi[keep], pj[keep]
    # a long row of the second block: 40 columns below the block, then an in-block run of 60 that straddles entry 64
    R = RMAX + 1000
    extra = np.concatenate([rng.choice(np.arange(100, 4000), 40, replace=False), RMAX + rng.choice(np.arange(10, 900), 30, replace=False),
                            R + 1 + rng.choice(np.arange(10, 900), 30, replace=False)])
    return np.concatenate([pi, np.full(len(extra), R)]), np.concatenate([pj, extra]), R, empty


FULL_LONG_ROW = RMAX + 1000
FULL_EMPTY_ROWS = (5, RMAX + 5, 8000)


def _make_full():
    rng = np.random.default_rng(8160)
    pi, pj, _, _ = _full_pairs(rng)
    return _case("FULL", 2 * RMAX, 2 * RMAX, 0, (pi, pj), None, rng, nb=2, what="two blocks of 4,080 rows, banded plus random")


def _make_offset():
    rng = np.random.default_rng(8160)
    pi, pj, _, _ = _full_pairs(rng)
    n, rb, n_total, n_pad = 2 * RMAX, 1900, 11500, 11776
    rng2 = np.random.default_rng(8161)
    orow = rng2.integers(0, n, 2 * n)
    oc = rng2.integers(0, n_total - n, 2 * n)
    ocol = np.where(oc < rb, oc, oc + n)  # outside the shard's own square
    keep = ~np.isin(orow, FULL_EMPTY_ROWS)
    return _case("OFFSET", n, n_pad, rb, (pi, pj), (orow[keep], ocol[keep]), rng, n_total=n_total, nb=2,
                 what="FULL as a row shard: row_begin 1,900, 11,500 columns padded to 11,776")


def _make_seg(plus):
    rng = np.random.default_rng(32768)
    n = RMAX
    i = np.arange(n)
    a = i[(i % NW != 0) & (i + 1 < n)]
    b = i[(i % NW != 0) & (i + 13 < n)]
    pairs = (np.concatenate([a, b]), np.concatenate([a + 1, b + 13]))  # wave 0 owns no pair
    heavy = np.arange(32) * NW  # 32 rows of wave 0, every column of the tile: 32 * 1024 = 32,768 entries
    orow = [np.repeat(heavy, CP)]
    ocol = [np.tile(n + np.arange(CP), 32)]
    others = i[i % NW != 0]
    orow.append(np.repeat(others, 2)); ocol.append(n + rng.integers(0, CP, 2 * len(others)))
    if plus:
        orow.append(np.array([32 * NW])); ocol.append(np.array([n + 17]))
    return _case("SEG+1" if plus else "SEG", n, n + CP, 0, pairs, (np.concatenate(orow), np.concatenate(ocol)), rng, nb=1, status=4 if plus else 0,
                 what="one block; wave 0 holds %d entries in its one tile" % (SEG_MAX + plus))


DESC_WAVE = 3
DESC_TILES = 8
DESC_COUNTS = (4033,) * 7 + (3968,)  # 7 x 64 chunks + 62 chunks, + 2 IN chunks = 512


def _make_desc(plus):
    rng = np.random.default_rng(512)
    n = RMAX
    i = np.arange(n)
    mine = i[i % NW == DESC_WAVE]  # 340 rows
    a = mine[:100]  # 100 pairs: 2 IN chunks
    b = i[(i % NW != DESC_WAVE) & (i + 2 < n)]
    pairs = (np.concatenate([a, b]), np.concatenate([a + 1, b + 2]))
    orow, ocol = [np.full(DESC_TILES * CP, 5)], [n + np.arange(DESC_TILES * CP)]  # row 5 touches every column: rank = column - n
    for tl, cnt in enumerate(DESC_COUNTS):
        per = np.full(len(mine), cnt // len(mine))
        per[: cnt % len(mine)] += 1
        for r, k in zip(mine, per):
            orow.append(np.full(k, r)); ocol.append(n + tl * CP + rng.choice(CP - 1, k, replace=False))  # (local column CP - 1 stays free)
    if plus:
        orow.append(np.array([mine[0]])); ocol.append(np.array([n + (DESC_TILES - 1) * CP + CP - 1]))
    return _case("DESC+1" if plus else "DESC", n, n + DESC_TILES * CP, 0, pairs, (np.concatenate(orow), np.concatenate(ocol)), rng, nb=1,
                 status=4 if plus else 0, what="one block; wave %d has %d chunk descriptors over %d tiles" % (DESC_WAVE, KMAX + plus, DESC_TILES))


def _make_pairs(plus):
    rng = np.random.default_rng(8192)
    n = RMAX
    rows0 = np.arange(0, n, NW)  # wave 0
    k = np.minimum(24, n - 1 - rows0)
    short = PAIR_MAX + plus - int(k.sum())
    assert 0 < short < 300
    k[:short] += 1
    pi = [np.repeat(rows0, k)]
    pj = [np.concatenate([r + 1 + np.arange(kk) for r, kk in zip(rows0, k)])]
    i = np.arange(n - 1)
    a = i[i % NW != 0]
    pi.append(a); pj.append(a + 1)
    return _case("PAIRS+1" if plus else "PAIRS", n, n, 0, (np.concatenate(pi), np.concatenate(pj)), None, rng, nb=1, status=4 if plus else 0,
                 what="one block, a band; wave 0 owns %d IN pairs" % (PAIR_MAX + plus))


def _make_tiles(plus):
    rng = np.random.default_rng(61)
    n, nd = 256, TMAX * CP + plus
    k = np.arange(nd)
    i = np.arange(n - 1)
    return _case("TILES+1" if plus else "TILES", n, n + nd, 0, (i, i + 1), (k % n, n + k), rng, status=2 if plus else 0,
                 what="256 rows with %d distinct OUT columns" % nd)


GROUPS_PER_PANEL = 41
GROUPS_ROW_BEGIN = 1_000_000
GROUPS_COLS = 1026 * BP  # 2,101,248


def _make_groups(panels):
    rng = np.random.default_rng(panels)
    n = 256
    pan = (np.arange(panels) * 1026) // panels
    assert len(np.unique(pan)) == panels
    cols = np.sort(np.concatenate([p * BP + 1000 + rng.choice(800, GROUPS_PER_PANEL, replace=False) for p in pan]))
    k = np.arange(len(cols))
    i = np.arange(n)
    pairs = (np.concatenate([i[: n - 1], i[: n - 5]]), np.concatenate([i[1:], i[5:]]))
    return _case("GROUPS%d" % panels, n, GROUPS_COLS, GROUPS_ROW_BEGIN, pairs, (k % n, cols), rng, n_total=GROUPS_COLS - 248,
                 what="256 rows of a 2.1M-column shard touching %d bitmap panels" % panels)


COLS_MAX = NPAN_MAX * BP  # 8,388,608


def _make_cols(plus):
    rng = np.random.default_rng(4096)
    n, n_cols = 6, COLS_MAX + plus
    rb = 4_000_000
    orow = np.repeat(np.arange(n), 50)
    ocol = rng.integers(0, rb, len(orow)) + np.where(rng.random(len(orow)) < 0.5, 0, rb + n)
    orow = np.concatenate([orow, [0, 1, 2]]); ocol = np.concatenate([ocol, [0, n_cols - 1, COLS_MAX - 1]])
    return _case("COLS+1" if plus else "COLS", n, n_cols, rb, (np.array([0, 1, 2, 0]), np.array([1, 2, 5, 3])), (orow, ocol), rng,
                 status=3 if plus else 0, what="6 rows against %d columns" % n_cols)


def _make_diag():
    W = lr.matrix("M257")[0].tolil()
    W[100, 100] = 0.5
    W = W.tocsr()
    W.sort_indices()
    n = W.shape[0]
    return SimpleNamespace(name="DIAG", W=W, rowptr=W.indptr.astype(np.int64), col=W.indices.astype(np.int32), val=W.data.astype(np.float64),
                           dw=np.ravel(W.sum(1)).astype(np.float64), n_rows=n, n_cols=n, row_begin=0, n_total=n, nb=num_blocks(n), production=True,
                           status=6, what="M257 of the Lanczos reference with one diagonal entry")


SPARSE_ROWS = 3 * RMAX  # 12,240


def _make_sparse(variant):
    rng = np.random.default_rng(12240 + (variant == "B"))
    n = SPARSE_ROWS
    if variant == "A":  # every entry within the first 2,000 rows
        cand = rng.integers(0, 2000, (2, 8000))
    else:  # none in the middle block
        side = rng.integers(0, 2, (2, 8000))
        cand = rng.integers(0, RMAX, (2, 8000)) + 2 * RMAX * side
    pi, pj = _uniq_pairs(cand[0], cand[1], n)
    sel = np.sort(rng.choice(len(pi), n // 2, replace=False))  # n / 2 pairs: one entry per row on average
    dw = rng.random(n) + 0.5  # NOT the row sums: the (alpha dw + beta) x term of the rows without entries is visible
    return _case("SPARSE-" + variant, n, n, 0, (pi[sel], pj[sel]), None, rng, nb=3, dw=dw,
                 what="12,240 rows, 12,240 entries, " + ("all in the first 2,000 rows" if variant == "A" else "none in the middle block"))


PLAN1M_ROWS = 1_000_000


def _make_plan1m():
    rng = np.random.default_rng(1_000_000)
    n, h = PLAN1M_ROWS, PLAN1M_ROWS // 2
    pi, pj = [np.arange(0, h, 2)], [np.arange(1, h, 2)]  # cheap rows: adjacent pairs, one entry each
    for _ in range(3):  # three random perfect matchings of the second half
        perm = h + rng.permutation(h)
        pi.append(perm[0::2]); pj.append(perm[1::2])
    return _case("PLAN-1M", n, n, 0, (np.concatenate(pi), np.concatenate(pj)), None, rng,
                 what="1M rows at the production block count: cheap rows first, then three random matchings")


_CASES = {
    "FULL": _make_full, "OFFSET": _make_offset,
    "SEG": lambda: _make_seg(0), "SEG+1": lambda: _make_seg(1),
    "DESC": lambda: _make_desc(0), "DESC+1": lambda: _make_desc(1),
    "PAIRS": lambda: _make_pairs(0), "PAIRS+1": lambda: _make_pairs(1),
    "TILES": lambda: _make_tiles(0), "TILES+1": lambda: _make_tiles(1),
    "GROUPS384": lambda: _make_groups(384), "GROUPS385": lambda: _make_groups(385), "GROUPS769": lambda: _make_groups(769),
    "COLS": lambda: _make_cols(0), "COLS+1": lambda: _make_cols(1),
    "DIAG": _make_diag,
    "SPARSE-A": lambda: _make_sparse("A"), "SPARSE-B": lambda: _make_sparse("B"),
    "PLAN-1M": _make_plan1m,
}
ACCEPTED = ("FULL", "OFFSET", "SEG", "DESC", "PAIRS", "TILES", "GROUPS384", "GROUPS385", "GROUPS769", "COLS")
REFUSED = ("SEG+1", "DESC+1", "PAIRS+1", "TILES+1", "COLS+1", "DIAG")
PLANS = ("SPARSE-A", "SPARSE-B", "PLAN-1M")
FORCED = {"FULL": (0, RMAX, 2 * RMAX), "OFFSET": (0, RMAX, 2 * RMAX), "SPARSE-A": (0, RMAX, 2 * RMAX, 3 * RMAX), "SPARSE-B": (0, RMAX, 2 * RMAX, 3 * RMAX)}


@functools.lru_cache(maxsize=None)
def case(name):
    """A named case, built once per process and not to be modified."""
    return _CASES[name]()


def forced_blk_row(c):
    """``blk_row`` of a case whose plan has no freedom (one block, or as many rows as the blocks can hold), else None."""
    if c.nb == 1:
        return np.array([0, c.n_rows], dtype=np.int64)
    if c.nb * RMAX == c.n_rows:
        return np.arange(c.nb + 1, dtype=np.int64) * RMAX
    return None


def case_facts(c, blk_row=None):
    blk_row = forced_blk_row(c) if blk_row is None else blk_row
    return facts(c.rowptr, c.col, blk_row, c.row_begin, True, c.n_cols)


def reference(c, fp32=False):
    return lr.reference_weights(c.W, fp32)


def signals(c, p, seed=0):
    """(x_full [n_cols, p], z, r [n_rows, p]) of a case: normal deviates, the padding rows of x zero."""
    rng = np.random.default_rng([seed, p, c.n_rows])
    x = np.zeros((c.n_cols, p))
    x[: c.n_total] = rng.normal(size=(c.n_total, p))
    return x, rng.normal(size=(c.n_rows, p)), rng.normal(size=(c.n_rows, p))
