"""Host tests of tests/tiled_reference.py: every case matrix sits exactly on the edge it exists for (and its +1 twin one past it), the
numpy model of the builder passes the layout checker and mutated layouts do not, the step contract holds for scipy's own product and
fails for four mutants.  The device is held to the same checker and the same bounds in tests/test_gpu_tiled_contract.py."""
import numpy as np
import pytest

from tests import lanczos_reference as lr
from tests import tiled_reference as tr

LD = tr.LD
RMAX, NW, CP = tr.RMAX, tr.NW, tr.CP


def _own_square(c):
    return c.W[:, c.row_begin : c.row_begin + c.n_rows].tocsr()


@pytest.mark.parametrize("name", tuple(tr._CASES))
def test_structure_of_every_case(name):
    """Sorted indices, int32 columns inside the padded column range, the shard's own square bitwise symmetric, no diagonal entry
    (DIAG: exactly one), padding columns beyond n_total untouched."""
    c = tr.case(name)
    assert c.W.has_sorted_indices and c.W.shape == (c.n_rows, c.n_cols)
    assert np.all(np.diff(c.rowptr) >= 0) and c.rowptr[-1] == len(c.col) == len(c.val)
    for i in (0, c.n_rows // 2, c.n_rows - 1):
        assert np.all(np.diff(c.col[c.rowptr[i] : c.rowptr[i + 1]]) > 0)
    assert c.col.min() >= 0 and c.col.max() < c.n_total <= c.n_cols and c.row_begin + c.n_rows <= c.n_total
    S = _own_square(c)
    D = (S - S.T).tocsr()
    assert D.nnz == 0 or np.abs(D.data).max() == 0.0
    assert int((S.diagonal() != 0).sum()) == (1 if name == "DIAG" else 0)
    assert np.all(c.val > 0)
    if name not in ("DIAG", "COLS", "COLS+1"):  # (M257 keeps its own weights; COLS has 300 entries)
        assert c.val.min() < 1e-3  # weights over four decades: small entries must count


def _full_like(c):
    F = tr.case_facts(c)
    assert list(F.rows) == [RMAX, RMAX] and F.status == 0 and max(F.tiles) <= tr.TMAX
    for b in range(2):
        E = tr._block_entries(c.rowptr, c.col, tr.forced_blk_row(c), b, c.row_begin, True)
        assert np.any(E.upper & (E.cg == RMAX - 1))  # a pair with j - row0 = 4079
        last = E.rl == RMAX - 1  # the row of wave 11 in slot 339
        assert tr.row_slot(RMAX - 1) == 11 * 340 + 339 and last.any() and not (E.upper & last).any() and (E.inb & last).any()
        only_lower = np.setdiff1d(E.rl[E.inb], E.rl[E.upper])
        assert len(only_lower) > 0  # rows whose in-block entries are all lower ones (dropped: their twins are stored)
    deg = np.diff(c.rowptr)
    assert all(deg[i] == 0 for i in tr.FULL_EMPTY_ROWS)
    R = tr.FULL_LONG_ROW
    E = tr._block_entries(c.rowptr, c.col, tr.forced_blk_row(c), 1, c.row_begin, True)
    mine = E.rl == R - RMAX
    k = np.nonzero(E.inb[mine])[0]
    assert mine.sum() > 64 and k[0] < 64 < k[-1] and np.all(np.diff(k) == 1)  # one in-block run, straddling the 64-entry part
    assert (E.upper[mine]).any() and (E.inb[mine] & ~E.upper[mine]).any()
    return F


def test_full_blocks():
    c = tr.case("FULL")
    assert c.row_begin == 0 and c.n_cols == c.n_rows == 2 * RMAX and c.nb == 2
    F = _full_like(c)
    assert max(F.groups) == 1 and min(p.min() for p in F.pairs) > 0
    assert max(int(p.sum()) % 64 for p in F.pairs) > 0  # there is padding to look at


def test_offset_shard():
    c = tr.case("OFFSET")
    assert c.row_begin > 0 and c.n_cols > c.n_total > c.row_begin + c.n_rows
    _full_like(c)
    assert (c.col < c.row_begin).any() and (c.col >= c.row_begin + c.n_rows).any()


@pytest.mark.parametrize("plus", [0, 1])
def test_segment_limit(plus):
    c = tr.case("SEG+1" if plus else "SEG")
    F = tr.case_facts(c)
    assert list(F.rows) == [RMAX] and F.tiles == [1]
    assert F.seg[0][0, 0] == tr.SEG_MAX + plus == F.seg[0].max() and F.seg[0][1:].max() < tr.SEG_MAX  # largest position 0x7FFF (+ 1)
    assert F.pairs[0][0] == 0 and F.pairs[0].max() < tr.PAIR_MAX
    assert F.desc[0][0] == tr.KMAX + plus and F.desc[0][1:].max() < tr.KMAX  # 32,768 entries ARE 512 chunks: at KMAX, not beyond
    assert F.status == (4 if plus else 0) == c.status


@pytest.mark.parametrize("plus", [0, 1])
def test_descriptor_limit(plus):
    c = tr.case("DESC+1" if plus else "DESC")
    F = tr.case_facts(c)
    w = tr.DESC_WAVE
    assert list(F.rows) == [RMAX] and F.tiles == [tr.DESC_TILES]
    assert F.desc[0][w] == tr.KMAX + plus == F.desc[0].max() and np.delete(F.desc[0], w).max() < tr.KMAX
    assert sorted(F.seg[0][w]) == sorted(tr.DESC_COUNTS[:-1] + (tr.DESC_COUNTS[-1] + plus,))
    assert F.seg[0].max() < tr.SEG_MAX and F.pairs[0].max() < tr.PAIR_MAX and F.pairs[0][w] == 100  # only the descriptors are at their limit
    assert F.status == (4 if plus else 0) == c.status


@pytest.mark.parametrize("plus", [0, 1])
def test_pair_limit(plus):
    c = tr.case("PAIRS+1" if plus else "PAIRS")
    F = tr.case_facts(c)
    assert list(F.rows) == [RMAX] and F.tiles == [0] and F.ndist == [0]
    assert F.pairs[0][0] == tr.PAIR_MAX + plus == F.pairs[0].max() and F.pairs[0][1:].max() < tr.PAIR_MAX
    assert F.desc[0].max() == (tr.PAIR_MAX + plus + 63) // 64 <= tr.KMAX
    assert F.status == (4 if plus else 0) == c.status


@pytest.mark.parametrize("plus", [0, 1])
def test_tile_limit(plus):
    c = tr.case("TILES+1" if plus else "TILES")
    F = tr.case_facts(c)
    assert c.production and c.nb == 1 and F.rows[0] <= 256
    assert F.ndist == [tr.TMAX * CP + plus] and F.tiles == [tr.TMAX + plus]
    assert F.panels[0] <= tr.TP_MAX and F.seg[0].max() < tr.SEG_MAX and F.desc[0].max() < tr.KMAX
    assert F.status == (2 if plus else 0) == c.status


@pytest.mark.parametrize("panels", [384, 385, 769])
def test_panel_groups(panels):
    c = tr.case("GROUPS%d" % panels)
    F = tr.case_facts(c)
    groups = -(-panels // tr.TP_MAX)
    assert c.production and c.nb == 1 and F.rows[0] <= 256 and c.row_begin > 0 and c.n_cols > 2_000_000
    assert F.panels == [panels] and F.groups == [groups] == [(1, 2, 3)[(panels > 384) + (panels > 768)]]
    assert F.tiles[0] <= tr.TMAX and F.status == 0
    if groups > 1:
        E = tr._block_entries(c.rowptr, c.col, tr.forced_blk_row(c), 0, c.row_begin, True)
        lst = np.unique(E.c[E.out])
        pan = np.unique(lst >> tr.BP_BITS)
        grp = np.searchsorted(pan, E.c >> tr.BP_BITS) // tr.TP_MAX
        tile = np.searchsorted(lst, E.c) >> 10
        o = E.out
        # a tile shared by two groups, and a row with entries on both sides of the boundary inside that tile (two flushes)
        key = np.unique(np.stack([tile[o], grp[o]]), axis=1)
        shared = [t for t in np.unique(key[0]) if (key[0] == t).sum() > 1]
        assert len(shared) >= groups - 1
        rt = np.unique(np.stack([E.rl[o], tile[o], grp[o]]), axis=1)
        two = np.unique(rt[:2], axis=1, return_counts=True)[1]
        assert (two > 1).any()


@pytest.mark.parametrize("plus", [0, 1])
def test_column_limit(plus):
    c = tr.case("COLS+1" if plus else "COLS")
    F = tr.case_facts(c)
    assert c.production and -(-c.n_cols // tr.BP) == tr.NPAN_MAX + plus and c.col.max() == c.n_cols - 1 and c.col.min() == 0
    assert F.status == (3 if plus else 0) == c.status
    assert tr.facts(c.rowptr, c.col, tr.forced_blk_row(c), c.row_begin).status == 0  # nothing else is wrong with it


def test_diagonal_entry():
    c = tr.case("DIAG")
    assert c.production and c.nb == 2
    for blk in (tr.plan_by_time(c.rowptr, c.col, c.nb), tr.plan_by_entries(c.rowptr, c.nb)):
        F = tr.facts(c.rowptr, c.col, blk, 0, True, c.n_cols)
        assert F.status == 6 == c.status and sum(F.diag) == 1


@pytest.mark.parametrize("variant", ["A", "B"])
def test_sparse_plan_runs_by_entries_and_is_capped(variant):
    c = tr.case("SPARSE-" + variant)
    n, nnz = c.n_rows, len(c.col)
    assert n == 3 * RMAX and nnz == n and c.nb == 3
    assert tr.plan_is_by_entries(n, nnz, c.nb, scan_bytes=0)  # the stream cannot hold the weights, whatever the scan needs
    assert not tr.plan_is_by_entries(2 * RMAX, len(tr.case("FULL").col), 2, scan_bytes=1 << 16)  # (FULL has room: by time)
    blk = tr.plan_by_entries(c.rowptr, c.nb)
    assert np.array_equal(blk, tr.forced_blk_row(c)) and np.diff(blk).max() == RMAX
    # the bisection alone would have cut elsewhere: the caps decide
    raw = np.searchsorted(c.rowptr[:n], [nnz // 3, 2 * (nnz // 3)])
    if variant == "A":
        assert c.rowptr[2000] == nnz and raw[0] < raw[1] < 2000  # both cuts lifted by ``must``
    else:
        assert raw[0] < RMAX and raw[1] > 2 * RMAX  # the first lifted by ``must``, the second held by the RMAX cap
        assert c.rowptr[RMAX] == c.rowptr[2 * RMAX]  # the middle block has no entry
    F = tr.case_facts(c)
    assert F.status == 0 and [int(s.sum() + p.sum()) > 0 for s, p in zip(F.seg, F.pairs)] == ([True, False, False] if variant == "A" else [True, False, True])
    assert not np.allclose(c.dw, np.ravel(c.W.sum(1)))


def test_plan_1m_is_capped_on_most_blocks():
    c = tr.case("PLAN-1M")
    assert c.production and c.nb == 256 and c.n_rows == 1_000_000
    blk = tr.plan_by_time(c.rowptr, c.col, c.nb)
    step = np.diff(blk)
    assert blk[0] == 0 and blk[-1] == c.n_rows and step.max() == RMAX and step.min() > 0
    assert (step == RMAX).sum() > c.nb // 2
    w = tr.row_weights(c.rowptr, c.col, c.nb)
    assert w[: c.n_rows // 2].max() == tr.W_ENTRY + tr.W_ROW and w.sum() // c.nb > RMAX * (tr.W_ENTRY + tr.W_ROW)  # wants more cheap rows than fit
    assert not np.array_equal(blk, tr.plan_by_entries(c.rowptr, c.nb))
    F = tr.facts(c.rowptr, c.col, blk, 0, True, c.n_cols)
    assert F.status == 0 and max(F.panels) <= tr.TP_MAX


def test_plan_transcription_on_a_hand_example():
    """12 rows in 3 blocks of at most RMAX: no cap binds, the cuts are the first rows whose prefix reaches 1/3 and 2/3."""
    rowptr = np.array([0, 0, 3, 3, 4, 9, 9, 10, 12, 12, 12, 14, 15])
    assert list(tr.plan_by_entries(rowptr, 3)) == [0, 5, 7, 12]
    assert list(tr._plan(np.arange(13) * 7, 12, 5)) == [0, 3, 5, 8, 10, 12]
    assert tr.num_blocks(1_000_000) == 256 and tr.num_blocks(257) == 2 and tr.num_blocks(16384) == 64 and tr.num_blocks(65536) == 256


# ---------------------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------------------
def _model(name, folded=True):
    c = tr.case(name)
    return c, tr.model_layout(c.rowptr, c.col, c.val, tr.forced_blk_row(c), c.row_begin, folded)


@pytest.mark.parametrize("name", tr.ACCEPTED + ("SPARSE-A", "SPARSE-B"))
def test_model_of_the_builder_passes_the_checker(name):
    c, t = _model(name)
    assert tr.check_layout(t, c.rowptr, c.col, c.val, c.row_begin) == []


def test_unfolded_model_passes_the_checker_and_a_folded_one_is_not_unfolded():
    c, t = _model("FULL", folded=False)
    assert tr.check_layout(t, c.rowptr, c.col, c.val, c.row_begin, folded=False) == []
    c, t = _model("FULL")
    assert tr.check_layout(t, c.rowptr, c.col, c.val, c.row_begin, folded=False) != []


def test_the_checker_reports_every_mutant():
    c, t = _model("FULL")
    seen = []
    for what, m in tr.layout_mutants(c, t):
        v = tr.check_layout(m, c.rowptr, c.col, c.val, c.row_begin)
        assert v, what
        seen.append((what, v[0]))
    assert len(seen) == 7
    # and plan / header mutations
    for key, idx, val in (("blk_row", 1, RMAX - 1), ("blk_ntile", 0, 3), ("blk_ndist", 1, 7)):
        m = {k: np.array(v, copy=True) for k, v in t.items()}
        m[key][idx] = val
        assert tr.check_layout(m, c.rowptr, c.col, c.val, c.row_begin), key
    m = {k: np.array(v, copy=True) for k, v in t.items()}
    pid = m["pidx"].view(np.uint32)
    e = int(np.nonzero((pid & 1) == 1)[0][0])
    pid[e] &= ~np.uint32(1)
    assert any("flush" in s for s in tr.check_layout(m, c.rowptr, c.col, c.val, c.row_begin))


# ---------------------------------------------------------------------------------------------------------------------------------
# the step contract: holds for scipy's product, fails for mutants
# ---------------------------------------------------------------------------------------------------------------------------------
SCALARS = dict(alpha=0.7, beta=-0.3, gamma=-1.0, coef=0.25, coef_x=-0.6)


def _fp64_step(W, dw, x_full, rb, z, r, alpha, beta, gamma, coef, coef_x, ignore_coef_x=False):
    x = x_full[rb : rb + W.shape[0]]
    y = alpha * (dw[:, None] * x - W @ x_full) + beta * x + gamma * z
    return y, r + coef * y + (0.0 if ignore_coef_x else coef_x * x)


@pytest.mark.parametrize("name", ["FULL", "OFFSET", "GROUPS385", "SPARSE-B"])
@pytest.mark.parametrize("p", [1, 2])
def test_step_contract_holds_for_scipys_product(name, p):
    c = tr.case(name)
    x, z, r = tr.signals(c, p)
    ref = tr.step_reference(tr.reference(c), c.dw, x, c.row_begin, z, r, **SCALARS)
    y, r1 = _fp64_step(c.W, c.dw, x, c.row_begin, z, r, **SCALARS)
    fy, fr = tr.step_fractions(ref, y, r1)
    print("%s p=%d: scipy uses %.2e of the y bound, %.2e of the r bound" % (name, p, fy, fr))
    assert fy <= 1.0 and fr <= 1.0
    if p == 1:
        fx, fyy = tr.dot_fractions(ref, float((y * x[c.row_begin : c.row_begin + c.n_rows]).sum()), float((y * y).sum()))
        assert fx <= 1.0 and fyy <= 1.0
    # fp32 weights against the fp32 reference hold as well
    W32 = c.W.copy()
    W32.data = W32.data.astype(np.float32).astype(np.float64)
    ref32 = tr.step_reference(tr.reference(c, True), c.dw, x, c.row_begin, z, r, **SCALARS)
    y32, r32 = _fp64_step(W32, c.dw, x, c.row_begin, z, r, **SCALARS)
    assert max(tr.step_fractions(ref32, y32, r32)) <= 1.0


def test_step_contract_fails_for_mutants():
    c = tr.case("FULL")
    x, z, r = tr.signals(c, 2)
    ref = tr.step_reference(tr.reference(c), c.dw, x, 0, z, r, **SCALARS)
    # one dropped entry of smallest weight
    Wd = c.W.copy()
    e = int(np.argmin(Wd.data))
    Wd.data[e] = 0.0
    fy, fr = tr.step_fractions(ref, *_fp64_step(Wd, c.dw, x, 0, z, r, **SCALARS))
    assert fy > 1.0 and fr > 1.0, (fy, fr, c.val[e])
    # fp32 weights against the fp64 reference
    W32 = c.W.copy()
    W32.data = W32.data.astype(np.float32).astype(np.float64)
    fy, fr = tr.step_fractions(ref, *_fp64_step(W32, c.dw, x, 0, z, r, **SCALARS))
    assert fy > 1.0 and fr > 1.0
    # an in-block pair applied to one side only: (i, j) kept, (j, i) lost
    E = tr._block_entries(c.rowptr, c.col, tr.forced_blk_row(c), 0, 0, True)
    k = int(np.nonzero(E.upper)[0][100])
    i, j = int(E.rl[k]), int(E.cg[k])
    Wp = c.W.tolil()
    Wp[j, i] = 0.0
    Wp = Wp.tocsr()
    y, r1 = _fp64_step(Wp, c.dw, x, 0, z, r, **SCALARS)
    f = lr._fraction(y.astype(LD) - ref.y, tr.y_bound(ref)).max(1)
    assert f[j] > 1.0 and f[i] <= 1.0 and (f > 1.0).sum() == 1
    # coef_x ignored
    y, r1 = _fp64_step(c.W, c.dw, x, 0, z, r, ignore_coef_x=True, **SCALARS)
    fy, fr = tr.step_fractions(ref, y, r1)
    assert fy <= 1.0 and fr > 1.0
