"""A plain host reference of what the split-fp16 search stages (csrc/knn16.hip) promise, and one function per promise.

NumPy only.  Distances are sums of squared fp64 differences (all terms non-negative: relative error below (d + 2) 2^-53); every
comparison that decides a verdict is made in ``np.longdouble`` against a threshold formed in long double, and a decision closer than
``BAND`` = 1e-9 relative to its boundary -- seven orders of magnitude beyond that rounding -- is counted as undecidable and skipped
(the callers cap and print the skipped share).  Nothing here looks at how the kernels work: no tiles spheres, no fp16, no lists.

Quantities (include/meld_hip.h, "second-generation search"), for cells X, the centring mean the caller passes, queries
[q_begin, q_begin + q_count):
    s        1 / max |x - mean|                    the operand scale; "scaled units" are input d2 times s^2
    n_i      |x_i - mean|^2, n_max their maximum   (input units)
    E_i      c_const n_max + c_lin sqrt(n_i n_max) the search-error allowance of row i (input units); the coefficients are the
                                                    library's (meld_knn16_error_coef_const / _lin), handed in by the caller
    D        exact squared distances queries x references
    bw2      the (knn + 1)-th smallest of a row of D, self counted; radius2 = rf^2 bw2
    pair_min per (wave of 64 queries, tile of 64 references) the smallest D of the pair
    needed   a (wave, tile) pair with some s^2 D[p, r] <= seed_p + s^2 E_p

Every ``check_*`` takes kernel outputs as plain arrays and returns a ``Verdict``: ok, the worst margin (what it is a fraction of is
said per function; for a failed verdict it is the violation), the offending (row, reference) -- (wave, tile) for the table, (block,
tile) for the lists -- a word on which clause failed, and the share of decisions skipped as undecidable.
"""
from collections import namedtuple

import numpy as np

LD = np.longdouble
BAND = 1e-9
WAVE = 64   # queries per wave of the search kernel = references per tile (meld_knn16_tile_refs)
BLOCK = 256  # queries per workgroup (meld_knn16_block_queries)

Verdict = namedtuple("Verdict", "ok margin row ref what skipped")


def _ok(margin=0.0, skipped=0.0):
    return Verdict(True, float(margin), -1, -1, "", float(skipped))


def _bad(what, row, ref, margin=np.inf, skipped=0.0):
    return Verdict(False, float(margin), int(row), int(ref), what, float(skipped))


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference quantities
# ---------------------------------------------------------------------------------------------------------------------------------
class Setup:
    """Centred cells, scale, norms and the exact distance matrix of a query range (computed once, read-only)."""

    def __init__(self, X, mean, q_begin=0, q_count=None):
        X = np.ascontiguousarray(X, dtype=np.float64)
        self.X, self.N, self.d = X, X.shape[0], X.shape[1]
        self.q_begin, self.q_count = int(q_begin), int(self.N - q_begin if q_count is None else q_count)
        Xc = X - np.asarray(mean, np.float64)[None, :]
        self.absmax = float(np.abs(Xc).max())
        self.s = 1.0 / self.absmax if self.absmax > 0 else 1.0
        self.n = np.sum(Xc * Xc, axis=1)
        self.n_max = float(self.n.max())
        Q = X[self.q_begin:self.q_begin + self.q_count]
        D = np.zeros((self.q_count, self.N))
        for k in range(self.d):  # (one coordinate at a time: differences, never the Gram form)
            t = Q[:, k][:, None] - X[:, k][None, :]
            D += t * t
        self.D = D
        self.order = np.lexsort((np.broadcast_to(np.arange(self.N), D.shape), D), axis=1)  # by (d2, index)
        self.Ds = np.take_along_axis(D, self.order, axis=1)
        for a in (self.X, self.n, self.D, self.order, self.Ds):
            a.setflags(write=False)
        self.n_waves = -(-self.q_count // WAVE)
        self.n_tiles = -(-self.N // WAVE)
        self.n_blocks = -(-self.q_count // BLOCK)

    def allowance(self, c_const, c_lin):
        """E per query row, input units, long double."""
        nq = self.n[self.q_begin:self.q_begin + self.q_count].astype(LD)
        return LD(c_const) * LD(self.n_max) + LD(c_lin) * np.sqrt(nq * LD(self.n_max))

    def true_rows(self, ksel):
        k = min(ksel, self.N)
        return self.order[:, :k], self.Ds[:, :k]

    def bandwidth2(self, knn):
        return self.Ds[:, knn]

    def radius2(self, knn, rf):
        return (LD(rf) * LD(rf)) * self.Ds[:, knn].astype(LD)

    def _block_min(self, G):
        P = np.full((self.n_waves * WAVE, self.n_tiles * WAVE), np.inf)
        P[:G.shape[0], :G.shape[1]] = G
        return P.reshape(self.n_waves, WAVE, self.n_tiles, WAVE).min(axis=(1, 3))

    def pair_min(self):
        """[n_waves][n_tiles]: the smallest exact d2 (input units) over the pairs of a wave's queries and a tile's references."""
        return self._block_min(self.D)

    def needed(self, seeds_scaled, E):
        """(needed, undecidable) [n_waves][n_tiles]: some pair has s^2 D <= seed_p + s^2 E_p.  seeds_scaled: per query, scaled
        units (+inf allowed)."""
        s2 = LD(self.s) * LD(self.s)
        bound = (np.asarray(seeds_scaled[:self.q_count]).astype(LD) + s2 * E) / s2  # input units
        with np.errstate(invalid="ignore"):
            G = self.D - bound.astype(np.float64)[:, None]
            G[np.isinf(bound), :] = -np.inf
            rel = np.abs(G) / np.maximum(np.abs(bound.astype(np.float64))[:, None], 1e-300)
        g = self._block_min(G)
        # a pair is undecidable when no member decides it for sure: nothing clearly inside, something on the boundary
        clearly = self._block_min(np.where(rel > BAND, G, np.inf)) <= 0
        near = self._block_min(np.where(rel <= BAND, -1.0, np.inf)) < 0
        return g <= 0, near & ~clearly


def scan_order(t0, n_tiles):
    """The tiles in the order a query block scans them (meld_knn16_bounds: "the scan of every workgroup starts at its own position
    among the references and wraps around"): its own four tiles, then alternately one further on and one further back."""
    out = []
    own = BLOCK // WAVE
    for sidx in range(n_tiles):
        off = sidx
        if sidx >= own:
            j = sidx - own
            off = (-1 - (j >> 1)) if (j & 1) else own + (j >> 1)
        out.append((t0 + off) % n_tiles)
    return out


def block_origin(q_begin, b, n_tiles):
    return (q_begin // WAVE + b * (BLOCK // WAVE)) % n_tiles


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs shared by the host and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------
def make_data(kind, N, d, seed):
    """clusters: well-separated groups of 256 cells in index (= locality) order; outliers: five cells at 1000 x the spread;
    duplicates: 24 exact copies of one cell and pairs elsewhere; grid: integer coordinates; noise: isotropic."""
    rng = np.random.default_rng(seed)
    if kind == "clusters":
        k = -(-N // 256)
        centres = rng.normal(size=(k, d)) * 40.0
        X = centres[np.arange(N) // 256] + rng.normal(size=(N, d)) * np.linspace(1.0, 0.2, d)[None, :]
    elif kind == "outliers":
        X = rng.normal(size=(N, d))
        X[rng.permutation(N)[:5]] *= 1000.0
    elif kind == "duplicates":
        X = rng.normal(size=(N, d))
        X[N // 2: N // 2 + 24] = X[3]
        X[N - 20: N - 10] = X[10:20]
    elif kind == "grid":
        side = max(3, int(round((N / 3.0) ** (1.0 / d))))
        X = rng.integers(0, side, size=(N, d)).astype(np.float64)
    elif kind == "noise":
        X = rng.normal(size=(N, d))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(X * 3.5 + 2.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# contracts: operands and seeds
# ---------------------------------------------------------------------------------------------------------------------------------
U32 = 2.0 ** -24


def check_operands(ref, norm2, norm2_max, scale_info, Qn):
    """norm2[N], norm2_max, scale_info = (s, 1 / s^2, absmax) and Qn[q_count] of meld_knn16_prepare*.  Margin: the largest
    deviation as a fraction of its bound.  Bounds (fp32, u = 2^-24): a coordinate is centred in fp64, cast (u), scaled (u); its
    square carries 4 u, the FMA chain over d non-negative terms d u, the scale 1 / s^2 three more and the product one:
    (d + 12) u on norm2 and on norm2_max; absmax is a cast (u), s its reciprocal (2 u), 1 / s^2 (4 u);
    Qn[i] against norm2[q_begin + i] * s^2 with the kernel's own s: s * s, its reciprocal, the product and the value read back:
    4 u."""
    d = ref.d
    worst = 0.0
    tol_n = (d + 12) * U32
    dev = np.abs(np.asarray(norm2, np.float64) - ref.n) / np.maximum(ref.n, 1e-300)
    i = int(np.argmax(dev))
    if dev[i] > tol_n:
        return _bad("norm2", i, -1, dev[i] / tol_n)
    worst = max(worst, dev[i] / tol_n)
    dv = abs(float(norm2_max) - ref.n_max) / ref.n_max
    if dv > tol_n:
        return _bad("norm2_max", -1, -1, dv / tol_n)
    worst = max(worst, dv / tol_n)
    for j, (want, tol) in enumerate(((ref.s, 2 * U32), (1.0 / ref.s ** 2, 4 * U32), (ref.absmax, U32))):
        dv = abs(float(scale_info[j]) - want) / want
        if dv > tol:
            return _bad("scale_info[%d]" % j, -1, -1, dv / tol)
        worst = max(worst, dv / tol)
    s_k = float(scale_info[0])
    want = np.asarray(norm2, np.float64)[ref.q_begin:ref.q_begin + ref.q_count] * s_k * s_k
    dev = np.abs(np.asarray(Qn, np.float64)[:ref.q_count] - want) / np.maximum(want, 1e-300)
    i = int(np.argmax(dev))
    if dev[i] > 4 * U32:
        return _bad("Qn", i, -1, dev[i] / (4 * U32))
    return _ok(max(worst, dev[i] / (4 * U32)))


def check_seeds(ref, seeds, knn, rf):
    """Every seed (scaled units) is at least s^2 times the exact kernel radius^2 of its row.  No slack.  Margin: the smallest
    seed / (s^2 radius2) - 1 (negative: the violation)."""
    if knn + 1 > 64:
        bad = np.nonzero(~np.isposinf(np.asarray(seeds)))[0]
        return _bad("seed finite although knn + 1 > 64", bad[0], -1) if len(bad) else _ok()
    want = LD(ref.s) * LD(ref.s) * ref.radius2(knn, rf)
    got = np.asarray(seeds[:ref.q_count]).astype(LD)
    ratio = np.where(want > 0, got / np.where(want > 0, want, 1) - 1, np.where(got >= 0, np.inf, -np.inf))
    i = int(np.argmin(ratio))
    if got[i] < want[i]:
        return _bad("seed below the kernel radius", i, int(ref.order[i, knn]), ratio[i])
    return _ok(ratio[i])


# ---------------------------------------------------------------------------------------------------------------------------------
# contracts: bounds and lists
# ---------------------------------------------------------------------------------------------------------------------------------
def check_bounds(ref, lb2, needed=None, undecidable=None):
    """lb2[n_waves][n_tiles] (scaled units, any float type): every finite entry is at most s^2 pair_min; +inf only where the pair
    is not needed (needed = None: no entry may be +inf... unless pair_min is).  No slack.  Margin: the largest finite
    lb2 / (s^2 pair_min) (> 1: the violation)."""
    lb = np.asarray(lb2, np.float64)[:ref.n_waves]
    pm = ref.pair_min().astype(LD) * (LD(ref.s) * LD(ref.s))
    fin = np.isfinite(lb)
    over = fin & (lb.astype(LD) > pm)
    ratio = np.where(fin & (pm > 0), lb / np.where(pm > 0, pm, 1).astype(np.float64), 0.0)
    if over.any():
        w, t = np.argwhere(over)[int(np.argmax(ratio[over]))] if ratio[over].max() > 0 else np.argwhere(over)[0]
        return _bad("bound above the pair's exact minimum", w, t, ratio[w, t] if pm[w, t] > 0 else np.inf)
    if np.isnan(lb).any() or (lb < 0).any():
        w, t = np.argwhere(np.isnan(lb) | (lb < 0))[0]
        return _bad("bound negative or NaN", w, t)
    need = np.ones_like(fin) if needed is None else needed
    und = np.zeros_like(fin) if undecidable is None else undecidable
    wrong = np.isposinf(lb) & need & ~und & np.isfinite(pm.astype(np.float64))
    if wrong.any():
        w, t = np.argwhere(wrong)[0]
        return _bad("+inf on a needed pair", w, t, skipped=und.mean())
    return _ok(ratio.max(), und.mean())


def decode_lists(lst, cnt, stride):
    """[(tiles, masks)] per block from list[b * stride + i] = tile | mask << 24."""
    lst = np.ascontiguousarray(lst).reshape(-1)
    lst = lst.view(np.uint32) if lst.dtype == np.int32 else lst.astype(np.uint32)
    out = []
    for b, c in enumerate(np.asarray(cnt)):
        e = lst[b * stride: b * stride + max(int(c), 0)]
        out.append(((e & 0xFFFFFF).astype(np.int64), (e >> 24).astype(np.int64)))
    return out


def check_lists(ref, lst, cnt, stride, needed, undecidable=None, thinned=False, work=None):
    """Step lists of every query block: cnt >= 1, entries distinct tiles in scan order starting at the block's own position (a
    thinned list: a subsequence of it), no bit beyond the block's waves... of a needed (wave, tile) pair missing; work[b] (when
    given) equals the length.  Margin: the share of (wave, tile) pairs the lists leave out."""
    und = np.zeros_like(needed) if undecidable is None else undecidable
    cnt = np.asarray(cnt)
    if len(cnt) < ref.n_blocks:
        return _bad("fewer counts than blocks", len(cnt), -1)
    lists = decode_lists(lst, cnt[:ref.n_blocks], stride)
    listed = 0
    for b, (tiles, masks) in enumerate(lists):
        if cnt[b] < 1 or cnt[b] > ref.n_tiles:
            return _bad("count outside [1, n_tiles]", b, -1)
        if work is not None and int(work[b]) != int(cnt[b]):
            return _bad("work differs from the list length", b, -1)
        if tiles.min() < 0 or tiles.max() >= ref.n_tiles:
            return _bad("tile out of range", b, tiles.max())
        if len(set(tiles.tolist())) != len(tiles):
            return _bad("tile listed twice", b, tiles[np.argmax(np.bincount(tiles))])
        order = scan_order(block_origin(ref.q_begin, b, ref.n_tiles), ref.n_tiles)
        pos = {t: i for i, t in enumerate(order)}
        p = np.array([pos[t] for t in tiles.tolist()])
        if np.any(np.diff(p) <= 0):
            return _bad("entries not in scan order", b, tiles[1 + int(np.argmax(np.diff(p) <= 0))])
        if not thinned and tiles[0] != order[0]:
            return _bad("list does not start at the block's own position", b, tiles[0])
        have = np.zeros((BLOCK // WAVE, ref.n_tiles), bool)
        for w in range(BLOCK // WAVE):
            have[w, tiles[(masks >> w) & 1 == 1]] = True
        for w in range(BLOCK // WAVE):
            gw = b * (BLOCK // WAVE) + w
            if gw >= ref.n_waves:
                break
            miss = needed[gw] & ~und[gw] & ~have[w]
            if miss.any():
                return _bad("needed pair missing from the list", gw, int(np.nonzero(miss)[0][0]), skipped=und.mean())
            listed += int(have[w].sum())
    return _ok(1.0 - listed / float(ref.n_waves * ref.n_tiles), und.mean())


# ---------------------------------------------------------------------------------------------------------------------------------
# contracts: candidate rows
# ---------------------------------------------------------------------------------------------------------------------------------
def check_rows(ref, idx, d2, cnt, ksel, E, thr=None, exact_rule=False, radius2=None):
    """Candidate rows idx / d2 [rows >= q_count][>= ksel], cnt, in input units; E per row; thr: per row, the bound the row was
    searched under (the published cand_thr, or the start threshold over s^2), or None.
      count in [1, ksel]; indices in [0, N), distinct; sorted by (d2, index); |d2 - exact| <= E_row;
      completeness: tau = min(d2[ksel - 1] if the row is full else +inf, thr): every reference with exact d2 < tau - E_row is there;
      exact_rule (no seeds, no cut): every reference with exact d2 < (exact ksel-th) - 2 E_row is there;
      radius2 (the cut; rows that are NOT full -- a full row can hold no more and is covered by tau): every reference with exact
      d2 <= radius2 is there and thr >= radius2.
    Margin: the largest |d2 - exact| / E_row."""
    N, D = ref.N, ref.D
    worst, skipped, decided = 0.0, 0, 0
    for i in range(ref.q_count):
        n = int(cnt[i])
        if n < 1 or n > ksel:
            return _bad("count outside [1, ksel]", i, -1)
        ids = np.asarray(idx[i, :n]).astype(np.int64)
        if ids.min() < 0 or ids.max() >= N:
            return _bad("index out of range", i, ids.max())
        if len(np.unique(ids)) != n:
            u, c = np.unique(ids, return_counts=True)
            return _bad("duplicate index", i, u[np.argmax(c)])
        a = np.asarray(d2[i, :n])
        if np.isnan(a).any():
            return _bad("NaN distance", i, ids[int(np.argmax(np.isnan(a)))])
        okk = (a[1:] > a[:-1]) | ((a[1:] == a[:-1]) & (ids[1:] > ids[:-1]))
        if not okk.all():
            return _bad("row not sorted by (d2, index)", i, ids[1 + int(np.argmin(okk))])
        Ei = LD(E[i])
        err = np.abs(a.astype(LD) - D[i, ids].astype(LD))
        j = int(np.argmax(err))
        if err[j] > Ei:
            return _bad("approximate d2 beyond the allowance", i, ids[j], err[j] / Ei)
        worst = max(worst, float(err[j] / Ei))
        inrow = np.zeros(N, bool)
        inrow[ids] = True
        Di = D[i].astype(LD)
        bounds = []
        tau = LD(a[ksel - 1]) if n == ksel else LD(np.inf)
        if thr is not None:
            tau = min(tau, LD(thr[i]))
        bounds.append(("reference below tau - E missing", tau - Ei, False))
        if exact_rule and N >= ksel:
            bounds.append(("reference below the exact ksel-th - 2E missing", LD(ref.Ds[i, ksel - 1]) - 2 * Ei, False))
        if radius2 is not None and n < ksel:
            r2 = LD(radius2[i])
            if thr is not None and LD(thr[i]) < r2 * (1 - LD(BAND)):
                return _bad("published threshold below the kernel radius", i, -1, float(LD(thr[i]) / r2))
            bounds.append(("reference inside the kernel radius missing", r2, True))
        for what, bnd, closed in bounds:
            if np.isinf(bnd):
                if bnd > 0 and not inrow.all():
                    return _bad(what + " (unbounded row)", i, int(np.argmin(inrow)))
                continue
            near = np.abs(Di - bnd) <= LD(BAND) * max(abs(bnd), LD(1e-300))
            inside = ((Di <= bnd) if closed else (Di < bnd)) & ~near
            skipped += int(near.sum())
            decided += N
            miss = inside & ~inrow
            if miss.any():
                r = int(np.argmin(np.where(miss, D[i], np.inf)))
                return _bad(what, i, r, float((bnd - Di[r]) / Ei), skipped / max(decided, 1))
    return _ok(worst, skipped / max(decided, 1))


def research_threshold_ref(ref, rows, d2, cnt, ksel, E1, e3_coef):
    """fp64 value of the documented start threshold of the re-search, scaled units: (tau + E1 + E3) s^2 for rows with a full first
    list (tau = their last entry), +inf otherwise.  rows: local rows; E1 per local row."""
    out = np.full(len(rows), np.inf)
    for k, r in enumerate(rows):
        if int(cnt[r]) >= ksel:
            out[k] = float((LD(d2[r, ksel - 1]) + LD(E1[r]) + LD(e3_coef) * LD(ref.n_max)) * LD(ref.s) * LD(ref.s))
    return out


def check_research(ref, rows, thr, d2, cnt, ksel, E1, e3_coef, upper_rel):
    """thr[k] for local row rows[k]: not below the documented value, not below s^2 (exact ksel-th + E3), +inf exactly on short
    lists, and not above the documented value by more than ``upper_rel`` (the caller derives it from the kernel's operation
    count).  Margin: the largest thr / documented - 1."""
    want = research_threshold_ref(ref, rows, d2, cnt, ksel, E1, e3_coef)
    worst = 0.0
    for k, r in enumerate(rows):
        t = float(thr[k])
        if np.isinf(want[k]):
            if not np.isposinf(t):
                return _bad("short list without +inf", r, -1)
            continue
        if not np.isfinite(t):
            return _bad("full list with a threshold that is not finite", r, -1)
        if t < want[k]:
            return _bad("threshold below tau + E1 + E3", r, -1, t / want[k] - 1)
        floor = float((LD(ref.Ds[r, ksel - 1]) + LD(e3_coef) * LD(ref.n_max)) * LD(ref.s) * LD(ref.s))
        if t < floor:
            return _bad("threshold below the exact ksel-th distance + E3", r, int(ref.order[r, ksel - 1]), t / floor - 1)
        if t > want[k] * (1 + upper_rel):
            return _bad("threshold above the documented value", r, -1, t / want[k] - 1)
        worst = max(worst, t / want[k] - 1)
    return _ok(worst)


# ---------------------------------------------------------------------------------------------------------------------------------
# conditions on the inputs, decided by the reference alone
# ---------------------------------------------------------------------------------------------------------------------------------
def share_not_needed(ref, seeds_scaled, E):
    need, und = ref.needed(seeds_scaled, E)
    return float((~need).mean()), float(und.mean())


def share_cut_engages(ref, knn, rf, ksel, E):
    """Share of rows with fewer than ksel references at exact d2 <= rf^2 (A + E) + 2 E, A = the exact bandwidth^2."""
    A = ref.bandwidth2(knn).astype(LD)
    lim = (LD(rf) * LD(rf)) * (A + E) + 2 * E
    inside = (ref.D.astype(LD) <= lim[:, None]).sum(axis=1) if ref.N <= 1100 else (ref.D <= lim.astype(np.float64)[:, None]).sum(axis=1)
    return float((inside < ksel).mean())


def share_allowance_beyond_neighbour(ref, E):
    """Share of rows whose allowance exceeds their nearest OTHER cell's d2."""
    return float((E.astype(np.float64) > ref.Ds[:, 1]).mean())


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_search_contract.py; tests/test_search_reference.py runs their host conditions
# ---------------------------------------------------------------------------------------------------------------------------------
RF = float((-np.log(1e-4)) ** (1.0 / 40.0))  # radius factor of the default kernel (decay 40, thresh 1e-4)

# name: kind, N, d, knn, ksel, q_begin, q_count (None: all).  What each is the smallest shape for:
#   clusters    4096 x 14: 64 tiles, 16 blocks; first split dimension (K block 0 + one more); pruning is real; the cut engages
#   clusters_q  1025 x 50: the product's d, queries a ragged range at a non-zero multiple of the block size, ksel 65 (two per lane)
#   outliers    1025 x 13: last unsplit d, one tile plus one cell beyond a block multiple, n_max >> n_i, ksel 8
#   duplicates   200 x 2 : fewer cells than one query block, no split, 24 copies of a cell (> knn + 1), zero distances
#   grid        1025 x 2 : ties at every threshold, ksel 128 = the largest meld_knn16_row_capacity accepts
#   noise       1025 x 141: nine K blocks, nothing can be pruned
#   tiny          65 x 50: one tile plus one cell; knn + 1 = 63
CASES = {
    "clusters": dict(kind="clusters", N=4096, d=14, knn=7, ksel=64, q_begin=0, q_count=None, seed=11),
    "clusters_q": dict(kind="clusters", N=1025, d=50, knn=15, ksel=65, q_begin=256, q_count=513, seed=12),
    "outliers": dict(kind="outliers", N=1025, d=13, knn=5, ksel=8, q_begin=0, q_count=None, seed=13),
    "duplicates": dict(kind="duplicates", N=200, d=2, knn=5, ksel=64, q_begin=0, q_count=None, seed=14),
    "grid": dict(kind="grid", N=1025, d=2, knn=7, ksel=128, q_begin=0, q_count=None, seed=15),
    "noise": dict(kind="noise", N=1025, d=141, knn=10, ksel=64, q_begin=0, q_count=None, seed=16),
    "tiny": dict(kind="noise", N=65, d=50, knn=62, ksel=64, q_begin=0, q_count=None, seed=17),
}
_SETUPS = {}


def case_setup(name):
    """(case dict, cells, mean, Setup), computed once per case and never modified."""
    if name not in _SETUPS:
        c = CASES[name]
        X = make_data(c["kind"], c["N"], c["d"], c["seed"])
        mean = X.mean(axis=0)
        _SETUPS[name] = (c, X, mean, Setup(X, mean, c["q_begin"], c["q_count"]))
    return _SETUPS[name]


def loose_seeds(ref, knn, rf, E, factor=3.0):
    """Start thresholds (scaled units) as loose as the suite lets the kernel's be (test_mfma_threshold_seeds_bound_the_kernel_radius:
    within 3 x of the radius): factor * s^2 * (rf^2 (bw2 + E) + E).  For the host conditions only."""
    s2 = LD(ref.s) * LD(ref.s)
    return (LD(factor) * s2 * ((LD(rf) * LD(rf)) * (ref.bandwidth2(knn).astype(LD) + E) + E)).astype(np.float64)
