"""The list filter (``knn16_partial_filter_kernel``, csrc/knn16.hip) called directly on hand-made operands, every verdict decided by
NumPy with no tolerance.

The kernel walks, per step of eight list entries, the set of tiles that list a wave (a scalar mask, ``s_ff1``), software-pipelined
at half-pair granularity, and forms a wave-uniform verdict from two compare masks (the second query group is skipped when the
first already hit); its tiles are staged from one buffer descriptor over the whole ``Rt16`` array, or from one per piece where the
launcher cannot bound the array below 4 GiB (``test_filter_with_a_descriptor_per_piece``).  What can go wrong there is a matter of list lengths, of which entries of a step list a wave, and of
where in the 64 x 64 block of partial values the one value below the threshold sits -- none of it a matter of size, so the shapes
are the smallest that reach every path:

  queries    512 = two query blocks (a workgroup each, so block 1 reads its own list, thresholds and queries); one case with 256
  tiles      40 at KB = 4 (d = 50), 37 at KB = 7 (d = 100): more than two steps' worth of distinct tiles, the last tile of the array
             listed (the end of the descriptor), an odd count; KB = 7 moves every tile (28 KiB apart instead of 16) and runs the
             |q_hiB|^2 loop over six K blocks
  lists      0, 1, 7, 8, 9, 16 and 17 entries: empty, one pair, a partial last step, exactly one step, a step boundary, exactly two
             steps (both ring buffers), two steps and one entry

Operands.  K block 0 holds, per reference and per query, sixteen fp16 slots: slots 0..7 one *plant* slot per wave of the launch,
8..12 noise in [-3, 3], 13 the reference's norm piece (100, or +inf on a padding row) against the query's 1.0, 14..15 zero.  All
values are small integers: every fp16 product and every fp32 partial sum is exact.  A *planted* query of wave W carries 8 in slot W
and no noise, a reference planted for W carries -8 there: their partial value is 100 - 64 = 36, every other value of that query is
100, and the query's threshold 36.5 lies strictly between -- so wave W must keep tile t exactly if t holds a reference planted for
W, and the position of the plant (query group, reference half, lane) is chosen per wave:

  wave 0   query 5  (group 0 only);  reference half A on even tiles, half B on odd ones
  wave 1   query 37 (group 1 only);  half B on even tiles, half A on odd ones
  wave 2   query 63, reference row 63: the value sits in lane 63 alone (group 1, half B)
  wave 3   query 31, reference row 31: lane 63 alone (group 0, half A)
  wave 4   query 0, reference row 0: lane 0 alone
  wave 5   query 49; on ragged tiles (rows 41.. are padding, +inf) the plant sits in row 40, next to the padding
  wave 6   query 9 carries 1 in its slot, references -3 or -4: values 97 and 96 against the INTEGER threshold 97 -- the tile with
           97 must be dropped (the test is <), the tile with 96 kept
  wave 7   three planted queries (3, 40, 63), both groups

Every other query has the threshold -1000.5 (never hit) in the "plants" mode.  The "noise" mode instead gives three queries per wave
a threshold half-way between two of their own partial values over the noise slots (about a third of the tiles below it), so hits sit
wherever the random values put them.  "drop" and "keep" put all thresholds at -1000.5 / +1000.5.  Everything outside K block 0's
hi planes (lo planes, the other K blocks of the tiles, the lo planes of the queries) is filled with 1000.0: a piece staged from a
wrong offset, or a wrong plane, fails every case.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TS, BQ = 64, 256  # references per tile, queries per block (checked against the library)
SENTINEL = 0x7EADBEEF  # list positions behind a list's end: never read, never written
SHAPES = {4: (50, 40), 7: (100, 37)}  # KB -> (d, tiles)
NORM = 100.0


def _env():
    import torch

    from meld_amd._lib import check, get_lib, ptr
    from meld_amd.graph import _stream

    return torch, get_lib(), check, ptr, _stream()


_OPS = {}


def operands(KB):
    """Host and device operands for one KB, made once and never modified: R [T][64][16], Qv [512][16] (K block 0 as integers),
    m [T][512] = the smallest partial value of every (tile, query), and the device arrays in the kernel's layouts."""
    if KB in _OPS:
        return _OPS[KB]
    torch, lib, check, ptr, st = _env()
    d, T = SHAPES[KB]
    assert lib.meld_knn16_kblocks(d) == KB and lib.meld_knn16_split_dims(d) > 0
    assert (lib.meld_knn16_tile_refs(), lib.meld_knn16_block_queries()) == (TS, BQ)
    assert lib.meld_knn16_tile_bytes(d) == KB * 4096 and lib.meld_knn16_query_bytes(d) == KB * 64
    rng = np.random.default_rng(1000 + KB)
    nq = 2 * BQ
    R = np.zeros((T, TS, 16))
    Qv = np.zeros((nq, 16))
    R[:, :, 8:13] = rng.integers(-3, 4, size=(T, TS, 5))
    Qv[:, 8:13] = rng.integers(-3, 4, size=(nq, 5))
    R[:, :, 13] = NORM
    Qv[:, 13:16] = 1.0
    ragged = np.array([t % 5 == 3 for t in range(T)])
    planted_q = {0: [5], 1: [37], 2: [63], 3: [31], 4: [0], 5: [49], 6: [9], 7: [3, 40, 63]}
    want = rng.random((8, T)) < 0.45  # which (wave, tile) pairs hold a plant
    want[:, T - 1] = True  # (the last tile of the array is kept by every wave)
    for W in range(8):
        for qi in planted_q[W]:
            Qv[W * 64 + qi, :] = 0.0
            Qv[W * 64 + qi, 13:16] = 1.0
            Qv[W * 64 + qi, W] = 1.0 if W == 6 else 8.0
    for t in range(T):
        for W in range(8):
            if W == 6:  # every tile: 97 (== threshold, dropped) or 96 (kept)
                R[t, (7 * t) % 41, W] = -4.0 if want[W, t] else -3.0
                continue
            if not want[W, t]:
                continue
            row = {0: (t % 2) * 32 + (t % 29), 1: (1 - t % 2) * 32 + (t % 31), 2: 63, 3: 31, 4: 0, 5: 40 if ragged[t] else 33,
                   7: (11 * t) % 41}[W]
            if ragged[t] and row > 40:  # (a plant on a padding row would be no plant: lane 63's waves keep whole tiles)
                continue
            R[t, row, W] = -8.0
    for t in np.nonzero(ragged)[0]:  # padding rows as the operand kernels write them: zero coordinates, +inf norm
        R[t, 41:, :] = 0.0
        R[t, 41:, 13] = np.inf
    with np.errstate(invalid="ignore"):
        c = np.einsum("trk,qk->trq", np.where(np.isinf(R), 0.0, R), Qv) + np.where(np.isinf(R[:, :, 13]), np.inf, 0.0)[:, :, None]
    m = c.min(axis=1)  # [T][nq]
    # device layouts.  Rt16: tile = KB x [k-half][plane][ref][8 halves]; Q16: row = KB x [k-half][plane][8 halves]
    Rt = np.full((T, 2 * KB, 2, TS, 8), 1000.0, dtype=np.float16)
    Q = np.full((nq, 2 * KB, 2, 8), 1000.0, dtype=np.float16)
    for g in range(2):
        Rt[:, g, 0] = R[:, :, 8 * g:8 * g + 8].astype(np.float16)
        Q[:, g, 0] = Qv[:, 8 * g:8 * g + 8].astype(np.float16)
    Q[:, 2:, 0] = 0.0  # hi planes of the K blocks behind the first: |q_hiB|^2 = 0, the threshold stays what the test sets
    o = dict(KB=KB, d=d, T=T, R=R, Qv=Qv, m=m, planted_q=planted_q, want=want, ragged=ragged,
             Rt=torch.from_numpy(Rt.view(np.uint8).reshape(-1)).cuda(), Q=torch.from_numpy(Q.view(np.uint8).reshape(-1)).cuda(),
             Qn=torch.zeros(nq, dtype=torch.float32, device="cuda"), nmax=torch.zeros(1, dtype=torch.float32, device="cuda"),
             sinfo=torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float32, device="cuda"))
    _OPS[KB] = o
    return o


def thresholds(o, mode):
    nq, m = 2 * BQ, o["m"]
    thr = np.full(nq, -1000.5, dtype=np.float32)
    if mode == "keep":
        thr[:] = 1000.5
    elif mode == "plants":
        for W, qs in o["planted_q"].items():
            for qi in qs:
                thr[W * 64 + qi] = 97.0 if W == 6 else 36.5
    elif mode == "noise":
        rng = np.random.default_rng(7)
        for W in range(8):
            free = [qi for qi in range(64) if qi not in o["planted_q"][W]]
            for qi in rng.choice(free, size=3, replace=False):
                v = np.sort(m[:, W * 64 + qi])
                k = len(v) // 3
                while v[k] == v[k - 1]:
                    k += 1
                thr[W * 64 + qi] = v[k - 1] + 0.5  # (the values are integers: strictly between two of them, exact in fp32)
                assert v[k - 1] == np.floor(v[k - 1]) and v[k] >= v[k - 1] + 1.0
    else:
        assert mode == "drop"
    return thr


def step_masks(i):
    """Masks of the seventeen-entry layout case: step 0 lists wave 0 in all eight entries, wave 2 in none, wave 1 in exactly one;
    step 1 lists wave 2 in all eight, wave 0 in none, wave 3 in exactly one; the last entry lists all four."""
    if i < 8:
        return 1 | (2 if i == 3 else 0) | (8 if i % 3 == 0 else 0)
    if i < 16:
        return 4 | (8 if i == 13 else 0) | (2 if i % 2 == 0 else 0)
    return 15


# name: (lengths per block, masks(block, entry) -> 1..15, threshold mode)
_mix = np.random.default_rng(3).integers(1, 16, size=(2, 64))
SCENARIOS = {
    "empty+one": ((0, 1), lambda b, i: 15, "plants"),
    "7+8 all waves": ((7, 8), lambda b, i: 15, "plants"),
    "9+16 mixed masks": ((9, 16), lambda b, i: int(_mix[b, i]), "plants"),
    "17+17 mixed masks": ((17, 17), lambda b, i: int(_mix[b, i + 20]), "plants"),
    "17 layout / single wave": ((17, 16), lambda b, i: step_masks(i) if b == 0 else 4, "plants"),
    "17+9 noise": ((17, 9), lambda b, i: int(_mix[b, i + 40]), "noise"),
    "16+17 noise all waves": ((16, 17), lambda b, i: 15, "noise"),
    "all dropped": ((17, 8), lambda b, i: int(_mix[b, i]), "drop"),
    "all kept": ((17, 9), lambda b, i: int(_mix[b, i + 7]), "keep"),
    "one block": ((17,), lambda b, i: int(_mix[1, i]), "plants"),
}


def expected(o, lens, masks, thr, lists):
    m = o["m"]
    out, cnt, tested = lists.copy(), [], 0
    for b, n in enumerate(lens):
        kept = []
        for i in range(n):
            t, mask = int(lists[b, i]) & 0xFFFFFF, int(lists[b, i]) >> 24
            assert mask == masks(b, i)
            tested += bin(mask).count("1")
            nm = 0
            for w in range(4):
                q = slice((4 * b + w) * 64, (4 * b + w + 1) * 64)
                if (mask >> w) & 1 and bool((m[t, q] < thr[q]).any()):
                    nm |= 1 << w
            if nm:
                kept.append(t | (nm << 24))
        out[b, :len(kept)] = kept
        cnt.append(len(kept))
    return out, np.array(cnt, dtype=np.int32), tested


@pytest.mark.parametrize("KB", [4, 7])
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_filter_verdicts_lists_and_counts(name, KB):
    """The thinned lists, ``cnt_out`` and ``tested`` equal what NumPy derives from the exact partial values; list positions behind
    the new length keep what they held (the rewrite never runs ahead of, or behind, what it has read); a second call on the same
    inputs returns the same bytes."""
    _run(name, KB, None)


@pytest.mark.parametrize("KB", [4, 7])
def test_filter_with_a_descriptor_per_piece(KB):
    """The launcher stages from one buffer descriptor where ``list_stride`` tiles are shorter than 4 GiB and from a descriptor per
    piece otherwise.  A list stride of 2^18 entries (1 MiB per list; legal: the stride only has to hold the tiles) is the smallest that
    selects the second kernel at KB = 4 (2^18 x 16 KiB = 4 GiB exactly); the operands stay the 40 / 37 tiles they are."""
    _run("17+17 mixed masks", KB, 1 << 18)


def _run(name, KB, stride):
    torch, lib, check, ptr, st = _env()
    o = operands(KB)
    lens, masks, mode = SCENARIOS[name]
    n_tiles, nb = o["T"], len(lens)
    T = stride or n_tiles  # the stride of the lists
    assert (T * KB * 4096 >= 1 << 32) == (stride is not None)
    thr = thresholds(o, mode)
    rng = np.random.default_rng(11)
    lists = np.full((nb, T), SENTINEL, dtype=np.int64)
    for b, n in enumerate(lens):
        tiles = rng.permutation(n_tiles - 1)[:max(n - 1, 0)].tolist()
        if n:
            tiles.insert(n // 2, n_tiles - 1)  # the last tile of the array in every list
        for i, t in enumerate(tiles):
            lists[b, i] = t | (masks(b, i) << 24)
    want_list, want_cnt, want_tested = expected(o, lens, masks, thr, lists)
    if mode == "plants":  # the construction itself: a listed wave keeps a tile exactly if the tile holds its plant
        for b, n in enumerate(lens):
            bits = {int(e) & 0xFFFFFF: int(e) >> 24 for e in want_list[b, :want_cnt[b]]}
            for i in range(n):
                t, mask = int(lists[b, i]) & 0xFFFFFF, int(lists[b, i]) >> 24
                plant = sum(1 << w for w in range(4) if (mask >> w) & 1 and (o["R"][t, :, 4 * b + w] <= (-4.0 if 4 * b + w == 6 else -8.0)).any())
                assert bits.get(t, 0) == plant, (b, i, t, mask)
    elif mode == "drop":
        assert not want_cnt.any()
    elif mode == "keep":
        assert (want_list == lists).all() and list(want_cnt) == list(lens)
    thr_d = torch.from_numpy(thr).cuda()
    cnt_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    runs = []
    for _ in range(2):
        lst_d = torch.from_numpy(lists.astype(np.uint32).view(np.int32).reshape(-1)).cuda()
        out_d = torch.full((nb,), -7, dtype=torch.int32, device="cuda")
        tested = torch.zeros(1, dtype=torch.int64, device="cuda")
        check(lib.meld_knn16_partial_filter(ptr(o["Q"]), ptr(o["Qn"]), ptr(o["Rt"]), ptr(o["sinfo"]), ptr(o["nmax"]), o["d"], nb * BQ, ptr(thr_d),
                                            ptr(lst_d), ptr(cnt_d), T, ptr(out_d), ptr(tested), None, st), "partial_filter")
        torch.cuda.synchronize()
        runs.append((lst_d.cpu().numpy().view(np.uint32).astype(np.int64).reshape(nb, T), out_d.cpu().numpy(), int(tested.item())))
    got_list, got_cnt, got_tested = runs[0]
    kept_pairs = sum(bin(int(e) >> 24).count("1") for b in range(nb) for e in got_list[b, :max(int(got_cnt[b]), 0)])
    print("FILTER-PIPELINE {} KB={}: listed pairs {} kept pairs {} entries {} -> {}".format(name, KB, want_tested, kept_pairs, list(lens),
                                                                                      list(got_cnt)))
    assert list(got_cnt) == list(want_cnt)
    assert got_tested == want_tested
    assert (got_list == want_list).all(), np.argwhere(got_list != want_list)[:8]
    assert (runs[1][0] == got_list).all() and (runs[1][1] == got_cnt).all() and runs[1][2] == got_tested
    assert list(cnt_d.cpu().numpy()) == list(lens)  # (step_cnt is an input: not written when cnt_out is another array)


def test_filter_cases_cover_what_they_claim():
    """The hand-made operands do hold the situations the module names (so that a change to the generator cannot empty a case)."""
    for KB in (4, 7):
        o = operands(KB)
        m, want, T = o["m"], o["want"], o["T"]
        thr = thresholds(o, "plants")
        hit = np.array([[bool((m[t, W * 64:(W + 1) * 64] < thr[W * 64:(W + 1) * 64]).any()) for t in range(T)] for W in range(8)])
        assert hit.any(axis=1).all() and (~hit).any(axis=1).all()  # every wave keeps some tiles and drops some
        assert (hit[6] == want[6]).all()
        assert (m[:, 6 * 64 + 9] == np.where(want[6], 96.0, 97.0)).all()  # equality with the threshold on every dropped tile of wave 6
        assert o["ragged"].any() and hit[5][o["ragged"]].any()  # a plant next to padding rows that is kept
        assert np.isinf(o["R"][o["ragged"]][:, 41:, 13]).all()
        assert hit[2].any() and hit[3].any() and hit[4].any()
    assert [n for lens, _, _ in SCENARIOS.values() for n in lens].count(0) == 1
    assert {0, 1, 7, 8, 9, 16, 17} <= {n for lens, _, _ in SCENARIOS.values() for n in lens}
    s0 = [step_masks(i) for i in range(17)]
    assert all(x & 1 for x in s0[:8]) and not any(x & 4 for x in s0[:8]) and sum(1 for x in s0[:8] if x & 2) == 1
    assert all(x & 4 for x in s0[8:16]) and not any(x & 1 for x in s0[8:16]) and sum(1 for x in s0[8:16] if x & 8) == 1
