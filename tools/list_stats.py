"""Statistics of the step lists of the first pass (meld_knn16_step_lists): how many waves of a block need a listed tile,
how long a wave's runs of needed / not needed steps are.   python tools/list_stats.py [N]"""
import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MELD_DEV", "1")  # (development tool: the MELD_* switches it sets or documents are read, see meld_amd/_options.py)
import torch
from meld_amd._lib import get_lib, ptr, check
from meld_amd.reorder import locality_permutation
from bench import synthetic_cells

# the benchmark cells in locality order, their operands, the product's seeds, the seeded table and the lists built from it
lib = get_lib()
X, _ = synthetic_cells(int(sys.argv[1]) if len(sys.argv) > 1 else 1000000, 50, seed=0)
Xd = torch.from_numpy(X).cuda()
Xd = Xd.index_select(0, locality_permutation(Xd)).contiguous()
N, d = Xd.shape
st = torch.cuda.current_stream().cuda_stream
TS, BQ = lib.meld_knn16_tile_refs(), lib.meld_knn16_block_queries()
n_tiles, q_pad = (N + TS - 1) // TS, ((N + BQ - 1) // BQ) * BQ
sums = torch.empty(d, dtype=torch.float64, device="cuda")
check(lib.meld_col_sums_f64(ptr(Xd), N, d, ptr(sums), st))
mean = sums / N
Rt = torch.empty(n_tiles * lib.meld_knn16_tile_bytes(d), dtype=torch.uint8, device="cuda")
Q = torch.empty(q_pad * lib.meld_knn16_query_bytes(d), dtype=torch.uint8, device="cuda")
Qn = torch.empty(q_pad, dtype=torch.float32, device="cuda")
norm2 = torch.empty(N, dtype=torch.float32, device="cuda")
nmax = torch.zeros(1, dtype=torch.float32, device="cuda")
sinfo = torch.empty(4, dtype=torch.float32, device="cuda")
check(lib.meld_knn16_prepare(ptr(Xd), N, d, ptr(mean), 0, N, ptr(Rt), ptr(Q), ptr(Qn), ptr(norm2), ptr(nmax), ptr(sinfo), st))
seed = torch.empty(q_pad, dtype=torch.float32, device="cuda")
check(lib.meld_knn16_seed_thresholds_mfma(ptr(Q), ptr(Qn), ptr(Rt), ptr(sinfo), ptr(nmax), N, d, 0, N, 15, (-math.log(1e-4)) ** (1 / 40), 1, 0,
                                          ptr(seed), st))
tmpb = torch.empty(lib.meld_knn16_bounds_temp_bytes(N, d, N), dtype=torch.uint8, device="cuda")
lb2 = torch.empty(lib.meld_knn16_bounds_bytes(N, N), dtype=torch.uint8, device="cuda")
check(lib.meld_knn16_bounds(ptr(Xd), N, d, ptr(mean), ptr(sinfo), ptr(nmax), ptr(Rt), 0, N, ptr(seed), ptr(Qn), 1, ptr(tmpb), ptr(lb2), st))
nb = q_pad // BQ
sl = torch.empty(nb * n_tiles, dtype=torch.int32, device="cuda")
sc = torch.empty(nb, dtype=torch.int32, device="cuda")
check(lib.meld_knn16_step_lists(ptr(lb2), ptr(seed), N, d, N, 1, ptr(nmax), ptr(sinfo), 0, ptr(sl), n_tiles, ptr(sc), st))
sl = sl.view(nb, n_tiles)
cnt = sc.to(torch.int64)
print("blocks %d, steps per block: mean %.0f  min %d  max %d  (tiles %d)" % (nb, float(cnt.float().mean()), int(cnt.min()), int(cnt.max()), n_tiles))
idx = torch.arange(n_tiles, device="cuda").unsqueeze(0)
valid = idx < cnt.unsqueeze(1)
mask = (sl >> 24) & 0xF
pc = ((mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1) + ((mask >> 3) & 1))
tot = int(valid.sum())
for k in range(5):
    print("steps needed by %d waves: %.1f %%" % (k, 100.0 * int(((pc == k) & valid).sum()) / tot))
print("live wave-steps: %.1f %%" % (100.0 * int((pc * valid).sum()) / (4 * tot)))
# run lengths of wave 0's bit along the lists of 200 sampled blocks
import numpy as np
runs_on, runs_off = [], []
for b in np.linspace(0, nb - 1, 200).astype(int):
    m = ((mask[b, : int(cnt[b])] >> 0) & 1).cpu().numpy()
    if len(m) == 0: continue
    ch = np.flatnonzero(np.diff(m)) + 1
    seg = np.diff(np.concatenate([[0], ch, [len(m)]]))
    vals = m[np.concatenate([[0], ch])]
    runs_on += list(seg[vals == 1]); runs_off += list(seg[vals == 0])
print("wave 0: runs of needed steps: mean %.1f median %d;  runs of not-needed steps: mean %.1f median %d  p90 %d" % (
    np.mean(runs_on), np.median(runs_on), np.mean(runs_off), np.median(runs_off), np.percentile(runs_off, 90)))
# per-block imbalance: steps of the block vs the live steps of its busiest / its average wave
live = torch.stack([(((mask >> w) & 1) * valid).sum(1) for w in range(4)], 1).float()
print("per block: steps / busiest wave's live steps = %.3f;  steps / mean wave's live steps = %.3f" % (
    float((cnt.float() / live.max(1).values.clamp(min=1)).mean()), float((cnt.float() / live.mean(1).clamp(min=1)).mean())))
print("sum over blocks: steps %.3e, busiest-wave live steps %.3e, mean-wave live steps %.3e" % (float(cnt.sum()), float(live.max(1).values.sum()), float(live.mean(1).sum())))
