"""Shortest paths on the benchmark's graph (meld_minplus_step, DeviceGraph.shortest_path_device) against the diffusion step that
shares its gather scheme and against the route that exists without them:

    python tools/geodesic_time.py [--n 1000000] [--knn 5,15] [--out FILE] [--label TEXT]

One process.  Per graph (bench.synthetic_cells(N, 50, seed 0), MELD(knn).fit; the first knn is MELD's default):
  (a) one meld_minplus_step and one meld_diffuse_step at p = 1, 16, 64, 100, 128, timed alternately (a round moves the bytes of a
      diffusion step, without the per-row diagonal and division and with one 4-byte flag), and the clear of that flag alone (the
      entry called with n_rows = 0), which the events around a round include;
  (b) the solve: 64 and 128 random sources under "affinity" and "data" -- rounds taken, total time, time per round -- and the one-off
      cost of the lengths;
  (c) the route without the kernel, for 8 of those sources and for 1: graph.edge_lengths exported to the host plus
      scipy.sparse.csgraph.dijkstra(indices=...), against shortest_path (device work and read-back) for the same sources, the two
      results compared bit for bit.
Device times of (a) are HIP events around single launches after warm-up: median (min, max).  (b) and (c) are host clocks around
calls that end in a read-back, each after one untimed call of the same shape; the scipy calls are timed once."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch
from scipy.sparse.csgraph import dijkstra

import meld_amd
from bench import synthetic_cells
from meld_amd import _lib
from meld_amd.diffuse import walk_vectors
from meld_amd.geodesic import edge_lengths_device

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--knn", default="5,15")
ap.add_argument("--out", default=None)
ap.add_argument("--label", default="")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--host-sources", type=int, default=8)
ap.add_argument("--rounds-only", action="store_true", help="(a) alone")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("tools/geodesic_time.py measures on the GPU: none found")

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternately(fa, fb, warm=3):
    """(median, min, max) in ms of single calls of fa and of fb between two events, the two taking turns"""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(args.reps):
        ta.append(event_ms(fa))
        tb.append(event_ms(fb))
    return (statistics.median(ta), min(ta), max(ta)), (statistics.median(tb), min(tb), max(tb))


def fmt(t):
    return "median {:.3f} ms ({:.3f} - {:.3f})".format(*t)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


prop = torch.cuda.get_device_properties(0)
free, total = torch.cuda.mem_get_info()
say("device: {} CUs {} HBM GiB {:.0f} | torch {} hip {} (clocks are not pinned)".format(
    prop.name, prop.multi_processor_count, prop.total_memory / 2**30, torch.__version__, torch.version.hip))
say("memory free/total GiB at start: {:.1f} / {:.1f} | {}".format(free / 2**30, total / 2**30, args.label))
N = args.n
say("data: synthetic_cells({}, 50, seed 0); (a): HIP events around single launches, 3 warm-up calls, n={}, the two kernels taking turns".format(N, args.reps))
X, _ = synthetic_cells(N, 50, seed=0)
lib = _lib.get_lib()
st = torch.cuda.current_stream().cuda_stream

for knn in [int(k) for k in args.knn.split(",")]:
    op = meld_amd.MELD(knn=knn, verbose=0).fit(X)
    G = op.graph
    kd, s = walk_vectors(G)
    nnz = G.nnz
    say("--- knn {} nnz {} mean degree {:.1f} max degree {} perm {}".format(
        knn, nnz, nnz / N, int((G.rowptr[1:] - G.rowptr[:-1]).max()), G.perm is not None))
    L, t_aff = wall(lambda: edge_lengths_device(G, "affinity"))
    Ld, t_data = wall(lambda: edge_lengths_device(G, "data"))
    say("lengths, once per graph: affinity (-log val, torch) {:.1f} ms, data (meld_edge_lengths_l2, d = 50, rows gathered to the device order "
        "and validation included) {:.1f} ms".format(t_aff * 1e3, t_data * 1e3))
    head_d = [_lib.ptr(G.rowptr), _lib.ptr(G.col), _lib.ptr(G.val), _lib.ptr(kd), _lib.ptr(s), N]
    head_m = [_lib.ptr(G.rowptr), _lib.ptr(G.col), _lib.ptr(L), N]
    changed = torch.zeros(1, dtype=torch.int32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    one = torch.zeros(8, dtype=torch.float64, device="cuda")

    def clear():
        _lib.check(lib.meld_minplus_step(_lib.ptr(G.rowptr), None, None, 0, _lib.ptr(one), 1, _lib.ptr(one), 1, 1, _lib.ptr(changed), st), "meld_minplus_step")

    tc, _ = alternately(clear, clear)
    say("(a) the clear of `changed` alone (n_rows = 0): {}".format(fmt(tc)))
    for p in (1, 16, 64, 100, 128):
        x = torch.rand(N, p, dtype=torch.float64, device="cuda", generator=gen)
        y = torch.empty_like(x)

        def round_(x=x, y=y, p=p):
            _lib.check(lib.meld_minplus_step(*head_m, _lib.ptr(x), p, _lib.ptr(y), p, p, _lib.ptr(changed), st), "meld_minplus_step")

        def step(x=x, y=y, p=p):
            _lib.check(lib.meld_diffuse_step(*head_d, _lib.ptr(x), p, _lib.ptr(y), p, p, st), "meld_diffuse_step")

        tr, td = alternately(round_, step)
        verdict = "not slower" if tr[0] <= td[0] else ("slower, ranges overlap" if tr[1] <= td[2] else "SLOWER BEYOND THE RANGES")
        say("(a) p={:3d}: meld_minplus_step {} | meld_diffuse_step {} | round / step {:.3f} ({})".format(p, fmt(tr), fmt(td), tr[0] / td[0], verdict))
        del x, y
    if args.rounds_only:
        continue
    # (b) the solve
    sources = np.random.default_rng(3).permutation(N)[:128]
    kept = {}
    for distance in ("affinity", "data"):
        for p in (64, 128):
            G.shortest_path_device(sources[:p], distance=distance)  # (one untimed call: allocations, first launches)
            D, t = wall(lambda: G.shortest_path_device(sources[:p], distance=distance))
            rounds = G.geodesic_info["rounds"]
            reached = float(torch.isfinite(D).double().mean())
            say("(b) {} sources, {}: rounds {} | {:.1f} ms in all, {:.3f} ms per round | reached {:.4f} of the cells, largest finite distance {:.4g}".format(
                p, distance, rounds, t * 1e3, t * 1e3 / sum(rounds), reached, float(D[torch.isfinite(D)].max())))
            if p == 128:
                kept[distance] = D[:, : args.host_sources].cpu().numpy()
            del D
    # (c) the route without the kernel, and the device for the same sources end to end
    for distance in ("affinity", "data"):
        for q in (args.host_sources, 1):
            src = sources[:q]
            t0 = time.perf_counter()
            Lh = G.edge_lengths(distance)
            t1 = time.perf_counter()
            ref = dijkstra(Lh, indices=src).T
            t2 = time.perf_counter()
            G.shortest_path(src, distance=distance)  # (one untimed call)
            Dh, td = wall(lambda: G.shortest_path(src, distance=distance))
            rounds = G.geodesic_info["rounds"]
            same = bool(np.array_equal(Dh, ref))
            say("(c) {} source(s), {}: host route = edge_lengths export {:.2f} s + scipy dijkstra {:.2f} s = {:.2f} s | device shortest_path "
                "(read-back included) {:.3f} s, rounds {} | device / scipy alone {:.3f}, device / host route {:.3f} | bit-equal to scipy: {}; "
                "equal to the first columns of the 128-source solve: {}".format(
                    q, distance, t1 - t0, t2 - t1, t2 - t0, td, rounds, td / (t2 - t1), td / (t2 - t0), same,
                    bool(np.array_equal(Dh, kept[distance][:, :q]))))
            del Lh, ref, Dh
    del op, G, L, Ld, kept
    torch.cuda.empty_cache()
