"""Louvain communities on the benchmark's graph (meld_amd/louvain.py, csrc/louvain.hip): one round timed apart, the whole run, and
the route that exists without it:

    python tools/louvain_time.py [--n 1000000] [--knn 5,15] [--host-n 100000] [--out FILE] [--label TEXT]

One process.  Per graph (bench.synthetic_cells(N, 50, seed 0), MELD(knn).fit):
  (a) one round at level 0 from the labels the first level ends with: the grouping of the cells by label (radix sort +
      meld_louvain_totals) and the move launch (meld_louvain_move with its reduction), wall clocks around synchronised calls after
      one untimed call, median (min - max);
  (b) the whole run, ``G.louvain(recompute=True)``: wall clock, levels, rounds, communities, modularity;
  (c) on a graph of --host-n cells built the same way: the export of ``G.W``, networkx's graph from it and
      ``networkx.community.louvain_communities(seed=0)`` with its modularity, against the device run there.
Clocks are not pinned; every figure is of this run."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import meld_amd
from bench import synthetic_cells
from meld_amd import louvain as lv
from meld_amd._lib import check, get_lib, ptr

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--knn", default="5,15")
ap.add_argument("--host-n", type=int, default=100_000)
ap.add_argument("--out", default=None)
ap.add_argument("--label", default="")
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("tools/louvain_time.py measures on the GPU: none found")

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def repeated(fn):
    """(median, min, max) in ms of ``fn`` (synchronised wall clock), after one untimed call"""
    fn()
    t = [wall(fn)[1] * 1e3 for _ in range(args.reps)]
    return statistics.median(t), min(t), max(t)


def fmt(t):
    return "median {:.3f} ms ({:.3f} - {:.3f})".format(*t)


def one_round(G, labels):
    """the two stages of a round at level 0 from ``labels`` (caller's order), timed apart"""
    lib, st = get_lib(), torch.cuda.current_stream().cuda_stream
    rowptr, col, val = lv._caller_order_csr(G, lib, st)
    n, dev = G.N, rowptr.device
    k = lv._degrees(lib, st, rowptr, val, n)
    two_m = float(k.sum().item())
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    lanes = int(lib.meld_louvain_lanes(n, int(col.shape[0])))
    blocks = int(lib.meld_louvain_move_blocks(n, 64))  # (the larger of the two counts)
    new, moved = torch.empty_like(labels), torch.empty_like(labels)
    own = torch.empty(n, dtype=torch.float64, device=dev)
    part_sum, part_moved = torch.empty(blocks, dtype=torch.float64, device=dev), torch.empty(blocks, dtype=torch.int32, device=dev)
    stats = torch.empty(3, dtype=torch.float64, device=dev)
    tot, size, _ = lv._totals(lib, st, labels, k, ar)

    def move(lanes):
        check(lib.meld_louvain_move(ptr(rowptr), ptr(col), ptr(val), n, ptr(labels), ptr(k), ptr(tot), ptr(size), two_m, 1.0, 0, lanes,
                                    ptr(new), ptr(own), ptr(moved), ptr(part_sum), ptr(part_moved), ptr(stats), st), "meld_louvain_move")

    return repeated(lambda: lv._totals(lib, st, labels, k, ar)), {w: repeated(lambda: move(w)) for w in (16, 64)}, lanes


prop = torch.cuda.get_device_properties(0)
free, total = torch.cuda.mem_get_info()
say("device: {} CUs {} HBM GiB {:.0f} | torch {} hip {} (clocks are not pinned)".format(
    prop.name, prop.multi_processor_count, prop.total_memory / 2**30, torch.__version__, torch.version.hip))
say("memory free/total GiB at start: {:.1f} / {:.1f} | {}".format(free / 2**30, total / 2**30, args.label))
say("data: synthetic_cells(N, 50, seed 0); resolution 1; wall clocks around synchronised calls, one untimed call first, n={}".format(args.reps))

for knn in [int(k) for k in args.knn.split(",")]:
    for N, host in ((args.n, False), (args.host_n, True)):
        X, _ = synthetic_cells(N, 50, seed=0)
        G = meld_amd.MELD(knn=knn, verbose=0).fit(X).graph
        say("--- knn {} N {} nnz {} mean degree {:.1f} max degree {} perm {}".format(
            knn, N, G.nnz, G.nnz / N, int((G.rowptr[1:] - G.rowptr[:-1]).max()), G.perm is not None))
        G.louvain()  # (untimed: the first call of these shapes)
        rec, t_run = wall(lambda: G.louvain(recompute=True))
        rounds = sum(level["rounds"] for level in rec.levels)
        say("(b) whole run {:.3f} s: {} levels, {} rounds ({:.2f} ms per round over all levels), {} communities, modularity {:.6f}; levels "
            "(vertices, communities, rounds): {}".format(t_run, len(rec.levels), rounds, 1e3 * t_run / max(rounds, 1), rec.n_communities,
                                                        rec.modularity, [(level["vertices"], level["communities"], level["rounds"]) for level in rec.levels]))
        t_group, t_move, lanes = one_round(G, rec._level_labels[0].contiguous())
        say("(a) one round at level 0: grouping by label + totals {} | move + reduction at 16 lanes per row {} | at 64 {} | the run takes {}".format(
            fmt(t_group), fmt(t_move[16]), fmt(t_move[64]), lanes))
        if host:
            import networkx as nx

            W, t_export = wall(lambda: G.W)
            t0 = time.perf_counter()
            H = nx.from_scipy_sparse_array(W)
            t_graph = time.perf_counter() - t0
            say("(c) host route at N = {}: export of G.W {:.2f} s, networkx graph {:.2f} s ...".format(N, t_export, t_graph))
            t0 = time.perf_counter()
            parts = nx.community.louvain_communities(H, weight="weight", resolution=1.0, seed=0)
            t_nx = time.perf_counter() - t0
            q_nx = nx.community.modularity(H, parts, weight="weight")
            say("    louvain_communities(seed=0) {:.2f} s: {} communities, modularity {:.6f} | device run {:.3f} s, modularity {:.6f} "
                "(device - networkx {:+.6f}) | device / host route {:.5f}".format(t_nx, len(parts), q_nx, t_run, rec.modularity,
                                                                                  rec.modularity - q_nx, t_run / (t_export + t_graph + t_nx)))
        del G, rec
        torch.cuda.empty_cache()
