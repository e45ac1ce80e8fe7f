"""Leiden communities on the benchmark's graph (meld_amd/leiden.py, csrc/leiden.hip): one refinement round timed apart, the whole
run, and the Louvain run of the same graph in the same process:

    python tools/leiden_time.py [--n 1000000] [--knn 5,15] [--out FILE] [--label TEXT] [--reps 7]

One process.  Per graph (bench.synthetic_cells(N, 50, seed 0), MELD(knn).fit):
  (a) one refinement round at level 0 inside the move partition of that level, from singletons (round 0: every row is alone) and
      from the state after two rounds (round 2: most rows have merged and leave the propose kernel before any gather): the
      grouping of the vertices by sub-community (radix sort + meld_louvain_totals), meld_leiden_propose at 16 and at 64 lanes per
      row and meld_leiden_commit with its count, wall clocks around synchronised calls after one untimed call, median (min - max);
  (b) the whole run, ``G.leiden(recompute=True)``, and ``G.louvain(recompute=True)``: median wall clock (min - max), levels,
      rounds, communities, modularity.
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
ap.add_argument("--out", default=None)
ap.add_argument("--label", default="")
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("tools/leiden_time.py measures on the GPU: none found")

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


def repeated(fn, scale=1e3):
    """(median, min, max) of ``fn`` (synchronised wall clock, ms unless scaled otherwise), after one untimed call"""
    fn()
    t = [wall(fn)[1] * scale for _ in range(args.reps)]
    return statistics.median(t), min(t), max(t)


def fmt(t):
    return "median {:.3f} ms ({:.3f} - {:.3f})".format(*t)


def refinement_rounds(G):
    """the stages of a refinement round at level 0, at round 0 and at round 2, timed apart"""
    lib, st = get_lib(), torch.cuda.current_stream().cuda_stream
    rowptr, col, val = lv._caller_order_csr(G, lib, st)
    n, dev = G.N, rowptr.device
    k = lv._degrees(lib, st, rowptr, val, n)
    two_m = float(k.sum().item())
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    lanes = int(lib.meld_louvain_lanes(n, int(col.shape[0])))
    c, _, _ = lv._run_level(lib, st, rowptr, col, val, k, two_m, 1.0, lv.DEFAULT_TOL, lv.DEFAULT_MAX_ROUNDS)
    P, L, _ = lv._renumber(lib, st, c, k)
    tot_comm, _, _ = lv._totals(lib, st, P, k, ar)
    prop, new = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    part = torch.empty(int(lib.meld_leiden_commit_blocks(n)), dtype=torch.int32, device=dev)
    movers = torch.empty(1, dtype=torch.int64, device=dev)

    def propose(sub, tot, size, rnd, width):
        check(lib.meld_leiden_propose(ptr(rowptr), ptr(col), ptr(val), n, ptr(P), ptr(sub), ptr(k), ptr(tot), ptr(size), ptr(tot_comm), two_m,
                                      1.0, rnd, width, ptr(prop), st), "meld_leiden_propose")

    def commit(sub, size):
        check(lib.meld_leiden_commit(ptr(sub), ptr(prop), ptr(size), n, ptr(new), ptr(part), ptr(movers), st), "meld_leiden_commit")

    sub = ar.to(torch.int32)
    out = []
    for rnd in range(3):
        tot, size, _ = lv._totals(lib, st, sub, k, ar)
        if rnd in (0, 2):
            alone = int((size[sub.to(torch.int64)] == 1).sum().item())
            t_group = repeated(lambda: lv._totals(lib, st, sub, k, ar))
            t_prop = {w: repeated(lambda: propose(sub, tot, size, rnd, w)) for w in (16, 64)}
            propose(sub, tot, size, rnd, lanes)
            t_commit = repeated(lambda: commit(sub, size))
            out.append((rnd, alone, int(movers.item()), t_group, t_prop, t_commit))
        propose(sub, tot, size, rnd, lanes)
        commit(sub, size)
        sub = new.clone()
    return L, lanes, out


prop = torch.cuda.get_device_properties(0)
free, total = torch.cuda.mem_get_info()
say("device: {} CUs {} HBM GiB {:.0f} | torch {} hip {} (clocks are not pinned)".format(
    prop.name, prop.multi_processor_count, prop.total_memory / 2**30, torch.__version__, torch.version.hip))
say("memory free/total GiB at start: {:.1f} / {:.1f} | {}".format(free / 2**30, total / 2**30, args.label))
say("data: synthetic_cells(N, 50, seed 0); resolution 1; wall clocks around synchronised calls, one untimed call first, n={}".format(args.reps))

for knn in [int(k) for k in args.knn.split(",")]:
    X, _ = synthetic_cells(args.n, 50, seed=0)
    G = meld_amd.MELD(knn=knn, verbose=0).fit(X).graph
    say("--- knn {} N {} nnz {} mean degree {:.1f} max degree {} perm {}".format(
        knn, args.n, G.nnz, G.nnz / args.n, int((G.rowptr[1:] - G.rowptr[:-1]).max()), G.perm is not None))
    t_leiden = repeated(lambda: G.leiden(recompute=True), 1.0)
    rec = G.leiden()
    say("(b) leiden  whole run median {:.3f} s ({:.3f} - {:.3f}): {} levels, {} move rounds, {} refinement rounds, {} communities, modularity "
        "{:.6f}; levels (vertices, communities, subcommunities, rounds, refine rounds): {}".format(
            *t_leiden, len(rec.levels), sum(level["rounds"] for level in rec.levels), sum(level["refine_rounds"] for level in rec.levels),
            rec.n_communities, rec.modularity,
            [(level["vertices"], level["communities"], level["subcommunities"], level["rounds"], level["refine_rounds"]) for level in rec.levels]))
    t_louvain = repeated(lambda: G.louvain(recompute=True), 1.0)
    theirs = G.louvain()
    say("    louvain whole run median {:.3f} s ({:.3f} - {:.3f}): {} levels, {} rounds, {} communities, modularity {:.6f} | leiden / louvain "
        "{:.2f}, modularity leiden - louvain {:+.6f}".format(*t_louvain, len(theirs.levels), sum(level["rounds"] for level in theirs.levels),
                                                             theirs.n_communities, theirs.modularity, t_leiden[0] / t_louvain[0],
                                                             rec.modularity - theirs.modularity))
    L, lanes, rounds = refinement_rounds(G)
    for rnd, alone, moved, t_group, t_prop, t_commit in rounds:
        say("(a) refinement round {} at level 0 ({} communities, {} of {} rows alone, {} movers): grouping + totals {} | propose at 16 lanes "
            "per row {} | at 64 {} | commit + count {} | the run takes {}".format(rnd, L, alone, args.n, moved, fmt(t_group), fmt(t_prop[16]),
                                                                                  fmt(t_prop[64]), fmt(t_commit), lanes))
    del G, rec, theirs
    torch.cuda.empty_cache()
