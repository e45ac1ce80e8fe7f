"""Rank-sum differential expression on the device (meld_amd/diffexp.py, csrc/ranksum.hip), timed by stage, next to a scipy loop on the
host in the same process:

    python tools/ranksum_time.py [--shapes quickstart,1M] [--out profiles/ranksum_timing.txt] [--reps 3] [--scipy-genes 500]

Shapes and generator: those of the sparse-input timings (tools/time_sparse_input.py, ``device_matrix``: a CSR matrix built on the
device, every cell holding the same number of genes drawn inside equal strata, fp32 counts 1..5): the Quickstart's 26,827 x 29,197 at
7 % and 1,000,000 x 30,000 at 2 %.  Cases: two groups (every cell in one of two random classes), and 20 random clusters, each against
the rest, from one run.  Per case, after one untimed run, ``--reps`` runs with the stream synchronised between the stages
(``rank_sums_device(timings=...)``): the transpose (``DeviceCSR.T``, rebuilt every run), the plan (class sizes, lists of short and
long genes), the classes' sums, the short route, the long route (gather + two radix sorts + scan), the read-back of the four tensors,
and the host arithmetic of the frames (p-values, Benjamini-Hochberg).  Median (min - max) of wall clocks; clocks are not pinned.

The scipy loop: ``scipy.stats.mannwhitneyu(x, y, method="asymptotic")`` per gene on the dense columns of the first ``--scipy-genes``
genes (one thread), two groups; for the clusters, one test per cluster and gene on ``--scipy-genes / 20`` genes.  Its time for ALL
genes is an EXTRAPOLATION by the ratio of gene counts, stated as such.  The device's statistic and p-values of those genes are
compared with scipy's on the way."""
import argparse
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch
from scipy import sparse, stats

from meld_amd import diffexp
from meld_amd._lib import get_lib
from time_sparse_input import device_matrix

SHAPES = {"quickstart": (26827, 29197, 2044), "1M": (1_000_000, 30_000, 600)}

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="quickstart,1M")
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--scipy-genes", type=int, default=500)
ap.add_argument("--label", default="")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("tools/ranksum_time.py measures on the GPU: none found")

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def fmt(ts, scale=1e3, unit="ms"):
    return "{:.2f} {} ({:.2f} - {:.2f})".format(statistics.median(ts) * scale, unit, min(ts) * scale, max(ts) * scale)


def device_case(A, code, k):
    """stage times of ``--reps`` runs (after one untimed run) and the host copies of the last run's tensors"""
    diffexp.rank_sums_device(A, code, k)
    runs, host = [], None
    for _ in range(args.reps):
        A._T = None
        t = {}
        res = diffexp.rank_sums_device(A, code, k, timings=t)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = [x.cpu().numpy() for x in (res.rank2, res.tie, res.nnz, res.sum, res.n_c)]
        t["read-back"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        m = int(host[4].sum())
        for c in range(k if k > 2 else 1):
            n1 = int(host[4][c])
            _, p = diffexp.pvalues(host[0][:, c], host[1], n1, m - n1)
            diffexp.bh_qvalues(p)
        t["host p and q"] = time.perf_counter() - t0
        t["total"] = sum(t.values())
        runs.append(t)
        del res
    return {name: [r[name] for r in runs] for name in runs[0]}, host


def host_columns(A, n_genes):
    """the first ``n_genes`` genes as a host CSC matrix [N, n_genes] (from the cached transpose)"""
    AT = A.T
    end = int(AT.rowptr[n_genes])
    return sparse.csc_matrix((AT.val[:end].cpu().numpy().astype(np.float64), AT.col[:end].cpu().numpy(), AT.rowptr[:n_genes + 1].cpu().numpy()),
                             shape=(A.shape[0], n_genes))


def scipy_loop(Xh, code, classes, genes):
    """seconds of one mannwhitneyu per (class, gene), each class against the other selected cells; (statistic, p) per class"""
    out = {}
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for c in classes:
            a, b = code == c, (code >= 0) & (code != c)
            stat, p = np.empty(genes), np.empty(genes)
            for g in range(genes):
                colv = np.asarray(Xh[:, g].todense()).ravel()
                r = stats.mannwhitneyu(colv[a], colv[b], use_continuity=True, alternative="two-sided", method="asymptotic")
                stat[g], p[g] = r.statistic, r.pvalue
            out[c] = (stat, p)
    return time.perf_counter() - t0, out


def agreement(host, k, code, theirs):
    m = int(host[4].sum())
    worst_u, worst_p = 0.0, 0.0
    for c, (stat, p) in theirs.items():
        n1 = int(host[4][c])
        g = len(stat)
        u1, ours = diffexp.pvalues(host[0][:g, c], host[1][:g], n1, m - n1)
        worst_u = max(worst_u, float(np.abs(u1 - stat).max()))
        ok = p > 1e-290
        worst_p = max(worst_p, float((np.abs(ours[ok] - p[ok]) / p[ok]).max()) if ok.any() else 0.0)
    return "statistic max |device - scipy| = {:g}, p max relative difference = {:.2e}".format(worst_u, worst_p)


prop = torch.cuda.get_device_properties(0)
lib = get_lib()
say("device: {} CUs {} HBM GiB {:.0f} | torch {} hip {} (clocks are not pinned) {}".format(
    prop.name, prop.multi_processor_count, prop.total_memory / 2**30, torch.__version__, torch.version.hip, args.label))
say("short route: genes of at most {} stored entries; k <= {}; at most {} selected cells; long route in batches of {} entries".format(
    lib.meld_ranksum_lds_max(), lib.meld_ranksum_max_classes(), lib.meld_ranksum_max_selected(), diffexp.LONG_BATCH_ENTRIES))
say("wall clocks around synchronised stages, one untimed run first, n = {}: median (min - max)".format(args.reps))

for name in args.shapes.split(","):
    N, G, per_row = SHAPES[name]
    A = device_matrix(N, G, per_row, 0, False, False)
    lens = (A.T.rowptr[1:] - A.T.rowptr[:-1])
    n_long = int((lens > lib.meld_ranksum_lds_max()).sum())
    say("--- {}: {} x {} at {:.1f} %, nnz {} (fp32 values 1..5); stored entries per gene {} - {}: {} genes short, {} long".format(
        name, N, G, 100.0 * A.nnz / (N * G), A.nnz, int(lens.min()), int(lens.max()), G - n_long, n_long))
    gen = torch.Generator(device="cuda").manual_seed(1)
    for what, k in (("two groups", 2), ("20 clusters, each against the rest", 20)):
        code = torch.randint(0, k, (N,), device="cuda", generator=gen, dtype=torch.int32)
        stages, host = device_case(A, code, k)
        say("{} (k = {}): ".format(what, k) + " | ".join("{} {}".format(s, fmt(ts)) for s, ts in stages.items()))
        genes = min(G, args.scipy_genes if k == 2 else max(1, args.scipy_genes // k))
        Xh = host_columns(A, genes)
        code_h = code.cpu().numpy()
        secs, theirs = scipy_loop(Xh, code_h, [0] if k == 2 else list(range(k)), genes)
        tests = genes * (1 if k == 2 else k)
        say("    scipy loop, one thread: {} tests ({} genes) in {:.2f} s = {:.2f} ms per test; EXTRAPOLATED to {} genes{}: {:.0f} s | device "
            "total {:.3f} s: {:.0f} x | {}".format(tests, genes, secs, 1e3 * secs / tests, G, "" if k == 2 else " x {} clusters".format(k),
                                                    secs / tests * G * (1 if k == 2 else k), statistics.median(stages["total"]),
                                                    secs / tests * G * (1 if k == 2 else k) / statistics.median(stages["total"]),
                                                    agreement(host, k, code_h, theirs)))
        del Xh
    del A
    torch.cuda.empty_cache()
