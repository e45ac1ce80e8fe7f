"""Per-gene moments and highly variable genes on the device (meld_amd/preprocess.py, ``meld_prep_gene_moments`` in csrc/preprocess.hip),
timed piece by piece, next to the project's own streaming kernel on the same matrix and to the host route on scipy / numpy:

    python tools/hvg_timing.py [--shapes quickstart,1M] [--out profiles/hvg_timing.txt] [--reps 7]

Runs on the GPU only.  Shapes and counts: tools/synthetic_counts.py (the Quickstart's 26,827 x 29,197 and 1,000,000 x 30,000), generated
on the device.  Reported separately:

* the transposition (``DeviceCSR.T``), first use and repeated: a host clock around the call, synchronised at both ends;
* the moments pass alone, plain and with the fused value map (kept cells, library-size scale, sqrt): device events around one launch,
  one untimed launch first, median (min - max) of ``--reps``.  The bytes are those the pass MUST read -- 12 per stored entry (value and
  cell index), the row pointers and the per-cell vectors it gathers from -- counted from the shapes; the kernel itself reads every
  entry twice (two-pass variance), the second time from whichever cache still holds it.  ``meld_prep_row_stats`` on the same matrix
  in the same run is the yardstick: the same kind of stream, 8 bytes per entry;
* ``run(..., n_top_genes=2000)`` against ``run`` without a rule, alternating, the gene-major copy cached; and once from cold;
* the host route: ``to_scipy()`` and the column means and variances with scipy on one thread (at 1M cells on the first 50,000 rows,
  its time for all rows an EXTRAPOLATION by the ratio of rows, stated as such)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from meld_amd import preprocess as pp
from meld_amd._lib import get_lib
from synthetic_counts import SHAPES, device_counts

HBM_PEAK = 8.0e12
PERCENTILE, MIN_CELLS, RESCALE, N_TOP = 5, 5, 10000.0, 2000

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="quickstart,1M")
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--host-rows", type=int, default=50000)
ap.add_argument("--label", default="")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("tools/hvg_timing.py measures on the GPU: none found")

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def fmt(ts, unit="ms"):
    return "{:.3f} {} ({:.3f} - {:.3f})".format(statistics.median(ts), unit, min(ts), max(ts))


def events_ms(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def wall_once_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def kernel_line(name, ts, nbytes):
    med = statistics.median(ts) * 1e-3
    say("  {:<58} {} | {:.2f} GB -> {:.2f} TB/s = {:.0f} % of the HBM peak".format(name, fmt(ts), nbytes / 1e9, nbytes / med / 1e12,
                                                                                 100.0 * nbytes / med / HBM_PEAK))
    return nbytes / med


def host_moments(X):
    """column means and variances (ddof=1) of a scipy CSR on one thread, two passes over the entries"""
    t0 = time.perf_counter()
    n = X.shape[0]
    mean = np.asarray(X.sum(axis=0)).ravel() / n
    C = X.tocsc()
    d = C.data - np.repeat(mean, np.diff(C.indptr))
    ss = np.add.reduceat(np.concatenate([d * d, [0.0]]), np.minimum(C.indptr[:-1], C.nnz))
    ss[np.diff(C.indptr) == 0] = 0.0
    var = (ss + (n - np.diff(C.indptr)) * mean * mean) / (n - 1)
    return time.perf_counter() - t0, mean, var


prop = torch.cuda.get_device_properties(0)
say("device: {} CUs {} HBM GiB {:.0f} | torch {} hip {} (clocks are not pinned) {}".format(
    prop.name, prop.multi_processor_count, prop.total_memory / 2**30, torch.__version__, torch.version.hip, args.label))
say("moments: a wave per gene up to {} stored entries, a workgroup of 1024 above; n = {} after one untimed call: median (min - max)".format(
    2048, args.reps))
get_lib()

for name in args.shapes.split(","):
    N, G, per_row = SHAPES[name]
    A = device_counts(N, G, per_row)
    nnz = A.nnz
    say("--- {}: {} x {} at {:.2f} %, nnz {} (fp64 counts 1 + Poisson(0.6))".format(name, N, G, 100.0 * nnz / (N * G), nnz))
    # the transposition
    first, T = wall_once_ms(A._transpose)
    again = []
    for _ in range(3):
        del T
        ms, T = wall_once_ms(A._transpose)
        again.append(ms)
    A._T = T
    glen = (T.rowptr[1:] - T.rowptr[:-1]).cpu().numpy()
    say("transposition (DeviceCSR.T): first use {:.1f} ms, then {} | {:.1f} GB at its peak".format(first, fmt(again), A.transpose_bytes() / 1e9))
    say("entries per gene: {} - {} (median {:.0f}, mean {:.0f}); {} genes above 2048 entries hold {:.1f} % of the entries".format(
        int(glen.min()), int(glen.max()), float(np.median(glen)), float(glen.mean()), int((glen > 2048).sum()),
        100.0 * glen[glen > 2048].sum() / max(nnz, 1)))
    # the pass alone, next to the row statistics
    say("kernels alone:")
    rate_rs = kernel_line("meld_prep_row_stats (val; the yardstick)", events_ms(lambda: pp.row_stats_device(A)), 8 * nnz + 28 * N)
    rate_plain = kernel_line("meld_prep_gene_moments, plain (col + val)", events_ms(lambda: pp._moments(T, N)), 12 * nnz + 28 * G)
    s, a, _ = pp.row_stats_device(A)
    libsize = s.cpu().numpy()
    keep_h = libsize > np.percentile(libsize, PERCENTILE)
    keep = torch.from_numpy(keep_h.astype(np.uint8)).cuda()
    n_kept = int(keep_h.sum())
    rate_map = kernel_line("meld_prep_gene_moments, kept cells + scale + sqrt", events_ms(
        lambda: pp._moments(T, n_kept, keep, a, RESCALE, pp.TRANSFORMS["sqrt"], 5.0, None, 1)), 12 * nnz + 28 * G + 9 * N)
    say("  the moments pass reaches {:.2f} (plain) and {:.2f} (fused map) of the row statistics' rate".format(rate_plain / rate_rs, rate_map / rate_rs))
    c1, m1, v1 = pp._moments(T, N)
    c2, m2, v2 = pp._moments(T, N)
    say("  two calls, same bits: {}".format(bool(torch.equal(c1, c2) and torch.equal(m1.view(torch.int64), m2.view(torch.int64))
                                                 and torch.equal(v1.view(torch.int64), v2.view(torch.int64)))))
    # run with and without the rule, alternating
    steps = dict(library_size_percentile=PERCENTILE, min_cells=MIN_CELLS, rescale=RESCALE, transform="sqrt")
    pp.run(A, **steps)
    pp.run(A, n_top_genes=N_TOP, **steps)
    t_plain, t_hvg = [], []
    for _ in range(args.reps):
        t_plain.append(wall_once_ms(lambda: pp.run(A, **steps))[0])
        t_hvg.append(wall_once_ms(lambda: pp.run(A, n_top_genes=N_TOP, **steps))[0])
    out = pp.run(A, n_top_genes=N_TOP, **steps)
    say("`run` without a rule: {} | with n_top_genes={} (gene-major copy cached): {} | nnz after: {}".format(fmt(t_plain), N_TOP, fmt(t_hvg), out.data.nnz))
    A._T = None
    del T
    torch.cuda.empty_cache()
    cold, _ = wall_once_ms(lambda: pp.run(A, n_top_genes=N_TOP, **steps))
    say("`run` with n_top_genes={} from cold (the transposition included): {:.1f} ms; the transposition's share {:.0f} %".format(
        N_TOP, cold, 100.0 * statistics.median(again) / cold))
    # the host route
    h_rows = N if name == "quickstart" else min(N, args.host_rows)
    t0 = time.perf_counter()
    Xh = A.to_scipy()
    t_copy = time.perf_counter() - t0
    Xh = Xh[:h_rows]
    secs, mean_h, var_h = host_moments(Xh)
    if h_rows == N:
        dm = float(np.abs(m1.cpu().numpy() - mean_h).max() / np.abs(mean_h).max())
        dv = float(np.abs(v1.cpu().numpy() - var_h).max() / np.abs(var_h).max())
        say("host route: to_scipy() {:.2f} s, column moments with scipy on one thread {:.2f} s = {:.0f} x the moments pass | largest difference "
            "{:.1e} (mean), {:.1e} (variance) of the largest value".format(t_copy, secs, secs * rate_plain / (12 * nnz + 28 * G), dm, dv))
    else:
        say("host route: to_scipy() {:.2f} s, column moments with scipy on one thread on the first {} rows {:.2f} s; EXTRAPOLATED to {} rows by "
            "the ratio of rows: {:.0f} s".format(t_copy, h_rows, secs, N, secs * N / h_rows))
    del A, out, Xh, c1, m1, v1, c2, m2, v2
    torch.cuda.empty_cache()
