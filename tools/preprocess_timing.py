"""Preprocessing on the device CSR (meld_amd/preprocess.py, csrc/preprocess.hip), timed kernel by kernel and end to end, next to the
same pipeline composed of torch library calls in the same process and to the host sequence on scipy / sklearn:

    python tools/preprocess_timing.py [--shapes quickstart,1M] [--out profiles/preprocess_timing.txt] [--reps 5]

Runs on the GPU only.  Shapes: the Quickstart's 26,827 x 29,197 at about 7 % and 1,000,000 x 30,000 at about 2 %.  The counts are
generated ON THE DEVICE (no upload is timed): a cell's depth is log-normal (sigma 0.5), a gene's popularity log-normal (sigma 1.5); a
cell draws its genes by stratified sampling of the popularity's distribution function (sorted; a gene drawn twice is kept once), the
values are 1 + Poisson(0.6) in fp64.  The pipeline everywhere: cells above the 5th percentile of library size, genes captured in at
least 5 kept cells, library-size normalisation to 10,000, square root, the normalised values kept next to the transformed ones.

Kernels: device events around one launch, one untimed launch first, median (min - max) of ``--reps``; bytes are the streams the kernel
has to read and write, counted from the shapes; the share of peak is against the 8.0 TB/s of the HBM's specification (a float4 copy
reaches 6.29 TB/s on this part).  ``run`` and the torch composition: a host clock around the call, synchronised at both ends (both read
a few vectors back on the way).  The scipy sequence runs on one thread on the matrix copied to the host (the copy is not timed); at 1M
cells it runs on the first 50,000 rows and its time for all rows is an EXTRAPOLATION by the ratio of rows, stated as such."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from meld_amd import preprocess as pp
from meld_amd import sparse as msp
from meld_amd._lib import check, get_lib, ptr
from synthetic_counts import SHAPES, device_counts  # (tools/synthetic_counts.py: the counts, generated on the device)

HBM_PEAK = 8.0e12
PERCENTILE, MIN_CELLS, RESCALE = 5, 5, 10000.0

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="quickstart,1M")
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--host-rows", type=int, default=50000)
ap.add_argument("--label", default="")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("tools/preprocess_timing.py measures on the GPU: none found")

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


def wall_ms(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
        del out
    return ts


def kernel_line(name, ts, nbytes):
    med = statistics.median(ts) * 1e-3
    say("  {:<46} {} | {:.2f} GB -> {:.2f} TB/s = {:.0f} % of the HBM peak".format(name, fmt(ts), nbytes / 1e9, nbytes / med / 1e12,
                                                                                 100.0 * nbytes / med / HBM_PEAK))
    return statistics.median(ts)


def torch_pipeline(A):
    """the same pipeline from torch library calls (atomics inside bincount / index_add_: sums in arrival order)"""
    N, G = A.shape
    dev = A.device
    lens = A.rowptr[1:] - A.rowptr[:-1]
    row = torch.repeat_interleave(torch.arange(N, device=dev), lens, output_size=A.nnz)
    col = A.col.long()
    lib = torch.bincount(row, weights=A.val, minlength=N)
    keep_row = lib > float(np.percentile(lib.cpu().numpy(), PERCENTILE))
    counted = keep_row[row] & (A.val > 0)
    gcount = torch.bincount(col[counted], minlength=G)
    keep_col = gcount >= MIN_CELLS
    m = keep_row[row] & keep_col[col]
    row_k, col_k, val_k = row[m], col[m], A.val[m]
    new_row = torch.cumsum(keep_row.long(), 0) - 1
    new_col = torch.cumsum(keep_col.long(), 0) - 1
    r2 = new_row[row_k]
    n_keep = int(keep_row.sum())
    norm = torch.bincount(r2, weights=val_k.abs(), minlength=n_keep)
    rowptr = torch.zeros(n_keep + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(r2, minlength=n_keep), 0)
    w = val_k / norm[r2] * RESCALE
    return rowptr, new_col[col_k].int(), torch.sqrt(w), w


def host_pipeline(X):
    from sklearn.preprocessing import normalize

    t0 = time.perf_counter()
    lib = np.asarray(X.sum(axis=1)).ravel()
    Y = X[lib > np.percentile(lib, PERCENTILE)]
    Y = Y[:, np.asarray((Y > 0).sum(axis=0)).ravel() >= MIN_CELLS]
    W = normalize(Y, "l1") * RESCALE
    T = W.sqrt()
    return time.perf_counter() - t0, T, W


prop = torch.cuda.get_device_properties(0)
lib = get_lib()
st = torch.cuda.current_stream().cuda_stream
say("device: {} CUs {} HBM GiB {:.0f} | torch {} hip {} (clocks are not pinned) {}".format(
    prop.name, prop.multi_processor_count, prop.total_memory / 2**30, torch.__version__, torch.version.hip, args.label))
say("column-count panel: {} int32 counters in LDS per workgroup; n = {} after one untimed call: median (min - max)".format(
    lib.meld_prep_panel_cols(), args.reps))

for name in args.shapes.split(","):
    N, G, per_row = SHAPES[name]
    A = device_counts(N, G, per_row)
    nnz = A.nnz
    lens = A.rowptr[1:] - A.rowptr[:-1]
    say("--- {}: {} x {} at {:.2f} %, nnz {} (fp64 counts 1 + Poisson(0.6)); entries per cell {} - {} (mean {:.0f})".format(
        name, N, G, 100.0 * nnz / (N * G), nnz, int(lens.min()), int(lens.max()), nnz / N))
    out = pp.run(A, library_size_percentile=PERCENTILE, min_cells=MIN_CELLS, rescale=RESCALE, transform="sqrt")
    n_keep, g_keep, nnz_out = out.data.shape[0], out.data.shape[1], out.data.nnz
    say("pipeline: cells above the {}th percentile of library size ({} kept), genes in >= {} kept cells ({} kept), nnz {} -> {}".format(
        PERCENTILE, n_keep, MIN_CELLS, g_keep, nnz, nnz_out))
    row_keep = torch.zeros(N, dtype=torch.uint8, device="cuda")
    row_keep[torch.from_numpy(out.cells).cuda()] = 1
    col_mask = torch.zeros(G, dtype=torch.uint8, device="cuda")
    col_mask[torch.from_numpy(out.genes).cuda()] = 1
    kept_nnz = int((row_keep[torch.repeat_interleave(torch.arange(N, device="cuda"), lens, output_size=nnz)] != 0).sum())
    say("kernels alone:")
    total = kernel_line("meld_prep_row_stats (val)", events_ms(lambda: pp.row_stats_device(A)), 8 * nnz + 28 * N)
    total += kernel_line("meld_prep_col_counts, LDS panel (col + val, kept rows)", events_ms(lambda: pp.col_counts_device(A, row_keep, 0)),
                         12 * kept_nnz + 17 * N)
    dev_before = os.environ.get("MELD_DEV")
    os.environ["MELD_DEV"] = "1"  # (the library reads its development switches at every call, and only under MELD_DEV=1)
    os.environ["MELD_PREP_COLCOUNT_GLOBAL"] = "1"
    ref_counts = pp.col_counts_device(A, row_keep, 0)
    kernel_line("  A-B: global atomics only", events_ms(lambda: pp.col_counts_device(A, row_keep, 0)), 12 * kept_nnz + 17 * N)
    del os.environ["MELD_PREP_COLCOUNT_GLOBAL"]
    if dev_before is None:
        del os.environ["MELD_DEV"]
    assert torch.equal(ref_counts, pp.col_counts_device(A, row_keep, 0))
    total += kernel_line("meld_prep_row_stats, column mask (col + val)", events_ms(lambda: pp.row_stats_device(A, col_mask)), 12 * nnz + 28 * N)
    rows_d = torch.from_numpy(out.cells.astype(np.int32)).cuda()
    col_map = torch.full((G,), -1, dtype=torch.int32, device="cuda")
    col_map[torch.from_numpy(out.genes).cuda()] = torch.arange(g_keep, dtype=torch.int32, device="cuda")
    counts = torch.empty(n_keep, dtype=torch.int32, device="cuda")
    mat = (ptr(A.rowptr), ptr(A.col), ptr(A.val), A.val_f32, N, G)
    total += kernel_line("meld_prep_select_count (col, kept rows)", events_ms(lambda: check(lib.meld_prep_select_count(
        mat[0], mat[1], N, G, ptr(rows_d), n_keep, ptr(col_map), ptr(counts), st))), 4 * kept_nnz + 16 * n_keep)
    scale = pp.row_stats_device(A, col_mask)[1][torch.from_numpy(out.cells).cuda()].contiguous()
    o_col, o_val, o_norm = torch.empty_like(out.data.col), torch.empty_like(out.data.val), torch.empty_like(out.data.val)
    total += kernel_line("meld_prep_select_fill (col + val -> col + 2 val)", events_ms(lambda: check(lib.meld_prep_select_fill(
        *mat, ptr(rows_d), n_keep, ptr(col_map), ptr(scale), RESCALE, 1, 5.0, ptr(out.data.rowptr), ptr(o_col), ptr(o_val), ptr(o_norm), st))),
        12 * kept_nnz + 20 * nnz_out + 24 * n_keep)
    assert torch.equal(o_val, out.data.val) and torch.equal(o_norm, out.normalized.val) and torch.equal(o_col, out.data.col)
    del o_col, o_val, o_norm
    say("  the five launches of `run` add up to {:.3f} ms".format(total))
    t_run = wall_ms(lambda: pp.run(A, library_size_percentile=PERCENTILE, min_cells=MIN_CELLS, rescale=RESCALE, transform="sqrt"))
    say("`run` end to end (host clock; read-backs of the vectors, the percentile and the scan included): {}".format(fmt(t_run)))
    t_steps = wall_ms(lambda: pp.sqrt(pp.library_size_normalize(pp.filter_rare_genes(pp.filter_library_size(A, percentile=PERCENTILE)[0], min_cells=MIN_CELLS)[0], RESCALE)))
    say("the single functions one after another (four rewrites): {}".format(fmt(t_steps)))
    t_torch = wall_ms(lambda: torch_pipeline(A))
    rp_t, col_t, val_t, w_t = torch_pipeline(A)
    same = torch.equal(rp_t, out.data.rowptr) and torch.equal(col_t, out.data.col)
    worst = float(((val_t - out.data.val).abs() / out.data.val).max())
    say("torch composition (repeat_interleave, bincount, masks, cumsum): {} | {:.1f} x `run` | same structure: {}, values within {:.1e} relative".format(
        fmt(t_torch), statistics.median(t_torch) / statistics.median(t_run), same, worst))
    del rp_t, col_t, val_t, w_t
    torch.cuda.empty_cache()
    h_rows = N if name == "quickstart" else min(N, args.host_rows)
    end = int(A.rowptr[h_rows])
    from scipy import sparse

    Xh = sparse.csr_matrix((A.val[:end].cpu().numpy(), A.col[:end].cpu().numpy(), A.rowptr[:h_rows + 1].cpu().numpy()), shape=(h_rows, G))
    secs, T, W = host_pipeline(Xh)
    if h_rows == N:
        ok = np.array_equal(T.indptr, out.data.rowptr.cpu().numpy()) and np.array_equal(T.indices, out.data.col.cpu().numpy()) \
            and np.array_equal(W.data, out.normalized.val.cpu().numpy())
        say("host sequence on scipy / sklearn, one thread, all {} rows: {:.2f} s = {:.0f} x `run` | same structure and normalised bits: {}".format(
            N, secs, 1e3 * secs / statistics.median(t_run), ok))
    else:
        say("host sequence on scipy / sklearn, one thread, the first {} rows: {:.2f} s; EXTRAPOLATED to {} rows by the ratio of rows: {:.0f} s = {:.0f} x `run`".format(
            h_rows, secs, N, secs * N / h_rows, 1e3 * secs * N / h_rows / statistics.median(t_run)))
    del A, out, Xh, T, W
    torch.cuda.empty_cache()
