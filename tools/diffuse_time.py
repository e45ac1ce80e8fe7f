"""One diffusion step (meld_diffuse_step) on the benchmark's graph against the routes that exist without it:

    python tools/diffuse_time.py [--n 1000000] [--knn 5,15] [--out FILE] [--label TEXT]

One process.  Per graph (bench.synthetic_cells(N, 50, seed 0), MELD(knn).fit; the first knn is MELD's default):
  (a) one meld_diffuse_step at p = 16, 50, 64, 100, 128;
  (b) the composition available without the kernel, p = 100: two meld_cheby_step_wide calls (64 + 36 columns, panels copied
      beforehand and the copies NOT timed, alpha = -1) plus the elementwise x + y / s in torch;
  (c) torch.sparse CSR P @ F, p = 100;
  (d) the host route: graph.diff_op export plus three scipy products, p = 100;
  (e) op.impute(genes=range(17), t=3) end to end (device work, read-back, DataFrame).
Device times are HIP events around single launches after warm-up: median (min, max) over repeated launches.  Achieved bytes per
second are the algorithmic traffic nnz * 12 + 2 N p 8 + N 24 over the median, also as a fraction of bench.PEAK_HBM_GBS."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import meld_amd
from bench import PEAK_HBM_GBS, synthetic_cells
from meld_amd import _lib
from meld_amd import filter as mf
from meld_amd.diffuse import walk_vectors

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--knn", default="5,15")
ap.add_argument("--out", default=None)
ap.add_argument("--label", default="")
ap.add_argument("--reps", type=int, default=15)
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("tools/diffuse_time.py measures on the GPU: none found")

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def timed(fn, reps=None, warm=3):
    """median, min, max in ms of single calls of fn between two events"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps or args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return "median {:.3f} ms (min {:.3f}, max {:.3f}, n={})".format(t[0], t[1], t[2], args.reps)


prop = torch.cuda.get_device_properties(0)
free, total = torch.cuda.mem_get_info()
mhz = getattr(prop, "clock_rate", 0) // 1000
say("device: {} CUs {} HBM GiB {:.0f} | torch {} hip {} | clock_rate {} (device property: the maximum engine clock; "
    "clocks are not pinned)".format(prop.name, prop.multi_processor_count, prop.total_memory / 2**30, torch.__version__,
                                   torch.version.hip, "{} MHz".format(mhz) if mhz else "not reported"))
say("memory free/total GiB at start: {:.1f} / {:.1f} | {}".format(free / 2**30, total / 2**30, args.label))
N = args.n
say("data: synthetic_cells({}, 50, seed 0); device times: HIP events around single launches after 3 warm-up calls".format(N))
X, _ = synthetic_cells(N, 50, seed=0)
lib = _lib.get_lib()
st = torch.cuda.current_stream().cuda_stream

for knn in [int(k) for k in args.knn.split(",")]:
    op = meld_amd.MELD(knn=knn, verbose=0).fit(X)
    G = op.graph
    ops = mf._ops_of(G)
    kd, s = walk_vectors(G)
    nnz = G.nnz
    say("--- knn {} nnz {} mean degree {:.1f} max degree {} perm {}".format(
        knn, nnz, nnz / N, int((G.rowptr[1:] - G.rowptr[:-1]).max()), G.perm is not None))
    head = [_lib.ptr(G.rowptr), _lib.ptr(G.col), _lib.ptr(G.val), _lib.ptr(kd), _lib.ptr(s), N]
    gen = torch.Generator(device="cuda").manual_seed(1)
    a100 = None
    for p in (16, 50, 64, 100, 128):
        x = torch.rand(N, p, dtype=torch.float64, device="cuda", generator=gen)
        y = torch.empty_like(x)

        def step(x=x, y=y, p=p):
            _lib.check(lib.meld_diffuse_step(*head, _lib.ptr(x), p, _lib.ptr(y), p, p, st), "meld_diffuse_step")

        t = timed(step)
        byts = nnz * 12 + 2 * N * p * 8 + N * 24
        say("(a) meld_diffuse_step p={:3d}: {} | {:.0f} GB/s of algorithmic traffic ({:.3f} GB), {:.3f} of {:.0f} GB/s".format(
            p, fmt(t), byts / t[0] / 1e6, byts / 1e9, byts / t[0] / 1e6 / PEAK_HBM_GBS, PEAK_HBM_GBS))
        if p == 100:
            a100, x100, y100 = t, x, y.clone()
    # (b) what exists without the kernel
    p = 100
    xa, xb = x100[:, :64].contiguous(), x100[:, 64:].contiguous()
    ya, yb = torch.empty_like(xa), torch.empty_like(xb)
    out_b = torch.empty_like(x100)
    s_col = s[:, None]

    def composed():
        ops.cheby_step_wide(G, 64, xa, 0, None, ya, -1.0, 0.0, 0.0)  # W x - dw .* x
        ops.cheby_step_wide(G, 36, xb, 0, None, yb, -1.0, 0.0, 0.0)
        torch.add(xa, ya / s_col, out=out_b[:, :64])  # x + (W x - dw x) / s = (W x + kd x) / s
        torch.add(xb, yb / s_col, out=out_b[:, 64:])

    tb = timed(composed)
    say("(b) two meld_cheby_step_wide (64 + 36 columns, copies not timed) + x + y / s in torch, p=100: {} | max |(a) - (b)| = {:.3e}".format(
        fmt(tb), float((out_b - y100).abs().max())))
    say("    (a) / (b) at p=100: {:.3f}  ({})".format(a100[0] / tb[0], "the fused step is not slower" if a100[0] <= tb[0] else "THE FUSED STEP IS SLOWER"))
    # (c) torch.sparse
    try:
        rows = torch.repeat_interleave(torch.arange(N, device="cuda"), G.rowptr[1:] - G.rowptr[:-1])
        diag = torch.arange(N, device="cuda")
        Pm = torch.sparse_coo_tensor(torch.stack([torch.cat([rows, diag]), torch.cat([G.col.to(torch.int64), diag])]),
                                     torch.cat([G.val / s[rows], kd / s]), (N, N)).coalesce().to_sparse_csr()
        del rows, diag
        out_c = Pm @ x100
        tc = timed(lambda: torch.matmul(Pm, x100), reps=5, warm=1)
        say("(c) torch.sparse CSR P @ F, p=100: median {:.3f} ms (min {:.3f}, max {:.3f}, n=5) | max |(a) - (c)| = {:.3e}".format(
            tc[0], tc[1], tc[2], float((out_c - y100).abs().max())))
        del Pm, out_c
    except Exception as e:  # noqa: BLE001  (a route that does not exist on this stack is a result, too)
        say("(c) torch.sparse CSR P @ F: not available here ({}: {})".format(type(e).__name__, str(e)[:200]))
    # (d) the host route, in the caller's order
    F_host = np.random.default_rng(2).random((N, p))
    t0 = time.perf_counter()
    P = G.diff_op
    t1 = time.perf_counter()
    R = F_host
    for _ in range(3):
        R = P @ R
    t2 = time.perf_counter()
    dev3 = G.diffuse_device(torch.from_numpy(F_host).cuda(), t=3)
    torch.cuda.synchronize()
    say("(d) host route, p=100: graph.diff_op export {:.3f} s + three scipy products {:.3f} s = {:.3f} s | max |device - host| after 3 steps = {:.3e}".format(
        t1 - t0, t2 - t1, t2 - t0, float(np.abs(dev3.cpu().numpy() - R).max())))
    t3 = timed(lambda: G.diffuse_device(dev3, t=3, device_order=True), reps=5, warm=1)
    say("    diffuse_device(F [N, 100], t=3, device_order=True): median {:.3f} ms (min {:.3f}, max {:.3f}, n=5)".format(*t3))
    del P, R, dev3, F_host
    # (e) impute end to end
    op.impute(genes=range(17), t=3)
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        df = op.impute(genes=range(17), t=3)
        ts.append((time.perf_counter() - t0) * 1e3)
    say("(e) op.impute(genes=range(17), t=3) end to end -> DataFrame {}: median {:.1f} ms (min {:.1f}, max {:.1f}, n=5)".format(
        df.shape, statistics.median(ts), min(ts), max(ts)))
    del op, G, df
    torch.cuda.empty_cache()
