"""Time the partial Fourier basis (meld_amd/spectrum.py, csrc/subspace.hip) on the GPU.

    python tools/time_fourier_partial.py [--n 1000000] [--d 50] [--knn 15] [--k 16,48] [--reps 5] [--block-reps 10] [--inner 3] [--host-n 100000]

Data: oracle.synthetic_cells(n, n_dims=d), graph by MELD(knn).fit.  Reports JSON lines:

1. per k: wall time of ``fourier_basis_device(k, recompute=True)`` (host clock around device synchronisations, median / min / max of
   ``--reps`` runs after a warm-up), the outer iterations and filter degrees, and the per-stage split from the library's own
   ``_EventSpan`` timers (device events; medians over the same runs): filter (every wide step), Gram, rotate, residuals;
2. each block operation at [n, 64] against the library route it replaces -- Gram: chunked ``torch.bmm`` (``_device_ops.tall_gram``);
   rotate: ``V @ S``; orthonormalisation (2 x (Gram + host eigh + rotate)): ``torch.linalg.qr``; residuals: the tensor expression --
   the two routes in turn, one sample = ``--inner`` calls between two device events, median and quartiles of ``--block-reps`` samples;
3. with ``--host-n`` > 0: ``scipy.sparse.linalg.eigsh`` in shift-invert mode on a graph of that many cells (the comparison pygsp
   would make, one host process), same k, against the device iteration on the same graph.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MELD_DEV", "1")
import numpy as np
import torch

from oracle import meld_oracle as mo

STAGES = ("fourier_filter", "fourier_gram", "fourier_rotate", "fourier_residuals")


def spread(ts, scale=1e3, nd=3):
    q = statistics.quantiles(ts, n=4) if len(ts) > 1 else [ts[0]] * 3
    return dict(median=round(scale * statistics.median(ts), nd), min=round(scale * min(ts), nd), q1=round(scale * q[0], nd), q3=round(scale * q[2], nd),
                max=round(scale * max(ts), nd))


def event_timed_alternating(fns, reps, inner):
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b) * 1e-3 / inner)
    return ts


def fit(n, d, knn):
    import meld_amd

    X, _ = mo.synthetic_cells(n, n_dims=d, seed=0)
    op = meld_amd.MELD(knn=knn, verbose=0)
    op.fit(X)
    return op.graph


def time_basis(G, k, reps):
    from meld_amd import graph as mg

    G.fourier_basis_device(k, recompute=True)  # warm-up: code objects, allocator
    wall, stages = [], {s: [] for s in STAGES}
    for _ in range(reps):
        mg.record_events(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        G.fourier_basis_device(k, recompute=True)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        ev = mg.event_times_ms()
        mg.record_events(False)
        for s in STAGES:
            stages[s].append(1e-3 * sum(ev.get(s, [])))
    info = G.fourier_partial_info
    return dict(stage="basis", n=G.N, k=k, reps=reps, wall_s=spread(wall, 1.0, 4), iterations=info["iterations"], degrees=info["degrees"],
                wide_steps=info["wide_steps"], ub_rule=info["ub_rule"], worst_residual_over_ub=info["worst_residual"] / info["ub"],
                stages_s={s: spread(v, 1.0, 4) for s, v in stages.items()},
                clock="host perf_counter around device synchronise; stages: device events of the library's _EventSpan")


def time_blocks(G, reps, inner):
    from meld_amd._device_ops import tall_gram
    from meld_amd.filter import _ops_of
    from meld_amd.spectrum import orthonormaliser

    ops, n, m = _ops_of(G), G.N, 64
    f64 = dict(dtype=torch.float64, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    V, W = torch.randn(n, m, generator=gen, **f64), torch.randn(n, m, generator=gen, **f64)
    S = torch.linalg.qr(torch.randn(m, m, generator=gen, **f64))[0].contiguous()
    theta = torch.rand(m, generator=gen, **f64)
    nb = ops.block_n_blocks(n)
    part, C, out, res = torch.empty(nb * m * m, **f64), torch.empty(m, m, **f64), torch.empty(n, m, **f64), torch.empty(m, **f64)
    Sd = torch.empty(m, m, **f64)

    def ortho_hip():
        out.copy_(V)
        for _ in range(2):
            ops.block_gram(out, out, n, m, part, nb, C)
            Sd.copy_(torch.from_numpy(orthonormaliser(C.cpu().numpy())))
            ops.block_rotate(out, Sd, n, m, out)

    pairs = dict(
        gram=(lambda: ops.block_gram(V, W, n, m, part, nb, C), lambda: tall_gram(V, W)),
        rotate=(lambda: ops.block_rotate(V, S, n, m, out), lambda: torch.matmul(V, S, out=out)),
        residuals=(lambda: ops.block_residuals(W, V, theta, n, m, part, nb, res), lambda: ((W - theta[None, :] * V) ** 2).sum(0)),
        orthonormalise=(ortho_hip, lambda: torch.linalg.qr(V)),
    )
    for name, (hip, lib) in pairs.items():
        hip(), lib()
        th, tl = event_timed_alternating([hip, lib], reps, inner)
        yield dict(stage="block", op=name, n=n, m=m, hip_ms=spread(th), library_ms=spread(tl), speedup=round(statistics.median(tl) / statistics.median(th), 2),
                   clock="device events around {} calls back to back, the two routes in turn".format(inner), reps=reps)


def time_host(n, d, knn, ks):
    from scipy.sparse.linalg import eigsh

    from meld_amd.spectrum import upper_bound

    G = fit(n, d, knn)
    L = G.L.tocsc()
    ub = upper_bound(G)[0]
    for k in ks:
        G.fourier_basis_device(k, recompute=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e_d = G.fourier_basis_device(k, recompute=True)[0].cpu().numpy()
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        e_h = np.sort(eigsh(L, k, sigma=-1e-3 * ub, which="LM", return_eigenvectors=True)[0])
        t_host = time.perf_counter() - t0
        yield dict(stage="host_comparison", n=n, k=k, device_s=round(t_dev, 3), eigsh_shift_invert_s=round(t_host, 3), iterations=G.fourier_partial_info["iterations"],
                   max_abs_diff_over_ub=float(np.abs(e_d - e_h).max() / ub), samples=1, clock="host perf_counter")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--knn", type=int, default=15)
    ap.add_argument("--k", default="16,48")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--block-reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--host-n", type=int, default=100_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_fourier_partial.py needs a GPU")
    ks = [int(v) for v in args.k.split(",") if v]
    if args.n > 0:
        G = fit(args.n, args.d, args.knn)
        for k in ks:
            print(json.dumps(time_basis(G, k, args.reps)), flush=True)
        if args.block_reps > 0:
            for line in time_blocks(G, args.block_reps, args.inner):
                print(json.dumps(line), flush=True)
        del G
    if args.host_n > 0:
        for line in time_host(args.host_n, args.d, args.knn, ks):
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
