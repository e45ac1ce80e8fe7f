"""Time the out-of-sample extension (meld_amd/extend.py, csrc/extend.hip) on the GPU: new cells against the benchmark graph.

    python tools/time_extend.py [--n 1000000] [--m 100000] [--d 50] [--knn 15] [--p 2] [--reps 5] [--cross-reps 3] [--apply-reps 20] [--inner 10]

Data: oracle.synthetic_cells(n + m, n_dims=d): the first n cells are fitted (MELD(knn).fit), the last m are new.  Reports JSON lines:

1. the kernel-to-data stage (``DeviceGraph.kernel_to_data_device``: MFMA search between two point sets, exact refinement,
   ``meld_extend_rows``) against the library route for the same work (``mnn.cross_kernel``: chunked fp64 GEMMs + topk); host clock
   around device synchronisations, median of ``--reps`` after a warm-up; both produce the same matrix (nnz and values compared);
2. ``meld_extend_apply`` at p columns against ``torch.sparse`` CSR x dense on the same matrix (the transitions normalised in
   advance for the library, which has no fused normalisation): the two routes in turn, one sample = ``--inner`` calls back to back
   between two device events (a call is some 50 us: around a single one the events' own cost would show), median and quartiles of
   ``--apply-reps`` samples after a warm-up, and the bytes the kernel
   must move (12 per entry + 8 p gathered per entry + 24 per row + 8 p written per row) over the time, as a fraction of the HBM
   rate MI355X_MICROARCH.md gives (6.29 TB/s measured copy rate, 8 TB/s spec).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MELD_DEV", "1")
import torch

from oracle import meld_oracle as mo

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12


def host_timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, ts


def event_timed_alternating(fns, reps, inner):
    """Seconds per call of each of ``fns``, taken in turn (a, b, a, b, ...) so that drift hits both alike; one sample is ``inner``
    calls back to back between two device events, so that the events' own cost is spread over them."""
    ts = [[] for _ in fns]
    outs = [None] * len(fns)
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                outs[i] = fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b) * 1e-3 / inner)
    return outs, ts


def spread_us(ts):
    q = statistics.quantiles(ts, n=4)
    return dict(median=round(1e6 * statistics.median(ts), 1), min=round(1e6 * min(ts), 1), q1=round(1e6 * q[0], 1), q3=round(1e6 * q[2], 1),
                max=round(1e6 * max(ts), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--knn", type=int, default=15)
    ap.add_argument("--p", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cross-reps", type=int, default=3)
    ap.add_argument("--apply-reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_extend.py needs a GPU")
    import meld_amd
    from meld_amd.extend import apply_transitions
    from meld_amd.mnn import cross_kernel

    X, _ = mo.synthetic_cells(args.n + args.m, n_dims=args.d, seed=0)
    op = meld_amd.MELD(knn=args.knn, verbose=0)
    op.fit(X[: args.n])
    G = op.graph
    st = G._extend_state
    Yd = torch.from_numpy(X[args.n:]).cuda()
    G.kernel_to_data_device(Yd[:4096])  # warm-up: code objects, allocator
    csr, ts = host_timed(lambda: G.kernel_to_data_device(Yd), args.reps)
    nnz = int(csr[1].shape[0])
    print(json.dumps(dict(stage="kernel_to_data", route="hip", n=args.n, m=args.m, d=args.d, knn=args.knn, nnz=nnz, median_s=round(statistics.median(ts), 4),
                          min_s=round(min(ts), 4), max_s=round(max(ts), 4), reps=args.reps, clock="host perf_counter around device synchronise")), flush=True)
    if args.cross_reps > 0:
        cross_kernel(Yd[:4096], st.X, args.knn, st.decay, st.thresh)
        (r, c, v), ts2 = host_timed(lambda: cross_kernel(Yd, st.X, args.knn, st.decay, st.thresh), args.cross_reps)
        same = int(r.shape[0]) == nnz
        if same:
            o = torch.argsort((r << 32) | c)
            same = bool(torch.equal(c[o].to(torch.int32), csr[1])) and float(((v[o] - csr[2]).abs() / csr[2]).max()) < 1e-9
        print(json.dumps(dict(stage="kernel_to_data", route="library (mnn.cross_kernel)", nnz=int(r.shape[0]), same_matrix=same,
                              median_s=round(statistics.median(ts2), 4), min_s=round(min(ts2), 4), max_s=round(max(ts2), 4), reps=args.cross_reps, speedup=round(statistics.median(ts2) / statistics.median(ts), 2),
                              clock="host perf_counter around device synchronise")), flush=True)
        del r, c, v
    p, M = args.p, args.m
    F = torch.randn(args.n, p, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    need = 12 * nnz + 8 * p * nnz + 24 * M + 8 * p * M
    rowptr, col, val, rowsum = csr
    tvals = val / torch.repeat_interleave(rowsum, rowptr[1:] - rowptr[:-1])
    A = torch.sparse_csr_tensor(rowptr, col.to(torch.int64), tvals, size=(M, args.n))
    apply_transitions(csr, F)
    torch.sparse.mm(A, F)
    (out, ref), (ta, tl) = event_timed_alternating([lambda: apply_transitions(csr, F), lambda: torch.sparse.mm(A, F)], args.apply_reps, args.inner)
    t_med = statistics.median(ta)
    diff = float((out - ref).abs().max() / ref.abs().max())
    print(json.dumps(dict(stage="apply", p=p, m=M, nnz=nnz, mean_row=round(nnz / M, 1), hip_us=spread_us(ta), torch_sparse_us=spread_us(tl),
                          speedup=round(statistics.median(tl) / t_med, 2), speedup_q1q3=[round(statistics.quantiles(tl, n=4)[0] / statistics.quantiles(ta, n=4)[2], 2),
                                                                                        round(statistics.quantiles(tl, n=4)[2] / statistics.quantiles(ta, n=4)[0], 2)],
                          max_rel_diff=diff, bytes_needed=need, gb_per_s=round(need / t_med / 1e9, 1),
                          frac_hbm_measured=round(need / t_med / HBM_MEASURED, 3), frac_hbm_spec=round(need / t_med / HBM_SPEC, 3),
                          note="F ({} MB) stays in the caches: the gathered bytes are not HBM traffic".format(round(8e-6 * p * args.n, 1)),
                          clock="device events around {} calls back to back, the two routes in turn".format(args.inner), reps=args.apply_reps)), flush=True)

if __name__ == "__main__":
    main()
