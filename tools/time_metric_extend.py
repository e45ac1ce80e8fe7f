"""Time new cells on the L1 / L-infinity graphs (meld_amd/metric_knn.py ``cross_kernel_rows``, csrc/metric_knn.hip) on the GPU.

    python tools/time_metric_extend.py [--n 1000000] [--d 50] [--knn 7] [--m 100000,1000] [--metrics manhattan,chebyshev]
                                       [--reps 5] [--brute-reps 5] [--brute-budget 600]

Data: oracle.synthetic_cells(n + max(m), n_dims=d): the first n cells are fitted (``MELD(distance=metric, knn, n_pca=None).fit``),
the next m are new.  Per metric and m, one JSON line:

* ``kernel_to_data_device`` (seed pre-pass, sort, search, refinement, sweep, ``meld_extend_rows``): median, min and max of ``--reps``
  calls after a warm-up, host clock around a device synchronise; the fraction of (query tile, reference tile) pairs visited;
* a library brute force of the same matrix in the same run, its calls alternating with those of the new path: ``torch.cdist`` with
  p = 1 / inf in chunks of rows (2^23 pairs a launch: the library's kernel is wrong beyond 2^32 threads in one), ``topk`` for the
  bandwidth, the kernel and the threshold.  ``same_matrix``: identical pattern, values within 1e-9.  Where ``--brute-reps`` full
  passes would take longer than ``--brute-budget`` seconds (estimated from the first chunks) fewer are run -- at least one --, and
  where even one would, that one covers the first ``brute_rows`` new cells only: its time is then scaled to all m
  (``extrapolated``) and the matrices are compared on those rows.  The line says which.
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

EPS = 2.0 ** -52


def brute_force(Yd, Xd, p, knn, decay, thresh, max_rows=None):
    """(keys (row << 32) | col ascending, values) of the kernel from Yd to Xd by library calls."""
    M, N = int(Yd.shape[0]), int(Xd.shape[0])
    M = M if max_rows is None else min(M, max_rows)
    rows = max(1, (1 << 23) // N)
    keys, vals = [], []
    for lo in range(0, M, rows):
        D = torch.cdist(Yd[lo:min(M, lo + rows)], Xd, p=p)
        bw = torch.clamp(torch.topk(D, knn, dim=1, largest=False).values[:, -1], min=EPS)
        K = torch.exp(-torch.pow(D / bw[:, None], decay))
        K = torch.where(torch.isnan(K), torch.ones_like(K), K)
        hit = torch.nonzero(K >= thresh)
        keys.append(((hit[:, 0] + lo) << 32) | hit[:, 1])
        vals.append(K[hit[:, 0], hit[:, 1]])
    return torch.cat(keys), torch.cat(vals)  # (nonzero is row-major: ascending already)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def same_matrix(csr, keys, vals, n_rows):
    rowptr, col, val, _ = csr
    rowptr = rowptr[: n_rows + 1]
    nnz = int(rowptr[-1])
    if nnz != int(keys.shape[0]):
        return False, nnz
    r = torch.repeat_interleave(torch.arange(n_rows, device=col.device), rowptr[1:] - rowptr[:-1])
    mine = (r << 32) | col[:nnz].to(torch.int64)
    if not bool(torch.equal(mine, keys)):
        return False, nnz
    return float(((val[:nnz] - vals).abs() / vals).max()) <= 1e-9, nnz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--knn", type=int, default=7)
    ap.add_argument("--m", default="100000,1000")
    ap.add_argument("--metrics", default="manhattan,chebyshev")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--brute-reps", type=int, default=5)
    ap.add_argument("--brute-budget", type=float, default=600.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_metric_extend.py needs a GPU")
    import meld_amd

    ms = [int(v) for v in args.m.split(",")]
    X, _ = mo.synthetic_cells(args.n + max(ms), n_dims=args.d, seed=0)
    for metric in args.metrics.split(","):
        op = meld_amd.MELD(knn=args.knn, distance=metric, n_pca=None, verbose=0)
        _, t_fit = timed(lambda: op.fit(X[: args.n]))
        G = op.graph
        st = G._extend_state
        p = 1.0 if metric != "chebyshev" else float("inf")
        Xd = st.X
        for m in ms:
            Yd = torch.from_numpy(X[args.n: args.n + m]).cuda()
            G.kernel_to_data_device(Yd)  # warm-up: code objects, allocator, the cached fitted cells and their boxes
            # the brute force: how long is a pass?
            probe = min(m, 4 * max(1, (1 << 23) // args.n))
            brute_force(Yd, Xd, p, args.knn, st.decay, st.thresh, max_rows=probe)
            _, t_probe = timed(lambda: brute_force(Yd, Xd, p, args.knn, st.decay, st.thresh, max_rows=probe))
            est = t_probe * m / probe
            brute_reps = int(max(1, min(args.brute_reps, args.brute_budget // max(est, 1e-9))))
            rows_b = m if est <= args.brute_budget else int(max(probe, m * args.brute_budget / est))
            ts, tb, same, nnz = [], [], None, None
            for rep in range(args.reps):
                csr, t = timed(lambda: G.kernel_to_data_device(Yd))
                ts.append(t)
                stats = dict(G.last_extend)
                if rep < brute_reps:
                    (keys, vals), t = timed(lambda: brute_force(Yd, Xd, p, args.knn, st.decay, st.thresh, max_rows=rows_b))
                    tb.append(t * m / rows_b)
                    if same is None:
                        same, nnz = same_matrix(csr, keys, vals, rows_b)
                    del keys, vals
            med, medb = statistics.median(ts), statistics.median(tb)
            print(json.dumps(dict(
                metric=metric, n=args.n, m=m, d=args.d, knn=args.knn, fit_s=round(t_fit, 3), nnz_compared=nnz,
                hip=dict(median_s=round(med, 4), min_s=round(min(ts), 4), max_s=round(max(ts), 4), reps=args.reps),
                tiles_visited_fraction=round(stats["tiles_done"] / max(stats["tile_pairs"], 1), 4), n_slices=stats["n_slices"],
                n_flagged_rows=stats["n_flagged_rows"],
                brute_force=dict(median_s=round(medb, 4), min_s=round(min(tb), 4), max_s=round(max(tb), 4), reps=brute_reps,
                                 reps_asked=args.brute_reps, estimated_pass_s=round(est, 2), brute_rows=rows_b, extrapolated=rows_b < m),
                same_matrix=bool(same), speedup=round(medb / med, 2),
                clock="host perf_counter around device synchronise, the two routes in turn")), flush=True)
            del Yd
        del op, G, st, Xd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
