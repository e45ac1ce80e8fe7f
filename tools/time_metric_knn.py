"""Time the L1 / L-infinity graph builder beyond the dense route (meld_amd/metric_knn.py, csrc/metric_knn.hip) on the GPU.

    python tools/time_metric_knn.py [--n 100000 1000000] [--d 50] [--metrics manhattan chebyshev] [--knn 7] [--no-prune] [--fit]

Data: oracle.synthetic_cells(n, n_dims=d).  Reports, as JSON lines per (n, metric): the per-stage seconds of one build after a
warm-up build at the smallest size (host clock around device syncs), the tile pairs computed and skipped, the flagged rows;
with --fit the wall time of MELD(distance=metric).fit(X) from host data (the acceptance figure of DESIGN.md section 4.8)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MELD_DEV", "1")
import torch

from oracle import meld_oracle as mo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--metrics", nargs="+", default=["manhattan", "chebyshev"])
    ap.add_argument("--knn", type=int, default=7)
    ap.add_argument("--no-prune", action="store_true")
    ap.add_argument("--fit", action="store_true")
    args = ap.parse_args()
    if args.no_prune:
        os.environ["MELD_METRIC_PRUNE"] = "0"
    import meld_amd
    from meld_amd.metric_knn import build_metric_knn_graph

    warm = mo.synthetic_cells(20000, n_dims=args.d, seed=1)[0]
    for metric in args.metrics:
        build_metric_knn_graph(torch.from_numpy(warm).cuda(), args.knn, 40, 1e-4, 1, metric)
    torch.cuda.synchronize()
    for n in args.n:
        X, _ = mo.synthetic_cells(n, n_dims=args.d, seed=0)
        Xd = torch.from_numpy(X).cuda()
        for metric in args.metrics:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            G = build_metric_knn_graph(Xd, args.knn, 40, 1e-4, 1, metric, profile=True)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            i = G.info
            row = dict(n=n, d=args.d, metric=metric, knn=args.knn, ksel=i["ksel"], prune=i["prune"], build_s=round(wall, 4),
                       stages_s={k: round(v, 4) for k, v in i["stage_seconds"].items()}, tiles_done=i["tiles_done"],
                       tile_skip_fraction=round(i["tile_skip_fraction"], 4), n_flagged_rows=i["n_flagged_rows"], nnz=i["nnz"])
            del G
            if args.fit:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                meld_amd.MELD(knn=args.knn, distance=metric, verbose=0).fit(X)
                torch.cuda.synchronize()
                row["fit_s"] = round(time.perf_counter() - t0, 4)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
