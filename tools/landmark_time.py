"""The landmark operator on the benchmark's graph (meld_amd/landmark.py, csrc/landmark.hip): its three stages timed apart, and the
route that exists without it:

    python tools/landmark_time.py [--n 1000000] [--knn 5,15] [--landmarks 2000] [--host-n 100000] [--out FILE] [--label TEXT]

One process.  Per graph (bench.synthetic_cells(N, 50, seed 0), MELD(knn).fit; the first knn is MELD's default):
  (a) the default clustering: the range finder with its singular vectors and features, and the k-means on them (a sequential
      k-means++ and library Lloyd steps), as wall clocks around calls that end in a synchronisation;
  (b) given those labels: the merge (count launch, scan, one word read back, fill launch), the transpose (keys, radix sort, CSR
      assembly) and the Gram launch -- HIP events / wall clocks after one untimed call of the same shape, median (min - max);
  (c) the host route on a graph of --host-n cells built the same way, with labels from the same clustering there: G.K exported, then
      scipy's three sparse products (K @ onehot, the two scaled copies, pmn @ pnm), against the device's merge + transpose + Gram on
      that graph, the two operators compared.
Clocks are not pinned; every figure is of this run."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch
from scipy import sparse

import meld_amd
from bench import synthetic_cells
from meld_amd import landmark
from meld_amd.diffuse import walk_vectors

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--knn", default="5,15")
ap.add_argument("--landmarks", type=int, default=2000)
ap.add_argument("--host-n", type=int, default=100_000)
ap.add_argument("--out", default=None)
ap.add_argument("--label", default="")
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("tools/landmark_time.py measures on the GPU: none found")

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
    return "median {:.2f} ms ({:.2f} - {:.2f})".format(*t)


def stages(G, label_dev, L):
    """the three device stages of the algebra for given compact labels; returns (A, op, s, timings)"""
    kd, _ = walk_vectors(G)
    merge = lambda: landmark.merge_by_label(G.rowptr, G.col, G.val, G.N, label_dev, L, kd=kd, colmap=G.perm)
    A = merge()
    from meld_amd.sparse import DeviceCSR

    transpose = lambda: DeviceCSR(A[0], A[1], A[2], (G.N, L)).T
    t_merge, t_tr = repeated(merge), repeated(transpose)
    gram = lambda: landmark._gram(A, G.N, L)
    t_both = repeated(gram)  # (transpose + Gram launch, as the product calls them)
    op, s = gram()
    return A, op, s, (t_merge, t_tr, t_both)


def clustering(G, n_landmark):
    """the default clustering with its two stages timed apart (landmark.default_clusters is the two in a row)"""
    from meld_amd.kmeans import kmeans_device

    info, km = {}, {}
    feats, t_feat = wall(lambda: landmark.spectral_features(G, n_landmark, n_svd=100, random_state=0, info=info))
    lab, t_km = wall(lambda: kmeans_device(feats, n_landmark, n_init=1, max_iter=landmark.KMEANS_MAX_ITER, seed=0, info=km,
                                           seeding="k-means++", prefer="lds")["labels"].to(torch.int64))
    info.update(kmeans_iterations=km.get("iterations"), seconds_features=t_feat, seconds_kmeans=t_km)
    if G.perm is not None:
        out = torch.empty_like(lab)
        out[G.perm] = lab
        lab = out
    return lab, t_feat + t_km, info


prop = torch.cuda.get_device_properties(0)
free, total = torch.cuda.mem_get_info()
say("device: {} CUs {} HBM GiB {:.0f} | torch {} hip {} (clocks are not pinned)".format(
    prop.name, prop.multi_processor_count, prop.total_memory / 2**30, torch.__version__, torch.version.hip))
say("memory free/total GiB at start: {:.1f} / {:.1f} | {}".format(free / 2**30, total / 2**30, args.label))
say("data: synthetic_cells(N, 50, seed 0); L = {} landmarks; wall clocks around synchronised calls, one untimed call first, n={}".format(
    args.landmarks, args.reps))

for knn in [int(k) for k in args.knn.split(",")]:
    for N, host in ((args.n, False), (args.host_n, True)):
        X, _ = synthetic_cells(N, 50, seed=0)
        G = meld_amd.MELD(knn=knn, verbose=0).fit(X).graph
        say("--- knn {} N {} nnz {} mean degree {:.1f} max degree {} perm {}".format(
            knn, N, G.nnz, G.nnz / N, int((G.rowptr[1:] - G.rowptr[:-1]).max()), G.perm is not None))
        lab, t_cluster, info = clustering(G, args.landmarks)
        compact, values = landmark.compact_labels(lab.cpu().numpy())
        L = int(values.shape[0])
        say("(a) default clustering: {:.2f} s in all, of which range finder + singular vectors + features {:.2f} s and k-means {:.2f} s "
            "({} Lloyd steps, n_svd {}); {} of {} landmarks are not empty".format(
                t_cluster, info.get("seconds_features", float("nan")), info.get("seconds_kmeans", float("nan")),
                info.get("kmeans_iterations"), info.get("n_svd"), L, args.landmarks))
        label_dev = torch.from_numpy(compact).cuda()
        A, op, s, (t_merge, t_tr, t_both) = stages(G, label_dev, L)
        say("(b) given the labels: merge {} | transpose {} | transpose + Gram {} | entries of A {} ({:.2f} per cell), rows of the operator "
            "sum to 1 within {:.1e}".format(fmt(t_merge), fmt(t_tr), fmt(t_both), int(A[1].shape[0]), int(A[1].shape[0]) / N,
                                            float((op.sum(1) - 1).abs().max())))
        algebra = t_merge[0] + t_both[0]
        say("    algebra (merge + transpose + Gram) {:.1f} ms; clustering share of clustering + algebra: {:.4f}".format(
            algebra, t_cluster / (t_cluster + algebra * 1e-3)))
        if host:
            t0 = time.perf_counter()
            K = G.K
            t_export = time.perf_counter() - t0
            t0 = time.perf_counter()
            C = sparse.csr_matrix((np.ones(N), (np.arange(N), compact)), shape=(N, L))
            Ah = (K @ C).tocsr()
            pnm = sparse.diags(1.0 / np.asarray(Ah.sum(1)).ravel()) @ Ah
            pmn = sparse.diags(1.0 / np.asarray(Ah.sum(0)).ravel()) @ Ah.T.tocsr()
            oph = np.asarray((pmn @ pnm).todense())
            t_host = time.perf_counter() - t0
            _, t_back = wall(lambda: op.cpu().numpy())
            diff = float(np.abs(op.cpu().numpy() - oph).max())
            say("(c) host route at N = {}: export of G.K {:.2f} s + scipy's products {:.2f} s = {:.2f} s | device algebra {:.4f} s + read-back "
                "of the operator {:.4f} s | device / scipy alone {:.4f}, device / host route {:.4f} | largest difference of the operators "
                "{:.1e}".format(N, t_export, t_host, t_export + t_host, algebra * 1e-3, t_back, (algebra * 1e-3 + t_back) / t_host,
                                (algebra * 1e-3 + t_back) / (t_export + t_host), diff))
        del G, A, op, s
        torch.cuda.empty_cache()
