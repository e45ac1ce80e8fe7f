"""k-means with thousands of centres (meld_amd/kmeans.py, csrc/kmeans_wide.hip) against the route that existed before it
(``kmeans_device`` with a sequential k-means++ and the LDS step preferred, here ``library_step``), in one run:

    python tools/kmeans_time.py [--shapes 1000000x100x2000,1000000x50x2000,100000x100x4096] [--landmarks-n 1000000] [--landmarks 2000]
                                [--reps 10] [--out FILE] [--label TEXT]

Per shape n x d x k (a seeded mixture of k Gaussians on the device, the starting centres k of its rows):
  (a) one Lloyd step through ``kmeans.library_step`` and through ``kmeans.lloyd_step``, the two alternating, device events around each
      call after two untimed calls of each; the device step's assign, sort + counts and sums launches apart; the two routes' labels
      and centres compared;
  (b) both seedings: ``kmeans_device(max_iter=0, seeding="k-means++", prefer="lds")`` (k passes, a read-back in each, then one
      library step) and ``kmeans_device(max_iter=0)`` (k-means||, then one assign), wall clocks around synchronised calls, with the
      inertia each seeding starts Lloyd from.
Then, on MELD(knn=5).fit(bench.synthetic_cells(N, 50, seed 0)): (c) ``spectral_features`` once and both k-means on them, (d) whole
``landmarks(L, recompute=True)`` by both routes (wall clocks).
The baseline of every ratio is the library route measured in this run.  Clocks are not pinned; every figure is of this run."""
import argparse
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import meld_amd
from meld_amd import kmeans as km


def _kmeans(Y, k, **kw):
    """the library route: sequential k-means++, the LDS step preferred (beyond what it stages: ``library_step``)"""
    return km.kmeans_device(Y, k, seeding="k-means++", prefer="lds", **kw)["labels"].to(torch.int64)


ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="1000000x100x2000,1000000x50x2000,100000x100x4096")
ap.add_argument("--landmarks-n", type=int, default=1_000_000)
ap.add_argument("--landmarks", type=int, default=2000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
ap.add_argument("--label", default="")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("tools/kmeans_time.py measures on the GPU: none found")

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def commit():
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out = subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
        return out.stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def alternating(fns):
    """{name: (median, min, max) ms} of the calls in ``fns`` by device events, the calls alternating, two untimed rounds first"""
    for _ in range(2):
        for fn in fns.values():
            fn()
    times = {name: [] for name in fns}
    for _ in range(args.reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def fmt(t):
    return "median {:.2f} ms ({:.2f} - {:.2f})".format(*t)


def mixture(n, d, k, seed=0):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    centres = 4.0 * torch.randn(k, d, dtype=torch.float64, device="cuda", generator=gen)
    which = torch.randint(0, k, (n,), device="cuda", generator=gen)
    return centres[which] + torch.randn(n, d, dtype=torch.float64, device="cuda", generator=gen)


prop = torch.cuda.get_device_properties(0)
say("commit {} (--label: {}) | device: {} CUs {} | torch {} hip {} (clocks are not pinned)".format(
    commit(), args.label, prop.name, prop.multi_processor_count, torch.__version__, torch.version.hip))
say("device events around alternating calls, two untimed rounds first, n={}; seedings and landmarks: wall clock around synchronised calls".format(args.reps))

for shape in [s for s in args.shapes.split(",") if s]:
    n, d, k = (int(v) for v in shape.split("x"))
    Y = mixture(n, d, k)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    C = Y[torch.randperm(n, device="cuda", generator=gen)[:k]].contiguous()
    say("--- n {} d {} k {}".format(n, d, k))
    lab_dev, _ = km.assign(Y, C)
    t = alternating({
        "library": lambda: km.library_step(Y, C),
        "device": lambda: km.lloyd_step(Y, C),
        "assign": lambda: km.assign(Y, C),
        "sort": lambda: (torch.sort(lab_dev, stable=True), torch.bincount(lab_dev, minlength=k)),
        "sort+sums": lambda: km.segment_sums(Y, lab_dev, k),
    })
    newC_lib, in_lib, lab_lib = km.library_step(Y, C)
    newC_dev, in_dev, lab_dev = km.lloyd_step(Y, C)
    flops = 2.0 * n * k * d
    say("(a) Lloyd step: library {} | device {} | device / library {:.3f}".format(fmt(t["library"]), fmt(t["device"]), t["device"][0] / t["library"][0]))
    say("    device step apart: assign {} ({:.2f} TFLOP/s of 2 n k d) | sort + counts {} | sort + counts + sums {}".format(
        fmt(t["assign"]), flops / (t["assign"][0] * 1e-3) / 1e12, fmt(t["sort"]), fmt(t["sort+sums"])))
    say("    labels that differ {} of {} | largest centre difference {:.2e} | inertia library {:.10g} device {:.10g}".format(
        int((lab_lib != lab_dev).sum()), n, float((newC_lib - newC_dev).abs().max()), float(in_lib), float(in_dev)))
    info_lib, info_dev = {}, {}
    _, t_lib = wall(lambda: _kmeans(Y, k, n_init=1, max_iter=0, seed=0, info=info_lib))
    km.kmeans_device(Y, k, n_init=1, max_iter=0, seed=1)  # (untimed: the shapes of the seeding's library calls)
    run, t_dev = wall(lambda: km.kmeans_device(Y, k, n_init=1, max_iter=0, seed=0, info=info_dev))
    say("(b) seeding + one assignment: k-means++ {:.3f} s (inertia {:.6g}) | k-means|| {:.3f} s (inertia {:.6g}, {} candidates) | "
        "device / library {:.4f}".format(t_lib, info_lib["inertia"], t_dev, info_dev["inertia"], run.get("seed_candidates"), t_dev / t_lib))
    del Y, C
    torch.cuda.empty_cache()

if args.landmarks_n > 0:
    from bench import synthetic_cells

    N, L = args.landmarks_n, args.landmarks
    X, _ = synthetic_cells(N, 50, seed=0)
    G = meld_amd.MELD(knn=5, verbose=0).fit(X).graph
    say("--- landmarks({}) on MELD(knn=5).fit(synthetic_cells({}, 50, seed 0))".format(L, N))
    G.landmarks(min(L, 64), random_state=0, kmeans="device")  # (untimed: first launches)
    from meld_amd import landmark

    info, info_lib, info_dev = {}, {}, {}
    feats, t_feat = wall(lambda: landmark.spectral_features(G, L, n_svd=100, random_state=0, info=info))
    _, t_km_lib = wall(lambda: _kmeans(feats, L, n_init=1, max_iter=landmark.KMEANS_MAX_ITER, seed=0, info=info_lib))
    _, t_km_dev = wall(lambda: km.kmeans_device(feats, L, n_init=1, max_iter=landmark.KMEANS_MAX_ITER, seed=0, info=info_dev))
    say("(c) features {} in {:.2f} s ({} passes of the range finder) | k-means on them: library {:.2f} s ({} steps, inertia {:.6g}) | device "
        "{:.2f} s ({} steps, inertia {:.6g}) | device / library {:.3f}".format(
            tuple(feats.shape), t_feat, info.get("range_finder_passes"), t_km_lib, info_lib["iterations"], info_lib["inertia"], t_km_dev,
            info_dev["iterations"], info_dev["inertia"], t_km_dev / t_km_lib))
    del feats
    lm_dev, t_dev = wall(lambda: G.landmarks(L, random_state=0, kmeans="device", recompute=True))
    lm_lib, t_lib = wall(lambda: G.landmarks(L, random_state=0, kmeans="library", recompute=True))
    say("(d) whole landmarks(): library {:.2f} s ({} Lloyd steps, {} landmarks not empty) | device {:.2f} s ({} Lloyd steps, {} not empty) | "
        "device / library {:.3f}".format(t_lib, lm_lib.info.get("kmeans_iterations"), lm_lib.n_landmark, t_dev,
                                         lm_dev.info.get("kmeans_iterations"), lm_dev.n_landmark, t_dev / t_lib))
