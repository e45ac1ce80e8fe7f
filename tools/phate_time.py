"""The PHATE embedding on a graph of the benchmark's cells (meld_amd/phate.py, csrc/mds.hip): its stages timed apart, and the SMACOF
step composed of library operations as a yardstick:

    python tools/phate_time.py [--n 100000] [--landmarks 2000,4096] [--dim 2] [--out FILE] [--label TEXT] [--reps 7] [--steps 32]

One process.  The graph: bench.synthetic_cells(N, 50, seed 0), MELD(knn=5, decay=40, anisotropy=0).fit.  The labels are given, not
clustered (the default clustering is timed by tools/landmark_time.py): the cells sorted by their first coordinate into sqrt(L)
strips of equal size, every strip sorted by the second coordinate into sqrt(L) runs -- L landmarks of N / L cells.  Per L:
  (a) the landmark record (merge, transpose, Gram), the singular values, the power P^t for the t the knee gives, the potential,
      the potential distances, the classical step -- wall clocks around calls that end in a synchronisation, one untimed call of
      the same shape first, median (min - max);
  (b) the SMACOF step: --steps launches of meld_smacof_step between two HIP events, against the same step composed of torch
      operations (cdist without the GEMM route, elementwise passes, a row sum, one GEMM) -- the two alternate, --reps windows each;
      the largest difference of the two after one step; then the whole run to its stopping rule;
  (c) the interpolation of the landmark coordinates to the N cells.
Clocks are not pinned; every figure is of this run."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import meld_amd
from bench import synthetic_cells
from meld_amd import phate

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100_000)
ap.add_argument("--landmarks", default="2000,4096")
ap.add_argument("--dim", type=int, default=2)
ap.add_argument("--out", default=None)
ap.add_argument("--label", default="")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--steps", type=int, default=32)
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("tools/phate_time.py measures on the GPU: none found")

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


def repeated(fn, reps=None):
    """(median, min, max) in ms of ``fn`` (synchronised wall clock), after one untimed call"""
    fn()
    t = [wall(fn)[1] * 1e3 for _ in range(reps or args.reps)]
    return statistics.median(t), min(t), max(t)


def fmt(t):
    return "median {:.3f} ms ({:.3f} - {:.3f})".format(*t)


def grid_labels(X, L):
    """L labels of equal size: strips along the first coordinate, runs along the second inside a strip"""
    n = X.shape[0]
    side = int(np.ceil(np.sqrt(L)))
    order = np.argsort(X[:, 0], kind="stable")
    lab = np.empty(n, dtype=np.int64)
    strips = np.array_split(order, side)
    per = [L // side + (1 if s < L % side else 0) for s in range(side)]
    first = 0
    for cells, k in zip(strips, per):
        inner = cells[np.argsort(X[cells, 1], kind="stable")]
        for r, run in enumerate(np.array_split(inner, k)):
            lab[run] = first + r
        first += k
    return lab


def torch_step(Dm, Z):
    """the SMACOF step of meld_smacof_step from library operations: (Z', row_stress)"""
    n = Z.shape[0]
    d = phate.distances_device(Z)  # (torch.cdist without its GEMM route, in row blocks where its grid would be refused)
    ratio = torch.where(d > 0, Dm / d, 0.0)  # (the diagonal: d = 0)
    gap = d - Dm
    row_stress = (gap * gap).sum(dim=1)
    B = -ratio
    B.diagonal().copy_(ratio.sum(dim=1))
    return (B @ Z) / n, row_stress


def step_windows(Dm, Z0):
    """ms per step of the kernel and of the yardstick: --reps windows of --steps steps each between two events, alternating"""
    n, dim = Z0.shape
    bufs = (Z0.clone(), torch.empty_like(Z0))
    rs = torch.empty(n, dtype=torch.float64, device=Z0.device)

    def kernel_window():
        for k in range(args.steps):
            phate.smacof_step_device(Dm, bufs[k & 1], bufs[(k + 1) & 1], rs)

    def torch_window():
        Z = Z0
        for _ in range(args.steps):
            Z, _ = torch_step(Dm, Z)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.steps

    kernel_window(), torch_window()  # (untimed: code objects, library plans)
    torch.cuda.synchronize()
    tk, tt = [], []
    for _ in range(args.reps):
        bufs[0].copy_(Z0)
        tk.append(timed(kernel_window))
        tt.append(timed(torch_window))
    return (statistics.median(tk), min(tk), max(tk)), (statistics.median(tt), min(tt), max(tt))


prop = torch.cuda.get_device_properties(0)
say("device: {} CUs {} HBM GiB {:.0f} | torch {} hip {} (clocks are not pinned) | {}".format(
    prop.name, prop.multi_processor_count, prop.total_memory / 2**30, torch.__version__, torch.version.hip, args.label))
X, _ = synthetic_cells(args.n, 50, seed=0)
op, t_fit = wall(lambda: meld_amd.MELD(knn=5, decay=40, anisotropy=0, verbose=0).fit(X))
G = op.graph
say("data: synthetic_cells({}, 50, seed 0); MELD(knn=5, decay=40, anisotropy=0).fit {:.2f} s, nnz {}; n_components {}; windows of {} "
    "steps, n={}".format(args.n, t_fit, G.nnz, args.dim, args.steps, args.reps))

for L in [int(v) for v in args.landmarks.split(",")]:
    lab = grid_labels(X, L)
    lm, t_lm = wall(lambda: G.landmarks(clusters=lab))
    P = lm.landmark_op_device
    n = int(P.shape[0])
    say("--- L {} ({} landmarks present): landmark record {:.1f} ms (first call)".format(L, n, t_lm * 1e3))
    t_svd = repeated(lambda: phate.singular_values(P), reps=3)
    s = phate.singular_values(P)
    h = phate.entropy_curve(s, 100)
    t = max(phate.knee(h), 1)
    t_pow = repeated(lambda: phate.power_device(P, t))
    Pt = phate.power_device(P, t)
    t_pot = repeated(lambda: phate.potential_device(Pt, 1))
    U = phate.potential_device(Pt, 1)
    t_dist = repeated(lambda: phate.distances_device(U), reps=3)
    Dm = phate.distances_device(U)
    t_cls = repeated(lambda: phate.classical_mds_device(Dm, args.dim), reps=3)
    Z0, _ = phate.classical_mds_device(Dm, args.dim)
    say("(a) singular values {} | t = {} | power {} | potential {} | distances {} | classical step {}".format(
        fmt(t_svd), t, fmt(t_pow), fmt(t_pot), fmt(t_dist), fmt(t_cls)))
    # one step both ways from Z0: the same map
    out = torch.empty_like(Z0)
    rs = torch.empty(n, dtype=torch.float64, device=Z0.device)
    phate.smacof_step_device(Dm, Z0, out, rs)
    want, want_rs = torch_step(Dm, Z0)
    say("(b) one step, kernel against library operations: Z' differs by {:.1e} at most (|Z'| up to {:.1e}), row_stress by {:.1e} "
        "relative".format(float((out - want).abs().max()), float(want.abs().max()), float(((rs - want_rs).abs() / want_rs).max())))
    tk, tt = step_windows(Dm, Z0)
    say("    per step: meld_smacof_step {} | library operations {} | kernel / library {:.3f}; D is {:.0f} MB: {:.0f} GB/s of D at the "
        "kernel's median".format(fmt(tk), fmt(tt), tk[0] / tt[0], 8e-6 * n * n, 8e-9 * n * n / (tk[0] * 1e-3)))
    run = lambda: phate.smacof_device(Dm, Z0, max_iter=3000, eps=1e-6)
    (Z, stress, iterations, log), t_run = wall(run)
    (_, _, _, _), t_run2 = wall(run)
    scale = 0.5 * float((Dm * Dm).sum())
    say("    whole run to eps = 1e-6: {} steps, {:.1f} ms ({:.1f} ms the second time; {:.3f} ms per step with the stress sums and one "
        "read-back per {} steps); normalised stress^2 {:.4f} -> {:.4f}".format(
            iterations, t_run * 1e3, t_run2 * 1e3, t_run2 * 1e3 / max(iterations, 1), phate.CHECK_EVERY, float(log[0]) / scale,
            stress / scale))
    t_int = repeated(lambda: lm.interpolate_device(Z))
    say("(c) interpolation to {} cells: {}".format(args.n, fmt(t_int)))
    total = t_svd[0] + t_pow[0] + t_pot[0] + t_dist[0] + t_cls[0] + t_run2 * 1e3 + t_int[0]
    say("    sum of the stages after the landmark record: {:.1f} ms, of which singular values {:.0f} %, SMACOF {:.0f} %".format(
        total, 100 * t_svd[0] / total, 100 * t_run2 * 1e3 / total))
    del lm, P, Pt, U, Dm, Z0, Z
    torch.cuda.empty_cache()
