"""Time the sparse front end (meld_amd/sparse.py, csrc/csr_dense.hip) on the GPU.

    python tools/time_sparse_input.py --n 26827 --g 29197 --per-row 2044 [--dense-col] [--dense-row] [--fit] [--sklearn]

The CSR matrix is built ON THE DEVICE from a seed (no host generation at 1M cells): every row holds --per-row columns, one
drawn uniformly inside each of --per-row equal strata of the genes (distinct and ascending by construction), fp32 counts.
--dense-col puts gene 0 in every cell (one row of N entries in the transpose); --dense-row gives cell 0 every gene.
Reports, as JSON lines: the transpose, X Q and X^T Y at r = k + 10 from HIP events after warm-up, with the gathered operand
bytes (nnz * r * 8) over time; with --fit the split of MELD.fit into upload, transpose, SVD, graph and filter; with
--sklearn sklearn's TruncatedSVD on the same matrix (host, --threads threads)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from meld_amd import sparse as msp


def device_matrix(N, G, m, seed, dense_col, dense_row):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(seed)
    m = min(m, G)
    lens = torch.full((N,), m, dtype=torch.int64, device=dev)
    if dense_row:
        lens[0] = G
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(lens, 0)
    nnz = int(rowptr[-1])
    col = torch.empty(nnz, dtype=torch.int32, device=dev)
    lo = torch.div(torch.arange(m, device=dev, dtype=torch.int64) * G, m, rounding_mode="floor")
    hi = torch.div((torch.arange(m, device=dev, dtype=torch.int64) + 1) * G, m, rounding_mode="floor")
    width = (hi - lo).to(torch.float64)
    rows_per_chunk = max(1, (1 << 27) // m)
    first = 1 if dense_row else 0
    for r0 in range(first, N, rows_per_chunk):
        r1 = min(N, r0 + rows_per_chunk)
        u = torch.rand(r1 - r0, m, dtype=torch.float64, device=dev, generator=gen)
        c = lo + torch.floor(u * width).to(torch.int64)
        if dense_col:
            c[:, 0] = 0
        b = int(rowptr[r0])
        col[b:b + (r1 - r0) * m] = c.flatten().to(torch.int32)
    if dense_row:
        col[:G] = torch.arange(G, dtype=torch.int32, device=dev)
    val = (torch.randint(1, 6, (nnz,), device=dev, generator=gen)).to(torch.float32)
    return msp.DeviceCSR(rowptr, col, val, (N, G))


def events_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return float(np.median(t)), float(min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=26827)
    ap.add_argument("--g", type=int, default=29197)
    ap.add_argument("--per-row", type=int, default=2044)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dense-col", action="store_true")
    ap.add_argument("--dense-row", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    A = device_matrix(a.n, a.g, a.per_row, a.seed, a.dense_col, a.dense_row)
    A._validate()
    shape = dict(N=a.n, G=a.g, nnz=A.nnz, density=A.nnz / (a.n * a.g), dense_col=a.dense_col, dense_row=a.dense_row)
    r = a.k + 10

    def transpose():
        A._T = None
        return A.T

    t_tr, t_tr_min = events_ms(transpose, a.reps)
    AT = A.T
    gen = torch.Generator(device="cuda").manual_seed(1)
    Q = torch.randn(a.g, r, dtype=torch.float64, device="cuda", generator=gen)
    Yn = torch.randn(a.n, r, dtype=torch.float64, device="cuda", generator=gen)
    Yout = torch.empty(a.n, r, dtype=torch.float64, device="cuda")
    Zout = torch.empty(a.g, r, dtype=torch.float64, device="cuda")
    A.plan(), AT.plan()
    t_f, t_f_min = events_ms(lambda: A.matmul(Q, out=Yout), a.reps)
    t_t, t_t_min = events_ms(lambda: AT.matmul(Yn, out=Zout), a.reps)
    gathered = A.nnz * r * 8
    emit(dict(shape, r=r, transpose_ms=t_tr, XQ_ms=t_f, XQ_min_ms=t_f_min, XQ_TBps=gathered / (t_f_min * 1e-3) / 1e12,
              XtY_ms=t_t, XtY_min_ms=t_t_min, XtY_TBps=gathered / (t_t_min * 1e-3) / 1e12,
              operand_MB=dict(XQ=a.g * r * 8 / 1e6, XtY=a.n * r * 8 / 1e6)))

    def svd():
        return msp.truncated_svd_project(A, a.k, seed=42)

    t_svd, _ = events_ms(svd, max(1, a.reps // 2))
    emit(dict(shape, k=a.k, truncated_svd_ms=t_svd, transpose_cached=True))

    if a.fit:
        import meld_amd

        stages = {}
        T = torch.sparse_csr_tensor(A.rowptr, A.col.to(torch.int64), A.val, size=(a.n, a.g))
        labels = np.where(np.arange(a.n) % 3 == 0, "treat", "ctrl")
        for rep in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            B = msp.DeviceCSR.from_input(T)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            B.T
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            Y = msp.truncated_svd_project(B, a.k, seed=42)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            op = meld_amd.MELD(n_pca=None, knn=5)
            op.fit(Y)
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            op.transform(labels)
            torch.cuda.synchronize()
            t5 = time.perf_counter()
            del B
            stages = dict(upload_s=t1 - t0, transpose_s=t2 - t1, svd_s=t3 - t2, graph_s=t4 - t3, filter_s=t5 - t4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        meld_amd.MELD(knn=5, n_pca=a.k).fit(T)
        torch.cuda.synchronize()
        emit(dict(shape, k=a.k, fit_split=stages, fit_end_to_end_s=time.perf_counter() - t0,
                  note="upload = validation and plan of a device torch.sparse_csr tensor (no PCIe)"))

    if a.sklearn:
        from scipy import sparse

        from sklearn.decomposition import TruncatedSVD

        Xh = sparse.csr_matrix((A.val.cpu().numpy(), A.col.cpu().numpy(), A.rowptr.cpu().numpy()), shape=(a.n, a.g))
        try:
            from threadpoolctl import threadpool_limits
        except ImportError:  # pragma: no cover
            threadpool_limits = None
        if threadpool_limits is not None:
            threadpool_limits(a.threads)
        t0 = time.perf_counter()
        TruncatedSVD(n_components=a.k, random_state=42).fit_transform(Xh)
        dt = time.perf_counter() - t0
        emit(dict(shape, k=a.k, sklearn_truncated_svd_s=dt, threads=a.threads))


if __name__ == "__main__":
    main()
