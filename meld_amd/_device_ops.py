"""The small device primitives the host modules share: the stream every launch goes to, the tall Gram, the exclusive scan, the radix sort of
``id << 32 | id`` keys, the reduce-by-key behind it and the CSR assembly from sorted keys; their scratch is sized and released
here."""
from __future__ import annotations

import torch

from ._lib import check, get_lib, ptr


def stream():
    """The current torch stream as the handle the library takes; the functions below launch on it."""
    return torch.cuda.current_stream().cuda_stream


def tall_gram(A, B, chunk=4096):
    """A^T B for tall-skinny A [n, r], B [n, s] (n ~ 1e6, r, s ~ 64): as a batch of chunk-row products summed at the end.
    The library GEMM runs this shape -- a 64 x 64 result with a million-long inner dimension -- on a handful of
    workgroups (54 ms at 1M x 64); split over the inner dimension it is bandwidth-bound (~1 ms)."""
    n = A.shape[0]
    nb = n // chunk
    out = torch.zeros(A.shape[1], B.shape[1], dtype=A.dtype, device=A.device)
    if nb > 0:
        out += torch.bmm(A[: nb * chunk].view(nb, chunk, -1).transpose(1, 2), B[: nb * chunk].view(nb, chunk, -1)).sum(0)
    if nb * chunk < n:
        out += A[nb * chunk :].T @ B[nb * chunk :]
    return out


def scan_i32(x):
    """The exclusive scan of the int32 device vector ``x [n]`` as int64 ``[n + 1]`` (the last entry is the total)."""
    lib, n = get_lib(), int(x.shape[0])
    if n == 0:
        return torch.zeros(1, dtype=torch.int64, device=x.device)
    out = torch.empty(n + 1, dtype=torch.int64, device=x.device)
    tb = lib.meld_scan_temp_bytes(n)
    tmp = torch.empty(tb, dtype=torch.uint8, device=x.device)
    check(lib.meld_exclusive_scan_i32_i64(ptr(x), ptr(out), n, ptr(tmp), tb, stream()), "meld_exclusive_scan_i32_i64")
    return out


def sort_pairs(keys, vals, n_ids):
    """``(keys, vals)`` sorted by key (stable); the keys are ``id << 32 | id`` with ids below ``n_ids``."""
    lib, n = get_lib(), int(keys.shape[0])
    keys2, vals2 = torch.empty_like(keys), torch.empty_like(vals)
    if n:
        tb = lib.meld_sort_temp_bytes(n)
        tmp = torch.empty(tb, dtype=torch.uint8, device=keys.device)
        end_bit = 32 + max(1, int(n_ids - 1).bit_length())
        check(lib.meld_sort_pairs_u64_f64(ptr(keys), ptr(keys2), ptr(vals), ptr(vals2), n, end_bit, ptr(tmp), tb, stream()),
              "meld_sort_pairs_u64_f64")
    return keys2, vals2


def coo_merge(keys, vals):
    """``(ukeys, uvals, n_unique)``: the values of equal neighbours of the sorted ``keys`` added in order; the first ``n_unique``
    (a host int: one read-back) entries of the outputs hold the result."""
    lib, n, dev = get_lib(), int(keys.shape[0]), keys.device
    tb = lib.meld_merge_temp_bytes(max(n, 1))
    tmp = torch.empty(tb, dtype=torch.uint8, device=dev)
    n_unique = torch.zeros(1, dtype=torch.int64, device=dev)
    ukeys, uvals = torch.empty_like(keys), torch.empty_like(vals)
    check(lib.meld_coo_merge(ptr(keys), ptr(vals), n, ptr(ukeys), ptr(uvals), ptr(n_unique), ptr(tmp), tb, stream()), "meld_coo_merge")
    return ukeys, uvals, int(n_unique.item())


def csr_from_keys(keys, nnz, row_begin, n_rows):
    """``(rowptr int64 [n_rows + 1], col int32 [nnz])`` of the rows ``[row_begin, row_begin + n_rows)`` from the first ``nnz`` sorted
    ``row << 32 | col`` keys."""
    dev = keys.device
    rowptr = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
    col = torch.empty(nnz, dtype=torch.int32, device=dev)
    check(get_lib().meld_csr_from_keys(ptr(keys), nnz, row_begin, n_rows, ptr(rowptr), ptr(col), stream()), "meld_csr_from_keys")
    return rowptr, col
