"""Synthetic counts generated ON THE DEVICE for the timing tools (tools/preprocess_timing.py, tools/hvg_timing.py): no upload is timed.

A cell's depth is log-normal (sigma 0.5), a gene's popularity log-normal (sigma 1.5); a cell draws its genes by stratified sampling of
the popularity's distribution function (sorted; a gene drawn twice is kept once), the values are 1 + Poisson(0.6) in fp64."""
import torch

from meld_amd import sparse as msp

# name -> (cells, genes, entries drawn per cell of mean depth)
SHAPES = {"quickstart": (26827, 29197, 2044), "1M": (1_000_000, 30_000, 600)}


def device_counts(N, G, m, seed=0):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(seed)
    pop = torch.exp(torch.randn(G, dtype=torch.float64, device=dev, generator=gen) * 1.5)
    cdf = torch.cumsum(pop / pop.sum(), 0)
    depth = torch.exp(torch.randn(N, dtype=torch.float64, device=dev, generator=gen) * 0.5)
    want = torch.clamp((m * depth / depth.mean()).round().to(torch.int64), 1, G)
    lens = torch.empty(N, dtype=torch.int64, device=dev)
    cols, rows_per_chunk = [], max(1, (1 << 26) // m)
    for r0 in range(0, N, rows_per_chunk):
        r1 = min(N, r0 + rows_per_chunk)
        L = want[r0:r1]
        off = torch.cumsum(L, 0) - L
        total = int(L.sum())
        row = torch.repeat_interleave(torch.arange(r1 - r0, device=dev), L, output_size=total)
        j = torch.arange(total, device=dev) - off[row]
        x = (j.to(torch.float64) + torch.rand(total, dtype=torch.float64, device=dev, generator=gen)) / L[row].to(torch.float64)
        gene = torch.clamp(torch.searchsorted(cdf, x), max=G - 1).to(torch.int32)
        keep = torch.ones(total, dtype=torch.bool, device=dev)
        keep[1:] = (gene[1:] != gene[:-1]) | (row[1:] != row[:-1])
        lens[r0:r1] = torch.bincount(row[keep], minlength=r1 - r0)
        cols.append(gene[keep])
        del row, j, x, gene, keep
    col = torch.cat(cols)
    del cols
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(lens, 0)
    val = 1.0 + torch.poisson(torch.full((int(col.shape[0]),), 0.6, dtype=torch.float64, device=dev), generator=gen)
    A = msp.DeviceCSR(rowptr, col.contiguous(), val, (N, G))
    A._validate()
    return A
