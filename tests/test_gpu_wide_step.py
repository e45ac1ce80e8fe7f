"""The wide recurrence step (``meld_cheby_step_wide``, ``cheby_step_wide_kernel`` of csrc/spmm.hip: the NC = 1 pass of
csrc/csr_wave_stream.hpp) against scipy on small graphs, element by element:

    y = alpha (dw .* x - W x) + beta x + gamma z

Tolerance, derived.  Row ``i`` with ``m_i`` entries: the kernel's sum of ``m_i`` products carries at most ``m_i`` roundings, the
epilogue (the product with ``dw``, the difference, three scalings, two sums) at most five more, each relative to a partial result
that ``|alpha| (dw_i + sum_e |w_e|) max|x| + |beta| max|x| + |gamma| max|z|`` bounds; scipy's own evaluation commits as much:

    |err_i| <= 2 (m_i + 5) 2^-53 ( |alpha| (dw_i + sum_e |w_e|) max|x| + |beta| max|x| + |gamma| max|z| )

``m_i`` is read from ``rowptr``.  Geometry: 8 consecutive rows per wave and 32 per workgroup, 16 entries per chunk, lanes = columns:
N in {1, 31, 32, 33, 257} straddles the row boundaries, the star's hub is one row of 4 096 entries (256 chunks) beside rows of one,
p in {1, 41, 63, 64} the lanes."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import sparse

from tests.test_gpu_diffuse import _MAKERS

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
P_MAX = 64
ALPHA, BETA = 0.7, -0.2
_CACHE = {}


def _case(kind, n):
    """One graph on the device, its host copy and seeded operands of P_MAX columns (shared by the tests, never changed)."""
    key = (kind, n)
    if key not in _CACHE:
        from meld_amd.graph import DeviceGraph

        G = DeviceGraph.from_scipy(_MAKERS[kind](n))
        assert G.perm is None
        W = sparse.csr_matrix((G.val.cpu().numpy(), G.col.cpu().numpy(), G.rowptr.cpu().numpy()), shape=(n, n))
        rng = np.random.default_rng(13 * n + len(kind))
        _CACHE[key] = dict(G=G, W=W, dw=G.dw_dev.cpu().numpy()[:n], x=rng.standard_normal((n, P_MAX)), z=rng.standard_normal((n, P_MAX)))
    return _CACHE[key]


def _step(G, r0, p, x_full, z, y, gamma):
    """The step on the rows ``[r0, N)`` of ``G`` as a row shard holds them: the record's row pointers and degrees start at row
    ``r0`` (entry offsets stay absolute, so ``col`` and ``val`` are whole), ``z`` and ``y`` are local, ``x_full`` is not."""
    from meld_amd import _lib

    col, val = G.col, G.val
    if G.nnz == 0:  # (the entry wants addresses; none is read)
        col, val = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
    rec = _lib.Laplacian(G.rowptr.data_ptr() + 8 * r0, col.data_ptr(), val.data_ptr(), G.dw_dev.data_ptr() + 8 * r0, G.N - r0, G.nnz, None)
    _lib.check(_lib.get_lib().meld_cheby_step_wide(ctypes.byref(rec), p, _lib.ptr(x_full), r0, _lib.ptr(z), _lib.ptr(y), ALPHA, BETA, gamma,
                                                   torch.cuda.current_stream().cuda_stream), "meld_cheby_step_wide")
    torch.cuda.synchronize()


def _check(c, p, gamma, r0=0):
    n = c["x"].shape[0]
    x, z = np.ascontiguousarray(c["x"][:, :p]), np.ascontiguousarray(c["z"][r0:, :p])
    y = torch.from_numpy(z).cuda()  # y aliases z: every element is read before it is written
    _step(c["G"], r0, p, torch.from_numpy(x).cuda(), y if gamma != 0.0 else None, y, gamma)
    W, dw = c["W"][r0:], c["dw"][r0:]
    ref = ALPHA * (dw[:, None] * x[r0:] - W @ x) + BETA * x[r0:] + gamma * z
    m = np.diff(W.indptr)
    wabs = np.ravel(abs(W).sum(1))
    xmax, zmax = float(np.abs(x).max()), float(np.abs(z).max())
    bound = 2 * (m + 5) * U * (abs(ALPHA) * (dw + wabs) * xmax + abs(BETA) * xmax + abs(gamma) * zmax)
    err = np.abs(y.cpu().numpy() - ref)
    print("N={} r0={} p={} gamma={}: max |device - host| = {:.3e}, largest bound {:.3e}, worst err / bound {:.3f}".format(
        n, r0, p, gamma, float(err.max()), float(bound.max()), float((err / bound[:, None]).max())))
    assert tuple(err.shape) == (n - r0, p) and bool((err <= bound[:, None]).all())


@pytest.mark.parametrize("gamma", [0.0, -1.0])
@pytest.mark.parametrize("p", [1, 41, 63, 64])
@pytest.mark.parametrize("kind,n", [(k, n) for k in ("path", "random") for n in (1, 31, 32, 33, 257)] + [("star", 4097)])
def test_step_against_scipy(kind, n, p, gamma):
    c = _case(kind, n)
    if kind == "star":
        m = np.diff(c["W"].indptr)
        assert int(m.max()) == n - 1 and int(m.min()) == 1
    _check(c, p, gamma)


@pytest.mark.parametrize("gamma", [0.0, -1.0])
@pytest.mark.parametrize("kind,n,r0", [("random", 257, 100), ("star", 4097, 1001)])
def test_trailing_rows_with_a_row_offset(kind, n, r0, gamma):
    """The gathers index ``x_full`` from row 0, the rows' own x from ``x_row_offset``: the rows ``[r0, N)`` alone.  ``r0`` is no
    multiple of 8, so the waves' row groups differ from the whole graph's; the star's hub (row 1365) is inside the slice."""
    _check(_case(kind, n), 41, gamma, r0=r0)
