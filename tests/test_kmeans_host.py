"""k-means without a device: the argument checks of ``meld_amd.KMeans`` (raised before any tensor is made), the ``kmeans=`` keyword
of ``landmarks()`` refused before the device is touched, the argument contract of the two C entries of csrc/kmeans_wide.hip (every
refusal comes before any launch), and what hipcc reports for their kernels (no private memory)."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kmeans_is_exported():
    import meld_amd
    from meld_amd.kmeans import KMeans

    assert meld_amd.KMeans is KMeans and "KMeans" in meld_amd.__all__
    km = KMeans()
    assert (km.n_clusters, km.init, km.n_init, km.max_iter, km.tol, km.random_state) == (8, "k-means||", 1, 300, 1e-4, None)


def test_kmeans_argument_checks():
    from meld_amd import KMeans

    for bad in (0, -1, 2.0, "3", True, None):
        with pytest.raises(ValueError, match="n_clusters"):
            KMeans(n_clusters=bad)
    for bad in (0, 1.5, False):
        with pytest.raises(ValueError, match="n_init"):
            KMeans(n_init=bad)
    for bad in (-1, 2.5, "10"):
        with pytest.raises(ValueError, match="max_iter"):
            KMeans(max_iter=bad)
    for bad in (-1e-3, "x", float("nan"), None):
        with pytest.raises(ValueError, match="tol"):
            KMeans(tol=bad)
    for bad in (1.5, "0", True):
        with pytest.raises(ValueError, match="random_state"):
            KMeans(random_state=bad)
    with pytest.raises(ValueError, match="init"):
        KMeans(init="random")
    with pytest.raises(ValueError, match="init"):
        KMeans(n_clusters=3, init=np.zeros((4, 2)))
    with pytest.raises(ValueError, match="init"):
        KMeans(n_clusters=3, init=np.zeros(3))
    with pytest.raises(ValueError, match="n_init"):
        KMeans(n_clusters=3, init=np.zeros((3, 2)), n_init=2)
    km = KMeans(n_clusters=3, init=np.zeros((3, 2)), max_iter=0, random_state=np.int64(4))
    assert km.n_clusters == 3 and km.max_iter == 0
    with pytest.raises(ValueError, match="two-dimensional"):
        km.fit(np.zeros(5))
    with pytest.raises(ValueError, match="must be `fit`"):
        km.predict(np.zeros((5, 2)))


def test_fit_needs_a_gpu(monkeypatch):
    import torch

    from meld_amd import KMeans

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        KMeans(2).fit(np.zeros((5, 2)))


def test_landmarks_refuses_an_unknown_kmeans_before_touching_the_device():
    from meld_amd.landmark import check_kmeans, landmarks
    from meld_amd.phate import phate

    def stub(**kw):
        return SimpleNamespace(**dict(dict(N=100, n_rows=100, comm=None, n_landmark=None), **kw))

    for bad in ("x", "Device", None, 1):
        with pytest.raises(ValueError, match="kmeans must be 'library' or 'device'"):
            landmarks(stub(), n_landmark=10, kmeans=bad)
        with pytest.raises(ValueError, match="kmeans must be 'library' or 'device'"):
            phate(stub(), n_landmark=10, kmeans=bad)
    assert check_kmeans("library") == "library" and check_kmeans("device") == "device"
    # the other refusals still come first to last as they did
    with pytest.raises(ValueError, match="less than the number of cells"):
        landmarks(stub(), n_landmark=250, kmeans="device")


def test_limits_and_argument_contract_of_the_library():
    from meld_amd import _lib
    from meld_amd.kmeans import MAX_D, MAX_K

    lib = _lib.get_lib()
    assert lib.meld_kmeans_wide_max_d() == MAX_D == 128 and lib.meld_kmeans_wide_max_k() == MAX_K == 4096
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)  # (host memory: nothing may touch it, and nothing does -- the checks come before any launch)

    def refused(name, status):
        assert status == -1, name
        assert lib.meld_last_error().decode().startswith(name + ":"), lib.meld_last_error()

    assign, sums = lib.meld_kmeans_wide_assign, lib.meld_kmeans_wide_sums
    name = "meld_kmeans_wide_assign"
    refused(name, assign(None, 4, 8, 4, a, 2, a, a, a, None))  # Y
    refused(name, assign(a, 4, 8, 4, None, 2, a, a, a, None))  # centres
    refused(name, assign(a, 4, 8, 4, a, 2, None, a, a, None))  # centre_norms
    refused(name, assign(a, 4, 8, 4, a, 2, a, None, a, None))  # labels
    refused(name, assign(a, 4, 8, 0, a, 2, a, a, a, None))
    refused(name, assign(a, 129, 8, 129, a, 2, a, a, a, None))
    refused(name, assign(a, 4, 8, 4, a, 0, a, a, a, None))
    refused(name, assign(a, 4, 8, 4, a, 4097, a, a, a, None))
    refused(name, assign(a, 3, 8, 4, a, 2, a, a, a, None))  # ldy < d
    refused(name, assign(a, 4, -1, 4, a, 2, a, a, a, None))
    refused(name, assign(a, 4, 2 ** 31, 4, a, 2, a, a, a, None))
    assert assign(None, 4, 0, 4, a, 2, a, None, None, None) == 0  # (no points: a successful no-op)
    name = "meld_kmeans_wide_sums"
    refused(name, sums(None, 4, 8, 4, a, a, 2, a, None))
    refused(name, sums(a, 4, 8, 4, None, a, 2, a, None))
    refused(name, sums(a, 4, 8, 4, a, None, 2, a, None))
    refused(name, sums(a, 4, 8, 4, a, a, 2, None, None))
    refused(name, sums(a, 4, 8, 0, a, a, 2, a, None))
    refused(name, sums(a, 129, 8, 129, a, a, 2, a, None))
    refused(name, sums(a, 4, 8, 4, a, a, 0, a, None))
    refused(name, sums(a, 3, 8, 4, a, a, 2, a, None))
    refused(name, sums(a, 4, -1, 4, a, a, 2, a, None))
    assert sums(None, 4, 0, 4, None, None, 5000, None, None) == 0  # (any k >= 1)


def test_wide_kmeans_kernels_do_not_spill():
    """The kernels of csrc/kmeans_wide.hip as hipcc compiles them with the build's flags: no private memory.  (No occupancy figure is
    asserted: none has been measured against.)"""
    from tests.test_kernel_resources import _resource_usage

    rows = _resource_usage(os.path.join(ROOT, "meld_amd", "csrc", "kmeans_wide.hip"))
    kernels = {k: v for k, v in rows.items() if "kmeans_wide_" in k and "_kernel" in k}
    # the assign kernel for padded widths 16, 32, ..., 128, the centre norms, the sums
    assert len(kernels) == 10 and sum("kmeans_wide_assign_kernel" in k for k in kernels) == 8, sorted(rows)
    for name, r in kernels.items():
        assert r["ScratchSize [bytes/lane]:"] == 0, (name, r)


@pytest.mark.parametrize("d, k, prefer, expected", [
    (32, 64, "lds", "lds"), (33, 64, "lds", "library"), (32, 65, "lds", "library"), (1, 1, "lds", "lds"),
    (128, 1, "wide", "wide"), (128, 5000, "wide", "wide"), (129, 1, "wide", "library"), (129, 5000, "wide", "library"),
])
def test_the_back_end_a_shape_takes(d, k, prefer, expected):
    from meld_amd.kmeans import pick_backend

    assert pick_backend(d, k, prefer) == expected
    with pytest.raises(ValueError, match="prefer must be"):
        pick_backend(d, k, "device")


def test_kmeans_imports_without_the_vfc_module():
    """k-means lives in ``meld_amd.kmeans`` alone: importing it, and ``meld_amd.landmark`` that calls it, does not import
    ``meld_amd.cluster`` (checked in a fresh interpreter)."""
    import subprocess
    import sys

    code = "import sys, meld_amd.kmeans, meld_amd.landmark; assert 'meld_amd.cluster' not in sys.modules, 'cluster imported'"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
