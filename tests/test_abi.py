"""The C-ABI library builds, loads and exports every symbol include/meld_hip.h declares
(no compute calls: this runs without a GPU)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "meld_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(meld_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from meld_amd import _lib, build

    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), "libmeld_hip.so does not export {}".format(s)
    assert sorted(_lib.SIGNATURES) == syms, set(_lib.SIGNATURES) ^ set(syms)


def test_geometry_queries_and_argument_checks():
    from meld_amd import _lib

    lib = _lib.get_lib()
    assert lib.meld_abi_version() == 1
    assert lib.meld_knn_padded_dim(50) == 52
    assert lib.meld_knn_padded_dim(100) == 104
    assert lib.meld_knn_padded_dim(2) == 8
    assert lib.meld_knn_padded_dim(127) < 0
    assert b"d=127" in lib.meld_last_error()
    assert lib.meld_knn_row_capacity(64) == 128
    assert lib.meld_knn_row_capacity(129) < 0
    assert lib.meld_knn_tile_refs() == 64 and lib.meld_knn_block_queries() == 128
    # null pointers are rejected before any launch
    assert lib.meld_scale_f64(None, 1.0, None, 10, None) == -1
    assert lib.meld_cheby_step(None, 2, None, 0, None, None, None, 1.0, 0.0, 0.0, 0.0, None, None) == -1


def test_recurrence_entries_check_their_operator_record():
    """Each of the six entries that take a ``meld_laplacian_t`` returns -1, naming itself, before any launch: for a NULL
    record, a record without row pointers, and a record that selects the CSR-stream kernel (``layout == NULL``) without
    columns.  Every other argument is a plausible non-null address (host memory: nothing may touch it)."""
    from meld_amd import _lib

    lib = _lib.get_lib()
    buf = (ctypes.c_double * 1024)()
    a = ctypes.addressof(buf)
    no_rowptr = _lib.Laplacian(None, a, a, a, 4, 8, None)
    no_col = _lib.Laplacian(a, None, a, a, 4, 8, None)
    calls = {
        "meld_cheby_step": lambda L: lib.meld_cheby_step(L, 1, a, 0, a, a, a, 1.0, 0.0, -1.0, 0.5, None, None),
        "meld_cheby_step_wide": lambda L: lib.meld_cheby_step_wide(L, 8, a, 0, a, a, 1.0, 0.0, -1.0, None),
        "meld_cheby_run": lambda L: lib.meld_cheby_run(None, L, 4, 0, 1, a, a, a, a, 4, 1.0, 0.0, None, None),
        "meld_lanczos_steps": lambda L: lib.meld_lanczos_steps(L, a, a, a, a, a, a, 0, 1, a, None, None),
        "meld_lanczos_spmv": lambda L: lib.meld_lanczos_spmv(L, a, 0, a, a, a, a, None),
        # (a non-null communicator that is never dereferenced: the record is checked first)
        "meld_lanczos_steps_sharded": lambda L: lib.meld_lanczos_steps_sharded(a, L, 4, 0, a, a, a, a, a, a, a, 0, 1, None),
    }
    for name, call in calls.items():
        for what, rec in (("NULL record", None), ("rowptr NULL", ctypes.byref(no_rowptr)), ("col NULL, no layout", ctypes.byref(no_col))):
            lib.meld_scale_f64(None, 1.0, None, 10, None)  # (leaves another entry's message behind)
            assert call(rec) == -1, (name, what)
            assert lib.meld_last_error().decode().startswith(name + ":"), (name, what, lib.meld_last_error())
    # the boundary has one entry per operation and no development hooks
    for gone in ("meld_pt_debug_ablate", "meld_pt_debug_stamps", "meld_pt_cheby_step", "meld_pt_cheby_run", "meld_pt_lanczos_steps",
                 "meld_pt_lanczos_spmv", "meld_cheby_run_sharded"):
        assert not hasattr(lib, gone), gone


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under meld_amd/ may import or execute it."""
    bad = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "meld_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                if re.search(r"^\s*(from|import)\s+oracle\b|meld_oracle|/root/reference", txt, flags=re.M):
                    bad.append(os.path.join(dirpath, f))
    assert not bad, bad


def test_split_layout_geometry_is_a_function_of_the_dimension():
    """No compute, no GPU: which dimensions get the split operand layout (13 coordinates and their norm pieces in K block 0, see
    include/meld_hip.h) -- wherever d > 13 and d + 6 K slots fit the K blocks d + 3 needs; a function of d alone."""
    from meld_amd._lib import get_lib

    lib = get_lib()
    want = {1: 0, 13: 0, 14: 13, 26: 13, 27: 0, 29: 0, 30: 13, 42: 13, 43: 0, 45: 0, 46: 13, 50: 13, 58: 13, 59: 0, 61: 0, 62: 13, 141: 0}
    for d, lead in want.items():
        kb = lib.meld_knn16_kblocks(d)
        assert kb == (d + 3 + 15) // 16
        assert lib.meld_knn16_split_dims(d) == lead, d
        assert (lead == 13) == (d > 13 and d + 6 <= 16 * kb)
    assert lib.meld_knn16_split_dims(500) == 0  # (no kernel for that many K blocks)
    assert lib.meld_knn16_split_dims(50) == 13
    assert not hasattr(lib, "meld_knn16_debug_split")  # (round 5's process-wide layout switch is gone from the boundary)
    assert lib.meld_frame_max_dims() == 64
