"""Diffusion of cell signals, host side (no GPU): the pure helpers of meld_amd/diffuse.py, the argument checks of
``meld_diffuse_step`` (every case of the contract in include/meld_hip.h is refused before any launch) and the estimator's
not-fitted error."""
import ctypes

import numpy as np
import pytest


def test_check_t_accepts_counts_and_names_what_it_rejects():
    from meld_amd.diffuse import check_t

    for t in (0, 1, 7, np.int32(3), np.int64(0), np.uint8(5)):
        out = check_t(t)
        assert type(out) is int and out == int(t)
    for bad in (-1, 1.5, None, "3", np.int64(-2)):
        with pytest.raises(ValueError, match=r"\bt\b"):
            check_t(bad)
    with pytest.raises(NotImplementedError, match="auto"):
        check_t("auto")


@pytest.mark.parametrize("p", [1, 64, 128, 129, 256, 257, 300])
def test_panels_cover_the_columns_once(p):
    from meld_amd.diffuse import panels

    ps = panels(p)
    assert all(1 <= w <= 128 for _, w in ps)
    at = 0
    for c0, w in ps:  # contiguous, in order
        assert c0 == at
        at += w
    assert at == p
    assert len(ps) == -(-p // 128)
    assert ps == panels(p)  # (a function of p alone)


def test_panels_of_one_launch():
    from meld_amd.diffuse import panels

    assert panels(128) == [(0, 128)]
    assert panels(129) == [(0, 128), (128, 1)]


def test_column_index():
    from meld_amd.diffuse import column_index

    out = column_index([3, 0, 3], 5)
    assert out.dtype == np.int64 and out.tolist() == [3, 0, 3]
    assert column_index(np.array([4], dtype=np.int32), 5).tolist() == [4]
    assert column_index(range(3), 5).tolist() == [0, 1, 2]
    for bad in ([-1], [5], [0, 7]):
        with pytest.raises(ValueError, match="out of range"):
            column_index(bad, 5)
    mask = np.array([True, False, True, False, False])
    out = column_index(mask, 5)
    assert out.dtype == np.int64 and out.tolist() == [0, 2]
    with pytest.raises(ValueError, match="mask"):
        column_index(mask[:4], 5)
    names = ["a", "b", "c", "d", "e"]
    out = column_index(["d", "a"], 5, names)
    assert out.dtype == np.int64 and out.tolist() == [3, 0]
    assert column_index("b", 5, names).tolist() == [1]
    with pytest.raises(ValueError, match="name"):
        column_index(["a"], 5)  # (the graph kept no names)
    with pytest.raises(ValueError, match="zz"):
        column_index(["a", "zz"], 5, names)


def test_step_entry_rejects_its_contract_before_any_launch():
    """Every pointer is a plausible host address: nothing may touch it.  Each case returns -1 and names the entry."""
    from meld_amd import _lib

    lib = _lib.get_lib()
    assert lib.meld_diffuse_max_cols() == 128
    buf = (ctypes.c_double * 4096)()
    a = ctypes.addressof(buf)
    x, y = a, a + 8 * 2048  # 4 rows of ld 8: [x, x + 32), [y, y + 32) doubles apart
    good = dict(rowptr=a, col=a, val=a, kd=a, s=a, n_rows=4, x=x, ldx=8, y=y, ldy=8, p=8)
    order = ("rowptr", "col", "val", "kd", "s", "n_rows", "x", "ldx", "y", "ldy", "p")
    cases = {name + " NULL": {name: None} for name in ("rowptr", "col", "val", "kd", "s", "x", "y")}
    cases.update({
        "p = 0": dict(p=0),
        "p = 129": dict(p=129, ldx=256, ldy=256),
        "ldx < p": dict(ldx=7),
        "ldy < p": dict(ldy=7),
        "n_rows < 0": dict(n_rows=-1),
        "y == x": dict(y=x),
        "y inside x's range": dict(y=x + 8 * 16),
        "x inside y's range": dict(x=y + 8 * 31),
    })
    for what, change in cases.items():
        args = dict(good, **change)
        lib.meld_scale_f64(None, 1.0, None, 10, None)  # (leaves another entry's message behind)
        assert lib.meld_diffuse_step(*[args[k] for k in order], None) == -1, what
        assert lib.meld_last_error().decode().startswith("meld_diffuse_step:"), (what, lib.meld_last_error())
    # no rows: a successful no-op, whatever col and val are
    assert lib.meld_diffuse_step(a, None, None, a, a, 0, x, 8, y, 8, 8, None) == 0


def test_max_cols_is_the_panel_width():
    from meld_amd import _lib, diffuse

    assert _lib.get_lib().meld_diffuse_max_cols() == 128 == diffuse.MAX_COLS


def test_impute_before_fit():
    import meld_amd

    with pytest.raises(ValueError, match="fit"):
        meld_amd.MELD().impute()
