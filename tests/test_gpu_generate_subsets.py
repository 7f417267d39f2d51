"""SudokuEngine.generate_subsets / generate_subsets_dev (sdk_generate_subsets): graded generation with
the subsets stage and the open4 range in the selection, against the same selection done by hand --
generate_batch over the window, subsets_batch of those rows, a numpy filter -- byte for byte, and against
generate_graded where the range filters nothing.  The window is seed 7, rows 1000..3047: about 7 % of
the stream's puzzles are level-4 boards that subsets close (tests/test_subsets_model.py), so 64 of them
lie within about a thousand rows, and 300 rows hold about twenty."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

from distributed_sudoku_solver_amd import _lib as L

pytestmark = pytest.mark.gpu

SEED, FIRST, ROWS = 7, 1000, 2048
N = 64
MASK_ALL = 0x1E

Window = namedtuple("Window", "puzzles grids status level open open4")


@pytest.fixture(scope="module")
def window(engine):
    """The window's candidates and their grades, by the batch calls (computed once)."""
    puz, grids, gst = engine.generate_batch(ROWS, seed=SEED, lo=FIRST)
    st, level, open_, open4, out = engine.subsets_batch(puz, budget=0)
    assert (gst == 1).all() and np.array_equal(out, grids)
    return Window(puz, grids, gst, level, open_, open4)


def by_hand(w, n, levels, rng, max_scan=ROWS):
    """(rows, found, scanned) of the call's contract on the window."""
    lo, hi = rng
    hit = (w.status == 1) & np.isin(w.level, levels)
    hit &= (w.level != 4) | ((w.open4 >= lo) & (w.open4 <= hi))
    where = np.flatnonzero(hit[:max_scan])
    found = min(n, len(where))
    k = where[:found]
    return k, found, (int(k[-1]) + 1 if found == n else max_scan)


def subsets(engine, n, levels, open4, **kw):
    kw.setdefault("max_scan", ROWS)
    return engine.generate_subsets(n, levels, seed=SEED, lo=FIRST, open4=open4, **kw)


def equals_by_hand(res, w, n, levels, rng, max_scan=ROWS):
    puz, sol, level, open_, o4, index, scanned = res
    k, found, ref_scanned = by_hand(w, n, levels, rng, max_scan)
    print("levels", levels, "open4", rng, "found", len(puz), "by hand", found, "scanned", scanned, "by hand", ref_scanned)
    assert len(puz) == len(sol) == len(level) == len(open_) == len(o4) == len(index) == found
    assert scanned == ref_scanned
    assert index.dtype == np.uint64 and np.array_equal(index, (k + FIRST).astype(np.uint64))
    assert np.array_equal(level, w.level[k]) and np.array_equal(open_, w.open[k])
    assert o4.dtype == np.uint8 and np.array_equal(o4, w.open4[k])
    assert np.array_equal(puz, w.puzzles[k]) and np.array_equal(sol, w.grids[k])
    return found


@pytest.mark.parametrize("levels,rng", [((4,), (0, 0)), ((4,), (1, 64)), ((1, 2, 3, 4), (0, 0)), ((1, 2, 3, 4), (20, 40))],
                         ids=["level4-closed", "level4-open", "all-closed", "all-20-40"])
def test_ranges_and_masks(engine, window, levels, rng):
    res = subsets(engine, N, levels, rng)
    assert equals_by_hand(res, window, N, levels, rng) == N
    lv, o4 = res[2], res[4]
    assert ((o4[lv == 4] >= rng[0]) & (o4[lv == 4] <= rng[1])).all()
    assert (o4[lv != 4] == L.SDK_SUBSETS_NONE).all()


def test_level_mask_without_level4_skips_the_stage(engine, window):
    res = subsets(engine, N, (2, 3), (0, 0))
    assert equals_by_hand(res, window, N, (2, 3), (0, 0)) == N
    assert (res[4] == L.SDK_SUBSETS_NONE).all()


def test_window_ends_early(engine, window):
    """found < n, and the rows past `found` are not written."""
    k, found, _ = by_hand(window, N, (4,), (0, 0), max_scan=300)
    assert 1 <= found < N
    res = subsets(engine, N, (4,), (0, 0), max_scan=300)
    assert equals_by_hand(res, window, N, (4,), (0, 0), max_scan=300) == found and res[6] == 300
    puz, grid = np.full((N, 81), 0xAB, dtype=np.uint8), np.full((N, 81), 0xCD, dtype=np.uint8)
    lv, op, o4 = (np.full(N, 0xEE, dtype=np.uint8) for _ in range(3))
    index = np.full(N, 12345, dtype=np.uint64)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    f, s = ctypes.c_uint64(), ctypes.c_uint64()
    rc = engine.lib.sdk_generate_subsets(engine.ctx, SEED, FIRST, N, 1 << 4, 0, 81, 0, 0, 300, 0, p(puz), p(grid), p(lv),
                                         p(op), p(o4), p(index), ctypes.byref(f), ctypes.byref(s))
    assert rc == L.SDK_OK and f.value == found and s.value == 300
    assert np.array_equal(puz[:found], window.puzzles[k]) and (o4[:found] == 0).all()
    assert (puz[found:] == 0xAB).all() and (grid[found:] == 0xCD).all() and (index[found:] == 12345).all()
    assert (lv[found:] == 0xEE).all() and (op[found:] == 0xEE).all() and (o4[found:] == 0xEE).all()


def test_chunk_independence(engine, window):
    auto = subsets(engine, N, (3, 4), (0, 30), chunk=0)
    assert equals_by_hand(auto, window, N, (3, 4), (0, 30)) == N
    got = subsets(engine, N, (3, 4), (0, 30), chunk=64)
    for x, y in zip(got[:6], auto[:6]):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert got[6] == auto[6]


def test_full_range_is_graded_generation(engine):
    for levels in ((1, 2, 3, 4), (4,), (2,)):
        r = subsets(engine, 100, levels, (0, 64))
        g = engine.generate_graded(100, levels, seed=SEED, lo=FIRST, max_scan=ROWS)
        for x, y in zip(r[:4] + r[5:], g):
            assert np.array_equal(x, y)


def test_device_form(engine):
    n = 40
    host = subsets(engine, n, (3, 4), (0, 25))
    assert len(host[0]) == n
    bufs = [engine.alloc(n * 81 + 16), engine.alloc(n * 81)] + [engine.alloc(n) for _ in range(3)] + [engine.alloc(n * 8)]
    d_puz, d_grid, d_level, d_open, d_o4, d_index = bufs
    u8 = lambda d: d.download(np.empty(n, dtype=np.uint8))
    try:
        got = engine.generate_subsets_dev(d_puz, d_grid, n, (3, 4), seed=SEED, lo=FIRST, open4=(0, 25), max_scan=ROWS,
                                          d_level=d_level, d_open=d_open, d_open4=d_o4, d_index=d_index)
        engine.synchronize()
        assert got == (n, host[6])
        assert np.array_equal(d_puz.download(np.empty((n, 81), dtype=np.uint8)), host[0])
        assert np.array_equal(d_grid.download(np.empty((n, 81), dtype=np.uint8)), host[1])
        for d, ref in zip((d_level, d_open, d_o4), host[2:5]):
            assert np.array_equal(u8(d), ref)
        assert np.array_equal(d_index.download(np.empty(n, dtype=np.uint64)), host[5])
        # the nullable outputs left out
        found = ctypes.c_uint64()
        assert engine.lib.sdk_generate_subsets_dev(engine.ctx, SEED, FIRST, n, (1 << 3) | (1 << 4), 0, 81, 0, 25, ROWS, 0,
                                                   d_puz.ptr, d_grid.ptr, None, None, None, None,
                                                   ctypes.byref(found), None) == L.SDK_OK
        engine.synchronize()
        assert found.value == n
        assert np.array_equal(d_puz.download(np.empty((n, 81), dtype=np.uint8)), host[0])
    finally:
        for b in bufs:
            b.free()


def test_argument_errors(engine):
    n = 4
    puz, grid = np.zeros((n, 81), dtype=np.uint8), np.zeros((n, 81), dtype=np.uint8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    found = ctypes.c_uint64(12345)
    for lo, hi in ((6, 5), (0, 65), (65, 65)):
        rc = engine.lib.sdk_generate_subsets(engine.ctx, SEED, FIRST, n, MASK_ALL, 0, 81, lo, hi, ROWS, 0, p(puz),
                                             p(grid), None, None, None, None, ctypes.byref(found), None)
        assert rc == L.SDK_EINVAL and b"open4" in engine.lib.sdk_last_error()
        assert found.value == 12345 and not puz.any()
    rc = engine.lib.sdk_generate_subsets(engine.ctx, SEED, FIRST, n, MASK_ALL, 0, 81, 0, 64, ROWS, 0, p(puz), p(grid),
                                         None, None, None, None, ctypes.byref(found), None)
    assert rc == L.SDK_OK and found.value == n
    for bad in ((6, 5), (0, 65), (-1, 3)):
        with pytest.raises(ValueError):
            engine.generate_subsets(4, open4=bad)
    e = engine.generate_subsets(0)
    assert len(e) == 7 and e[0].shape == (0, 81) and e[6] == 0
