"""SudokuEngine.generate_fish / generate_fish_dev (sdk_generate_fish): graded generation with the fish stage
and the open4 and open5 ranges in the selection, against the same selection done by hand -- generate_batch
over the window, fish_batch of those rows, a numpy filter -- byte for byte, and against generate_graded
where the ranges filter nothing.  The window is seed 7, rows 1000..3047, as in
test_gpu_generate_subsets.py: three of its puzzles need a fish and close with one (stream rows 2394, 2457,
2765; tests/test_fish_model.py has the rate), so those requests use small quotas."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

from distributed_sudoku_solver_amd import _lib as L

pytestmark = pytest.mark.gpu

SEED, FIRST, ROWS = 7, 1000, 2048
N = 64
MASK_ALL = 0x1E
ANY = (0, 64)
NEED_FISH = dict(levels=(4,), open4=(1, 64), open5=(0, 0))

Window = namedtuple("Window", "puzzles grids status level open open4 open5")


@pytest.fixture(scope="module")
def window(engine):
    """The window's candidates and their grades, by the batch calls (computed once)."""
    puz, grids, gst = engine.generate_batch(ROWS, seed=SEED, lo=FIRST)
    st, level, open_, open4, open5, out = engine.fish_batch(puz, budget=0)
    assert (gst == 1).all() and np.array_equal(out, grids)
    return Window(puz, grids, gst, level, open_, open4, open5)


def by_hand(w, n, levels, r4, r5, max_scan=ROWS):
    """(rows, found, scanned) of the call's contract on the window."""
    hit = (w.status == 1) & np.isin(w.level, levels)
    hit &= (w.level != 4) | ((w.open4 >= r4[0]) & (w.open4 <= r4[1]) & (w.open5 >= r5[0]) & (w.open5 <= r5[1]))
    where = np.flatnonzero(hit[:max_scan])
    found = min(n, len(where))
    k = where[:found]
    return k, found, (int(k[-1]) + 1 if found == n else max_scan)


def fish(engine, n, levels, open4, open5, **kw):
    kw.setdefault("max_scan", ROWS)
    return engine.generate_fish(n, levels, seed=SEED, lo=FIRST, open4=open4, open5=open5, **kw)


def equals_by_hand(res, w, n, levels, r4, r5, max_scan=ROWS):
    puz, sol, level, open_, o4, o5, index, scanned = res
    k, found, ref_scanned = by_hand(w, n, levels, r4, r5, max_scan)
    print("levels", levels, "open4", r4, "open5", r5, "found", len(puz), "by hand", found, "scanned", scanned,
          "by hand", ref_scanned)
    assert len(puz) == len(sol) == len(level) == len(open_) == len(o4) == len(o5) == len(index) == found
    assert scanned == ref_scanned
    assert index.dtype == np.uint64 and np.array_equal(index, (k + FIRST).astype(np.uint64))
    assert np.array_equal(level, w.level[k]) and np.array_equal(open_, w.open[k])
    assert o4.dtype == np.uint8 and np.array_equal(o4, w.open4[k])
    assert o5.dtype == np.uint8 and np.array_equal(o5, w.open5[k])
    assert np.array_equal(puz, w.puzzles[k]) and np.array_equal(sol, w.grids[k])
    return found


def test_puzzles_that_need_a_fish(engine, window):
    """n = 3: stream rows 2394, 2457, 2765, found at the 1766th row of the window."""
    res = fish(engine, 3, **NEED_FISH)
    assert equals_by_hand(res, window, 3, (4,), (1, 64), (0, 0)) == 3
    puz, sol, level, open_, o4, o5, index, scanned = res
    assert index.tolist() == [2394, 2457, 2765] and scanned == 1766
    assert (level == 4).all() and (o4 > 0).all() and (o5 == 0).all()


def test_window_holds_only_three(engine, window):
    """n = 8: found == 3, scanned == max_scan, and nothing is written past row 3."""
    res = fish(engine, 8, **NEED_FISH)
    assert equals_by_hand(res, window, 8, (4,), (1, 64), (0, 0)) == 3 and res[7] == ROWS
    n = 8
    puz, grid = np.full((n, 81), 0xAB, dtype=np.uint8), np.full((n, 81), 0xCD, dtype=np.uint8)
    lv, op, o4, o5 = (np.full(n, 0xEE, dtype=np.uint8) for _ in range(4))
    index = np.full(n, 12345, dtype=np.uint64)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    f, s = ctypes.c_uint64(), ctypes.c_uint64()
    rc = engine.lib.sdk_generate_fish(engine.ctx, SEED, FIRST, n, 1 << 4, 0, 81, 1, 64, 0, 0, ROWS, 0, p(puz), p(grid),
                                      p(lv), p(op), p(o4), p(o5), p(index), ctypes.byref(f), ctypes.byref(s))
    assert rc == L.SDK_OK and f.value == 3 and s.value == ROWS
    assert np.array_equal(puz[:3], res[0]) and (o5[:3] == 0).all() and np.array_equal(o4[:3], res[4])
    assert (puz[3:] == 0xAB).all() and (grid[3:] == 0xCD).all() and (index[3:] == 12345).all()
    for col in (lv, op, o4, o5):
        assert (col[3:] == 0xEE).all()


@pytest.mark.parametrize("levels,r4,r5", [((4,), ANY, (0, 0)), ((4,), ANY, (1, 64)), ((1, 2, 3, 4), ANY, (20, 40)),
                                          ((1, 2, 3, 4), (20, 40), (20, 40))],
                         ids=["level4-closed", "level4-open", "all-20-40", "all-both-20-40"])
def test_ranges_and_masks(engine, window, levels, r4, r5):
    res = fish(engine, N, levels, r4, r5)
    assert equals_by_hand(res, window, N, levels, r4, r5) == N
    lv, o4, o5 = res[2], res[4], res[5]
    assert ((o5[lv == 4] >= r5[0]) & (o5[lv == 4] <= r5[1])).all()
    assert ((o4[lv == 4] >= r4[0]) & (o4[lv == 4] <= r4[1])).all()
    assert (o5[lv != 4] == L.SDK_FISH_NONE).all() and (o4[lv != 4] == L.SDK_SUBSETS_NONE).all()


def test_level_mask_without_level4_skips_the_stage(engine, window):
    res = fish(engine, N, (2, 3), (1, 64), (0, 0))
    assert equals_by_hand(res, window, N, (2, 3), (1, 64), (0, 0)) == N
    assert (res[4] == 0xFF).all() and (res[5] == 0xFF).all()


def test_full_ranges_are_graded_generation(engine):
    for levels in ((1, 2, 3, 4), (4,), (2,)):
        r = fish(engine, 100, levels, ANY, ANY)
        g = engine.generate_graded(100, levels, seed=SEED, lo=FIRST, max_scan=ROWS)
        for x, y in zip(r[:4] + r[6:], g):
            assert np.array_equal(x, y)


def test_chunk_independence(engine, window):
    auto = fish(engine, N, (3, 4), (0, 30), (0, 25), chunk=0)
    assert equals_by_hand(auto, window, N, (3, 4), (0, 30), (0, 25)) == N
    for chunk in (64, 1000):
        got = fish(engine, N, (3, 4), (0, 30), (0, 25), chunk=chunk)
        for x, y in zip(got[:7], auto[:7]):
            assert x.dtype == y.dtype and np.array_equal(x, y)
        assert got[7] == auto[7]
    few = fish(engine, 3, chunk=64, **NEED_FISH)
    assert few[6].tolist() == [2394, 2457, 2765] and few[7] == 1766


def test_device_form(engine):
    n = 40
    host = fish(engine, n, (3, 4), (0, 30), (0, 25))
    assert len(host[0]) == n
    bufs = [engine.alloc(n * 81 + 16), engine.alloc(n * 81)] + [engine.alloc(n) for _ in range(4)] + [engine.alloc(n * 8)]
    d_puz, d_grid, d_level, d_open, d_o4, d_o5, d_index = bufs
    u8 = lambda d: d.download(np.empty(n, dtype=np.uint8))
    try:
        got = engine.generate_fish_dev(d_puz, d_grid, n, (3, 4), seed=SEED, lo=FIRST, open4=(0, 30), open5=(0, 25),
                                       max_scan=ROWS, d_level=d_level, d_open=d_open, d_open4=d_o4, d_open5=d_o5,
                                       d_index=d_index)
        engine.synchronize()
        assert got == (n, host[7])
        assert np.array_equal(d_puz.download(np.empty((n, 81), dtype=np.uint8)), host[0])
        assert np.array_equal(d_grid.download(np.empty((n, 81), dtype=np.uint8)), host[1])
        for d, ref in zip((d_level, d_open, d_o4, d_o5), host[2:6]):
            assert np.array_equal(u8(d), ref)
        assert np.array_equal(d_index.download(np.empty(n, dtype=np.uint64)), host[6])
        # the nullable outputs left out
        found = ctypes.c_uint64()
        assert engine.lib.sdk_generate_fish_dev(engine.ctx, SEED, FIRST, n, (1 << 3) | (1 << 4), 0, 81, 0, 30, 0, 25, ROWS,
                                                0, d_puz.ptr, d_grid.ptr, None, None, None, None, None,
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
        for ranges, word in (((lo, hi, 0, 64), b"open4"), ((0, 64, lo, hi), b"open5")):
            rc = engine.lib.sdk_generate_fish(engine.ctx, SEED, FIRST, n, MASK_ALL, 0, 81, *ranges, ROWS, 0, p(puz),
                                              p(grid), None, None, None, None, None, ctypes.byref(found), None)
            assert rc == L.SDK_EINVAL and word in engine.lib.sdk_last_error()
            assert found.value == 12345 and not puz.any()
    rc = engine.lib.sdk_generate_fish(engine.ctx, SEED, FIRST, n, MASK_ALL, 0, 81, 0, 64, 0, 64, ROWS, 0, p(puz), p(grid),
                                      None, None, None, None, None, ctypes.byref(found), None)
    assert rc == L.SDK_OK and found.value == n
    for bad in ((6, 5), (0, 65), (-1, 3)):
        with pytest.raises(ValueError):
            engine.generate_fish(4, open4=bad)
        with pytest.raises(ValueError):
            engine.generate_fish(4, open5=bad)
    e = engine.generate_fish(0)
    assert len(e) == 8 and e[0].shape == (0, 81) and e[7] == 0
