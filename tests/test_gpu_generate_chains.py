"""SudokuEngine.generate_chains / generate_chains_dev (sdk_generate_chains): graded generation with the chains
stage and the open6 and open7 ranges in the selection, against the same selection done by hand --
generate_batch over the window, chains_batch of those rows, a numpy filter -- byte for byte; against
generate_wings where open7 filters nothing, and against generate_graded where neither range does.  The window
is seed 7, rows 1000..3047, as in test_gpu_generate_wings.py."""
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
NEED_CHAINS = dict(levels=(4,), open6=(1, 64), open7=(0, 0))

Window = namedtuple("Window", "puzzles grids status level open open4 open5 open6 open7")


@pytest.fixture(scope="module")
def window(engine):
    """The window's candidates and their grades, by the batch calls (computed once)."""
    puz, grids, gst = engine.generate_batch(ROWS, seed=SEED, lo=FIRST)
    st, level, open_, open4, open5, open6, open7, out = engine.chains_batch(puz, budget=0)
    assert (gst == 1).all() and np.array_equal(out, grids)
    return Window(puz, grids, gst, level, open_, open4, open5, open6, open7)


def by_hand(w, n, levels, r6, r7, clues=(0, 81), max_scan=ROWS):
    """(rows, found, scanned) of the call's contract on the window."""
    given = (w.puzzles != 0).sum(axis=1)
    hit = (w.status == 1) & np.isin(w.level, levels) & (given >= clues[0]) & (given <= clues[1])
    hit &= (w.level != 4) | ((w.open6 >= r6[0]) & (w.open6 <= r6[1]) & (w.open7 >= r7[0]) & (w.open7 <= r7[1]))
    where = np.flatnonzero(hit[:max_scan])
    found = min(n, len(where))
    k = where[:found]
    return k, found, (int(k[-1]) + 1 if found == n else max_scan)


def chains(engine, n, levels, open6, open7, **kw):
    kw.setdefault("max_scan", ROWS)
    return engine.generate_chains(n, levels, seed=SEED, lo=FIRST, open6=open6, open7=open7, **kw)


def equals_by_hand(res, w, n, levels, r6, r7, clues=(0, 81), max_scan=ROWS):
    puz, sol, level, open_, o6, o7, index, scanned = res
    k, found, ref_scanned = by_hand(w, n, levels, r6, r7, clues, max_scan)
    print("levels", levels, "open6", r6, "open7", r7, "clues", clues, "found", len(puz), "by hand", found, "scanned",
          scanned, "by hand", ref_scanned)
    assert len(puz) == len(sol) == len(level) == len(open_) == len(o6) == len(o7) == len(index) == found
    assert scanned == ref_scanned
    assert index.dtype == np.uint64 and np.array_equal(index, (k + FIRST).astype(np.uint64))
    assert np.array_equal(level, w.level[k]) and np.array_equal(open_, w.open[k])
    assert o6.dtype == np.uint8 and np.array_equal(o6, w.open6[k])
    assert o7.dtype == np.uint8 and np.array_equal(o7, w.open7[k])
    assert np.array_equal(puz, w.puzzles[k]) and np.array_equal(sol, w.grids[k])
    return found


def test_puzzles_that_need_a_chain(engine, window):
    """In stream order: the level-4 puzzles the wings and colouring leave open and the chains close."""
    res = chains(engine, N, **NEED_CHAINS)
    assert equals_by_hand(res, window, N, (4,), (1, 64), (0, 0)) == N
    puz, sol, level, open_, o6, o7, index, scanned = res
    assert (level == 4).all() and (o6 > 0).all() and (o7 == 0).all() and (np.diff(index.astype(np.int64)) > 0).all()
    share = ((window.level == 4) & (window.open6 > 0) & (window.open7 == 0)).sum() / (window.level == 4).sum()
    print("share of the window's level-4 puzzles that need a chain: %.1f %%" % (100 * share))


def test_window_runs_out(engine, window):
    """A quota above what the window holds: found < n, scanned == max_scan, nothing written past the rows found."""
    total = int(((window.level == 4) & (window.open6 > 0) & (window.open7 == 0)).sum())
    n = total + 8
    puz, grid = np.full((n, 81), 0xAB, dtype=np.uint8), np.full((n, 81), 0xCD, dtype=np.uint8)
    lv, op, o6, o7 = (np.full(n, 0xEE, dtype=np.uint8) for _ in range(4))
    index = np.full(n, 12345, dtype=np.uint64)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    f, s = ctypes.c_uint64(), ctypes.c_uint64()
    rc = engine.lib.sdk_generate_chains(engine.ctx, SEED, FIRST, n, 1 << 4, 0, 81, 1, 64, 0, 0, ROWS, 0, p(puz), p(grid),
                                        p(lv), p(op), p(o6), p(o7), p(index), ctypes.byref(f), ctypes.byref(s))
    assert rc == L.SDK_OK and f.value == total and s.value == ROWS
    res = (puz[:total], grid[:total], lv[:total], op[:total], o6[:total], o7[:total], index[:total], s.value)
    assert equals_by_hand(res, window, n, (4,), (1, 64), (0, 0)) == total
    assert (puz[total:] == 0xAB).all() and (grid[total:] == 0xCD).all() and (index[total:] == 12345).all()
    for col in (lv, op, o6, o7):
        assert (col[total:] == 0xEE).all()


@pytest.mark.parametrize("levels,r6,r7,clues", [((1, 2, 3, 4), (1, 64), (0, 0), (24, 26)),
                                                ((3, 4), (10, 50), (1, 40), (0, 81)),
                                                ((1, 2, 3, 4), ANY, (20, 40), (22, 25))],
                         ids=["all-need-chains-24-26-clues", "3-4-both-ranges", "all-open7-20-40-22-25-clues"])
def test_mixed_levels_ranges_and_clues(engine, window, levels, r6, r7, clues):
    res = chains(engine, N, levels, r6, r7, clues=clues)
    assert equals_by_hand(res, window, N, levels, r6, r7, clues) >= 8
    lv, o6, o7 = res[2], res[4], res[5]
    assert ((o6[lv == 4] >= r6[0]) & (o6[lv == 4] <= r6[1])).all()
    assert ((o7[lv == 4] >= r7[0]) & (o7[lv == 4] <= r7[1])).all()
    assert (o6[lv != 4] == L.SDK_WINGS_NONE).all() and (o7[lv != 4] == L.SDK_CHAINS_NONE).all()


def test_level_mask_without_level4_skips_the_stage(engine, window):
    res = chains(engine, N, (2, 3), (1, 64), (0, 0))
    assert equals_by_hand(res, window, N, (2, 3), (1, 64), (0, 0)) == N
    assert (res[4] == 0xFF).all() and (res[5] == 0xFF).all()


def test_chunk_independence(engine, window):
    auto = chains(engine, N, chunk=0, **NEED_CHAINS)
    assert equals_by_hand(auto, window, N, (4,), (1, 64), (0, 0)) == N
    for chunk in (64, 1000):
        got = chains(engine, N, chunk=chunk, **NEED_CHAINS)
        for x, y in zip(got[:7], auto[:7]):
            assert x.dtype == y.dtype and np.array_equal(x, y)
        assert got[7] == auto[7]


def test_open7_any_is_wings_generation(engine):
    """open7 = (0, 64): the rows of generate_wings with open5 = (0, 64) and the same open6 range."""
    for levels, r6 in (((4,), (0, 0)), ((1, 2, 3, 4), (20, 40))):
        c = chains(engine, N, levels, r6, ANY)
        w = engine.generate_wings(N, levels, seed=SEED, lo=FIRST, open5=ANY, open6=r6, max_scan=ROWS)
        # puzzles, solutions, level, open; open6; index, scanned
        for x, y in zip(c[:4] + (c[4],) + c[6:], w[:4] + (w[5],) + w[6:]):
            assert np.array_equal(x, y)


def test_full_ranges_are_graded_generation(engine):
    for levels in ((1, 2, 3, 4), (4,), (2,)):
        r = chains(engine, 100, levels, ANY, ANY)
        g = engine.generate_graded(100, levels, seed=SEED, lo=FIRST, max_scan=ROWS)
        for x, y in zip(r[:4] + r[6:], g):
            assert np.array_equal(x, y)


def test_device_form(engine):
    n = 40
    host = chains(engine, n, (3, 4), (1, 64), (0, 30))
    assert len(host[0]) == n
    bufs = [engine.alloc(n * 81 + 16), engine.alloc(n * 81)] + [engine.alloc(n) for _ in range(4)] + [engine.alloc(n * 8)]
    d_puz, d_grid, d_level, d_open, d_o6, d_o7, d_index = bufs
    u8 = lambda d: d.download(np.empty(n, dtype=np.uint8))
    try:
        got = engine.generate_chains_dev(d_puz, d_grid, n, (3, 4), seed=SEED, lo=FIRST, open6=(1, 64), open7=(0, 30),
                                         max_scan=ROWS, d_level=d_level, d_open=d_open, d_open6=d_o6, d_open7=d_o7,
                                         d_index=d_index)
        engine.synchronize()
        assert got == (n, host[7])
        assert np.array_equal(d_puz.download(np.empty((n, 81), dtype=np.uint8)), host[0])
        assert np.array_equal(d_grid.download(np.empty((n, 81), dtype=np.uint8)), host[1])
        for d, ref in zip((d_level, d_open, d_o6, d_o7), host[2:6]):
            assert np.array_equal(u8(d), ref)
        assert np.array_equal(d_index.download(np.empty(n, dtype=np.uint64)), host[6])
        # the nullable outputs left out
        found = ctypes.c_uint64()
        d_puz.upload(np.zeros((n, 81), dtype=np.uint8))
        assert engine.lib.sdk_generate_chains_dev(engine.ctx, SEED, FIRST, n, (1 << 3) | (1 << 4), 0, 81, 1, 64, 0, 30,
                                                  ROWS, 0, d_puz.ptr, d_grid.ptr, None, None, None, None, None,
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
        for ranges, word in (((lo, hi, 0, 64), b"open6"), ((0, 64, lo, hi), b"open7")):
            rc = engine.lib.sdk_generate_chains(engine.ctx, SEED, FIRST, n, MASK_ALL, 0, 81, *ranges, ROWS, 0, p(puz),
                                                p(grid), None, None, None, None, None, ctypes.byref(found), None)
            assert rc == L.SDK_EINVAL and word in engine.lib.sdk_last_error()
            assert found.value == 12345 and not puz.any()
    rc = engine.lib.sdk_generate_chains(engine.ctx, SEED, FIRST, n, MASK_ALL, 0, 81, 0, 64, 0, 64, ROWS, 0, p(puz), p(grid),
                                        None, None, None, None, None, ctypes.byref(found), None)
    assert rc == L.SDK_OK and found.value == n
    for bad in ((6, 5), (0, 65), (-1, 3)):
        with pytest.raises(ValueError):
            engine.generate_chains(4, open6=bad)
        with pytest.raises(ValueError):
            engine.generate_chains(4, open7=bad)
    e = engine.generate_chains(0)
    assert len(e) == 8 and e[0].shape == (0, 81) and e[7] == 0
