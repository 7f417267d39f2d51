"""SudokuEngine.generate_rated / generate_rated_dev (sdk_generate_rated): graded generation with the
rate stage and the backdoor range in the selection, against the selection restated from the CPU
models (rated_model.py: graded_model's window, rate_model's counts), byte for byte -- and against
generate_graded where the range filters nothing.  The window is seed 7, rows 1000..3047."""
import ctypes

import numpy as np
import pytest

import rated_model as RM
from distributed_sudoku_solver_amd import _lib as L

pytestmark = pytest.mark.gpu

SEED, FIRST, ROWS = RM.SEED, RM.FIRST, RM.ROWS
N = 64
RANGES = [(0, 64), (0, 5), (10, 10)]
MASKS = [(4,), (3, 4), (1, 2)]


def mask_of(levels):
    return sum(1 << v for v in levels)


def rated(engine, n, levels, backdoors, **kw):
    kw.setdefault("max_scan", ROWS)
    return engine.generate_rated(n, levels, seed=SEED, lo=FIRST, backdoors=backdoors, **kw)


def equals_model(res, ref, n):
    puz, sol, level, open_, bd, key, index, scanned = res
    print("found", len(puz), "model", ref.found, "scanned", scanned, "model", ref.scanned)
    assert len(puz) == len(sol) == len(level) == len(open_) == len(bd) == len(key) == len(index) == ref.found
    if ref.found < n:          # the window ran out (a range without a hit included)
        assert scanned == ROWS
    assert scanned == ref.scanned
    assert index.dtype == np.uint64 and np.array_equal(index, ref.index)
    assert np.array_equal(level, ref.level) and np.array_equal(open_, ref.open)
    assert bd.dtype == np.uint8 and np.array_equal(bd, ref.backdoors)
    assert key.dtype == np.uint8 and np.array_equal(key, ref.key)
    assert np.array_equal(puz, ref.puzzles) and np.array_equal(sol, ref.grids)


@pytest.mark.parametrize("levels", MASKS, ids=lambda v: "levels" + "".join(map(str, v)))
@pytest.mark.parametrize("rng", RANGES, ids=lambda v: f"bd{v[0]}-{v[1]}")
def test_ranges_and_masks(engine, rng, levels):
    ref = RM.select(N, mask_of(levels), *rng)
    res = rated(engine, N, levels, rng)
    if ref.found == 0:
        assert len(res[0]) == 0 and res[7] == ROWS
    equals_model(res, ref, N)
    # only the search-level rows are held to the range; the others carry no rating
    lv, bd = res[2], res[4]
    assert ((bd[lv == 4] >= rng[0]) & (bd[lv == 4] <= rng[1])).all()
    assert (bd[lv != 4] == L.SDK_RATE_NONE).all() and (res[5][lv != 4] == L.SDK_RATE_NONE).all()


def test_a_partial_and_a_full_range(engine):
    """One range the window cannot fill and one it can, chosen by the model (not assumed)."""
    found = {r: RM.select(N, 1 << 4, *r).found for r in [(0, 0), (0, 1), (0, 2), (0, 3), (0, 5), (10, 10), (0, 64)]}
    print(found)
    partial = [r for r, f in found.items() if 1 <= f < N]
    fullr = [r for r, f in found.items() if f == N]
    assert partial and fullr
    for r in (partial[0], fullr[0]):
        equals_model(rated(engine, N, (4,), r), RM.select(N, 1 << 4, *r), N)


def test_chunk_independence(engine):
    ref = RM.select(N, mask_of((3, 4)), 0, 15)
    assert ref.found >= 1
    auto = rated(engine, N, (3, 4), (0, 15), chunk=0)
    equals_model(auto, ref, N)
    for chunk in (64, 100):
        got = rated(engine, N, (3, 4), (0, 15), chunk=chunk)
        for x, y in zip(got[:7], auto[:7]):
            assert x.dtype == y.dtype and np.array_equal(x, y)
        assert got[7] == auto[7]


def test_full_range_is_graded_generation(engine):
    for levels in ((1, 2, 3, 4), (4,), (2,)):
        r = rated(engine, 100, levels, (0, 64))
        g = engine.generate_graded(100, levels, seed=SEED, lo=FIRST, max_scan=ROWS)
        for x, y in zip(r[:4] + r[6:], g):
            assert np.array_equal(x, y)


def test_device_form(engine):
    host = rated(engine, 40, (3, 4), (0, 12))
    n = 40
    assert len(host[0]) == n
    bufs = [engine.alloc(n * 81 + 16), engine.alloc(n * 81)] + [engine.alloc(n) for _ in range(4)] + [engine.alloc(n * 8)]
    d_puz, d_grid, d_level, d_open, d_bd, d_key, d_index = bufs
    u8 = lambda d: d.download(np.empty(n, dtype=np.uint8))
    try:
        got = engine.generate_rated_dev(d_puz, d_grid, n, (3, 4), seed=SEED, lo=FIRST, backdoors=(0, 12), max_scan=ROWS,
                                        d_level=d_level, d_open=d_open, d_backdoors=d_bd, d_key=d_key, d_index=d_index)
        engine.synchronize()
        assert got == (n, host[7])
        assert np.array_equal(d_puz.download(np.empty((n, 81), dtype=np.uint8)), host[0])
        assert np.array_equal(d_grid.download(np.empty((n, 81), dtype=np.uint8)), host[1])
        for d, ref in zip((d_level, d_open, d_bd, d_key), host[2:6]):
            assert np.array_equal(u8(d), ref)
        assert np.array_equal(d_index.download(np.empty(n, dtype=np.uint64)), host[6])
        # the nullable outputs left out
        found = ctypes.c_uint64()
        assert engine.lib.sdk_generate_rated_dev(engine.ctx, SEED, FIRST, n, mask_of((3, 4)), 0, 81, 0, 12, ROWS, 0,
                                                 d_puz.ptr, d_grid.ptr, None, None, None, None, None,
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
        rc = engine.lib.sdk_generate_rated(engine.ctx, SEED, FIRST, n, RM.MASK_ALL, 0, 81, lo, hi, ROWS, 0, p(puz),
                                           p(grid), None, None, None, None, None, ctypes.byref(found), None)
        assert rc == L.SDK_EINVAL and b"backdoor" in engine.lib.sdk_last_error()
        assert found.value == 12345 and not puz.any()
    rc = engine.lib.sdk_generate_rated(engine.ctx, SEED, FIRST, n, RM.MASK_ALL, 0, 81, 0, 64, ROWS, 0, p(puz), p(grid),
                                       None, None, None, None, None, ctypes.byref(found), None)
    assert rc == L.SDK_OK and found.value == n
    for bad in ((6, 5), (0, 65), (-1, 3)):
        with pytest.raises(ValueError):
            engine.generate_rated(4, backdoors=bad)
    e = engine.generate_rated(0)
    assert len(e) == 8 and e[0].shape == (0, 81) and e[7] == 0
