"""SudokuEngine.generate_graded / generate_graded_dev (sdk_generate_graded): generation, grading and
the ordered selection on the GPU against the selection restated from the CPU oracles (graded_model.py:
synth.make_minimal rows, grade_model grades, a numpy filter), byte for byte -- and against
generate_batch / grade_batch where no model is needed.  The window is seed 7, rows 1000..3047
(test_graded_model.py pins what it holds)."""
import ctypes

import numpy as np
import pytest

import graded_model as M
from distributed_sudoku_solver_amd import synth, _lib as L

pytestmark = pytest.mark.gpu

SEED, FIRST, ROWS, ALL = M.SEED, M.FIRST, M.ROWS, (1, 2, 3, 4)
FILL = 0xEE


@pytest.fixture
def eng(engine):
    keys = (L.SDK_OPT_GEN_CAP, L.SDK_OPT_NODE_BUDGET)
    old = {k: engine.get_option(k) for k in keys}
    yield engine
    for k, v in old.items():
        engine.set_option(k, v)


def graded(eng, n, levels, **kw):
    kw.setdefault("max_scan", ROWS)
    return eng.generate_graded(n, levels, seed=SEED, lo=FIRST, **kw)


def same(a, b):
    """two results of generate_graded, every array and the scanned count"""
    assert len(a) == len(b) == 6
    for x, y in zip(a[:5], b[:5]):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert a[5] == b[5]


def equals_model(res, ref):
    puz, sol, level, open_, index, scanned = res
    print("found", len(puz), "model", ref.found, "scanned", scanned, "model", ref.scanned)
    assert len(puz) == len(sol) == len(level) == len(open_) == len(index) == ref.found
    assert scanned == ref.scanned
    assert index.dtype == np.uint64 and np.array_equal(index, ref.index)
    assert level.dtype == np.uint8 and np.array_equal(level, ref.level)
    assert open_.dtype == np.uint8 and np.array_equal(open_, ref.open)
    assert np.array_equal(puz, ref.puzzles), np.flatnonzero((puz != ref.puzzles).any(axis=1))[:8]
    assert np.array_equal(sol, ref.grids), np.flatnonzero((sol != ref.grids).any(axis=1))[:8]


def raw(eng, n, mask, lo=0, hi=81, max_scan=ROWS, chunk=0, first=FIRST, rows=None, skip=()):
    """sdk_generate_graded itself on host arrays of `rows` rows pre-filled with FILL:
    (rc, arrays, found, scanned); the outputs named in `skip` are passed as NULL."""
    rows = n if rows is None else rows
    arrs = {"puzzles": np.full((rows, 81), FILL, dtype=np.uint8), "grids": np.full((rows, 81), FILL, dtype=np.uint8),
            "level": np.full(rows, FILL, dtype=np.uint8), "open": np.full(rows, FILL, dtype=np.uint8),
            "index": np.full(rows, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)}
    found, scanned = ctypes.c_uint64(12345), ctypes.c_uint64(12345)
    ptr = [None if k in skip else ctypes.c_void_p(a.ctypes.data) for k, a in arrs.items()]
    rc = eng.lib.sdk_generate_graded(eng.ctx, SEED, first, n, mask, lo, hi, max_scan, chunk, *ptr,
                                     None if "found" in skip else ctypes.byref(found),
                                     None if "scanned" in skip else ctypes.byref(scanned))
    return rc, arrs, found.value, scanned.value


def untouched(arrs, start=0):
    return all((a[start:] == (FILL if a.dtype == np.uint8 else 0xEEEEEEEEEEEEEEEE)).all() for a in arrs.values())


@pytest.mark.parametrize("level,n", [(1, 8), (2, 64), (3, 64), (4, 64)])
def test_single_levels(eng, level, n):
    ref = M.select(n, 1 << level)
    assert ref.found == n
    equals_model(graded(eng, n, (level,)), ref)


def test_identity(eng):
    """Every level, every clue count: the selection is the stream itself (no model involved)."""
    puz, sol, level, open_, index, scanned = graded(eng, 300, ALL)
    rp, rs, st = eng.generate_batch(300, seed=SEED, lo=FIRST)
    _, rl, ro, _ = eng.grade_batch(rp, budget=0)
    assert (st == L.SDK_SOLVED).all()
    assert np.array_equal(puz, rp) and np.array_equal(sol, rs)
    assert np.array_equal(index, np.arange(FIRST, FIRST + 300, dtype=np.uint64))
    assert np.array_equal(level, rl) and np.array_equal(open_, ro)
    assert scanned == 300


def test_chunk_independence(eng):
    """The 40th level-3 hit is at offset 282: the quota falls before, on and after a round's end."""
    ref = M.select(40, 1 << 3)
    assert ref.scanned == 283
    auto = graded(eng, 40, (3,), chunk=0)
    equals_model(auto, ref)
    for chunk in (63, 64, 65, 100, 282, 283, 284, 4096):
        same(graded(eng, 40, (3,), chunk=chunk), auto)


def test_chunk_of_one(eng):
    equals_model(graded(eng, 5, ALL, chunk=1), M.select(5, M.MASK_ALL))


@pytest.mark.parametrize("max_scan", [1, 63, 64, 65])
def test_window_edges(eng, max_scan):
    ref = M.select(100, M.MASK_ALL, max_scan=max_scan)
    assert (ref.found, ref.scanned) == (max_scan, max_scan)
    equals_model(graded(eng, 100, ALL, max_scan=max_scan), ref)


def test_exhausted_window_writes_nothing_behind_found(eng):
    ref = M.select(64, 1 << 1)
    assert (ref.found, ref.scanned) == (14, ROWS)
    rc, arrs, found, scanned = raw(eng, 64, 1 << 1)
    assert rc == L.SDK_OK and (found, scanned) == (14, ROWS)
    assert np.array_equal(arrs["puzzles"][:14], ref.puzzles) and np.array_equal(arrs["grids"][:14], ref.grids)
    assert np.array_equal(arrs["level"][:14], ref.level) and np.array_equal(arrs["open"][:14], ref.open)
    assert np.array_equal(arrs["index"][:14], ref.index)
    assert untouched(arrs, 14)
    # the device form: the same rows, and the device arrays unchanged from row 14 on
    n = 64
    bufs = [eng.alloc(n * 81), eng.alloc(n * 81), eng.alloc(n), eng.alloc(n), eng.alloc(n * 8)]
    try:
        for b in bufs:
            b.upload(np.full(b.nbytes, FILL, dtype=np.uint8))
        got = eng.generate_graded_dev(bufs[0], bufs[1], n, (1,), seed=SEED, lo=FIRST, max_scan=ROWS,
                                      d_level=bufs[2], d_open=bufs[3], d_index=bufs[4])
        eng.synchronize()
        assert got == (14, ROWS)
        dev = {k: b.download(np.empty_like(arrs[k])) for k, b in zip(arrs, bufs)}
        for k in arrs:
            assert np.array_equal(dev[k], arrs[k]), k
    finally:
        for b in bufs:
            b.free()


def test_clue_ranges(eng):
    ref = M.select(512, M.MASK_ALL, 21, 23)
    assert (ref.found, ref.scanned) == (415, ROWS)
    equals_model(graded(eng, 512, ALL, clues=(21, 23)), ref)
    ref = M.select(128, 1 << 2, 26, 28)
    assert ref.found == 95
    equals_model(graded(eng, 128, (2,), clues=(26, 28)), ref)
    ref = M.select(64, 1 << 2, 26, 28)
    assert ref.found == 64 and ref.scanned < ROWS
    equals_model(graded(eng, 64, (2,), clues=(26, 28)), ref)
    res = graded(eng, 64, ALL, clues=(17, 17))
    assert len(res[0]) == 0 and res[0].shape == (0, 81) and res[5] == ROWS
    equals_model(res, M.select(64, M.MASK_ALL, 17, 17))


def test_gen_cap(eng):
    """SDK_OPT_GEN_CAP = 100: the rows the cap drops are never selected."""
    ref = M.select(256, M.MASK_ALL, gen_cap=100)
    assert ref.found == 256 and ref.scanned == 1035
    old = eng.get_option(L.SDK_OPT_GEN_CAP)
    eng.set_option(L.SDK_OPT_GEN_CAP, 100)
    try:
        res = graded(eng, 256, ALL)
    finally:
        eng.set_option(L.SDK_OPT_GEN_CAP, old)
    assert eng.get_option(L.SDK_OPT_GEN_CAP) == old
    equals_model(res, ref)
    assert (res[0] != 0).any(axis=1).all()


def test_many_tiles_against_model(eng):
    ref = M.select(64, 1 << 1, max_scan=16384, rows=16384)
    assert (ref.found, ref.scanned) == (64, 6446)
    equals_model(graded(eng, 64, (1,), max_scan=16384), ref)


def test_many_tiles_scan_loop(eng):
    """2^17 rows in one round are 2,048 tiles: the scan's workgroup loops (1,024 tiles a step).  The
    same window in rounds of 4,096 gives the same result (consistency only, no model)."""
    for n in (500, 1000):
        one = graded(eng, n, (1,), max_scan=1 << 17, chunk=1 << 17)
        many = graded(eng, n, (1,), max_scan=1 << 17, chunk=4096)
        print("n", n, "found", len(one[0]), "scanned", one[5])
        same(one, many)
        assert len(one[0]) == n
        assert (one[2] == 1).all() and (np.diff(one[4].astype(np.int64)) > 0).all()
        assert int(one[4][-1]) == FIRST + one[5] - 1
    # about one row in a hundred is of level 1 (the 500th is at offset 52,563): the last of 1,000 lies in
    # a tile that only the scan's second step reaches
    assert one[5] > 1024 * 64


def test_device_form(eng):
    n = 40
    host = graded(eng, n, (3,))
    assert len(host[0]) == n
    bufs = [eng.alloc(n * 81 + 16), eng.alloc(n * 81), eng.alloc(n), eng.alloc(n), eng.alloc(n * 8)]
    d_puz, d_grid, d_level, d_open, d_index = bufs
    try:
        got = eng.generate_graded_dev(d_puz, d_grid, n, (3,), seed=SEED, lo=FIRST, max_scan=ROWS, d_level=d_level,
                                      d_open=d_open, d_index=d_index)
        eng.synchronize()
        assert got == (n, host[5])
        assert np.array_equal(d_puz.download(np.empty((n, 81), dtype=np.uint8)), host[0])
        assert np.array_equal(d_grid.download(np.empty((n, 81), dtype=np.uint8)), host[1])
        assert np.array_equal(d_level.download(np.empty(n, dtype=np.uint8)), host[2])
        assert np.array_equal(d_open.download(np.empty(n, dtype=np.uint8)), host[3])
        assert np.array_equal(d_index.download(np.empty(n, dtype=np.uint64)), host[4])
        # the nullable outputs left out
        for b in (d_puz, d_grid):
            b.upload(np.zeros(n * 81, dtype=np.uint8))
        lib, ctx = eng.lib, eng.ctx
        found = ctypes.c_uint64()
        assert lib.sdk_generate_graded_dev(ctx, SEED, FIRST, n, 1 << 3, 0, 81, ROWS, 0, d_puz.ptr, d_grid.ptr, None,
                                           None, None, ctypes.byref(found), None) == L.SDK_OK
        eng.synchronize()
        assert found.value == n
        assert np.array_equal(d_puz.download(np.empty((n, 81), dtype=np.uint8)), host[0])
        assert np.array_equal(d_grid.download(np.empty((n, 81), dtype=np.uint8)), host[1])
        # a misaligned board pointer
        off = ctypes.c_void_p(d_puz.ptr.value + 1)
        scanned = ctypes.c_uint64()
        for args in ((off, d_grid.ptr), (d_grid.ptr, off)):
            assert lib.sdk_generate_graded_dev(ctx, SEED, FIRST, n, 1 << 3, 0, 81, ROWS, 0, *args, None, None, None,
                                               ctypes.byref(found), ctypes.byref(scanned)) == L.SDK_EINVAL
            assert b"aligned" in lib.sdk_last_error()
        assert lib.sdk_generate_graded_dev(ctx, SEED, FIRST, n, 1 << 3, 0, 81, ROWS, 0, None, d_grid.ptr, None, None,
                                           None, ctypes.byref(found), None) == L.SDK_EINVAL
        assert b"NULL" in lib.sdk_last_error()
    finally:
        for b in bufs:
            b.free()


def test_argument_errors(eng):
    top = (1 << 64) - 1
    bad = [dict(mask=0), dict(mask=1), dict(mask=1 << 5), dict(mask=0x1E | 1), dict(lo=30, hi=29), dict(hi=82),
           dict(max_scan=0), dict(first=top - 9, max_scan=10), dict(chunk=(1 << 24) + 1), dict(skip=("puzzles",)),
           dict(skip=("grids",)), dict(skip=("found",))]
    for kw in bad:
        kw.setdefault("mask", M.MASK_ALL)
        rc, arrs, found, scanned = raw(eng, 4, **kw)
        assert rc == L.SDK_EINVAL, kw
        assert eng.lib.sdk_last_error(), kw
        assert untouched(arrs) and (found, scanned) == (12345, 12345), kw
    # the last indices of the stream are a valid window
    rc, arrs, found, scanned = raw(eng, 4, M.MASK_ALL, first=top - 10, max_scan=10)
    assert rc == L.SDK_OK and (found, scanned) == (4, 4)
    assert np.array_equal(arrs["index"], np.arange(top - 10, top - 6, dtype=np.uint64))
    # n == 0: nothing is launched or written
    rc, arrs, found, scanned = raw(eng, 0, M.MASK_ALL, rows=4)
    assert rc == L.SDK_OK and (found, scanned) == (0, 0) and untouched(arrs)
    e = eng.generate_graded(0)
    assert e[0].shape == (0, 81) and e[1].shape == (0, 81) and e[4].shape == (0,) and e[5] == 0
    # the nullable outputs
    rc, arrs, found, scanned = raw(eng, 4, M.MASK_ALL, skip=("level", "open", "index", "scanned"))
    assert rc == L.SDK_OK and found == 4 and scanned == 12345
    assert np.array_equal(arrs["puzzles"], M.window().puzzles[:4])
    assert untouched({k: arrs[k] for k in ("level", "open", "index")})
    for kw in (dict(levels=()), dict(levels=(0,)), dict(levels=(5,)), dict(clues=(30, 29)), dict(clues=(0, 82)),
               dict(max_scan=0), dict(lo=top, max_scan=1), dict(chunk=(1 << 24) + 1), dict(chunk=-1), dict(n=-1)):
        with pytest.raises(ValueError):
            eng.generate_graded(**{"n": 4, **kw})


def test_one_timing_span(eng):
    """SDK_OPT_TIMING: a call is one span, whatever its rounds."""
    try:
        for chunk in (0, 100):
            eng.timer_reset()
            res = graded(eng, 40, (3,), chunk=chunk)
            eng.synchronize()
            ms, spans = eng.timer_read()
            assert len(res[0]) == 40 and spans == 1 and ms > 0.0
    finally:
        eng.timer_stop()


def test_no_residue(eng):
    """The context's node budget neither changes the result nor is changed, and a solve gives the same
    answers before and after a graded call."""
    boards = np.concatenate([synth.make_17clue(256, seed=3)[0], M.window().puzzles[:256]])
    before = eng.solve_batch(boards)
    assert (before[1] == L.SDK_SOLVED).all()
    ref = graded(eng, 40, (3, 4))
    eng.set_option(L.SDK_OPT_NODE_BUDGET, 1)
    try:
        tight = graded(eng, 40, (3, 4))
        assert eng.get_option(L.SDK_OPT_NODE_BUDGET) == 1
    finally:
        eng.set_option(L.SDK_OPT_NODE_BUDGET, 0)
    same(tight, ref)
    equals_model(ref, M.select(40, (1 << 3) | (1 << 4)))
    after = eng.solve_batch(boards)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
