"""The model of graded generation (graded_model.py) on the window the GPU tests use
(test_gpu_generate_graded.py): seed 7, rows 1000..3047.  It pins that the window holds what those tests
rely on -- every level, rows inside and outside every clue range, rows SDK_OPT_GEN_CAP drops, a quota
that ends inside the window and one that does not -- so that none of them can pass vacuously.  Runs
without a GPU."""
import numpy as np
import pytest

import graded_model as M
from distributed_sudoku_solver_amd import synth


@pytest.fixture(scope="module")
def w():
    return M.window()


def test_window_is_the_stream(w):
    assert M.FIRST % 64 != 0
    p, g = synth.make_minimal(5, seed=M.SEED, lo=M.FIRST + 100)
    assert np.array_equal(w.puzzles[100:105], p) and np.array_equal(w.grids[100:105], g)
    assert ((w.puzzles == 0) | (w.puzzles == w.grids)).all()


def test_level_counts_and_clues(w):
    assert [int((w.level == k).sum()) for k in (1, 2, 3, 4)] == [14, 822, 270, 942]
    assert (int(w.clues.min()), int(w.clues.max())) == (21, 28)
    assert ((w.open > 0) == (w.level == 4)).all()


def test_clue_ranges(w):
    assert int(M.hits(w, M.MASK_ALL, 21, 23).sum()) == 415
    assert int(M.hits(w, 1 << 2, 26, 28).sum()) == 95
    assert not M.hits(w, M.MASK_ALL, 17, 17).any()
    r = M.select(64, M.MASK_ALL, 17, 17)
    assert (r.found, r.scanned) == (0, M.ROWS) and r.puzzles.shape == (0, 81)


def test_gen_cap_drops_rows(w):
    kept = M.hits(w, M.MASK_ALL, gen_cap=100)
    assert int(kept.sum()) == 513
    r = M.select(256, M.MASK_ALL, gen_cap=100)
    assert (r.found, r.scanned) == (256, 1035)
    assert (w.placements[r.index - M.FIRST] <= 100).all()
    assert (w.placements[:r.scanned] > 100).sum() == r.scanned - 256


def test_quota_inside_the_window():
    r = M.select(40, 1 << 3)
    assert (r.found, r.scanned) == (40, 283)
    assert int(r.index[-1]) == M.FIRST + 282 and (r.level == 3).all()
    assert (np.diff(r.index.astype(np.int64)) > 0).all()


def test_exhausted_window():
    r = M.select(64, 1 << 1)
    assert (r.found, r.scanned) == (14, M.ROWS)
    assert (r.level == 1).all() and (r.open == 0).all()


def test_single_levels_fill_their_quota():
    for level, n in ((2, 64), (3, 64), (4, 64)):
        r = M.select(n, 1 << level)
        assert r.found == n and r.scanned < M.ROWS and (r.level == level).all()
    assert M.select(8, 1 << 1).found == 8


def test_identity_selection(w):
    r = M.select(300, M.MASK_ALL)
    assert (r.found, r.scanned) == (300, 300)
    assert np.array_equal(r.index, np.arange(M.FIRST, M.FIRST + 300, dtype=np.uint64))
    assert np.array_equal(r.puzzles, w.puzzles[:300])


def test_many_tiles_window():
    """16,384 rows hold 170 level-1 puzzles (23 of them with at most 23 clues); the 64th is at offset
    6445, past 100 tiles of 64 rows."""
    big = M.window(M.SEED, M.FIRST, 16384)
    h = M.hits(big, 1 << 1)
    assert int(h.sum()) == 170
    r = M.select(64, 1 << 1, max_scan=16384, rows=16384)
    assert (r.found, r.scanned) == (64, 6446)
    assert np.array_equal(big.puzzles[:M.ROWS], M.window().puzzles)
