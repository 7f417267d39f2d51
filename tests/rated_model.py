"""A plain model of rated generation (sdk_generate_rated, include/sudoku_hip.h): graded_model's window
and predicate with rate_model's backdoor counts.  A candidate is a hit when it is a hit of graded
generation and, if its level is 4, lo <= backdoors <= hi; candidates of levels 1..3 are not filtered
by the range.  Nothing of the GPU path is used.
"""
import functools
from collections import namedtuple

import numpy as np

import graded_model as M
import rate_model as R

SEED, FIRST, ROWS, MASK_ALL = M.SEED, M.FIRST, M.ROWS, M.MASK_ALL

Result = namedtuple("Result", "puzzles grids level open backdoors key index found scanned")


@functools.lru_cache(maxsize=None)
def ratings():
    """(backdoors, key) of graded_model.window()'s rows (computed once; read-only)."""
    w = M.window()
    backdoors, key = R.rate(w.puzzles, w.grids)
    backdoors.setflags(write=False)
    key.setflags(write=False)
    return backdoors, key


def hits(level_mask, bd_lo=0, bd_hi=64, clues_lo=0, clues_hi=81):
    w = M.window()
    backdoors, _ = ratings()
    in_range = (backdoors >= bd_lo) & (backdoors <= bd_hi)
    return M.hits(w, level_mask, clues_lo, clues_hi) & ((w.level != 4) | in_range)


def select(n, level_mask, bd_lo=0, bd_hi=64, clues_lo=0, clues_hi=81, max_scan=ROWS):
    """The call's result on the window [FIRST, FIRST + max_scan), max_scan <= ROWS."""
    assert 1 <= max_scan <= ROWS
    w = M.window()
    backdoors, key = ratings()
    where = np.flatnonzero(hits(level_mask, bd_lo, bd_hi, clues_lo, clues_hi)[:max_scan])
    found = min(n, len(where))
    k = where[:found]
    scanned = int(k[-1]) + 1 if found == n and n > 0 else (0 if n == 0 else max_scan)
    return Result(w.puzzles[k], w.grids[k], w.level[k], w.open[k], backdoors[k], key[k],
                  (k + FIRST).astype(np.uint64), found, scanned)
