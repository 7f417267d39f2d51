"""A plain model of graded generation (sdk_generate_graded, include/sudoku_hip.h), restated from the
oracles the tree already has: synth.make_minimal for the rows of the stream, grade_model.grade for a
row's level and open count, synth.grid_orders' placement counts for SDK_OPT_GEN_CAP, and a numpy
filter for the predicate and the first n hits in stream order.  Nothing of the GPU path is used.

Candidate k of (seed) is row k of the stream.  It is a hit when it was kept by the cap, bit `level` of
the mask is set and lo <= clues <= hi; a row the cap drops is zeros with level 0 and never a hit.  The
window is [first, first + max_scan); found = min(n, hits in it); scanned = offset of the n-th hit + 1
when found == n, else max_scan.
"""
import functools
from collections import namedtuple

import numpy as np

import grade_model as G
from distributed_sudoku_solver_amd import synth

SEED = 7
FIRST = 1000          # not a multiple of 64
ROWS = 2048
MASK_ALL = 0x1E
NO_CAP = 1 << 20      # the default SDK_OPT_GEN_CAP

Window = namedtuple("Window", "puzzles grids level open clues placements")
Result = namedtuple("Result", "puzzles grids level open index found scanned")


@functools.lru_cache(maxsize=None)
def window(seed=SEED, first=FIRST, rows=ROWS):
    """Rows [first, first + rows) of the stream with their grades (computed once; read-only)."""
    puzzles, grids = synth.make_minimal(rows, seed=seed, lo=first)
    level, open_ = G.grade(puzzles)
    clues = (puzzles != 0).sum(axis=1).astype(np.uint32)
    _, _, placements = synth.grid_orders(np.arange(first, first + rows, dtype=np.uint64), seed=seed)
    w = Window(np.ascontiguousarray(puzzles), np.ascontiguousarray(grids), level, open_, clues, placements)
    for a in w:
        a.setflags(write=False)
    return w


def hits(w, level_mask, clues_lo=0, clues_hi=81, gen_cap=NO_CAP):
    """bool[rows]: which rows of the window match the predicate."""
    kept = w.placements <= gen_cap
    in_mask = ((level_mask >> w.level.astype(np.uint32)) & 1).astype(bool)
    return kept & in_mask & (w.clues >= clues_lo) & (w.clues <= clues_hi)


def select(n, level_mask, clues_lo=0, clues_hi=81, max_scan=ROWS, gen_cap=NO_CAP, seed=SEED, first=FIRST,
           rows=ROWS):
    """The call's result on the window [first, first + max_scan), max_scan <= rows."""
    assert 1 <= max_scan <= rows
    w = window(seed, first, rows)
    where = np.flatnonzero(hits(w, level_mask, clues_lo, clues_hi, gen_cap)[:max_scan])
    found = min(n, len(where))
    k = where[:found]
    scanned = int(k[-1]) + 1 if found == n and n > 0 else (0 if n == 0 else max_scan)
    return Result(w.puzzles[k], w.grids[k], w.level[k], w.open[k], (k + first).astype(np.uint64), found, scanned)
