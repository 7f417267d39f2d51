"""The boards and masks the frontier model tests share (test_frontier_model.py on the CPU,
test_gpu_frontier_model.py against the kernels)."""
import functools

import numpy as np

from distributed_sudoku_solver_amd import synth
from oracle import oracle as O
import prop_inputs
from prop_model import CELL_UNITS, UNITS

S1 = synth.SEEDS17["S1"]
C5_16 = S1[:-9] + "000800000"          # 7,309 completions
C5_15 = S1[:-9] + "0" * 9              # 3,481,026 completions
DEMO = "000100000000320000000009000000000070000000000000900000000000900000000003000000000"


def sparse_boards(n, seed, lo_clues, hi_clues):
    """n boards of lo_clues..hi_clues random cells of a valid grid: mostly many completions."""
    rng = np.random.default_rng(seed)
    sol = synth.make_17clue(n, seed=seed)[1]
    out = np.zeros((n, 81), dtype=np.uint8)
    for b, s, k in zip(out, sol, rng.integers(lo_clues, hi_clues + 1, n)):
        cells = rng.choice(81, int(k), replace=False)
        b[cells] = s[cells]
    return out


def with_duplicate(boards, seed):
    """Each board with one given repeated in an empty cell of its row, column or box (a unit with a
    digit given twice is inexact; the two clues do not conflict)."""
    rng = np.random.default_rng(seed)
    out = boards.copy()
    for b in out:
        for c in rng.permutation(np.flatnonzero(b)):
            u = UNITS[CELL_UNITS[c][rng.integers(3)]]
            free = [int(k) for k in u if b[k] == 0]
            if free:
                b[free[rng.integers(len(free))]] = b[c]
                break
    return out


def with_inert(boards, seed):
    """Each board with one cell (given or empty) set to a byte of 10..255, 255 among them."""
    rng = np.random.default_rng(seed)
    out = boards.copy()
    for i, b in enumerate(out):
        b[rng.integers(81)] = 255 if i % 4 == 0 else rng.integers(10, 256)
    return out


def range_masks(n, seed):
    """TASK ranges as first-cell masks: random ranges (empty ones among them), then in turn an empty,
    a one-digit and the full range."""
    rng = np.random.default_rng(seed)
    out = np.empty(n, dtype=np.uint16)
    for i in range(n):
        k = i % 6
        if k == 3:
            lo = int(rng.integers(0, 10))
            hi = lo
        elif k == 4:
            lo = int(rng.integers(1, 10))
            hi = lo + 1
        elif k == 5:
            lo, hi = 0, 10
        else:
            lo = int(rng.integers(0, 10))
            hi = int(rng.integers(lo, 11))
        out[i] = O.range_mask(lo, hi)
    return out


def dead_wiki():
    b = synth.parse(synth.WIKI).copy()
    b[2] = 5
    return b


@functools.lru_cache(maxsize=None)
def seed_pool():
    """The shuffled mix of boards one expansion level is compared on (read-only, 8,193 rows at
    least): the named sets of prop_inputs, sparse boards, duplicated and inert givens, complete
    grids, grids with one empty cell, boards whose first 64 cells are all given, boards whose lowest
    empty cell lies in 27..53 and in 54..80, and the empty board."""
    rng = np.random.default_rng(77)
    parts = [prop_inputs.named_set(k)[0] for k in ("minimal", "hard", "17clue", "edge", "broken")]
    sparse = sparse_boards(900, 31, 18, 34)
    parts += [sparse, with_duplicate(sparse[:300], 32), with_inert(sparse[300:600], 33)]
    sol = synth.make_17clue(700, seed=34)[1]
    parts.append(sol[:100])
    one = sol[100:300].copy()
    one[np.arange(200), rng.integers(0, 81, 200)] = 0
    parts.append(one)
    for k, (lo, hi) in enumerate(((64, 81), (27, 54), (54, 81))):
        late = sol[300 + 100 * k:400 + 100 * k].copy()
        for b in late:
            first = int(rng.integers(lo, hi))
            b[first] = 0
            rest = np.arange(first + 1, 81)
            b[rest[rng.random(rest.size) < 0.7]] = 0
        parts.append(late)
    parts.append(with_inert(one[:50], 35))
    parts.append(np.zeros((3, 81), dtype=np.uint8))
    pool = np.concatenate(parts)
    pool = np.ascontiguousarray(pool[rng.permutation(pool.shape[0])])
    assert pool.shape[0] >= 8193
    pool.setflags(write=False)
    return pool


@functools.lru_cache(maxsize=None)
def seed_masks():
    """One first-cell mask per seed_pool row: ranges (range_masks), and every fifth with the unused
    bits 0 and 10..15 set as well."""
    m = range_masks(seed_pool().shape[0], 78)
    m[::5] |= 0xFC01
    m.setflags(write=False)
    return m
