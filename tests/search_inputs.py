"""The boards, masks and model results the search model tests share (test_search_model.py on the CPU,
test_gpu_search_model.py against the kernels), built once per process."""
import functools
import json
import os

import numpy as np

from distributed_sudoku_solver_amd import synth
from oracle import oracle as O
import frontier_inputs
import search_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_cases.json")
FULL_MASK = O.ALL_DIGITS
# The model searches every board under this node budget, and so does one GPU pass: a board that needs
# more (the '55' board never finishes; a planted conflict can take exponentially long) is compared
# under budgets only.
CAP = 1500
# the SDK_OPT_NODE_BUDGET values of the GPU budget test (49: no board here takes 51 nodes under LEX)
BUDGETS = (1, 2, 3, 5, 8, 20, 25, 49)
ORDERS = (M.ORDER_LEX, M.ORDER_MRV_UNIQUE)


def golden_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def sparse_boards(n, seed, lo_clues, hi_clues):
    """Boards that keep each cell of a valid grid with a per-board probability of lo..hi clues / 81:
    mostly many completions (test_gpu_solve._random_puzzles)."""
    rng = np.random.default_rng(seed)
    sol = synth.make_17clue(n, seed=seed)[1]
    keep = rng.random((n, 81)) < rng.uniform(lo_clues, hi_clues, (n, 1)) / 81.0
    return np.where(keep, sol, 0).astype(np.uint8)


def planted_boards(n, seed):
    """Boards of 20..45 clues, in turn with one given copied over another (where a unit of the
    overwritten cell holds that digit as a given already, the unit has it twice and is inexact), with
    two cells set to bytes of 10..255, and as they are
    (test_gpu_solve.test_conflicting_and_inert_givens_vs_oracle)."""
    rng = np.random.default_rng(seed)
    puz = sparse_boards(n, seed, 20, 45)
    for i in range(n):
        nz = np.flatnonzero(puz[i])
        if i % 3 == 0 and len(nz) >= 2:
            a, b = rng.choice(nz, 2, replace=False)
            puz[i, b] = puz[i, a]
        elif i % 3 == 1:
            puz[i, rng.choice(81, 2, replace=False)] = rng.integers(10, 256, 2)
    return puz


def edge_boards():
    """(boards, masks): the empty board; a full valid grid; a full grid with a duplicated given; a board
    whose mask allows no digit; a board with no empty cell and a non-trivial mask; '55' + 79 zeros
    (no completion and no refutation by singles: it ends only at a budget)."""
    full = synth.parse(synth.WIKI_SOLUTION)
    dup = full.copy()
    dup[10] = dup[0]
    fifty_five = np.zeros(81, np.uint8)
    fifty_five[0] = fifty_five[1] = 5
    boards = [np.zeros(81, np.uint8), full, dup, synth.parse(synth.WIKI), full, fifty_five]
    masks = [FULL_MASK, FULL_MASK, FULL_MASK, O.range_mask(5, 5), O.range_mask(3, 4), FULL_MASK]
    return np.stack(boards).astype(np.uint8), np.array(masks, dtype=np.uint16)


@functools.lru_cache(maxsize=None)
def inputs():
    """(boards uint8[n,81], masks uint16[n], families {name: slice}); read-only.  Families without a
    mask of their own carry the full range."""
    cases = golden_cases()
    parts, masks, families = [], [], {}

    def add(name, boards, m=None):
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
        start = sum(len(p) for p in parts)
        families[name] = slice(start, start + len(boards))
        parts.append(boards)
        masks.append(np.full(len(boards), FULL_MASK, np.uint16) if m is None else np.asarray(m, np.uint16))

    add("golden", np.array([c["puzzle"] for c in cases], dtype=np.uint8),
        [O.range_mask(*c["range"]) for c in cases])
    add("17clue", synth.make_17clue(64, seed=7)[0])
    add("minimal", synth.minimal_nodes(200)[0])
    add("hard", synth.load_hard(160)[0])
    add("heaviest", synth.make_hard_heaviest(16)[0])
    add("sparse", sparse_boards(200, 8, 8, 30), frontier_inputs.range_masks(200, 9))
    add("planted", planted_boards(90, 31))
    add("edge", *edge_boards())
    boards, masks = np.concatenate(parts), np.concatenate(masks)
    boards.setflags(write=False)
    masks.setflags(write=False)
    return boards, masks, families


def one_digit_mask(boards, masks):
    """The boards FIRST_CELL_OPEN can tell apart: an empty cell and a mask of exactly one digit."""
    real = (masks >> 1) & M.ALL
    return (boards == 0).any(axis=1) & (real != 0) & ((real & (real - 1)) == 0)


class Results:
    """The model's answer per board of inputs(): status int8[n], out uint8[n,81], nodes, rounds, depth
    int64[n]; read-only.  A board that needed more than `budget` nodes has status -2, its input as out
    and budget + 1 nodes."""

    def __init__(self, rows, budget):
        self.budget = budget
        self.status = np.array([r[0] for r in rows], dtype=np.int8)
        self.out = np.array([r[1] for r in rows], dtype=np.uint8).reshape(-1, 81)
        self.nodes, self.rounds, self.depth = (np.array([r[k] for r in rows], dtype=np.int64) for k in (2, 3, 4))
        for a in (self.status, self.out, self.nodes, self.rounds, self.depth):
            a.setflags(write=False)

    def counter(self, kind):
        """The counter work[] holds under SDK_OPT_WORK_COUNTER = kind (SDK_WORK_NODES, _ROUNDS, _DEPTH)."""
        return (self.nodes, self.rounds, self.depth)[kind]

    def under(self, budget):
        """(hit bool[n], status, out) under a smaller node budget: a board is cut exactly when it needs
        more nodes (the searches are deterministic and nodes only grows), everything else is unchanged."""
        assert 0 < budget <= self.budget
        hit = self.nodes > budget
        boards = inputs()[0]
        return hit, np.where(hit, M.ST_BUDGET_HIT, self.status).astype(np.int8), np.where(hit[:, None], boards, self.out)


def model(order, first_cell_open=False):
    """Results of M.solve under the budget CAP for every board of inputs().  first_cell_open: with
    solve4_kernel's first-cell rule (search_model.FIRST_CELL_OPEN), which only boards with a
    one-digit mask can tell from the plain one: the others are the plain model's rows."""
    return _model(int(order), bool(first_cell_open))


@functools.lru_cache(maxsize=None)
def _model(order, first_cell_open):
    boards, masks, _ = inputs()
    if not first_cell_open:
        return Results([M.solve(b, m, order, CAP) for b, m in zip(boards, masks)], CAP)
    plain = model(order)
    rows = [(plain.status[i], plain.out[i], plain.nodes[i], plain.rounds[i], plain.depth[i]) for i in range(len(boards))]
    for i in np.flatnonzero(one_digit_mask(boards, masks)):
        rows[i] = M.solve(boards[i], masks[i], order, CAP, first_cell_open=True)
    return Results(rows, CAP)
