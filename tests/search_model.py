"""A plain model of the search kernels (csrc/solve_kernel.h + solve_launch.hip, which solve2_kernel.h and
solve4_kernel.h claim to equal node for node): what a solve call does to ONE board, restated from
`propagate`, `search` and solve_kernel's board loop with integer bit sets -- no lanes, halves, LDS or
stacks.  It gives the status and the board, and the three counters a call can report in work[]:
search nodes (SDK_WORK_NODES), propagation rounds (SDK_WORK_ROUNDS) and the deepest DFS level
(SDK_WORK_DEPTH).

Cells.  An input byte 0 is an open cell with candidates 1..9 (a 9-bit set, bit d - 1 = digit d); 1..9
is a clue; 10..255 is inert: it holds no digit and makes its three units inexact.  Which cells are
clues is the INPUT's for the whole search: a cell the search closes never becomes a clue (the frontier
model's records do turn closed cells into clues; this model never re-reads a board).

First-cell mask (bit d = digit d allowed, the TASK range).  The lowest-index input-0 cell keeps only the
digits the mask allows.  A board with no empty cell ignores its mask.  An empty mask leaves that cell
without a candidate: a contradiction, found in round 1.

One synchronous round: everything is computed from the state at the round's start, and the round
counter advances at its head, also for a round that ends in a contradiction.
  * per unit: T = the digits of its clues and of its closed non-clue cells (a non-clue cell with
    exactly one candidate is closed).  Two closed non-clue cells with the same digit, or a closed
    non-clue cell that repeats a clue, are a conflict (two clues with the same digit are not: clues are
    never validated).  A unit is exact when it has no inert cell and no clue digit given twice; an
    exact unit in which some digit is held by no cell at all is a conflict.  In exact units only,
    `once` = the digits held by exactly one cell of the unit.
  * per non-clue, non-inert cell: no candidate is a contradiction.  A cell with two or more candidates
    loses the T of its three units; then, if some of what is left is in a unit's `once`, it is
    restricted to that -- two such digits are a contradiction, and so is ending with none.
  * rounds repeat until one changes nothing.  The verdict is CONTRA, SOLVED (no cell with two or more
    candidates) or OPEN.

Search.  Propagate, then nodes += 1.  With a budget, nodes > budget ends the search as a budget hit.
SOLVED counts a completion (the first one is recorded: the input bytes, open cells filled) and stops at
`limit`, else goes on as a contradiction.  OPEN branches on the lowest-index cell with two or more
candidates (LEX) or on the one with the fewest candidates, lowest index on a tie (MRV); digits are
tried ascending.  A level is stacked per branch; depth is the number of stacked levels, maxd its
maximum.  A contradiction resumes the deepest level that still has untried digits -- a level leaves the
stack when its LAST digit is taken, not when that digit fails -- and at depth 0 the search ends.

A solve call.  SDK_ORDER_LEX: one LEX search with limit 1.  SDK_ORDER_MRV_UNIQUE: an MRV search with
limit 2 (a unique completion is the lexicographically first one); if it finds two, a LEX search with
limit 1 follows from the input and the mask again, ON THE SAME COUNTERS: nodes, rounds and maxd carry
over, and the budget applies to the sum.  Status 1 (the board: the last search's first completion), 0
or -2 (budget hit); for 0 and -2 the input comes back.

FIRST_CELL_OPEN -- solve4_kernel's one documented difference (its header, "the first-cell `range`
restriction is the exception").  solve_kernel and solve2_kernel restrict the first cell's candidate
set, so a one-digit mask makes it a closed non-clue cell from the start: its digit is in T in round 1.
solve4_kernel starts that cell OPEN whatever the mask's size: in round 1 it is updated like any open
cell (it loses T, which refutes a digit its units already hold) and closes at the end of that round,
which counts as a change, so its peers lose the digit in round 2.  The fixpoint, and with it every
node, branch, depth and answer, is the same; only the round count of a search's first node can differ,
and only under a one-digit mask.  `first_cell_open=True` models that rule.
"""
from prop_model import CELL_UNITS, UNITS

ALL = 0x1FF
CONTRA, SOLVED, OPEN = 0, 1, 2
ORDER_MRV_UNIQUE, ORDER_LEX = 0, 1          # SDK_ORDER_* (include/sudoku_hip.h)
_LEX, _MRV = 0, 1                           # the order of one search
ST_SOLVED, ST_UNSOLVABLE, ST_BUDGET_HIT = 1, 0, -2

_UNITS = [[int(c) for c in u] for u in UNITS]
_CELL_UNITS = [tuple(int(u) for u in cu) for cu in CELL_UNITS]
_POP = [bin(v).count("1") for v in range(ALL + 1)]


class _Board:
    """What stays fixed during a search: the input, its open cells, and per unit the clue digits,
    whether the unit is exact and its open cells."""

    def __init__(self, board, mask):
        self.inp = [int(v) for v in board]
        assert len(self.inp) == 81 and all(0 <= v <= 255 for v in self.inp)
        self.free = [k for k, v in enumerate(self.inp) if v == 0]
        self.clue_t, self.exact, self.unit_free = [], [], []
        for cells in _UNITS:
            t, dup, inert = 0, 0, False
            for k in cells:
                v = self.inp[k]
                if 1 <= v <= 9:
                    dup |= t & (1 << (v - 1))
                    t |= 1 << (v - 1)
                elif v > 9:
                    inert = True
            self.clue_t.append(t)
            self.exact.append(not inert and dup == 0)
            self.unit_free.append([k for k in cells if self.inp[k] == 0])
        self.start = [ALL if v == 0 else 0 for v in self.inp]
        self.first = self.free[0] if self.free else None
        if self.first is not None and mask is not None:
            self.start[self.first] = (int(mask) >> 1) & ALL

    def filled(self, c):
        return [v if v else c[k].bit_length() for k, v in enumerate(self.inp)]


class _Counters:
    def __init__(self):
        self.nodes = self.rounds = self.maxd = 0
        self.first = None


def _round(b, c, late):
    """One round on the candidate sets c (updated in place: a cell's update reads only its own set and
    the unit summaries, which are complete before the first update).  late: the cell FIRST_CELL_OPEN
    keeps open for this round, or None.  Returns (contradiction, changed)."""
    taken, once = [0] * 27, [0] * 27
    for u in range(27):
        t = b.clue_t[u]
        ones, twos, n1, n2 = t, 0, 0, 0
        for k in b.unit_free[u]:
            v = c[k]
            twos |= ones & v
            ones |= v
            if v & (v - 1) == 0 and k != late:      # a closed non-clue cell (an empty set adds nothing)
                n2 |= n1 & v
                n1 |= v
        if n2 | (n1 & t):
            return True, False
        if b.exact[u]:
            if ones != ALL:
                return True, False
            once[u] = ones & ~twos
        taken[u] = t | n1
    changed = False
    for k in b.free:
        v = c[k]
        if v & (v - 1) or (k == late and v):
            r, col, box = _CELL_UNITS[k]
            v1 = v & ~(taken[r] | taken[col] | taken[box])
            h = v1 & (once[r] | once[col] | once[box])
            if h:
                if h & (h - 1):
                    return True, False
                v1 = h
            if v1 == 0:
                return True, False
            if v1 != v or k == late:                # (the late cell closes: a change)
                changed = True
                c[k] = v1
        elif v == 0:
            return True, False
    return False, changed


def propagate(b, c, cnt, late=None):
    """Rounds to a fixpoint or a contradiction: CONTRA, SOLVED or OPEN."""
    while True:
        cnt.rounds += 1
        bad, changed = _round(b, c, late)
        late = None
        if bad:
            return CONTRA
        if not changed:
            for k in b.free:
                if c[k] & (c[k] - 1):
                    return OPEN
            return SOLVED


def _branch_cell(b, c, order):
    """The branch cell of an OPEN state."""
    if order == _LEX:
        return next(k for k in b.free if c[k] & (c[k] - 1))
    best, cell = 10, None
    for k in b.free:
        n = _POP[c[k]]
        if 2 <= n < best:
            best, cell = n, k
    return cell


def search(b, order, limit, budget, cnt, first_cell_open=False):
    """One search from the input and the mask: the number of completions found (stopping at `limit`, 0 =
    none), or -1 at a budget hit.  The first completion goes to cnt.first."""
    c = list(b.start)
    late = b.first if first_cell_open else None
    stack, count = [], 0
    while True:
        r = propagate(b, c, cnt, late)
        late = None
        cnt.nodes += 1
        if budget and cnt.nodes > budget:
            return -1
        if r == SOLVED:
            count += 1
            if count == 1:
                cnt.first = b.filled(c)
            if limit and count >= limit:
                return count
            r = CONTRA
        if r == OPEN:
            cell = _branch_cell(b, c, order)
            m = c[cell]
            d = m & -m
            stack.append((list(c), cell, m ^ d))
            cnt.maxd = max(cnt.maxd, len(stack))
            c[cell] = d
            continue
        if not stack:
            return count
        snap, cell, rest = stack[-1]
        d = rest & -rest
        rest ^= d
        c = list(snap)
        if rest == 0:
            stack.pop()
        else:
            stack[-1] = (snap, cell, rest)
        c[cell] = d


def solve(board, mask=None, order=ORDER_LEX, budget=0, first_cell_open=False):
    """One board of a solve call: (status, out list[81], nodes, rounds, depth)."""
    b = _Board(board, mask)
    cnt = _Counters()
    if order == ORDER_LEX:
        n = search(b, _LEX, 1, budget, cnt, first_cell_open)
    else:
        n = search(b, _MRV, 2, budget, cnt, first_cell_open)
        if n >= 2:
            n = search(b, _LEX, 1, budget, cnt, first_cell_open)
    status = ST_BUDGET_HIT if n < 0 else (ST_SOLVED if n > 0 else ST_UNSOLVABLE)
    out = cnt.first if status == ST_SOLVED else list(b.inp)
    return status, out, cnt.nodes, cnt.rounds, cnt.maxd
