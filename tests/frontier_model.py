"""A plain model of the breadth-first frontier family (csrc/frontier_kernel.h, expand4_kernel.h and
run_frontier_levels / refine_frontier / refine_head in csrc/sudoku_hip.hip): sdk_expand_boards,
sdk_frontier_build, sdk_frontier_refine[_range|_head] and sdk_frontier_load_dev as pure functions of
their boards, restated from the headers' comments without lanes, tiles or prefix sums.

Cells and units.  An input byte 0 is an open cell with candidates {1..9}, 1..9 a clue, 10..255 an
inert given: it holds nothing and makes its three units inexact.  A unit is exact iff it has no
inert given and no digit given twice; only an exact unit must hold every digit.  Clues never
conflict with clues.

First-cell mask (level 0 only): the lowest-index cell whose input byte is 0 keeps only the digits d
with bit d of the mask set (bits 0 and 10..15 mean nothing).  A board without an empty cell ignores
its mask; an empty mask leaves the cell without candidates, which is a contradiction.

One synchronous round, everything from the state at its start.  Per unit, T = the digits of its clues
and of its closed (one candidate) non-clue cells.  Contradiction: a digit closed in two non-clue
cells of a unit, or in a non-clue cell and a clue; an exact unit with a digit that no cell holds; a
non-clue cell without a candidate.  A cell with two or more candidates loses the T of its three
units, and is then restricted to those of its remaining candidates that one of its exact units holds
in exactly one cell, if there are any; two such candidates, or no candidate left, is a
contradiction.  Rounds repeat until one changes nothing.  Verdict: CONTRA, SOLVED (no cell with two
or more candidates) or OPEN.

The propagated record keeps every non-zero input byte (inert ones too), a closed cell becomes its
digit, an open cell stays 0.

A level.  CONTRA: no child.  SOLVED: a leaf and no child (count mode), the record as its own only
child (first mode).  OPEN: the branch cell is the cell with the fewest candidates, lowest index on a
tie (count mode), or the lowest-index open cell (first mode); one child per candidate, digits
ascending: the record with that cell set.  Children are concatenated in parent order.

The loop.  Before a level: stop when the frontier is empty, when it holds >= target boards (unless
this is level 0 and it is forced), or after 81 levels.  After it: the children are the frontier, the
leaves add up, and the build stops when there is no child or, in first mode, when nothing branched.
sdk_expand_boards forces level 0; sdk_frontier_build forces it iff a mask is given.  (The capacity
rule -- a level above min(2^25, 9 * max(m0, target)) children is rejected -- is left out: with at
most nine children per parent it needs millions of boards.)

`propagate_batch` / `level` work on many boards at once only to be quick: every array operation is
row by row, so a board's row is what `propagate_one` (plain Python, one board) gives for it alone
(pinned in test_frontier_model.py).
"""
import numpy as np

from prop_model import CELL_UNITS, UNITS

ALL = 0x1FF
CONTRA, SOLVED, OPEN = 0, 1, 2
COUNT, FIRST = 0, 1          # SDK_FRONTIER_COUNT, SDK_FRONTIER_FIRST
MAX_LEVELS = 81

_POP = np.array([bin(v).count("1") for v in range(ALL + 1)], dtype=np.uint8)
_DIGIT_OF = np.zeros(ALL + 1, dtype=np.uint8)
for _d in range(9):
    _DIGIT_OF[1 << _d] = _d + 1


def _mask_bits(mask):
    """first-cell mask (bit d = digit d) -> candidate set (bit d - 1 = digit d)"""
    return (int(mask) >> 1) & ALL


# ------------------------------------------------------------------ one board, plain Python
def propagate_one(board, mask=None, staged=False):
    """One board -> (verdict, cand list[81], record uint8[81]).

    staged = the second rule order: the unit eliminations alone to a fixpoint, then one round of
    hidden singles, and so on until neither changes anything.  Same contradiction tests."""
    board = [int(v) for v in np.asarray(board).reshape(81)]
    clue = [1 <= v <= 9 for v in board]
    inert = [v > 9 for v in board]
    cand = [ALL if v == 0 else (1 << (v - 1) if v <= 9 else 0) for v in board]
    if mask is not None and 0 in board:
        cand[board.index(0)] &= _mask_bits(mask)
    units = [[int(c) for c in u] for u in UNITS]
    exact = []
    for u in units:
        given = [board[c] for c in u if clue[c]]
        exact.append(not any(inert[c] for c in u) and len(set(given)) == len(given))

    def one_round(eliminate, hidden):
        """-> (contradicted, new candidates)"""
        T, once = [], []
        for k, u in enumerate(units):
            tc = tn = 0
            holders = {}
            for c in u:
                if inert[c]:
                    continue
                v = cand[c]
                if clue[c]:
                    tc |= v
                elif v and not v & (v - 1):
                    if tn & v:
                        return True, None          # closed in two non-clue cells
                    tn |= v
                for d in range(9):
                    if v >> d & 1:
                        holders[d] = holders.get(d, 0) + 1
            if tn & tc:
                return True, None                  # closed in a non-clue cell and a clue
            if exact[k] and len(holders) != 9:
                return True, None                  # an exact unit lost a digit
            T.append(tc | tn)
            once.append(sum(1 << d for d, h in holders.items() if h == 1) if exact[k] else 0)
        new = list(cand)
        for c in range(81):
            if clue[c] or inert[c]:
                continue
            v = cand[c]
            if v == 0:
                return True, None                  # a non-clue cell without a candidate
            if not v & (v - 1):
                continue
            a, b, x = (int(k) for k in CELL_UNITS[c])
            if eliminate:
                v &= ~(T[a] | T[b] | T[x])
            if hidden:
                h = v & (once[a] | once[b] | once[x])
                if h:
                    if h & (h - 1):
                        return True, None          # two hidden singles for one cell
                    v = h
            if v == 0:
                return True, None
            new[c] = v
        return False, new

    while True:
        if staged:
            bad, new = one_round(True, False)
            if not bad and new == cand:
                bad, new = one_round(False, True)
        else:
            bad, new = one_round(True, True)
        if bad:
            return CONTRA, None, None
        if new == cand:
            break
        cand = new
    is_open = [not clue[c] and not inert[c] and cand[c] & (cand[c] - 1) != 0 for c in range(81)]
    rec = np.array([board[c] if board[c] else (0 if is_open[c] else int(_DIGIT_OF[cand[c]])) for c in range(81)],
                   dtype=np.uint8)
    return (OPEN if any(is_open) else SOLVED), cand, rec


def level_one(board, mask=None, mode=COUNT):
    """One board's level -> (verdict, children uint8[k,81], leaves)."""
    verdict, cand, rec = propagate_one(board, mask)
    none = np.empty((0, 81), dtype=np.uint8)
    if verdict == CONTRA:
        return verdict, none, 0
    if verdict == SOLVED:
        return (verdict, rec[None].copy(), 0) if mode == FIRST else (verdict, none, 1)
    opens = [c for c in range(81) if rec[c] == 0]
    cell = opens[0] if mode == FIRST else min(opens, key=lambda c: (bin(cand[c]).count("1"), c))
    kids = []
    for d in range(9):
        if cand[cell] >> d & 1:
            k = rec.copy()
            k[cell] = d + 1
            kids.append(k)
    return verdict, np.array(kids, dtype=np.uint8), 0


# ------------------------------------------------------------------ many boards, row by row
def propagate_batch(boards, masks=None):
    """boards uint8[n,81] (+ first-cell masks uint16[n]) -> (verdict int8[n], cand uint16[n,81],
    records uint8[n,81]); cand and records of a contradicted board mean nothing."""
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    n = boards.shape[0]
    clue = (boards >= 1) & (boards <= 9)
    inert = boards > 9
    X = np.where(boards == 0, ALL, np.where(clue, 1 << ((boards.astype(np.int32) - 1) & 15), 0)).astype(np.uint16)
    if masks is not None:
        masks = np.asarray(masks, dtype=np.uint16).reshape(n)
        has = (boards == 0).any(axis=1)
        z = np.argmax(boards == 0, axis=1)
        rows = np.flatnonzero(has)
        X[rows, z[rows]] &= ((masks[rows] >> 1) & ALL).astype(np.uint16)
    CU = clue[:, UNITS]                                              # [n,27,9]
    GU = np.where(CU, X[:, UNITS], 0)
    seen = np.zeros((n, 27), dtype=np.uint16)
    twice = np.zeros((n, 27), dtype=np.uint16)
    for q in range(9):
        twice |= seen & GU[:, :, q]
        seen |= GU[:, :, q]
    exact = ~inert[:, UNITS].any(axis=2) & (twice == 0)              # [n,27]
    free = ~clue & ~inert                                            # the non-clue cells

    verdict = np.full(n, -1, dtype=np.int8)
    live = np.arange(n)
    cu = CELL_UNITS
    while live.size:
        x, fr, cl, ex = X[live], free[live], clue[live], exact[live]
        single = fr & (x != 0) & ((x & (x - 1)) == 0)
        XU = x[:, UNITS]
        NU = np.where(single[:, UNITS], XU, 0)
        TC = np.bitwise_or.reduce(np.where(cl[:, UNITS], XU, 0), axis=2)
        m = live.size
        ones = np.zeros((m, 27), dtype=np.uint16)
        twos = np.zeros_like(ones)
        TN = np.zeros_like(ones)
        TN2 = np.zeros_like(ones)
        for q in range(9):
            twos |= ones & XU[:, :, q]
            ones |= XU[:, :, q]
            TN2 |= TN & NU[:, :, q]
            TN |= NU[:, :, q]
        bad = ((TN2 | (TN & TC)) != 0).any(axis=1) | (ex & (ones != ALL)).any(axis=1) | (fr & (x == 0)).any(axis=1)
        T = TC | TN
        once = np.where(ex, ones & ~twos, 0).astype(np.uint16)
        U = T[:, cu[:, 0]] | T[:, cu[:, 1]] | T[:, cu[:, 2]]
        H = once[:, cu[:, 0]] | once[:, cu[:, 1]] | once[:, cu[:, 2]]
        multi = fr & ((x & (x - 1)) != 0)
        v = x & ~U
        h = v & H
        bad |= (multi & ((h & (h - 1)) != 0)).any(axis=1)
        v = np.where(h != 0, h, v)
        bad |= (multi & (v == 0)).any(axis=1)
        new = np.where(multi, v, x).astype(np.uint16)
        same = (new == x).all(axis=1)
        X[live] = new
        verdict[live[bad]] = CONTRA
        done = ~bad & same
        still = (fr & ((new & (new - 1)) != 0)).any(axis=1)
        verdict[live[done]] = np.where(still[done], OPEN, SOLVED)
        live = live[~bad & ~same]
    is_open = free & ((X & (X - 1)) != 0)
    rec = np.where(boards != 0, boards, np.where(is_open, 0, _DIGIT_OF[X & ALL])).astype(np.uint8)
    return verdict, X, rec


def level(boards, masks=None, mode=COUNT):
    """One expansion level of a frontier -> (children uint8[k,81], leaves, boards that branched)."""
    verdict, X, rec = propagate_batch(boards, masks)
    n = rec.shape[0]
    is_open = (rec == 0)
    pop = _POP[X & ALL].astype(np.int32)
    if mode == FIRST:
        cell = np.argmax(is_open, axis=1)
    else:
        cell = np.argmin(np.where(is_open, pop, 99), axis=1)        # the first of the lowest counts
    bm = np.where(verdict == OPEN, X[np.arange(n), cell], 0).astype(np.int64)
    nch = _POP[bm].astype(np.int64)
    keep = (verdict == SOLVED) & (mode == FIRST)
    nch[keep] = 1
    off = np.concatenate(([0], np.cumsum(nch)))
    out = np.empty((int(off[-1]), 81), dtype=np.uint8)
    rows = np.flatnonzero(keep)
    out[off[rows]] = rec[rows]
    for d in range(9):
        rows = np.flatnonzero(bm >> d & 1)
        pos = off[rows] + _POP[bm[rows] & ((1 << d) - 1)]
        out[pos] = rec[rows]
        out[pos, cell[rows]] = d + 1
    leaves = 0 if mode == FIRST else int((verdict == SOLVED).sum())
    return out, leaves, int((verdict == OPEN).sum())


def run_levels(boards, masks, mode, target, force0):
    """The level loop -> (records, leaves, levels, parents of every expanded level)."""
    fr = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    leaves, lvl, parents = 0, 0, []
    while True:
        m = fr.shape[0]
        if m == 0 or (m >= target and not (lvl == 0 and force0)) or lvl >= MAX_LEVELS:
            break
        parents.append(m)
        fr, lv, branched = level(fr, masks if lvl == 0 else None, mode)
        leaves += lv
        lvl += 1
        if fr.shape[0] == 0 or (mode == FIRST and branched == 0):
            break
    return fr, leaves, lvl, parents


def expand_boards(boards, masks=None, target=64):
    """sdk_expand_boards: the first-mode frontier below n seed boards, level 0 forced."""
    return run_levels(boards, masks, FIRST, target, True)[0]


class Frontier:
    """A context's frontier: records, the leaves of the call that made it, its mode."""

    def __init__(self, records, leaves, mode, levels=0, parents=()):
        self.records = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, 81)
        self.leaves, self.mode, self.levels, self.parents = leaves, mode, levels, list(parents)

    @property
    def size(self):
        return self.records.shape[0]

    def load(self, records):
        return Frontier(np.array(records, dtype=np.uint8).reshape(-1, 81), 0, self.mode)

    def refine(self, first, step, end, target):
        share = self.records[first:min(end, self.size):step] if first < min(end, self.size) else self.records[:0]
        n = share.shape[0]
        if n == 0:
            return Frontier(share, 0, self.mode)
        rec, leaves, levels, parents = run_levels(share, None, self.mode, max(target, n), False)
        return Frontier(rec, leaves, self.mode, levels, parents)

    def refine_head(self, lo, mid, hi, target):
        hi = min(hi, self.size)
        lo = min(lo, hi)
        mid = min(max(mid, lo), hi)
        head = self.refine(lo, 1, mid, target)
        return Frontier(np.concatenate([head.records, self.records[mid:hi]]), head.leaves, self.mode, head.levels,
                        head.parents)


def build(board, mask=None, mode=COUNT, target=1):
    """sdk_frontier_build of one board (an explicit target): level 0 is forced iff a mask is given."""
    m = None if mask is None else np.array([mask], dtype=np.uint16)
    rec, leaves, levels, parents = run_levels(np.asarray(board, dtype=np.uint8).reshape(1, 81), m, mode, target,
                                              mask is not None)
    return Frontier(rec, leaves, mode, levels, parents)
