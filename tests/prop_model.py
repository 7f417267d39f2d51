"""A plain model of the propagation pass (csrc/prop32_kernel.h): what prop32_kernel does to ONE board,
restated from its header comment and prop32_body without bit slices, lanes or LDS.

A board is 81 candidate sets (9-bit masks, bit d - 1 = digit d).  `propagate_batch` advances many
boards at once only to be quick: every array operation below works row by row, no value of one board
ever reaches another, and the schedule (which step is followed by a locked-candidates pass) is a
function of the step number alone -- so a board's row of the result is what `propagate` gives for that
board alone (pinned in test_prop_model.py), as a board's path through the kernel does not depend on
the boards it shares a group with.

The rules, in the kernel's order:
  * a given above 9 makes a board inexact: undecided from the start, listed with its input;
  * a step: (a) closed cells, empty cells, per unit the digits of its closed cells (T), the digits held
    by two or more of its cells (twos) and the digits no cell holds (missing).  At step 0 a digit
    closed twice in a unit (a duplicated given) makes the board inexact.  An empty cell or a missing
    digit refutes; all cells closed and nothing missing solves.  (b) the step counter advances (a
    board still live at max_steps is given up), and the cells phase: an open cell loses the T of its
    three units, then is restricted to those of its remaining candidates that some unit holds in no
    other cell, if there are any (two such candidates are both kept); everything from the state at the
    start of the step;
  * after step lc_first and every lc_every-th step after it one locked-candidates pass: presence P of
    the 54 box-line triads over all cells, claim(L,B) = P(L,B) & ~P(L,B1) & ~P(L,B2), point(L,B) =
    P(L,B) & ~P(L1,B) & ~P(L2,B), the open cells of triad (L,B) lose claim(L1,B) | claim(L2,B) |
    point(L,B1) | point(L,B2);
  * a board unchanged by the cells phase of the step before such a pass and by the pass is stuck;
  * handover: a stuck board with a digit closed twice in a unit is refuted, any other stuck board is
    listed with its closed cells as givens; without handover every undecided board is listed with
    its input;
  * the tail (SDK_OPT_PROP32_TAIL = live | step << 8, handover only): at the first step numbered
    `step` or later at which at most `live` boards of a group are live, they are handed over as they
    stand after that step's cells phase.  With live = 64 that is every board still live at that step,
    whatever its group -- a snapshot of the pass at a step of one's choice, which is what tail_step
    models (and all it models: a smaller `live` does depend on the group).
"""
import numpy as np

ALL = 0x1FF

# class of a board after the pass
SOLVED, REFUTED, LISTED = 1, 0, -4
# why
R_SOLVED, R_CONTRA, R_DUP_CLOSED, R_STUCK, R_INEXACT, R_MAX_STEPS, R_TAIL = range(7)

UNITS = np.array([[9 * r + c for c in range(9)] for r in range(9)] +
                 [[9 * r + c for r in range(9)] for c in range(9)] +
                 [[9 * (3 * (b // 3) + i // 3) + 3 * (b % 3) + i % 3 for i in range(9)] for b in range(9)])
# the row, column and box of every cell
CELL_UNITS = np.array([[c // 9, 9 + c % 9, 18 + 3 * (c // 27) + (c % 9) // 3] for c in range(81)])

_DIGIT_OF = np.zeros(ALL + 1, dtype=np.uint8)
for _d in range(9):
    _DIGIT_OF[1 << _d] = _d + 1


def schedule(lc):
    """(lc_first, lc_every) of an SDK_OPT_PROP32_LC value: period | first step << 8, first step 0 =
    the period."""
    every = max(1, lc & 0xFF)
    return ((lc >> 8) or every), every


def _closed(X):
    return (X != 0) & ((X & (X - 1)) == 0)


def _unit_summary(X, closed):
    """Per unit [n,27]: T, twos, ones (digits some cell holds), dup (digits closed in two cells)."""
    XU = X[:, UNITS]                                   # [n,27,9]
    CU = np.where(closed[:, UNITS], XU, 0)
    n = X.shape[0]
    ones = np.zeros((n, 27), dtype=np.uint16)
    twos = np.zeros_like(ones)
    T = np.zeros_like(ones)
    dup = np.zeros_like(ones)
    for q in range(9):
        twos |= ones & XU[:, :, q]
        ones |= XU[:, :, q]
        dup |= T & CU[:, :, q]
        T |= CU[:, :, q]
    return T, twos, ones, dup


def _cells_phase(X, closed, T, twos):
    cu = CELL_UNITS
    U = T[:, cu[:, 0]] | T[:, cu[:, 1]] | T[:, cu[:, 2]]                     # [n,81]
    alone = ~(twos[:, cu[:, 0]] & twos[:, cu[:, 1]] & twos[:, cu[:, 2]]) & ALL   # held once by some unit
    v = np.where(closed, X, X & ~U)
    h = v & alone
    return np.where(h != 0, h, v).astype(np.uint16)


def _others(P, axis):
    return np.roll(P, 1, axis=axis), np.roll(P, 2, axis=axis)


def _triad_elims(P):
    """P [n,3,3,3]: presence of triad (band or stack, line in it, box along the line).  Returns what
    the open cells of each triad lose."""
    b1, b2 = _others(P, 3)        # the line's triads in the other two boxes
    l1, l2 = _others(P, 2)        # the box's triads in the other two lines
    claim = P & ~b1 & ~b2
    point = P & ~l1 & ~l2
    c1, c2 = _others(claim, 2)    # claim(L1,B), claim(L2,B)
    p1, p2 = _others(point, 3)    # point(L,B1), point(L,B2)
    return c1 | c2 | p1 | p2


def _locked_pass(X, closed):
    n = X.shape[0]
    G = X.reshape(n, 3, 3, 3, 3)                      # [band, row in band, stack, column in stack]
    # row triads: (band, row in band, stack), over the three columns of the stack
    Er = _triad_elims(np.bitwise_or.reduce(G, axis=4))
    # column triads: (stack, column in stack, band), over the three rows of the band
    Ec = _triad_elims(np.bitwise_or.reduce(G, axis=2).transpose(0, 2, 3, 1))
    lose = Er[:, :, :, :, None] | Ec.transpose(0, 3, 1, 2)[:, :, None, :, :]
    lose = np.broadcast_to(lose, G.shape).reshape(n, 81)
    return np.where(closed, X, X & ~lose).astype(np.uint16)


def propagate_batch(boards, lc_first=3, lc_every=5, handover=True, max_steps=96, tail_step=None):
    """boards uint8[n,81] -> (cls int8[n], grids uint8[n,81], steps int32[n], reason int8[n]).

    cls: SOLVED (grids = the solution), REFUTED (grids = the input: what the solver returns for it),
    LISTED (grids = what the search is given).  steps: the pass's step counter when the board was
    decided or given up (the kernel gives up at max_steps)."""
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    n = boards.shape[0]
    X = np.where(boards == 0, ALL, 1 << ((boards.astype(np.int32) - 1) & 15)).astype(np.uint16)
    X[boards > 9] = ALL                                # (an inexact board's sets do not matter)
    cls = np.full(n, LISTED, dtype=np.int8)
    reason = np.full(n, -1, dtype=np.int8)
    steps = np.zeros(n, dtype=np.int32)
    grids = boards.copy()

    live = np.ones(n, dtype=bool)

    def leave(mask, c, why, it):
        cls[mask], reason[mask], steps[mask] = c, why, it
        live[mask] = False

    leave((boards > 9).any(axis=1), LISTED, R_INEXACT, 0)
    it, next_lc, lc = 0, lc_first, False
    unchanged = np.zeros(n, dtype=bool)
    while live.any():
        closed = _closed(X)
        if lc:
            new = _locked_pass(X, closed)
            leave(live & unchanged & (new == X).all(axis=1), LISTED, R_STUCK, it)
            X, lc = new, False
            unchanged[:] = False
            continue
        T, twos, ones, dup = _unit_summary(X, closed)
        if it == 0:
            leave(live & (dup != 0).any(axis=1), LISTED, R_INEXACT, 0)
        bad = (X == 0).any(axis=1) | (ones != ALL).any(axis=1)
        leave(live & bad, REFUTED, R_CONTRA, it)
        leave(live & closed.all(axis=1), SOLVED, R_SOLVED, it)      # (bad ones have left)
        if live.any():
            if handover and tail_step is not None and it >= tail_step:
                leave(live.copy(), LISTED, R_TAIL, it)
            else:
                it += 1
                if it >= max_steps:
                    leave(live.copy(), LISTED, R_MAX_STEPS, it)
        lc = bool(live.any()) and it == next_lc
        if lc:
            next_lc += lc_every
        new = _cells_phase(X, closed, T, twos)
        if lc:
            unchanged = live & (new == X).all(axis=1)
        X = new

    closed = _closed(X)
    solved = cls == SOLVED
    grids[solved] = _DIGIT_OF[X[solved]]
    if handover:
        handed = (reason == R_STUCK) | (reason == R_MAX_STEPS) | (reason == R_TAIL)
        _, _, _, dup = _unit_summary(X, closed)
        refuted = handed & (dup != 0).any(axis=1)
        cls[refuted], reason[refuted] = REFUTED, R_DUP_CLOSED
        handed &= ~refuted
        grids[handed] = _DIGIT_OF[np.where(closed, X, 0)[handed]]
    return cls, grids, steps, reason


def propagate(board, lc_first=3, lc_every=5, handover=True, max_steps=96, tail_step=None):
    """One board: (class, grid uint8[81], steps, reason)."""
    c, g, s, r = propagate_batch(np.asarray(board, dtype=np.uint8).reshape(1, 81), lc_first, lc_every, handover,
                                 max_steps, tail_step)
    return int(c[0]), g[0], int(s[0]), int(r[0])
