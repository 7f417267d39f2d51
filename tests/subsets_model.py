"""A plain model of the subsets stage (csrc/subsets_kernel.h): F_4 and `open4` of ONE board, restated
from include/sudoku_hip.h (sdk_subsets_batch) on grade_model's candidate sets and rule helpers.

Two rules on the nine candidate sets of a unit, beside N, H and L of grade_model.py:
  naked S_k    k cells of a unit whose candidate sets have a union of at most k digits: every other
               cell of the unit loses those digits;
  hidden S_k   k digits that only k or fewer cells of a unit hold: those cells lose every other digit.
Both are ONE primitive on a 9 x 9 bit matrix (`subset_removals`): for every subset of 1..kmax rows whose
union has at most as many bits as the subset has rows, the union is cleared from the other rows.  The
naked rule is the primitive on the matrix cell -> digits of a unit, the hidden rule the primitive on its
transpose digit -> cells.  k = 1 of each is N and H (on a state that holds a completion).
R4 = R3 + {naked and hidden S_2, S_3, S_4}; F_4 is the state no rule of R4 changes.  `open4` is the number
of open cells of F_4 for a board of level 4, SDK_SUBSETS_NONE = 0xFF for every other board.

The rules only remove candidates and their premises survive further removals, so F_4 is one state
whatever the order of application; `order` picks between orders so that a test can pin that:
  "f3"      from F_3: a subset pass, then the R3 fixpoint again, until a subset pass changes nothing;
  "input"   the same alternation, but the first subset pass runs on the input's candidate sets;
  "mixed"   rounds of one N + H phase, one subset pass and one locked pass, from the input.

As in grade_model.py everything is batched over boards only to be quick: every array operation works
row by row, and a board's row of the result is what the model gives for that board alone.
"""
import functools
import itertools

import numpy as np

import grade_model as G
from prop_model import ALL, UNITS, _closed, _locked_pass

NONE = 0xFF
ORDERS = ("f3", "input", "mixed")

_POP = np.array([bin(v).count("1") for v in range(ALL + 1)], dtype=np.uint8)


def subset_removals(rows, kmax=4):
    """rows uint16[m,9] (m matrices of nine 9-bit rows) -> uint16[m,9]: what each row loses.  For every
    subset of 1..kmax rows whose union has at most as many bits as the subset has rows, the other rows
    lose the union."""
    rows = np.asarray(rows, dtype=np.uint16)
    rem = np.zeros_like(rows)
    for k in range(1, kmax + 1):
        for sub in itertools.combinations(range(9), k):
            u = rows[:, sub[0]].copy()
            for r in sub[1:]:
                u |= rows[:, r]
            u[_POP[u] > k] = 0
            if not u.any():
                continue
            others = [r for r in range(9) if r not in sub]
            rem[:, others] |= u[:, None]
    return rem


def transpose(rows):
    """uint16[m,9] -> uint16[m,9]: bit q of row d of the result is bit d of row q."""
    rows = np.asarray(rows, dtype=np.uint16)
    out = np.zeros_like(rows)
    for d in range(9):
        for q in range(9):
            out[:, d] |= ((rows[:, q] >> d) & 1) << q
    return out


def unit_pass(rows, kmax=4):
    """One unit's nine candidate sets uint16[m,9] -> the sets after the naked and the hidden rule, both
    from the state given."""
    rows = np.asarray(rows, dtype=np.uint16)
    naked = subset_removals(rows, kmax)
    hidden = transpose(subset_removals(transpose(rows), kmax))
    return rows & ~(naked | hidden)


def subset_pass(X, kmax=4):
    """One pass of naked and hidden S_1..S_kmax over the 27 units of every row of X, all from X."""
    n = X.shape[0]
    new = unit_pass(X[:, UNITS].reshape(n * 27, 9), kmax).reshape(n, 27, 9)
    out = X.copy()
    for u in range(27):
        out[:, UNITS[u]] &= new[:, u]
    return out


def fixpoint4(X, kmax=4, order="f3"):
    """F_4 of every row of the candidate sets X uint16[n,81] -> (F uint16[n,81], alternations): the
    largest number of subset passes any row needed."""
    if order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}")
    X = np.asarray(X, dtype=np.uint16).copy()
    live = np.ones(X.shape[0], dtype=bool)
    passes = 0
    if order == "f3":
        X = G.fixpoint(X, 3)
    while live.any():
        idx = np.flatnonzero(live)
        cur = X[idx]
        if order == "mixed":
            new = G._round(cur, True)
            new = subset_pass(new, kmax)
            new = _locked_pass(new, _closed(new))
        else:
            new = subset_pass(cur, kmax)
            same = (new == cur).all(axis=1)
            new[~same] = G.fixpoint(new[~same], 3)
        passes += 1
        X[idx] = new
        live[idx[(new == cur).all(axis=1)]] = False
    return X, passes


def open4_of(boards, level, kmax=4, order="f3"):
    """boards uint8[n,81] with their grade_model levels -> open4 uint8[n]."""
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    out = np.full(len(boards), NONE, dtype=np.uint8)
    rows = np.flatnonzero(np.asarray(level) == 4)
    if len(rows):
        F, _ = fixpoint4(G.candidates(boards[rows]), kmax, order)
        out[rows] = (~_closed(F)).sum(axis=1)
    return out


@functools.lru_cache(maxsize=None)
def pool():
    """(boards, sol, level, open, open4) of grade_model's pool, computed once; read-only."""
    boards, sol = G.make_pool()
    level, open_ = G.grade(boards)
    return _frozen(boards, sol, level, open_, open4_of(boards, level))


@functools.lru_cache(maxsize=None)
def minimal(n=2048):
    """(boards, sol, level, open, open4) of synth.make_minimal(n), computed once; read-only."""
    from distributed_sudoku_solver_amd import synth
    boards, sol = synth.make_minimal(n)
    level, open_ = G.grade(boards)
    return _frozen(boards, sol, level, open_, open4_of(boards, level))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays
