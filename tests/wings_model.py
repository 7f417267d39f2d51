"""A plain model of the wings stage (csrc/wings_kernel.h): F_6 and `open6` of ONE board, restated from
include/sudoku_hip.h (sdk_wings_batch) on fish_model's F_5.

R6 = R5 + {W, C} on the grader's candidate sets; F_6 is the state no rule of R6 changes.  `open6` is the
number of open cells of F_6 for a board of level 4, SDK_WINGS_NONE = 0xFF for every other board.

W (wings).  The pivot p is an open cell with 2 or 3 candidates P.  The pincers q != r are bivalue cells,
each sharing a unit with p, with candidate sets Q != R and Q & R a single digit z.
  XY-wing    P == (Q | R) & ~z: every cell other than p, q, r that shares a unit with q and with r loses z;
  XYZ-wing   P == Q | R: every cell other than p, q, r that shares a unit with p, with q and with r loses z.
C (simple colouring, one digit d at a time).  The places of d are the cells that hold candidate d, closed
cells included (M_d of the fish).  A link is a unit with exactly two places.  The links make a graph on the
places; each connected component with at least one link is two-coloured.
  wrap       two places of one colour share a unit: every place of that colour loses d;
  trap       a place outside the component that shares a unit with a place of each colour loses d.
A component is grown as the kernel grows it: from the lowest uncoloured linked place, by closure over the
link units (a link with one end of a colour puts its other end into the other colour).

Both rules remove no digit of a completion, and a premise that further removals break is taken over by
singles, so F_6 should be one state whatever the order of application; `order` picks between orders so that
a test can pin that:
  "f5"      from F_5: a W + C pass (both from one snapshot), then fish_model.fixpoint5 again, until a pass
            changes nothing.  This is the kernel's order;
  "split"   W (with R5) to its fixpoint, then C (with R5) to its fixpoint, alternated until neither changes;
  "mixed"   fish_model's mixed rounds from the input's candidates with one W + C pass inside every round.
`wings`, `xyz`, `colour` and `wrap` switch parts of the rule set off, for the per-rule figures.

Cell sets are Python integers of 81 bits, a board at a time: this model is scalar on purpose.  The R5
fixpoints between the passes are fish_model's, batched over boards only to be quick.
"""
import functools

import numpy as np

import fish_model as F
import grade_model as G
import subsets_model as S
from prop_model import UNITS, _closed, _locked_pass

NONE = 0xFF
ORDERS = ("f5", "split", "mixed")

UNIT_MASKS = tuple(sum(1 << int(c) for c in u) for u in UNITS)                      # 27 cell sets
PEERS = tuple(functools.reduce(lambda a, b: a | b, (m for m in UNIT_MASKS if m >> c & 1)) & ~(1 << c)
              for c in range(81))
_POP = [bin(v).count("1") for v in range(512)]

# rows of synth.make_minimal(2048) (test_wings_model.py derives the properties again): level-4 boards with
# open5 > 0 that close with ...
NEEDS_WINGS_2048 = (21, 62)       # XY-wings alone, and not with colouring alone
NEEDS_COLOUR_2048 = (0, 24)       # colouring alone, and not with the wings alone
NEEDS_BOTH_2048 = (4, 67)         # both families together only
NEEDS_XYZ_2048 = (99, 199)        # the wings only when XYZ-wings are included


def _cells(mask):
    while mask:
        low = mask & -mask
        yield low.bit_length() - 1
        mask ^= low


def wing_removals(x, xyz=True):
    """One board's candidate sets (81 ints) -> {cell: digits lost} to every XY- (and XYZ-) wing of x."""
    lose = {}
    bivalue = [c for c in range(81) if _POP[x[c]] == 2]
    for p in range(81):
        P = x[p]
        if _POP[P] not in (2, 3):
            continue
        pincers = [q for q in bivalue if PEERS[p] >> q & 1]
        for i, q in enumerate(pincers):
            for r in pincers[i + 1:]:
                Q, R = x[q], x[r]
                z = Q & R
                if Q == R or _POP[z] != 1:
                    continue
                if P == (Q | R) & ~z:
                    targets = PEERS[q] & PEERS[r]
                elif xyz and P == Q | R:
                    targets = PEERS[p] & PEERS[q] & PEERS[r]
                else:
                    continue
                for t in _cells(targets & ~(1 << p | 1 << q | 1 << r)):
                    if x[t] & z:
                        lose[t] = lose.get(t, 0) | z
    return lose


def colour_components(places):
    """The places of one digit (an 81-bit cell set) -> [(A, B)]: the two colours of every component with
    at least one link, grown from the lowest uncoloured linked place."""
    links = [u & places for u in UNIT_MASKS if bin(u & places).count("1") == 2]
    linked = functools.reduce(lambda a, b: a | b, links, 0)
    out, done = [], 0
    while linked & ~done:
        rest = linked & ~done
        A, B = rest & -rest, 0
        while True:
            a, b = A, B
            for ln in links:
                if ln & A:
                    B |= ln & ~A
                if ln & B:
                    A |= ln & ~B
            if (a, b) == (A, B):
                break
        out.append((A, B))
        done |= A | B
    return out


def _seen(colour):
    return functools.reduce(lambda a, b: a | b, (u for u in UNIT_MASKS if u & colour), 0)


def colour_removals(x, wrap=True):
    """One board's candidate sets -> {cell: digits lost} to the traps (and wraps) of every digit."""
    lose = {}
    for d in range(9):
        places = sum(1 << c for c in range(81) if x[c] >> d & 1)
        gone = 0
        for A, B in colour_components(places):
            if wrap:
                for col in (A, B):
                    if any(bin(col & u).count("1") >= 2 for u in UNIT_MASKS):
                        gone |= col
            gone |= places & _seen(A) & _seen(B) & ~(A | B)
        for t in _cells(gone):
            lose[t] = lose.get(t, 0) | 1 << d
    return lose


def _apply(X, removals):
    out = np.asarray(X, dtype=np.uint16).copy()
    for i in range(len(out)):
        x = [int(v) for v in X[i]]
        for fn in removals:
            for t, bits in fn(x).items():
                out[i, t] &= np.uint16(~bits & 0x1FF)
    return out


def wing_pass(X, xyz=True):
    """One pass of XY- (and XYZ-) wings over every row of X uint16[n,81], all from X."""
    return _apply(X, [lambda x: wing_removals(x, xyz)])


def colour_pass(X, wrap=True):
    """One pass of simple colouring over the nine digits of every row of X, all from X."""
    return _apply(X, [lambda x: colour_removals(x, wrap)])


def wide_pass(X, wings=True, xyz=True, colour=True, wrap=True):
    """One W + C pass, both from X."""
    fns = ([lambda x: wing_removals(x, xyz)] if wings else []) + ([lambda x: colour_removals(x, wrap)] if colour else [])
    return _apply(X, fns)


def _alternate(X, step):
    """`step` (one pass, from a state at F_5) and fish_model.fixpoint5, until a pass changes nothing:
    -> (F, changing passes per row)."""
    X = np.asarray(X, dtype=np.uint16).copy()
    passes = np.zeros(len(X), dtype=np.int64)
    live = np.ones(len(X), dtype=bool)
    while live.any():
        idx = np.flatnonzero(live)
        cur = X[idx]
        new = step(cur)
        same = (new == cur).all(axis=1)
        if (~same).any():
            new[~same], _ = F.fixpoint5(new[~same], order="f4")
        X[idx] = new
        passes[idx[~same]] += 1
        live[idx[same]] = False
    return X, passes


def fixpoint6(X, order="f5", wings=True, xyz=True, colour=True, wrap=True):
    """F_6 of every row of the candidate sets X uint16[n,81] -> (F uint16[n,81], passes int[n]): the
    changing wide passes (order "f5"), alternations ("split") or rounds ("mixed") each row needed."""
    if order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}")
    X = np.asarray(X, dtype=np.uint16).copy()
    if not len(X):
        return X, np.zeros(0, dtype=np.int64)
    if order == "mixed":
        passes = np.zeros(len(X), dtype=np.int64)
        live = np.ones(len(X), dtype=bool)
        while live.any():
            idx = np.flatnonzero(live)
            cur = X[idx]
            new = G._round(cur, True)
            new = S.subset_pass(new)
            new = F.fish_pass(new)
            new = wide_pass(new, wings, xyz, colour, wrap)
            new = _locked_pass(new, _closed(new))
            X[idx] = new
            same = (new == cur).all(axis=1)
            passes[idx[~same]] += 1
            live[idx[same]] = False
        return X, passes
    X, _ = F.fixpoint5(X, order="f4")
    if order == "f5":
        return _alternate(X, lambda cur: wide_pass(cur, wings, xyz, colour, wrap))
    passes = np.zeros(len(X), dtype=np.int64)
    while True:
        before = X
        if wings:
            X, _ = _alternate(X, lambda cur: wing_pass(cur, xyz))
        if colour:
            X, _ = _alternate(X, lambda cur: colour_pass(cur, wrap))
        changed = (X != before).any(axis=1)
        passes[changed] += 1
        if not changed.any():
            return X, passes


def open6_of(boards, level, order="f5", **rules):
    """boards uint8[n,81] with their grade_model levels -> open6 uint8[n]."""
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    out = np.full(len(boards), NONE, dtype=np.uint8)
    rows = np.flatnonzero(np.asarray(level) == 4)
    if len(rows):
        F6, _ = fixpoint6(G.candidates(boards[rows]), order, **rules)
        out[rows] = (~_closed(F6)).sum(axis=1)
    return out


@functools.lru_cache(maxsize=None)
def pool():
    """(boards, sol, level, open, open4, open5, open6) of grade_model's pool, computed once; read-only."""
    boards, sol, level, open_, open4, open5 = F.pool()
    return S._frozen(boards, sol, level, open_, open4, open5, open6_of(boards, level))


@functools.lru_cache(maxsize=None)
def minimal(n=2048):
    """(boards, sol, level, open, open4, open5, open6) of synth.make_minimal(n), computed once; read-only."""
    boards, sol, level, open_, open4, open5 = F.minimal(n)
    return S._frozen(boards, sol, level, open_, open4, open5, open6_of(boards, level))
