"""A plain model of the chains stage (csrc/chains_kernel.h): F_7 and `open7` of ONE board, restated from
include/sudoku_hip.h (sdk_chains_batch) on wings_model's F_6.

R7 = R6 + {X, Y} on the grader's candidate sets; F_7 is the state no rule of R7 changes.  `open7` is the
number of open cells of F_7 for a board of level 4, SDK_CHAINS_NONE = 0xFF for every other board.

X (X-chains, one digit d at a time).  The places of d are the cells that hold candidate d, closed cells
included (M_d of the fish, the colouring's places).  A link is a unit with exactly two places.  For every
open place s:
  ON starts as the other ends of the links through s;  until ON stops growing:
    OFF = the places that share a unit with a cell of ON,
    every link with exactly one end in OFF puts its other end into ON (s itself never goes into ON);
  for every t in ON either s or t holds d: every open cell that shares a unit with s and with t loses d.
Y (XY-chains).  For every bivalue cell s and each of its two digits z, a state (c, v) means "c is v".  The
start state is (s, the other digit of s).  From (c, v) the chain goes to every bivalue cell c2 != s that
shares a unit with c and holds v, in the state (c2, the other digit of c2).  For every reached state (c, z)
with c != s either s or c holds z: every open cell that shares a unit with s and with c loses z.

Both rules remove no digit of a completion, and a premise that further removals break becomes a single, so
F_7 should be one state whatever the order of application; `order` picks between orders so that a test can
pin that:
  "f6"      from F_6: an X + Y pass (both from one snapshot), then wings_model.fixpoint6 again, until a pass
            changes nothing.  This is the kernel's order;
  "split"   X (with R6) to its fixpoint, then Y (with R6) to its fixpoint, alternated until neither changes;
  "mixed"   fish_model's mixed rounds from the input's candidates with one W + C pass and one X + Y pass
            inside every round.
`x` and `xy` switch the two families off, for the per-family figures.

Cell sets are Python integers of 81 bits, a board at a time: this model is scalar on purpose.  The R6
fixpoints between the passes are wings_model's.
"""
import functools

import numpy as np

import fish_model as F
import grade_model as G
import subsets_model as S
import wings_model as W
from prop_model import _closed, _locked_pass
from wings_model import PEERS, UNIT_MASKS, _POP, _cells

NONE = 0xFF
ORDERS = ("f6", "split", "mixed")

# rows of synth.make_minimal(2048) (test_chains_model.py derives the properties again): level-4 boards with
# open6 > 0 that close with ...
NEEDS_X_2048 = (87, 105)          # X-chains alone, and not with XY-chains alone
NEEDS_XY_2048 = (12, 16)          # XY-chains alone, and not with X-chains alone
NEEDS_XANDXY_2048 = (197, 346)    # both families together only


def _seen(cells):
    """The cells that share a unit with a cell of the set (those cells included when a unit holds them)."""
    out = 0
    for c in _cells(cells):
        out |= PEERS[c] | 1 << c
    return out


def xchain_on(places, s):
    """The places of one digit and a start place s -> ON: the places that hold the digit if s does not."""
    links = [u & places for u in UNIT_MASKS if bin(u & places).count("1") == 2]
    start = 1 << s
    on = 0
    for ln in links:
        if ln & start:
            on |= ln & ~start
    while on:
        off = _seen(on) & places
        grown = on
        for ln in links:
            hit = ln & off
            if hit and hit != ln:
                grown |= ln & ~off & ~start
        if grown == on:
            break
        on = grown
    return on


def xchain_removals(x):
    """One board's candidate sets (81 ints) -> {cell: digits lost} to every X-chain of x."""
    lose = {}
    opened = sum(1 << c for c in range(81) if _POP[x[c]] != 1)
    for d in range(9):
        places = sum(1 << c for c in range(81) if x[c] >> d & 1)
        gone = 0
        for s in _cells(places & opened):
            for t in _cells(xchain_on(places, s)):
                gone |= PEERS[s] & PEERS[t]
        for t in _cells(gone & places & opened):
            lose[t] = lose.get(t, 0) | 1 << d
    return lose


def xychain_ends(x, s, z):
    """Candidate sets, a bivalue cell s and one of its digits z (a bit) -> the cells c != s with a reached
    state (c, z), as a cell set."""
    bivalue = sum(1 << c for c in range(81) if _POP[x[c]] == 2) & ~(1 << s)
    todo = [(s, x[s] & ~z)]
    reached = set(todo)
    ends = 0
    while todo:
        c, v = todo.pop()
        for c2 in _cells(PEERS[c] & bivalue):
            if x[c2] & v:
                nxt = (c2, x[c2] & ~v)
                if nxt not in reached:
                    reached.add(nxt)
                    todo.append(nxt)
                    if nxt[1] == z:
                        ends |= 1 << c2
    return ends


def xychain_removals(x):
    """One board's candidate sets -> {cell: digits lost} to every XY-chain of x."""
    lose = {}
    opened = sum(1 << c for c in range(81) if _POP[x[c]] != 1)
    for s in range(81):
        if _POP[x[s]] != 2:
            continue
        for z in (x[s] & -x[s], x[s] & (x[s] - 1)):
            targets = 0
            for c in _cells(xychain_ends(x, s, z)):
                targets |= PEERS[s] & PEERS[c]
            for t in _cells(targets & opened):
                if x[t] & z:
                    lose[t] = lose.get(t, 0) | z
    return lose


def chain_pass(X, x=True, xy=True):
    """One X + Y pass over every row of X uint16[n,81], both from X."""
    return W._apply(X, ([xchain_removals] if x else []) + ([xychain_removals] if xy else []))


def _alternate(X, step):
    """`step` (one pass, from a state at F_6) and wings_model.fixpoint6, until a pass changes nothing:
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
            new[~same], _ = W.fixpoint6(new[~same], order="f5")
        X[idx] = new
        passes[idx[~same]] += 1
        live[idx[same]] = False
    return X, passes


def fixpoint7(X, order="f6", x=True, xy=True):
    """F_7 of every row of the candidate sets X uint16[n,81] -> (F uint16[n,81], passes int[n]): the
    changing chain passes (order "f6"), alternations ("split") or rounds ("mixed") each row needed."""
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
            new = W.wide_pass(new)
            new = chain_pass(new, x, xy)
            new = _locked_pass(new, _closed(new))
            X[idx] = new
            same = (new == cur).all(axis=1)
            passes[idx[~same]] += 1
            live[idx[same]] = False
        return X, passes
    X, _ = W.fixpoint6(X, order="f5")
    if order == "f6":
        return _alternate(X, lambda cur: chain_pass(cur, x, xy))
    passes = np.zeros(len(X), dtype=np.int64)
    while True:
        before = X
        if x:
            X, _ = _alternate(X, lambda cur: chain_pass(cur, True, False))
        if xy:
            X, _ = _alternate(X, lambda cur: chain_pass(cur, False, True))
        changed = (X != before).any(axis=1)
        passes[changed] += 1
        if not changed.any():
            return X, passes


def open7_of(boards, level, order="f6", **rules):
    """boards uint8[n,81] with their grade_model levels -> open7 uint8[n]."""
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    out = np.full(len(boards), NONE, dtype=np.uint8)
    rows = np.flatnonzero(np.asarray(level) == 4)
    if len(rows):
        F7, _ = fixpoint7(G.candidates(boards[rows]), order, **rules)
        out[rows] = (~_closed(F7)).sum(axis=1)
    return out


@functools.lru_cache(maxsize=None)
def pool():
    """(boards, sol, level, open, open4, open5, open6, open7) of grade_model's pool, computed once; read-only."""
    boards, sol, level, open_, open4, open5, open6 = W.pool()
    return S._frozen(boards, sol, level, open_, open4, open5, open6, open7_of(boards, level))


@functools.lru_cache(maxsize=None)
def minimal(n=2048):
    """(boards, sol, level, open, open4, open5, open6, open7) of synth.make_minimal(n), computed once; read-only."""
    boards, sol, level, open_, open4, open5, open6 = W.minimal(n)
    return S._frozen(boards, sol, level, open_, open4, open5, open6, open7_of(boards, level))
