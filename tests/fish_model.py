"""A plain model of the fish stage (csrc/fish_kernel.h): F_5 and `open5` of ONE board, restated from
include/sudoku_hip.h (sdk_fish_batch) on subsets_model's primitive.

For a digit d, M_d is the 9 x 9 bit matrix whose row r holds the columns c at which cell (r, c) still has
candidate d (closed cells included).
  row fish of size k      k rows of M_d whose union has at most k columns: every other row loses those
                          columns, i.e. the cells lose candidate d;
  column fish of size k   the same on the transpose of M_d.
Both are subsets_model.subset_removals -- the primitive of the naked and hidden subsets -- on a third kind of
slice of the candidate cube.  k = 2, 3, 4 are X-wing, swordfish and jellyfish; k = 1 is a line's hidden
single followed by N, which R4 has already.
R5 = R4 + {row and column fish of sizes 2..4, every digit}; F_5 is the state no rule of R5 changes.  `open5`
is the number of open cells of F_5 for a board of level 4, SDK_FISH_NONE = 0xFF for every other board.

A fish removes no digit of a completion and its premise survives further removals, so F_5 is one state
whatever the order of application; `order` picks between orders so that a test can pin that:
  "f4"      from F_4: a fish pass, then the R4 fixpoint again, until a fish pass changes nothing.  The R4
            fixpoint is subsets_model.fixpoint4 with order "f3", which starts with the R3 fixpoint: a fish can
            enable a locked candidate where no subset fires, and fixpoint4's order "input" -- made for a
            board's input row -- would end on its unchanged subset pass without looking at L;
  "fish"    a fish pass on the input's candidate sets first, then the R4 fixpoint and the same alternation;
  "mixed"   rounds of one N + H phase, one subset pass, one fish pass and one locked pass, from the input.
`kmax` bounds the size of the fish only; the subsets keep their sizes 1..4.

As in subsets_model.py everything is batched over boards only to be quick: a board's row of the result is
what the model gives for that board alone.
"""
import functools

import numpy as np

import grade_model as G
import subsets_model as S
from prop_model import _closed, _locked_pass

NONE = 0xFF
ORDERS = ("f4", "fish", "mixed")

# rows of synth.make_minimal(8192) (test_fish_model.py derives them again):
# the level-4 boards that close with fish and not without (open4 > 0, open5 == 0)
NEEDS_FISH_8192 = (343, 1708, 2051, 2238, 3933, 5032, 5421, 5629, 5748, 6230, 6922, 7438, 7957)
# the first boards whose F_5 differs between fish of sizes <= 2 and <= 4 (59 in all)
SWORDFISH_8192 = (36, 60, 254, 480, 876, 901, 1003, 1365)
# all the boards whose F_5 differs between fish of sizes <= 3 and <= 4
JELLYFISH_8192 = (3030, 3508, 4559, 6828)


def digit_matrix(X, d):
    """Candidate sets uint16[n,81] -> M_d uint16[n,9] for digit index d (0..8): bit c of row r."""
    bit = (np.asarray(X, dtype=np.uint16).reshape(-1, 9, 9) >> np.uint16(d)) & np.uint16(1)
    return (bit << np.arange(9, dtype=np.uint16)).sum(axis=2).astype(np.uint16)


def fish_removals(M, kmax=4):
    """M_d uint16[m,9] -> uint16[m,9]: the columns each row loses to the row and the column fish of sizes
    1..kmax, both from the state given."""
    M = np.asarray(M, dtype=np.uint16)
    return S.subset_removals(M, kmax) | S.transpose(S.subset_removals(S.transpose(M), kmax))


def fish_pass(X, kmax=4):
    """One pass of row and column fish of sizes 1..kmax over the nine digits of every row of X, all from X."""
    X = np.asarray(X, dtype=np.uint16)
    out = X.copy().reshape(-1, 9, 9)
    cols = np.arange(9, dtype=np.uint16)
    for d in range(9):
        rem = fish_removals(digit_matrix(X, d), kmax)
        lose = ((rem[:, :, None] >> cols) & 1).astype(np.uint16)        # [n, r, c]
        out &= ~(lose << np.uint16(d))
    return out.reshape(-1, 81)


def fixpoint5(X, kmax=4, order="f4"):
    """F_5 of every row of the candidate sets X uint16[n,81] -> (F uint16[n,81], alternations): the largest
    number of fish passes any row needed."""
    if order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}")
    X = np.asarray(X, dtype=np.uint16).copy()
    live = np.ones(X.shape[0], dtype=bool)
    passes = 0
    if order == "fish":
        X = fish_pass(X, kmax)
    if order != "mixed" and len(X):
        X, _ = S.fixpoint4(X, order="f3")
    while live.any():
        idx = np.flatnonzero(live)
        cur = X[idx]
        if order == "mixed":
            new = G._round(cur, True)
            new = S.subset_pass(new)
            new = fish_pass(new, kmax)
            new = _locked_pass(new, _closed(new))
        else:
            new = fish_pass(cur, kmax)
            same = (new == cur).all(axis=1)
            if (~same).any():
                new[~same], _ = S.fixpoint4(new[~same], order="f3")
        passes += 1
        X[idx] = new
        live[idx[(new == cur).all(axis=1)]] = False
    return X, passes


def open5_of(boards, level, kmax=4, order="f4"):
    """boards uint8[n,81] with their grade_model levels -> open5 uint8[n]."""
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    out = np.full(len(boards), NONE, dtype=np.uint8)
    rows = np.flatnonzero(np.asarray(level) == 4)
    if len(rows):
        F, _ = fixpoint5(G.candidates(boards[rows]), kmax, order)
        out[rows] = (~_closed(F)).sum(axis=1)
    return out


@functools.lru_cache(maxsize=None)
def pool():
    """(boards, sol, level, open, open4, open5) of grade_model's pool, computed once; read-only."""
    boards, sol, level, open_, open4 = S.pool()
    return S._frozen(boards, sol, level, open_, open4, open5_of(boards, level))


@functools.lru_cache(maxsize=None)
def minimal(n=2048):
    """(boards, sol, level, open, open4, open5) of synth.make_minimal(n), computed once; read-only."""
    boards, sol, level, open_, open4 = S.minimal(n)
    return S._frozen(boards, sol, level, open_, open4, open5_of(boards, level))
