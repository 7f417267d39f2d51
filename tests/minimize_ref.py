"""CPU reference for SudokuEngine.classify_batch / minimize_batch (test helper, not a test file).

verdict(): min(oracle.count(board, limit=2), 2) -- 0 none, 1 exactly one, 2 several.
minimize(): the greedy clue-removal loop of csrc/gen_minimal.c with a given cell order, over that
verdict: the result is a pure function of (board, order row), which is what makes the GPU
minimiser testable bit for bit.
"""
import numpy as np

from oracle import oracle as O


def verdict(board):
    return min(O.count(board, limit=2), 2)


def verdicts(boards):
    boards = np.asarray(boards, dtype=np.uint8).reshape(-1, 81)
    return np.array([verdict(b) for b in boards], dtype=np.int8)


def orders(n, seed):
    """n seeded cell orders, uint8[n,81], every row a permutation of 0..80."""
    rng = np.random.default_rng(seed)
    return rng.permuted(np.tile(np.arange(81, dtype=np.uint8), (n, 1)), axis=1)


def minimize_one(board, order):
    """(result uint8[81], verdict of the input).  A board that is not unique comes back unchanged;
    otherwise every non-zero cell, in `order`, is cleared and put back unless the board still has
    exactly one completion."""
    cur = np.array(board, dtype=np.uint8).reshape(81).copy()
    v = verdict(cur)
    if v != 1:
        return cur, v
    for cell in np.asarray(order).reshape(-1):
        cell = int(cell)
        if cur[cell] == 0:
            continue
        keep = cur[cell]
        cur[cell] = 0
        if verdict(cur) != 1:
            cur[cell] = keep
    return cur, v


def minimize(boards, order):
    """(results uint8[n,81], input verdicts int8[n]) of minimize_one over a batch."""
    boards = np.asarray(boards, dtype=np.uint8).reshape(-1, 81)
    order = np.asarray(order).reshape(-1, 81)
    out = np.empty_like(boards)
    st = np.empty(len(boards), dtype=np.int8)
    for i in range(len(boards)):
        out[i], st[i] = minimize_one(boards[i], order[i])
    return out, st


def is_minimal(board):
    """Unique, and no single clue can go."""
    board = np.asarray(board, dtype=np.uint8).reshape(81)
    if verdict(board) != 1:
        return False
    for cell in np.flatnonzero(board):
        b = board.copy()
        b[cell] = 0
        if verdict(b) == 1:
            return False
    return True
