"""The definition of the rating (include/sudoku_hip.h, sdk_rate_batch) pinned on the scalar model
(rate_model.py), with no GPU: the three ways to build the children agree, the key is the lowest
backdoor, the known extreme puzzles of the stream, and the invariance the kernel's tests lean on."""
import numpy as np
import pytest

import grade_model as G
import rate_model as R
from prop_model import _closed
from distributed_sudoku_solver_amd import synth


@pytest.fixture(scope="module")
def pool():
    return R.pool()


def test_variants_agree(pool):
    boards, sol, level, open_, backdoors, key = pool
    grades = G.grade_states(boards)
    for variant in ("open", "closed"):
        bd, k = R.rate(boards, sol, variant, grades=grades)
        assert np.array_equal(bd, backdoors), (variant, np.flatnonzero(bd != backdoors)[:8])
        assert np.array_equal(k, key), (variant, np.flatnonzero(k != key)[:8])


def test_other_levels_are_not_rated(pool):
    boards, sol, level, open_, backdoors, key = pool
    other = level != 4
    assert other.any() and (level == 4).sum() == 296
    assert (backdoors[other] == R.NONE).all() and (key[other] == R.NONE).all()
    assert (backdoors[~other] <= 64).all()


def test_key_is_the_lowest_backdoor(pool):
    boards, sol, level, open_, backdoors, key = pool
    kids, owner, cell = [], [], []
    for i in np.flatnonzero(level == 4):
        last = 80 if key[i] == R.NONE else key[i]
        cells = np.flatnonzero(boards[i, :last + 1] == 0)
        kids.append(R.children(boards[i], sol[i], cells))
        owner.append(np.full(len(cells), i))
        cell.append(cells)
        assert (key[i] == R.NONE) == (backdoors[i] == 0)
    kids, owner, cell = np.concatenate(kids), np.concatenate(owner), np.concatenate(cell)
    done = _closed(G.fixpoint(G.candidates(kids), 3)).all(axis=1)
    # the only closed child at or below the key is the key's own
    assert np.array_equal(cell[done], key[owner[done]])
    assert done.sum() == (backdoors[level == 4] > 0).sum()


def test_counts_spread(pool):
    boards, sol, level, open_, backdoors, key = pool
    counts = backdoors[level == 4]
    print("backdoors", counts.min(), "..", counts.max(), "distinct", len(np.unique(counts)))
    assert counts.min() == 1 and counts.max() == 42
    assert len(np.unique(counts)) >= 30


def test_the_zero_backdoor_puzzle():
    p, s = synth.make_minimal(1, lo=896)
    level, open_ = G.grade(p)
    assert level[0] == 4 and open_[0] == 50 and (p[0] != 0).sum() == 23
    bd, key = R.rate(p, s)
    assert bd[0] == 0 and key[0] == R.NONE


def test_one_backdoor_puzzles():
    p, s = synth.make_minimal(180)
    idx = [44, 94, 179]
    level, _ = G.grade(p[idx])
    assert (level == 4).all()
    bd, key = R.rate(p[idx], s[idx])
    assert bd.tolist() == [1, 1, 1]
    for i, k in zip(idx, key):
        assert p[i, k] == 0 and R.is_backdoor(p[i], s[i], k)


def test_filling_closed_cells_changes_nothing(pool):
    """Any grid between the input and F_3's closed cells has the input's rating."""
    boards, sol, level, open_, backdoors, key = pool
    _, _, F = G.grade_states(boards)
    rng = np.random.default_rng(3)
    rows = np.flatnonzero(level == 4)[:64]
    filled = boards[rows].copy()
    some = 0
    for r, i in enumerate(rows):
        free = np.flatnonzero(_closed(F[i:i + 1])[0] & (boards[i] == 0))
        take = free[rng.random(len(free)) < 0.5]
        filled[r, take] = sol[i, take]
        some += len(take)
    assert some > 0
    bd, k = R.rate(filled, sol[rows])
    assert np.array_equal(bd, backdoors[rows]) and np.array_equal(k, key[rows])
