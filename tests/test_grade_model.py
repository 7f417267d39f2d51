"""The scalar model of the grading pass (grade_model.py) on the pool the kernel is compared on
(test_gpu_grade.py): the grade does not depend on the order in which the rules are applied, a board
of level 1..3 ends as its known solution, and the pool holds every level.  Runs without a GPU."""
import numpy as np
import pytest

import grade_model as G
import prop_model as M
from distributed_sudoku_solver_amd import _lib as L


@pytest.fixture(scope="module")
def pool():
    return G.make_pool()


@pytest.fixture(scope="module")
def graded(pool):
    return G.grade_states(pool[0])


@pytest.mark.parametrize("schedule", ["locked", "restart"])
def test_schedules_agree(pool, graded, schedule):
    level, open_, F = G.grade_states(pool[0], schedule)
    assert np.array_equal(level, graded[0])
    assert np.array_equal(open_, graded[1])
    assert np.array_equal(F, graded[2])


def test_levels_1_to_3_are_the_boards_propagation_completes(pool, graded):
    boards, sol = pool
    level, _, F = graded
    X = G.candidates(boards)
    solution_sets = (1 << (sol.astype(np.int32) - 1)).astype(np.uint16)
    for k in (1, 2, 3):
        Fk = G.fixpoint(X, k)
        complete = M._closed(Fk).all(axis=1)
        assert np.array_equal(complete, level <= k), k
        assert np.array_equal(Fk[complete], solution_sets[complete]), k
        X = Fk
    done = level <= 3
    assert np.array_equal(F[done], solution_sets[done])
    # no rule removes a digit of the completion: the open boards still hold it
    assert ((F[~done] & solution_sets[~done]) == solution_sets[~done]).all()


def test_pool_holds_every_level(graded):
    level = graded[0]
    counts = np.bincount(level, minlength=5)
    print("levels 1..4:", counts[1:].tolist())
    assert counts[0] == 0 and (counts[1:] >= 8).all(), counts
    # every run of 32 boards (a half-wave of the kernel) mixes at least three levels
    assert all(len(set(h.tolist())) >= 3 for h in level.reshape(-1, 32))


def test_open_counts(graded):
    level, open_, F = graded
    assert (open_[level < 4] == 0).all()
    o = open_[level == 4]
    print("open:", o.min(), "..", o.max())
    assert (o >= 13).all() and (o <= 60).all(), (o.min(), o.max())
    assert np.array_equal(o, (~M._closed(F[level == 4])).sum(axis=1))


def test_binding_declares_the_grade_calls():
    for name in ("sdk_grade_batch", "sdk_grade_batch_dev"):
        assert name in L.SIGNATURES, name
    assert [L.SDK_GRADE_NONE, L.SDK_GRADE_NAKED, L.SDK_GRADE_HIDDEN, L.SDK_GRADE_LOCKED, L.SDK_GRADE_SEARCH] == \
        [0, 1, 2, 3, 4]
