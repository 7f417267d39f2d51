"""The propagation pass on batches in which every workgroup runs several groups of 64 boards, one
after another in the same LDS (csrc/prop32_kernel.h: the two halves' regions, the answers' staging
over them, the shared read-order table behind them).  The other prop32 tests' batches have at most
as many groups as the launch has workgroups (20 per CU), so none of their workgroups ever takes a
second group: a table entry or a record overwritten by one group's staging would go unseen there.

Every board is compared with its known solution; every status must be 1."""
import numpy as np
import pytest

from distributed_sudoku_solver_amd import synth, _lib as L

pytestmark = pytest.mark.gpu

N_17 = 1_000_037      # ~15,600 groups, about three per workgroup on 256 CUs; the last group is ragged
N_MIN = 1 << 20


@pytest.fixture
def quad(engine):
    old = engine.get_option(L.SDK_OPT_SOLVER)
    try:
        engine.set_option(L.SDK_OPT_SOLVER, L.SDK_SOLVER_QUAD)
        engine.set_option(L.SDK_OPT_PROP32, 1)
        yield engine
    finally:
        engine.set_option(L.SDK_OPT_PROP32, 1)
        engine.set_option(L.SDK_OPT_SOLVER, old)


@pytest.fixture(scope="module")
def minimal():
    return synth.make_minimal_sym(N_MIN, base=65536, threads=16)


def solve(engine, boards, prop32):
    engine.set_option(L.SDK_OPT_PROP32, prop32)
    try:
        out, st, _ = engine.solve_batch(boards)
    finally:
        engine.set_option(L.SDK_OPT_PROP32, 1)
    return out, st


def assert_solved(out, st, sol, what):
    bad = np.flatnonzero(st != 1)
    assert len(bad) == 0, (what, "status", bad[:8].tolist(), st[bad[:8]].tolist())
    diff = np.flatnonzero((out != sol).any(axis=1))
    assert len(diff) == 0, (what, "boards", diff[:8].tolist())


def test_17clue_several_groups_per_workgroup(quad):
    p, s = synth.make_17clue(N_17)
    assert len(p) == N_17 and N_17 % 64 != 0
    out, st = solve(quad, p, 1)
    assert_solved(out, st, s, "17-clue")


def test_minimal_several_groups_per_workgroup(quad, minimal):
    p, s = minimal
    assert len(p) == N_MIN
    out, st = solve(quad, p, 1)
    # the undecided list, the handover and the scatter ran: some boards went to the search
    assert quad.get_option(L.SDK_OPT_PROP32_UNDECIDED) > 0
    assert_solved(out, st, s, "minimal, pass on")
    out0, st0 = solve(quad, p, 0)
    assert_solved(out0, st0, s, "minimal, pass off")
    assert out.tobytes() == out0.tobytes() and st.tobytes() == st0.tobytes()
