"""How a group of the propagation pass ends (csrc/prop32_launch.hip, prop32_body's step; csrc/prop32_kernel.h,
p32_run and p32_decide), against the scalar model (prop_model.py), board by board: statuses, listed
indices, listed grids byte for byte, final answers.

The step that empties a group returns after its verdicts, without a cells phase: sound only because a
board declared stuck earlier in the group is at a fixpoint of the step (its handed-over grid is the one
it had then), and because a group ended by the tail hand-off does not take that exit (its grids carry
that step's cell update).  The step's two verdict words, "refuted" and "some cell open", are reduced
over the half in one chain that leaves one in the even and one in the odd rows of 16 lanes: boards
whose only signal comes from one lane, in either row, in either half."""
import functools

import numpy as np
import pytest

import prop_model as M
from distributed_sudoku_solver_amd import _lib as L
from prop_inputs import DEFAULT_LC, model_of, named_set
from test_gpu_prop32_model import check_pass, p32, search_only  # noqa: F401  (p32: the fixture)

pytestmark = pytest.mark.gpu

LC_FIRST, LC_EVERY = M.schedule(DEFAULT_LC)
EARLY = 3            # "several steps before": a stuck board leaves at least this many steps before the end


def run_and_check(engine, boards, model, what):
    """One solve with the pass: its list and answers against the model, and the final answers against
    the search alone."""
    out, st, _ = engine.solve_batch(boards)
    check_pass(engine, boards, model, out, st, what)
    o0, s0 = search_only(engine, boards)
    assert np.array_equal(st, s0) and np.array_equal(out, o0), what


# --------------------------------------------------------------------------- stuck, then solved
def _calls(step):
    """The calls of the group's step up to and with the verdicts of step `step`: the steps and the
    locked-candidates passes before it (p32_run unrolls two calls per iteration)."""
    return step + 1 + len(range(LC_FIRST, step + 1, LC_EVERY))


@functools.lru_cache(maxsize=None)
def stuck_then_solved():
    """(boards of five full groups, boards of two full groups and a ragged one of 37).  Every group:
    in each half a minimal or hard board that the model declares stuck at least EARLY steps before the
    group's last board, a 17-clue board, is solved."""
    def pool(kind, why):
        m = model_of(kind)
        i = np.flatnonzero(m[3] == why)
        return named_set(kind)[0][i], m[2][i]
    mn, mn_steps = pool("minimal", M.R_STUCK)
    hd, hd_steps = pool("hard", M.R_STUCK)
    sv, sv_steps = pool("17clue", M.R_SOLVED)
    mn, hd = mn[np.argsort(mn_steps, kind="stable")], hd[np.argsort(hd_steps, kind="stable")]   # stuck early first

    def group(k, size=64):
        # 17-clue boards, quick and slow as they come, none solved after step `end`, one of them at it:
        # the set's last step, or its last one that ends the group in the other copy of the unrolled step
        ends = np.unique(sv_steps)[::-1]
        end = ends[0] if k % 2 == 0 else next(e for e in ends if (_calls(int(e)) - _calls(int(ends[0]))) % 2)
        upto = np.flatnonzero(sv_steps <= end)
        g = sv[upto[(64 * k + np.arange(size)) % len(upto)]]
        g[16 + k] = sv[np.flatnonzero(sv_steps == end)[k]]
        # the stuck boards, at slots that move with k: two in half 0, two in half 1 (one past board 36
        # only in a full group)
        g[(3 * k) % 32] = mn[k]
        g[31 - k] = hd[k]
        g[32 + k % 5] = hd[8 + k]
        if size == 64:
            g[63 - 2 * k] = mn[8 + k]
        return g
    full = np.concatenate([group(k) for k in range(5)])
    ragged = np.concatenate([group(5), group(6), group(7, 37)])
    return full, ragged


def _groups(n):
    return [(lo, min(lo + 64, n)) for lo in range(0, n, 64)]


@pytest.mark.parametrize("which", ["full", "ragged"])
def test_stuck_boards_keep_their_grids_when_the_group_ends_solved(p32, which):
    """The case the skipped cells phase relies on: every group ends in the step that solves its last
    17-clue board, long after a board of each half was declared stuck -- which is handed over with the
    grid it had then.  Asserted from the model first, so the test cannot pass for want of such groups."""
    boards = stuck_then_solved()[which == "ragged"]
    model = M.propagate_batch(boards, LC_FIRST, LC_EVERY)
    cls, _, steps, reason = model
    assert len(boards) == (320 if which == "full" else 165)
    parities = set()
    for lo, hi in _groups(len(boards)):
        end = steps[lo:hi].max()
        last = np.flatnonzero(steps[lo:hi] == end) + lo
        assert (reason[last] == M.R_SOLVED).all(), (lo, "the group must end in the step that solves its last board")
        for h0, h1 in ((lo, min(lo + 32, hi)), (lo + 32, hi)):
            early = (reason[h0:h1] == M.R_STUCK) & (steps[h0:h1] + EARLY <= end)
            assert early.any(), (lo, h0, "no board stuck early in this half")
        parities.add(_calls(int(end)) % 2)
    assert parities == {0, 1}      # the exit is taken in both copies of the unrolled step
    run_and_check(p32, boards, model, f"stuck then solved, {which}")


# -------------------------------------------------------------------------- ended by hand-off
def _first_solved(boards):
    cls, _, steps, _ = M.propagate_batch(boards, LC_FIRST, LC_EVERY)
    return int(steps[cls == M.SOLVED].min())


@pytest.mark.parametrize("which", ["full", "ragged"])
@pytest.mark.parametrize("rel", [-1, 0, 1], ids=["before", "at", "after"])
def test_a_group_ended_by_the_tail_hands_over_that_steps_update(p32, rel, which):
    """SDK_OPT_PROP32_TAIL = 64 | step << 8 ends every group with a live board at `step`: the grids
    handed over are the model's after that step's cells phase.  (max_steps is no option: 96, past every
    board here.)"""
    boards = stuck_then_solved()[which == "ragged"]
    step = _first_solved(boards) + rel
    model = M.propagate_batch(boards, LC_FIRST, LC_EVERY, tail_step=step)
    cls, grids, steps, reason = model
    tail = reason == M.R_TAIL
    # (at the step after the first solved board some groups end solved, in that very step: no hand-off)
    ended = [bool(tail[lo:hi].any()) for lo, hi in _groups(len(boards))]
    assert all(ended) if rel <= 0 else any(ended), "groups must end by the hand-off"
    # the update is visible: some handed-over board closed a cell in that very step
    before = M.propagate_batch(boards[tail], LC_FIRST, LC_EVERY, tail_step=step - 1)
    assert step >= 1 and ((grids[tail] != 0).sum(axis=1) > (before[1] != 0).sum(axis=1)).any()
    if rel >= 0:
        assert (cls == M.SOLVED).any()
    p32.set_option(L.SDK_OPT_PROP32_TAIL, 64 | (step << 8))
    run_and_check(p32, boards, model, f"tail at step {step}, {which}")


# -------------------------------------------------------------------------------- verdict rows
def _complete_grids(n):
    sol = named_set("17clue")[1]
    return sol[:n].copy()


def _one_open(base, triad):
    """A complete grid with one cell of the triad opened: at step 0 the only open cell of the board."""
    b = base.copy()
    b[3 * triad + triad % 3] = 0
    return b


def _one_contradiction(unit, cell, seed):
    """Nine givens: the eight other cells of `unit` hold eight digits, the ninth digit stands in `cell`'s
    row or column outside the unit.  Step 0 leaves `cell` without a candidate and the unit without a
    cell for that digit; no given is duplicated."""
    rng = np.random.default_rng(seed)
    digits = rng.permutation(9) + 1
    b = np.zeros(81, dtype=np.uint8)
    others = [c for c in M.UNITS[unit] if c != cell]
    b[others] = digits[:8]
    r, k = divmod(cell, 9)
    line = [9 * r + j for j in range(9)] + [9 * i + k for i in range(9)]
    outside = [c for c in line if c not in set(M.UNITS[unit].tolist())]
    b[outside[rng.integers(len(outside))]] = digits[8]
    return b


def _signal_lanes(board, step):
    """The lanes (triad of an empty cell, unit that misses a digit) that report a contradiction, and
    the lanes (triads) with an open cell, at the verdicts of step `step` (before any locked pass)."""
    assert step < LC_FIRST
    X = np.where(board == 0, M.ALL, 1 << ((board.astype(np.int32) - 1) & 15)).astype(np.uint16)[None, :]
    for _ in range(step):
        closed = M._closed(X)
        T, twos, _, _ = M._unit_summary(X, closed)
        X = M._cells_phase(X, closed, T, twos)
    closed = M._closed(X)
    ones = M._unit_summary(X, closed)[2]
    bad = set((np.flatnonzero(X[0] == 0) // 3).tolist()) | set(np.flatnonzero(ones[0] != M.ALL).tolist())
    return bad, set((np.flatnonzero(~closed[0]) // 3).tolist())


@functools.lru_cache(maxsize=None)
def verdict_rows():
    """(boards, the step-1 contradictions' count): four groups --
      0: the 27 one-open boards in half 0 and again in half 1, among complete grids;
      1: contradictions signalled from lanes 0..15 only and from lanes 16..26 only, in both halves,
         among complete grids;
      2: 64 contradictions;  3: 64 complete grids."""
    done = _complete_grids(64)
    assert (M.propagate_batch(done)[2] == 0).all()
    opened = [_one_open(done[t], t) for t in range(27)]
    for t, b in enumerate(opened):
        assert _signal_lanes(b, 0) == (set(), {t})
    # row 0 of 16 lanes: a row unit r <= 4 (unit lane r, triad lanes 3r .. 3r + 2) or a column unit
    # k <= 6 with the cell in rows 0..4 (unit lane 9 + k <= 15); row 1: a box unit of the bottom band
    # (unit lanes 24..26, triad lanes 18..26) or a column unit k >= 7 with the cell in rows 6..8 (unit
    # lanes 16, 17)
    low = [(r, 9 * r + (2 * r + 1) % 9) for r in range(5)] + [(9 + k, 9 * (k % 5) + k) for k in range(7)]
    high = [(24 + b, 9 * (6 + b) + 3 * b + (b + 1) % 3) for b in range(3)] + \
           [(9 + k, 9 * (6 + i) + k) for k in (7, 8) for i in range(3)]
    lows = [_one_contradiction(u, c, 100 + i) for i, (u, c) in enumerate(low)]
    highs = [_one_contradiction(u, c, 200 + i) for i, (u, c) in enumerate(high)]
    for b in lows:
        bad, _ = _signal_lanes(b, 1)
        assert bad and max(bad) <= 15 and not _signal_lanes(b, 0)[0]
    for b in highs:
        bad, _ = _signal_lanes(b, 1)
        assert bad and 16 <= min(bad) and max(bad) <= 26 and not _signal_lanes(b, 0)[0]
    contra = np.array(lows + highs)                   # 12 + 9
    assert len(np.unique(contra, axis=0)) == len(contra) == 21
    g0 = done.copy()
    g0[0:27] = opened
    g0[37:64] = opened
    g1 = np.roll(done, 7, axis=0)
    g1[5:26] = contra
    g1[40:61] = contra[::-1]
    g2 = contra[np.arange(64) % 21]
    return np.concatenate([g0, g1, g2, np.roll(done, 13, axis=0)]), len(contra)


@pytest.mark.parametrize("tail", [None, 0, 1], ids=["to_the_end", "stop_at_0", "stop_at_1"])
def test_a_verdict_from_one_lane_of_either_row_reaches_the_board(p32, tail):
    """The open cell keeps its board from being taken as solved at step 0, the contradiction refutes
    its board at step 1 -- at exactly those steps: with the pass stopped there (tail) a board whose
    verdict came late is listed instead."""
    boards, ncontra = verdict_rows()
    model = M.propagate_batch(boards, LC_FIRST, LC_EVERY, tail_step=tail)
    cls, _, steps, reason = model
    assert ((reason == M.R_CONTRA) & (steps == 1)).sum() == (0 if tail == 0 else 2 * ncontra + 64)
    assert ((cls == M.SOLVED) & (steps == 0)).sum() == 10 + (64 - 2 * ncontra) + 64
    if tail is None:
        assert ((cls == M.SOLVED) & (steps == 1)).sum() == 54
    else:
        assert (reason == M.R_TAIL).sum() == (54 + 2 * ncontra + 64 if tail == 0 else 0)
        p32.set_option(L.SDK_OPT_PROP32_TAIL, 64 | (tail << 8))
    run_and_check(p32, boards, model, f"verdict rows, tail {tail}")
