"""The propagation pass (csrc/prop32_kernel.h) against a scalar model of its own rules
(prop_model.py), board by board: which boards it solves, refutes and leaves to the search, and the
grid it hands over for each of those -- what the end-to-end tests cannot see, because the search
repairs whatever the pass leaves open.  The model's own soundness is pinned on the CPU
(test_prop_model.py); sdk_debug_p32_list reads back the pass's list."""
import numpy as np
import pytest

import prop_model as M
from distributed_sudoku_solver_amd import synth, _lib as L
from distributed_sudoku_solver_amd.engine import ALL_DIGITS_MASK
from oracle import oracle as O
from prop_inputs import DEFAULT_LC, SNAPSHOT_STEPS, STEP_CAP, model_of, named_set

pytestmark = pytest.mark.gpu

ORDERS = [L.SDK_ORDER_LEX, L.SDK_ORDER_MRV_UNIQUE]
ORDER_IDS = ["lex", "mrv_unique"]


@pytest.fixture
def p32(engine):
    """The engine with the pass on for batches of any size; every option a test may touch is put back."""
    old_min = engine.get_option(L.SDK_OPT_PROP32_MIN)
    try:
        engine.set_option(L.SDK_OPT_SOLVER, L.SDK_SOLVER_QUAD)
        engine.set_option(L.SDK_OPT_PROP32, 1)
        engine.set_option(L.SDK_OPT_PROP32_MIN, 1)
        engine.p32_default_min = old_min
        yield engine
    finally:
        engine.set_option(L.SDK_OPT_PROP32, 1)
        engine.set_option(L.SDK_OPT_PROP32_MIN, old_min)
        engine.set_option(L.SDK_OPT_PROP32_LC, DEFAULT_LC)
        engine.set_option(L.SDK_OPT_PROP32_HANDOVER, 1)
        engine.set_option(L.SDK_OPT_PROP32_TAIL, 0)
        engine.set_option(L.SDK_OPT_NODE_BUDGET, 0)
        engine.set_option(L.SDK_OPT_ORDER, L.SDK_ORDER_LEX)


def check_pass(engine, boards, model, out, st, what=""):
    """Right after a solve of `boards` that ran the pass: its undecided count, its list (sorted by
    board index) and the final answers of the boards it decided, against the model.  Returns the
    listed indices."""
    cls, grids, steps, reason = model
    listed = np.flatnonzero(cls == M.LISTED)
    und = engine.get_option(L.SDK_OPT_PROP32_UNDECIDED)
    count, idx, lgrids = engine.debug_p32_list(len(boards))
    print(f"{what}: n {len(boards)} model solved {(cls == M.SOLVED).sum()} refuted {(cls == M.REFUTED).sum()} "
          f"(closed twice {(reason == M.R_DUP_CLOSED).sum()}) listed {len(listed)} (inexact "
          f"{(reason == M.R_INEXACT).sum()}, max_steps {(reason == M.R_MAX_STEPS).sum()}) max steps {steps.max()}; "
          f"kernel undecided {und} listed {count}")
    assert und == count == len(listed), what
    order = np.argsort(idx, kind="stable")
    assert np.array_equal(idx[order], listed), what
    diff = np.flatnonzero((lgrids[order] != grids[listed]).any(axis=1))
    assert len(diff) == 0, (what, listed[diff][:8].tolist())
    solved, refuted = cls == M.SOLVED, cls == M.REFUTED
    assert (st[solved] == 1).all() and np.array_equal(out[solved], grids[solved]), what
    assert (st[refuted] == 0).all() and np.array_equal(out[refuted], boards[refuted]), what
    return listed


def search_only(engine, boards, budget=None):
    engine.set_option(L.SDK_OPT_PROP32, 0)
    try:
        out, st, _ = engine.solve_batch(boards, budget=budget)
    finally:
        engine.set_option(L.SDK_OPT_PROP32, 1)
    assert engine.debug_p32_list(1)[0] == 0 and engine.get_option(L.SDK_OPT_PROP32_UNDECIDED) == 0
    return out, st


def solve_and_check(engine, boards, model, what, budget=None):
    out, st, _ = engine.solve_batch(boards, budget=budget)
    listed = check_pass(engine, boards, model, out, st, what)
    return out, st, listed


# ------------------------------------------------------------------------------ workload classes
@pytest.mark.parametrize("order", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("kind", ["minimal", "hard", "17clue", "30clue", "edge", "broken"])
def test_pass_matches_model_on_workload_classes(p32, kind, order):
    boards, sol = named_set(kind)
    model = model_of(kind)
    assert model[2].max() <= STEP_CAP
    p32.set_option(L.SDK_OPT_ORDER, order)
    out, st, _ = solve_and_check(p32, boards, model, f"{kind} order {order}")
    o0, s0 = search_only(p32, boards)
    assert np.array_equal(st, s0) and np.array_equal(out, o0)
    if sol is not None:
        assert (st == 1).all() and np.array_equal(out, sol)


# ------------------------------------------------------------------------------------- schedules
@pytest.mark.parametrize("lc", [1, 4, 7 | (1 << 8), 64])
@pytest.mark.parametrize("kind", ["minimal", "hard", "edge", "broken"])
def test_pass_matches_model_at_every_schedule(p32, kind, lc):
    """The model follows the schedule.  A schedule changes when a board is found stuck, never its class
    or grid -- up to a period of 64, where a board that needs two locked-candidates passes reaches
    max_steps first and is handed over as it stands then (test_prop_model.test_step_cap)."""
    boards, sol = named_set(kind)
    model, base = model_of(kind, lc), model_of(kind)
    if lc != 64:
        assert model[2].max() <= STEP_CAP
        assert np.array_equal(model[0], base[0]) and np.array_equal(model[1], base[1])
    p32.set_option(L.SDK_OPT_PROP32_LC, lc)
    out, st, _ = solve_and_check(p32, boards, model, f"{kind} lc {lc}")
    o0, s0 = search_only(p32, boards)
    assert np.array_equal(st, s0) and np.array_equal(out, o0)


# ------------------------------------------------------------------------------------- snapshots
@pytest.mark.parametrize("step", SNAPSHOT_STEPS)
@pytest.mark.parametrize("kind", ["minimal", "hard", "broken"])
def test_pass_matches_model_step_by_step(p32, kind, step):
    """At a fixpoint a dropped deduction is mostly made up for by a later one (a pass whose hidden single
    never fires through one box gives the same stuck grids on these sets), so the pass is also stopped
    early: with SDK_OPT_PROP32_TAIL = 64 | step << 8 every board still live at that step is handed over as
    it stands after it, whatever its group (at most 64 are live in any), and the listed grids are the
    model's state of that step."""
    boards, _ = named_set(kind)
    model = model_of(kind, tail_step=step)
    if kind != "broken":
        assert (model[3] == M.R_TAIL).sum() >= 100
    p32.set_option(L.SDK_OPT_PROP32_TAIL, 64 | (step << 8))
    out, st, _ = solve_and_check(p32, boards, model, f"{kind} snapshot at step {step}")
    o0, s0 = search_only(p32, boards)
    assert np.array_equal(st, s0) and np.array_equal(out, o0)


# ----------------------------------------------------------------------------------- no handover
@pytest.mark.parametrize("how", ["handover_off", "node_budget"])
@pytest.mark.parametrize("kind", ["minimal", "edge", "broken"])
def test_pass_without_handover_lists_inputs(p32, kind, how):
    """prop32_body: `handed` is empty without handover, so the closed-twice test at the end does not run:
    the boards it would refute stay on the list, and every listed board goes to the search as it came."""
    boards, _ = named_set(kind)
    with_h, without = model_of(kind), model_of(kind, handover=False)
    out1, st1, listed1 = solve_and_check(p32, boards, with_h, f"{kind} handover")
    budget = None
    if how == "handover_off":
        p32.set_option(L.SDK_OPT_PROP32_HANDOVER, 0)
    else:
        budget = 1000
    out0, st0, listed0 = solve_and_check(p32, boards, without, f"{kind} {how}", budget=budget)
    cnt, idx, lgrids = p32.debug_p32_list(len(boards))
    assert np.array_equal(lgrids, boards[idx])
    twice = np.flatnonzero(with_h[3] == M.R_DUP_CLOSED)
    assert np.array_equal(listed0, np.union1d(listed1, twice)) and not np.intersect1d(listed1, twice).size
    assert np.array_equal(without[0] == M.SOLVED, with_h[0] == M.SOLVED)
    if kind == "broken":
        assert len(twice) >= 20
    if budget is None:
        assert np.array_equal(st0, st1) and np.array_equal(out0, out1)
    else:
        # a budget hit comes back as its input; every other board as without a budget
        hit = st0 == L.SDK_BUDGET_HIT
        assert np.array_equal(st0[~hit], st1[~hit]) and np.array_equal(out0[~hit], out1[~hit])
        assert np.array_equal(out0[hit], boards[hit])
        assert not hit[without[0] != M.LISTED].any()


# ------------------------------------------------------------------------ ragged and tiny batches
def _mix():
    a, b = named_set("minimal")[0], named_set("edge")[0]
    mix = np.empty((130, 81), dtype=np.uint8)
    mix[0::2], mix[1::2] = a[:65], b[:65]
    return mix


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 63, 64, 65, 127, 129])
def test_pass_on_ragged_and_tiny_batches(p32, n):
    """A batch whose only (or last) group is ragged -- the nb < 64 load and store path, an empty second
    half for n <= 32 -- and nothing written past board n of the outputs."""
    boards = _mix()[:n]
    model = M.propagate_batch(boards)
    pad = 64
    d_in, d_out, d_st = p32.alloc(n * 81), p32.alloc((n + pad) * 81), p32.alloc(n + pad)
    try:
        d_in.upload(boards)
        d_out.upload(np.full((n + pad) * 81, 0xA5, dtype=np.uint8))
        d_st.upload(np.full(n + pad, 0x5A, dtype=np.int8))
        p32.solve_batch_dev(d_in, d_out, d_st, n)
        out = d_out.download(np.empty((n + pad, 81), dtype=np.uint8))
        st = d_st.download(np.empty(n + pad, dtype=np.int8))
        check_pass(p32, boards, model, out[:n], st[:n], f"ragged n {n}")
    finally:
        for d in (d_in, d_out, d_st):
            d.free()
    assert (out[n:] == 0xA5).all() and (st[n:] == 0x5A).all()
    o0, s0 = search_only(p32, boards)
    assert np.array_equal(st[:n], s0) and np.array_equal(out[:n], o0)


# ------------------------------------------------------------------------------------- every slot
def _slot_boards():
    """64 distinct boards of every class."""
    def pick(kind, mask_of, k):
        boards, m = named_set(kind)[0], model_of(kind)
        i = np.flatnonzero(mask_of(m))
        i = i[np.sort(np.unique(boards[i], axis=0, return_index=True)[1])][:k]     # (the edge set repeats boards)
        assert len(i) == k, (kind, k)
        return boards[i]
    b = np.concatenate([
        pick("minimal", lambda m: m[0] == M.SOLVED, 12), pick("minimal", lambda m: m[3] == M.R_STUCK, 12),
        pick("hard", lambda m: m[3] == M.R_STUCK, 11), pick("broken", lambda m: m[3] == M.R_CONTRA, 10),
        pick("broken", lambda m: m[3] == M.R_DUP_CLOSED, 6), pick("edge", lambda m: m[3] == M.R_INEXACT, 12),
        pick("edge", lambda m: m[3] == M.R_STUCK, 1)])     # (the empty board)
    assert b.shape == (64, 81) and len(np.unique(b, axis=0)) == 64
    return b


def test_pass_is_the_same_in_every_slot(p32):
    """Row r of a 64 x 64 batch holds the 64 boards rotated by r, so every board sits once in each slot
    of a group (bit of the slice, half, lane of the load and store): class, listed grid and final answer
    are the model's in every slot."""
    b64 = _slot_boards()
    m64 = M.propagate_batch(b64)
    assert set(m64[3].tolist()) >= {M.R_SOLVED, M.R_CONTRA, M.R_DUP_CLOSED, M.R_STUCK, M.R_INEXACT}
    src = ((np.arange(64)[None, :] + np.arange(64)[:, None]) % 64).reshape(-1)    # slot s of row r: board s + r
    boards = b64[src]
    model = tuple(a[src] for a in m64)
    out, st, _ = solve_and_check(p32, boards, model, "every slot")
    first = np.argsort(src, kind="stable").reshape(64, 64)        # row k: the 64 places of board k
    for k in range(64):
        assert (st[first[k]] == st[first[k][0]]).all(), k
        assert (out[first[k]] == out[first[k][0]]).all(), k
    o0, s0 = search_only(p32, b64)
    assert np.array_equal(st, s0[src]) and np.array_equal(out, o0[src])


# -------------------------------------------------------------------------- inert-given boundaries
INERT_VALUES = (10, 127, 128, 137, 255)


def _inert_boards():
    base = named_set("30clue")[0][0]
    boards = np.tile(base, (405, 1))
    for c in range(81):
        for k, v in enumerate(INERT_VALUES):
            boards[5 * c + k, c] = v
    return base, boards


def test_pass_lists_every_board_with_an_inert_given(p32):
    """A value above 9 in any cell (the bytewise test of the full group's load at 10, 127, 128, 137 and
    255, the per-row rescan, and the ragged group's rescan alone): the board goes to the search as it came."""
    base, boards = _inert_boards()
    ref_out, ref_st, _ = O.naive_solve_batch(boards, threads=8)
    for lo, hi in ((0, 405), (0, 384), (384, 405), (0, 37)):     # 405 = 6 x 64 + 21
        part = boards[lo:hi]
        model = M.propagate_batch(part)
        assert (model[3] == M.R_INEXACT).all() and np.array_equal(model[1], part)
        out, st, listed = solve_and_check(p32, part, model, f"inert [{lo}, {hi})")
        assert len(listed) == hi - lo
        assert np.array_equal(st == 1, ref_st[lo:hi] == 1) and np.array_equal(out, ref_out[lo:hi])


def test_pass_takes_a_nine_as_a_digit(p32):
    """The same boards with 9 in that cell are exact unless the 9 duplicates a given."""
    base, _ = _inert_boards()
    boards = np.tile(base, (81, 1))
    boards[np.arange(81), np.arange(81)] = 9
    dup = np.zeros(81, dtype=bool)
    for c in range(81):
        r, k = divmod(c, 9)
        others = boards[c].reshape(9, 9).copy()
        others[r, k] = 0
        dup[c] = 9 in others[r] or 9 in others[:, k] or 9 in others[3 * (r // 3):3 * (r // 3) + 3, 3 * (k // 3):3 * (k // 3) + 3]
    assert dup.any() and not dup.all()
    model = M.propagate_batch(boards)
    assert np.array_equal(model[3] == M.R_INEXACT, dup)
    out, st, _ = solve_and_check(p32, boards, model, "nines")
    ref_out, ref_st, _ = O.naive_solve_batch(boards, threads=8)
    assert np.array_equal(st == 1, ref_st == 1) and np.array_equal(out, ref_out)


# --------------------------------------------------------------------------------------- the gate
def test_pass_is_not_run_with_masks_or_work_counters(p32):
    """First-cell masks or work counters leave the batch to the search alone (launch_solve's gate): one
    timed span, an empty list, and the answers of the plain call, which runs the pass."""
    p32.set_option(L.SDK_OPT_PROP32_MIN, p32.p32_default_min)
    boards, sol = synth.make_17clue(4096 + 37, seed=6)
    assert len(boards) >= p32.p32_default_min

    def timed(**kw):
        p32.timer_reset()
        try:
            out, st, _ = p32.solve_batch(boards, **kw)
            _, spans = p32.timer_read()
        finally:
            p32.timer_stop()
        return out, st, spans, p32.debug_p32_list(len(boards))[0], p32.get_option(L.SDK_OPT_PROP32_UNDECIDED)

    out, st, spans, count, und = timed()
    assert spans == 2 and (count, und) == (0, 0)               # the pass decides every 17-clue board
    assert (st == 1).all() and np.array_equal(out, sol)
    masks = np.full(len(boards), ALL_DIGITS_MASK, dtype=np.uint16)
    hard = named_set("hard")[0][:200]
    for kw in (dict(masks=masks), dict(want_work=True)):
        # a pass that lists boards first, so that an empty list afterwards is not a leftover
        p32.set_option(L.SDK_OPT_PROP32_MIN, 1)
        p32.solve_batch(hard)
        assert p32.debug_p32_list(len(hard))[0] == (model_of("hard")[0][:200] == M.LISTED).sum() > 0
        p32.set_option(L.SDK_OPT_PROP32_MIN, p32.p32_default_min)
        o, s, spans, count, und = timed(**kw)
        assert spans == 1 and (count, und) == (0, 0), kw.keys()
        assert np.array_equal(s, st) and np.array_equal(o, out)
