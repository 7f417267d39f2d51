"""SudokuEngine.rate_batch (sdk_rate_batch; csrc/rate32_kernel.h): backdoor counts and keys against
the scalar model (rate_model.py), byte for byte, on grade_model's pool; the grade outputs against
grade_batch; the shapes of a probe group (one group is all the probes of one parent, so its shape is
the parent's number of empty cells); batches without work; broken boards, budgets, options, the device
form and what the call leaves behind.

Slices of 2^24 boards are not run here (see test_gpu_grade.py): the rate stage sits inside
launch_grade's slice loop, with the slice's own offsets, and every slice is a whole run of the path
tested below."""
import ctypes

import numpy as np
import pytest

import grade_model as G
import rate_model as R
import test_gpu_grade as TG
from prop_model import _closed
from distributed_sudoku_solver_amd import synth, _lib as L

pytestmark = pytest.mark.gpu

NONE = L.SDK_RATE_NONE


@pytest.fixture(scope="module")
def pool():
    """(boards, sol, model level, model open, model backdoors, model key), computed once."""
    return R.pool()


@pytest.fixture(scope="module")
def full(engine, pool):
    """rate_batch of the whole pool under default options."""
    return engine.rate_batch(pool[0])


def same(got, ref, n=None):
    assert len(got) == len(ref) == 6
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and np.array_equal(g, r[:n])


def test_pool_matches_model(engine, pool, full):
    boards, sol, level, open_, backdoors, key = pool
    st, lv, op, bd, ky, out = full
    rated = lv == 4
    print("level-4 boards", rated.sum(), "backdoors", bd[rated].min(), "..", bd[rated].max())
    assert bd.dtype == np.uint8 and ky.dtype == np.uint8
    assert np.array_equal(bd, backdoors), np.flatnonzero(bd != backdoors)[:8]
    assert np.array_equal(ky, key), np.flatnonzero(ky != key)[:8]
    assert (st == 1).all() and np.array_equal(out, sol)
    assert np.array_equal(lv, level) and np.array_equal(op, open_)
    gst, glv, gop, gout = engine.grade_batch(boards)
    assert np.array_equal(st, gst) and np.array_equal(lv, glv) and np.array_equal(op, gop)
    assert np.array_equal(out, gout)


@pytest.mark.parametrize("n", [1, 31, 33, 64, 65, 129])
def test_ragged_batches(engine, pool, full, n):
    """The number of parents is not tied to the board count."""
    same(engine.rate_batch(pool[0][:n]), full, n)


def fill_to(board, sol, closed, empties):
    """`board` with solution digits in F_3-closed empty cells (lowest first) until `empties` are left."""
    b = board.copy()
    free = np.flatnonzero(closed & (board == 0))
    take = int((board == 0).sum()) - empties
    assert 0 <= take <= len(free)
    b[free[:take]] = sol[free[:take]]
    assert (b == 0).sum() == empties
    return b


def test_group_shape_edges(engine, pool, full):
    """33, 32 and 31 empty cells -- the second half holds one probe, then none -- and exactly `open`
    of them, the fewest a board of that F_3 can have: the outputs are the unfilled board's and the
    model's (a cell closed in F_3 is never a backdoor, and filling it in changes no child's F_3)."""
    boards, sol, level, open_, backdoors, key = pool
    empties = (boards == 0).sum(axis=1)
    rows = np.flatnonzero((level == 4) & (open_ <= 31) & (empties >= 33))[:4]
    assert len(rows) == 4
    _, _, F = G.grade_states(boards[rows])
    variants, owner = [], []
    for r, i in enumerate(rows):
        closed = _closed(F[r:r + 1])[0]
        for e in (33, 32, 31, int(open_[i])):
            variants.append(fill_to(boards[i], sol[i], closed, e))
            owner.append(i)
    variants, owner = np.array(variants), np.array(owner)
    st, lv, op, bd, ky, out = engine.rate_batch(variants)
    assert (st == 1).all() and (lv == 4).all() and np.array_equal(out, sol[owner])
    assert np.array_equal(op, open_[owner])
    assert np.array_equal(bd, backdoors[owner]) and np.array_equal(ky, key[owner])
    assert np.array_equal(bd, full[3][owner]) and np.array_equal(ky, full[4][owner])
    mbd, mky = R.rate(variants, sol[owner])
    assert np.array_equal(bd, mbd) and np.array_equal(ky, mky)


def test_most_empties(engine, pool, full):
    """The other end: the pool's level-4 boards with the most empty cells, 60, alone in their batch.
    No uniquely solvable level-4 board with 61..64 empty cells exists in any of the project's sources
    (17-clue puzzles are solved by the techniques): probe slots 60..63 are covered only by the logic
    of the `valid` mask, which is the same expression for every count below 64."""
    boards, sol, level, open_, backdoors, key = pool
    empties = (boards == 0).sum(axis=1)
    assert empties[level == 4].max() == 60
    rows = np.flatnonzero((level == 4) & (empties == 60))
    st, lv, op, bd, ky, out = engine.rate_batch(boards[rows])
    assert (lv == 4).all()
    assert np.array_equal(bd, backdoors[rows]) and np.array_equal(ky, key[rows])


def test_batches_without_work(engine, pool):
    boards, sol, level, open_, backdoors, key = pool
    easy = boards[level == 1][:100]
    st, lv, op, bd, ky, out = engine.rate_batch(easy)
    assert (st == 1).all() and (lv == 1).all() and (bd == NONE).all() and (ky == NONE).all()
    changed = boards[:256].copy()
    for b, s in zip(changed, sol[:256]):      # one given changed: most such boards have no completion
        c = np.flatnonzero(b)[0]
        b[c] = s[c] % 9 + 1
    refuted = changed[engine.classify_batch(changed)[0] == 0]
    assert len(refuted) >= 65
    st, lv, op, bd, ky, out = engine.rate_batch(refuted)
    assert (st == 0).all() and (lv == 0).all() and (bd == NONE).all() and (ky == NONE).all()


def test_one_parent_sixty_four_times(engine, pool):
    boards, sol, level, open_, backdoors, key = pool
    i = np.flatnonzero(level == 4)[3]
    st, lv, op, bd, ky, out = engine.rate_batch(np.tile(boards[i], (64, 1)))
    assert (lv == 4).all() and (bd == backdoors[i]).all() and (ky == key[i]).all()


def test_extreme_puzzles(engine):
    """The stream's puzzle without a backdoor (it needs two guesses) and three with exactly one."""
    p, s = synth.make_minimal(897)
    idx = np.array([896, 44, 94, 179])
    mbd, mky = R.rate(p[idx], s[idx])
    assert mbd.tolist() == [0, 1, 1, 1] and mky[0] == NONE
    st, lv, op, bd, ky, out = engine.rate_batch(p[idx])
    assert (lv == 4).all() and op[0] == 50
    assert np.array_equal(bd, mbd) and np.array_equal(ky, mky)


def test_broken_boards(engine):
    """Inert and duplicated givens, several completions, none: grade's verdicts, and no rating."""
    boards = TG.mixed_pool()
    gst, glv, gop, gout = engine.grade_batch(boards)
    st, lv, op, bd, ky, out = engine.rate_batch(boards)
    assert np.array_equal(st, gst) and np.array_equal(lv, glv) and np.array_equal(op, gop)
    assert np.array_equal(out, gout)
    clean = np.array([TG.clean_givens(b) for b in boards])
    assert ((st == 1) & ~clean).any() and (st == 2).any() and (st == 0).any()
    other = lv != 4
    assert (bd[other] == NONE).all() and (ky[other] == NONE).all()
    rated = np.flatnonzero(~other)
    assert len(rated)
    mbd, mky = R.rate(boards[rated], out[rated])
    assert np.array_equal(bd[rated], mbd) and np.array_equal(ky[rated], mky)


def test_budget(engine, pool, full):
    """A budget hit is level 0, hence no rating; the boards the techniques solve keep their level.
    (Which level-4 boards run out depends on the boards sharing their wave: no count is asserted.)"""
    boards, sol, level, open_, backdoors, key = pool
    for budget in (2, 12, 40):
        st, lv, op, bd, ky, out = engine.rate_batch(boards, budget=budget)
        hit = st == -2
        print("budget", budget, ": hits", hit.sum(), "of", (level == 4).sum(), "level-4 boards")
        assert np.isin(st, (1, -2)).all() and (hit.any() or budget > 2)
        assert np.array_equal(lv == 0, hit) and (level[hit] == 4).all()
        assert (bd[hit] == NONE).all() and (ky[hit] == NONE).all() and (op[hit] == 0).all()
        assert np.array_equal(lv[~hit], level[~hit]) and np.array_equal(op[~hit], open_[~hit])
        assert np.array_equal(bd[~hit], backdoors[~hit]) and np.array_equal(ky[~hit], key[~hit])
        assert np.array_equal(out[hit], boards[hit]) and np.array_equal(out[~hit], sol[~hit])


def test_independent_of_pass_options_and_no_residue(engine, pool, full):
    boards = pool[0]
    before = engine.solve_batch(boards)
    keys = (L.SDK_OPT_PROP32, L.SDK_OPT_PROP32_LC, L.SDK_OPT_NODE_BUDGET, L.SDK_OPT_SOLVER, L.SDK_OPT_ORDER,
            L.SDK_OPT_DONATE)
    options = {k: engine.get_option(k) for k in keys}
    for key, value in ((L.SDK_OPT_PROP32, 0), (L.SDK_OPT_PROP32_LC, 1 | 1 << 8), (L.SDK_OPT_PROP32_LC, 7 | 2 << 8)):
        old = engine.get_option(key)
        try:
            engine.set_option(key, value)
            got = engine.rate_batch(boards)
            assert engine.get_option(key) == value
        finally:
            engine.set_option(key, old)
        same(got, full)
    assert {k: engine.get_option(k) for k in keys} == options
    after = engine.solve_batch(boards)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert (after[1] == 1).all()


def test_device_form(engine, pool, full):
    boards = pool[0][:129]
    n = len(boards)
    bufs = [engine.alloc(boards.nbytes + 16)] + [engine.alloc(n) for _ in range(5)]
    d_io, d_st, d_lv, d_op, d_bd, d_ky = bufs
    u8 = lambda d: d.download(np.empty(n, dtype=np.uint8))
    try:
        d_io.upload(boards)
        engine.rate_batch_dev(d_io, d_io, d_st, d_lv, d_bd, n, d_open=d_op, d_key=d_ky, budget=0)      # in place
        engine.synchronize()
        got = (d_st.download(np.empty(n, dtype=np.int8)), u8(d_lv), u8(d_op), u8(d_bd), u8(d_ky),
               d_io.download(np.empty_like(boards)))
        same(got, full, n)
        # no open counts and no keys wanted
        d_io.upload(boards)
        d_bd.upload(np.zeros(n, dtype=np.uint8))
        engine.rate_batch_dev(d_io, d_io, d_st, d_lv, d_bd, n, budget=0)
        engine.synchronize()
        assert np.array_equal(u8(d_lv), full[1][:n]) and np.array_equal(u8(d_bd), full[3][:n])
        # a misaligned input
        odd = ctypes.c_void_p(d_io.ptr.value + 1)
        rc = engine.lib.sdk_rate_batch_dev(engine.ctx, odd, d_io.ptr, d_st.ptr, d_lv.ptr, None, d_bd.ptr, None, n, 0)
        assert rc == L.SDK_EINVAL and b"aligned" in engine.lib.sdk_last_error()
    finally:
        for d in bufs:
            d.free()


def test_arguments(engine, pool, full):
    got = engine.rate_batch(np.zeros((0, 81), dtype=np.uint8))
    assert [a.shape for a in got] == [(0,)] * 5 + [(0, 81)]
    boards = np.ascontiguousarray(pool[0][:40])
    out, st = np.empty_like(boards), np.empty(40, dtype=np.int8)
    lv, bd = np.empty(40, dtype=np.uint8), np.empty(40, dtype=np.uint8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    good = [p(boards), p(out), p(st), p(lv), None, p(bd), None]
    for missing in (0, 1, 2, 3, 5):           # backdoors is required, like level
        args = list(good)
        args[missing] = None
        assert engine.lib.sdk_rate_batch(engine.ctx, *args, 40, 0) == L.SDK_EINVAL
    # open and key may be null
    assert engine.lib.sdk_rate_batch(engine.ctx, *good, 40, 0) == L.SDK_OK
    assert np.array_equal(lv, full[1][:40]) and np.array_equal(bd, full[3][:40]) and np.array_equal(out, full[5][:40])
    with pytest.raises(ValueError):
        engine.rate_batch(boards, budget=-1)


def test_one_timing_span(engine, pool):
    try:
        engine.timer_reset()
        engine.rate_batch(pool[0][:256])
        engine.synchronize()
        ms, spans = engine.timer_read()
        assert spans == 1 and ms > 0.0
    finally:
        engine.timer_stop()
