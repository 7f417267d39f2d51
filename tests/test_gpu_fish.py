"""SudokuEngine.fish_batch (sdk_fish_batch; csrc/fish_kernel.h): `open5` against the scalar model
(fish_model.py) on grade_model's pool and on make_minimal(2048), byte for byte; `open4` against
subsets_batch and the grade outputs against grade_batch, also under other pass options; the 21 boards of
make_minimal(8192) that need a fish, a swordfish or a jellyfish; small and odd batch shapes (the dequeue of
two entries per wave, the idle half, the list's tail); batches without and with nothing but work; the
board's position in the batch, which pins that a wave-mate changes neither count; refusals; the device
form in place; what the call leaves behind.

Slices of 2^24 boards are not run here (see test_gpu_grade.py): the stage sits inside launch_grade's
slice loop, with the slice's own offsets, and every slice is a whole run of the path tested below."""
import ctypes

import numpy as np
import pytest

import fish_model as F
import grade_model as G
import test_gpu_grade as TG
from distributed_sudoku_solver_amd import _lib as L

pytestmark = pytest.mark.gpu

NONE = L.SDK_FISH_NONE


@pytest.fixture(scope="module")
def pool():
    """(boards, sol, model level, model open, model open4, model open5), computed once."""
    return F.pool()


@pytest.fixture(scope="module")
def full(engine, pool):
    """fish_batch of the whole pool under default options."""
    return engine.fish_batch(pool[0])


def same(got, ref, n=None):
    assert len(got) == len(ref) == 6
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and np.array_equal(g, r[:n])


def test_pool_matches_model_subsets_and_grade(engine, pool, full):
    boards, sol, level, open_, open4, open5 = pool
    st, lv, op, o4, o5, out = full
    assert NONE == 0xFF and o5.dtype == np.uint8 and o4.dtype == np.uint8
    assert np.array_equal(o5, open5), np.flatnonzero(o5 != open5)[:8]
    assert np.array_equal(o4, open4), np.flatnonzero(o4 != open4)[:8]
    assert np.array_equal(o5 == NONE, lv != 4) and np.array_equal(o4 == NONE, lv != 4)
    print("level-4 boards", (lv == 4).sum(), "closed by subsets", (o4 == 0).sum(), "closed with fish", (o5 == 0).sum(),
          "fewer open cells with fish", (o5 < o4).sum())
    assert (o4 == 0).sum() == 38 and (o5 == 0).sum() == 39 and (o5 < o4).sum() == 7
    assert (st == 1).all() and np.array_equal(out, sol)
    assert np.array_equal(lv, level) and np.array_equal(op, open_)
    sst, slv, sop, so4, sout = engine.subsets_batch(boards)
    assert np.array_equal(o4, so4) and np.array_equal(st, sst) and np.array_equal(out, sout)
    gst, glv, gop, gout = engine.grade_batch(boards)
    assert np.array_equal(st, gst) and np.array_equal(lv, glv) and np.array_equal(op, gop)
    assert np.array_equal(out, gout)


def test_minimal_puzzles_match_model(engine):
    boards, sol, level, open_, open4, open5 = F.minimal()
    st, lv, op, o4, o5, out = engine.fish_batch(boards)
    assert np.array_equal(o5, open5), np.flatnonzero(o5 != open5)[:8]
    assert np.array_equal(o4, open4), np.flatnonzero(o4 != open4)[:8]
    assert np.array_equal(o5 == NONE, lv != 4)
    assert np.array_equal(lv, level) and np.array_equal(op, open_) and np.array_equal(out, sol)
    assert (lv == 4).sum() == 934 and (o4 == 0).sum() == 143 and (o5 == 0).sum() == 145
    sst, slv, sop, so4, sout = engine.subsets_batch(boards)
    assert np.array_equal(o4, so4)


def test_boards_that_need_each_fish(engine):
    """The 21 boards of make_minimal(8192) at fish_model's rows: 13 that only a fish closes, the first 4
    whose F_5 needs a swordfish, the 4 that need a jellyfish.  open5 is compared with the model; the model
    also says which path of the kernel a board takes: how many deep rounds change it (fish passes that
    change F), and whether the table's entries of size 3 and 4 fire on a digit's matrix."""
    from distributed_sudoku_solver_amd import synth
    boards, sol = synth.make_minimal(8192)
    rows = np.array(F.NEEDS_FISH_8192 + F.SWORDFISH_8192[:4] + F.JELLYFISH_8192)
    assert len(rows) == 21
    boards = np.ascontiguousarray(boards[rows])
    level, open_ = G.grade(boards)
    assert (level == 4).all()
    X = G.candidates(boards)
    F5, passes = F.fixpoint5(X)
    F2, _ = F.fixpoint5(X, kmax=2)
    F3, _ = F.fixpoint5(X, kmax=3)
    ref = F.open5_of(boards, level)
    st, lv, op, o4, o5, out = engine.fish_batch(boards)
    for i, row in enumerate(rows):
        print("row", row, "open4", o4[i], "open5", o5[i], "needs size 3:", bool((F2[i] != F5[i]).any()),
              "needs size 4:", bool((F3[i] != F5[i]).any()))
    print("fish passes of the slowest board:", passes)
    assert (lv == 4).all() and np.array_equal(o5, ref) and np.array_equal(out, sol[rows])
    assert (o4[:13] > 0).all() and (o5[:13] == 0).all()
    assert (F2[13:17] != F5[13:17]).any(axis=1).all() and (F3[17:] != F5[17:]).any(axis=1).all()
    assert passes >= 2                                   # some board's fish pass changes it: deep rounds that change
    sst, slv, sop, so4, sout = engine.subsets_batch(boards)
    assert np.array_equal(o4, so4)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65])
def test_small_and_odd_batches(engine, pool, full, n):
    same(engine.fish_batch(pool[0][:n]), full, n)


@pytest.mark.parametrize("count", [1, 2, 3, 5])
def test_few_level4_boards(engine, pool, count):
    """The list holds `count` entries: one wave, its second half idle when the count is odd."""
    boards, sol, level, open_, open4, open5 = pool
    rows = np.flatnonzero(level == 4)[-count:]
    st, lv, op, o4, o5, out = engine.fish_batch(boards[rows])
    assert (lv == 4).all() and np.array_equal(o4, open4[rows]) and np.array_equal(o5, open5[rows])


def test_batches_without_work(engine, pool):
    boards, sol, level, open_, open4, open5 = pool
    easy = boards[level != 4][:200]
    st, lv, op, o4, o5, out = engine.fish_batch(easy)
    assert (st == 1).all() and (lv != 4).all() and (lv != 0).all() and (o4 == NONE).all() and (o5 == NONE).all()


def test_only_level4_boards(engine, pool):
    boards, sol, level, open_, open4, open5 = pool
    rows = np.flatnonzero(level == 4)
    st, lv, op, o4, o5, out = engine.fish_batch(boards[rows])
    assert (lv == 4).all() and np.array_equal(o5, open5[rows]) and np.array_equal(o4, open4[rows])
    assert np.array_equal(op, open_[rows])


def test_position_does_not_matter(engine, pool, full):
    """Two permutations of the pool: a board's half, wave-mate and place in the list change nothing, open4
    (taken before any fish removal, whatever the other half of the wave is doing) included."""
    boards = pool[0]
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(len(boards))
        got = engine.fish_batch(boards[perm])
        same(got, tuple(a[perm] for a in full))


def test_one_board_sixty_four_times(engine, pool):
    boards, sol, level, open_, open4, open5 = pool
    i = np.flatnonzero((level == 4) & (open5 < open4))[0]
    st, lv, op, o4, o5, out = engine.fish_batch(np.tile(boards[i], (64, 1)))
    assert (lv == 4).all() and (o4 == open4[i]).all() and (o5 == open5[i]).all()


def test_broken_boards(engine):
    """Inert and duplicated givens, several completions, none: grade's verdicts, and no count."""
    boards = TG.mixed_pool()
    gst, glv, gop, gout = engine.grade_batch(boards)
    st, lv, op, o4, o5, out = engine.fish_batch(boards)
    assert np.array_equal(st, gst) and np.array_equal(lv, glv) and np.array_equal(op, gop)
    assert np.array_equal(out, gout)
    clean = np.array([TG.clean_givens(b) for b in boards])
    assert ((st == 1) & ~clean).any() and (st == 2).any() and (st == 0).any()
    for col in (o4, o5):
        assert (col[(st == 1) & ~clean] == NONE).all() and (col[st == 2] == NONE).all() and (col[st == 0] == NONE).all()
        assert np.array_equal(col == NONE, lv != 4)
    rows = np.flatnonzero(lv == 4)
    assert len(rows)
    assert np.array_equal(o5[rows], F.open5_of(boards[rows], lv[rows]))


def test_budget(engine, pool, full):
    """A budget hit is level 0, hence no count in either column; the other boards keep theirs.  (Which
    level-4 boards run out depends on the boards sharing their wave: no count of hits is asserted.)"""
    boards, sol, level, open_, open4, open5 = pool
    for budget in (2, 12):
        st, lv, op, o4, o5, out = engine.fish_batch(boards, budget=budget)
        gst, glv, gop, gout = engine.grade_batch(boards, budget=budget)
        hit = st == -2
        print("budget", budget, ": hits", hit.sum(), "of", (level == 4).sum(), "level-4 boards")
        assert np.isin(st, (1, -2)).all() and (hit.any() or budget > 2)
        assert np.array_equal(lv == 0, hit) and (level[hit] == 4).all()
        assert (o5[hit] == NONE).all() and np.array_equal(o5[~hit], open5[~hit])
        assert (o4[hit] == NONE).all() and np.array_equal(o4[~hit], open4[~hit])
        assert np.array_equal(lv[~hit], level[~hit]) and np.array_equal(op[~hit], open_[~hit])
        assert np.array_equal(out[~hit], sol[~hit]) and np.array_equal(out[hit], boards[hit])
        assert np.array_equal(glv[gst != -2], level[gst != -2])


def test_same_as_grade_under_pass_options_and_no_residue(engine, pool, full):
    boards = pool[0]
    before = engine.solve_batch(boards)
    keys = (L.SDK_OPT_PROP32, L.SDK_OPT_PROP32_LC, L.SDK_OPT_NODE_BUDGET, L.SDK_OPT_SOLVER, L.SDK_OPT_ORDER,
            L.SDK_OPT_DONATE)
    options = {k: engine.get_option(k) for k in keys}
    for key, value in ((L.SDK_OPT_PROP32, 0), (L.SDK_OPT_PROP32_LC, 1 | 1 << 8), (L.SDK_OPT_PROP32_LC, 7 | 2 << 8)):
        old = engine.get_option(key)
        try:
            engine.set_option(key, value)
            got = engine.fish_batch(boards)
            gst, glv, gop, gout = engine.grade_batch(boards)
            assert engine.get_option(key) == value
        finally:
            engine.set_option(key, old)
        same(got, full)
        assert np.array_equal(got[0], gst) and np.array_equal(got[1], glv) and np.array_equal(got[2], gop)
        assert np.array_equal(got[5], gout)
    assert {k: engine.get_option(k) for k in keys} == options
    after = engine.solve_batch(boards)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert (after[1] == 1).all()


def test_device_form_in_place(engine, pool, full):
    boards = pool[0][:129]
    n = len(boards)
    bufs = [engine.alloc(boards.nbytes + 16)] + [engine.alloc(n) for _ in range(5)]
    d_io, d_st, d_lv, d_op, d_o4, d_o5 = bufs
    u8 = lambda d: d.download(np.empty(n, dtype=np.uint8))
    try:
        d_io.upload(boards)
        engine.fish_batch_dev(d_io, d_io, d_st, d_lv, d_o5, n, d_open=d_op, d_open4=d_o4, budget=0)   # in place
        engine.synchronize()
        got = (d_st.download(np.empty(n, dtype=np.int8)), u8(d_lv), u8(d_op), u8(d_o4), u8(d_o5),
               d_io.download(np.empty_like(boards)))
        same(got, full, n)
        # neither nullable column wanted: open4 goes to the context's own buffer
        d_io.upload(boards)
        d_o5.upload(np.zeros(n, dtype=np.uint8))
        d_o4.upload(np.full(n, 0xEE, dtype=np.uint8))
        engine.fish_batch_dev(d_io, d_io, d_st, d_lv, d_o5, n, budget=0)
        engine.synchronize()
        assert np.array_equal(u8(d_lv), full[1][:n]) and np.array_equal(u8(d_o5), full[4][:n])
        assert (u8(d_o4) == 0xEE).all()
        # a misaligned input
        odd = ctypes.c_void_p(d_io.ptr.value + 1)
        rc = engine.lib.sdk_fish_batch_dev(engine.ctx, odd, d_io.ptr, d_st.ptr, d_lv.ptr, None, None, d_o5.ptr, n, 0)
        assert rc == L.SDK_EINVAL and b"aligned" in engine.lib.sdk_last_error()
    finally:
        for d in bufs:
            d.free()


def test_arguments(engine, pool, full):
    got = engine.fish_batch(np.zeros((0, 81), dtype=np.uint8))
    assert [a.shape for a in got] == [(0,)] * 5 + [(0, 81)]
    boards = np.ascontiguousarray(pool[0][:40])
    out, st = np.empty_like(boards), np.empty(40, dtype=np.int8)
    lv, o5 = np.empty(40, dtype=np.uint8), np.empty(40, dtype=np.uint8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    good = [p(boards), p(out), p(st), p(lv), None, None, p(o5)]
    for missing in (0, 1, 2, 3, 6):           # open5 is required, like level
        args = list(good)
        args[missing] = None
        assert engine.lib.sdk_fish_batch(engine.ctx, *args, 40, 0) == L.SDK_EINVAL
    assert engine.lib.sdk_fish_batch(engine.ctx, *good, 40, 0) == L.SDK_OK      # open and open4 may be null
    assert np.array_equal(lv, full[1][:40]) and np.array_equal(o5, full[4][:40]) and np.array_equal(out, full[5][:40])
    with pytest.raises(ValueError):
        engine.fish_batch(boards, budget=-1)


def test_one_timing_span(engine, pool):
    try:
        engine.timer_reset()
        engine.fish_batch(pool[0][:256])
        engine.synchronize()
        ms, spans = engine.timer_read()
        assert spans == 1 and ms > 0.0
    finally:
        engine.timer_stop()
