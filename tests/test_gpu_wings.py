"""SudokuEngine.wings_batch (sdk_wings_batch; csrc/wings_kernel.h): `open6` against the scalar model
(wings_model.py) on grade_model's pool and on make_minimal(2048), byte for byte; `open4` and `open5` against
fish_batch and the grade outputs against grade_batch; small and odd batch shapes (the dequeue of two entries
per wave, the idle half, the list's tail); every level-4 board of the pool alone and beside a wave-mate of
each kind, which pins the waiting logic of the tiers with all three columns; the board's position in the
batch; refusals; the device form in place and with each nullable column absent; what the call leaves behind
for fish_batch and subsets_batch.

Slices of 2^24 boards are not run here (see test_gpu_grade.py): the stage sits inside launch_grade's slice
loop, with the slice's own offsets, and every slice is a whole run of the path tested below."""
import ctypes

import numpy as np
import pytest

import test_gpu_grade as TG
import wings_model as W
from distributed_sudoku_solver_amd import _lib as L

pytestmark = pytest.mark.gpu

NONE = L.SDK_WINGS_NONE


@pytest.fixture(scope="module")
def pool():
    """(boards, sol, model level, open, open4, open5, open6), computed once."""
    return W.pool()


@pytest.fixture(scope="module")
def minimal():
    return W.minimal()


@pytest.fixture(scope="module")
def full(engine, pool):
    """wings_batch of the whole pool under default options."""
    return engine.wings_batch(pool[0])


def same(got, ref, n=None):
    assert len(got) == len(ref) == 7
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and np.array_equal(g, r[:n])


def against_model_fish_and_grade(engine, data, got):
    boards, sol, level, open_, open4, open5, open6 = data
    st, lv, op, o4, o5, o6, out = got
    assert o6.dtype == np.uint8 and np.array_equal(o6, open6), np.flatnonzero(o6 != open6)[:8]
    assert np.array_equal(o5, open5), np.flatnonzero(o5 != open5)[:8]
    assert np.array_equal(o4, open4), np.flatnonzero(o4 != open4)[:8]
    for col in (o4, o5, o6):
        assert np.array_equal(col == NONE, lv != 4)
    assert (st == 1).all() and np.array_equal(out, sol)
    assert np.array_equal(lv, level) and np.array_equal(op, open_)
    fst, flv, fop, fo4, fo5, fout = engine.fish_batch(boards)
    assert np.array_equal(o4, fo4) and np.array_equal(o5, fo5)
    gst, glv, gop, gout = engine.grade_batch(boards)
    assert np.array_equal(st, gst) and np.array_equal(lv, glv) and np.array_equal(op, gop)
    assert np.array_equal(out, gout)
    return lv, o5, o6


def test_pool_matches_model_fish_and_grade(engine, pool, full):
    assert NONE == 0xFF and len(pool[0]) == 1536
    lv, o5, o6 = against_model_fish_and_grade(engine, pool, full)
    need = (lv == 4) & (o5 > 0) & (o6 == 0)
    print("level-4 boards", (lv == 4).sum(), "closed with fish", (o5 == 0).sum(), "closed with wings and colouring",
          (o6 == 0).sum(), "need the new rules", need.sum())
    assert ((lv == 4).sum(), (o5 == 0).sum(), (o6 == 0).sum(), need.sum(), (o6 < o5).sum()) == (296, 39, 122, 83, 99)


def test_minimal_puzzles_match_model(engine, minimal):
    lv, o5, o6 = against_model_fish_and_grade(engine, minimal, engine.wings_batch(minimal[0]))
    need = (lv == 4) & (o5 > 0) & (o6 == 0)
    assert ((lv == 4).sum(), (o5 == 0).sum(), (o6 == 0).sum(), need.sum(), (o6 < o5).sum()) == (934, 145, 348, 203, 254)


def test_no_boards(engine):
    got = engine.wings_batch(np.zeros((0, 81), dtype=np.uint8))
    assert [a.shape for a in got] == [(0,)] * 6 + [(0, 81)]


@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_small_and_odd_batches(engine, pool, full, n):
    same(engine.wings_batch(pool[0][:n]), full, n)


@pytest.mark.parametrize("count", [1, 2, 3, 65])
def test_few_level4_boards(engine, pool, count):
    """The list holds `count` entries, nothing else in the batch: with 1 a half idles, with 3 and 65 the last
    wave's second half."""
    boards, sol, level, open_, open4, open5, open6 = pool
    rows = np.flatnonzero(level == 4)[-count:]
    st, lv, op, o4, o5, o6, out = engine.wings_batch(boards[rows])
    assert (lv == 4).all()
    assert np.array_equal(o4, open4[rows]) and np.array_equal(o5, open5[rows]) and np.array_equal(o6, open6[rows])


def mates(pool, minimal):
    """{kind: (boards, open4, open5, open6)}: the wave-mates, two of each kind, with the model's counts."""
    mb, _, mlevel, _, mo4, mo5, mo6 = minimal
    pb, _, plevel, _, po4, po5, po6 = pool

    def pick(data, rows):
        rows = np.asarray(rows)
        assert (data[2][rows] == 4).all()
        return data[0][rows], data[4][rows], data[5][rows], data[6][rows]

    def first(data, mask, k=2):
        rows = np.flatnonzero((data[2] == 4) & mask)[:k]
        assert len(rows) == k
        return pick(data, rows)

    kinds = {
        "open4 == 0": first(pool, po4 == 0),
        "needs fish": first(pool, (po4 > 0) & (po5 < po4)),
        "needs wings": pick(minimal, W.NEEDS_WINGS_2048),
        "needs colouring": pick(minimal, W.NEEDS_COLOUR_2048),
        "needs both": pick(minimal, W.NEEDS_BOTH_2048),
        "needs XYZ": pick(minimal, W.NEEDS_XYZ_2048),
        "stays open": first(pool, (po6 > 0) & (po6 == po5) & (po5 == po4)),
    }
    for kind in ("needs wings", "needs colouring", "needs both", "needs XYZ"):
        assert (kinds[kind][2] > 0).all() and (kinds[kind][3] == 0).all(), kind
    return kinds


def test_every_level4_board_alone_and_beside_each_kind_of_wave_mate(engine, pool, minimal):
    """A batch of level-4 boards only: the list is the batch in order, so entries 2 k and 2 k + 1 share a wave.
    Every level-4 board of the pool goes first and second beside a mate of each kind, and beside an idle half
    (a batch of one).  Each board's three counts are the model's whatever the other half of its wave needs: no
    wing or colouring removal reaches a board before its open4 and open5 are stored, and no board's tiers are
    held up for good by a mate that waits."""
    boards, sol, level, open_, open4, open5, open6 = pool
    rows = np.flatnonzero(level == 4)
    assert len(rows) == 296
    want = np.stack([open4[rows], open5[rows], open6[rows]], axis=1)
    for kind, (mb, m4, m5, m6) in mates(pool, minimal).items():
        for k in range(len(mb)):
            mate = np.array([m4[k], m5[k], m6[k]])
            for mate_first in (False, True):
                batch = np.empty((2 * len(rows), 81), dtype=np.uint8)
                batch[int(mate_first)::2] = boards[rows]
                batch[1 - int(mate_first)::2] = mb[k]
                st, lv, op, o4, o5, o6, out = engine.wings_batch(batch)
                assert (lv == 4).all(), kind
                got = np.stack([o4, o5, o6], axis=1)
                bad = np.flatnonzero((got[int(mate_first)::2] != want).any(axis=1))
                assert not len(bad), (kind, k, mate_first, rows[bad][:8])
                assert (got[1 - int(mate_first)::2] == mate).all(), (kind, k, mate_first)
    # alone: every one of them in a batch of one, the second half of its wave idle
    for k, i in enumerate(rows):
        st, lv, op, o4, o5, o6, out = engine.wings_batch(boards[i:i + 1])
        assert lv[0] == 4 and (int(o4[0]), int(o5[0]), int(o6[0])) == tuple(int(v) for v in want[k]), i


def test_position_does_not_matter(engine, pool, full):
    boards = pool[0]
    perm = np.random.default_rng(1).permutation(len(boards))
    same(engine.wings_batch(boards[perm]), tuple(a[perm] for a in full))


def test_batches_without_work(engine, pool):
    boards, sol, level = pool[:3]
    easy = boards[level != 4][:200]
    st, lv, op, o4, o5, o6, out = engine.wings_batch(easy)
    assert (st == 1).all() and (lv != 4).all() and (lv != 0).all()
    assert (o4 == NONE).all() and (o5 == NONE).all() and (o6 == NONE).all()


def test_broken_boards(engine):
    """Inert and duplicated givens, several completions, none: grade's verdicts, and no count."""
    boards = TG.mixed_pool()
    gst, glv, gop, gout = engine.grade_batch(boards)
    st, lv, op, o4, o5, o6, out = engine.wings_batch(boards)
    assert np.array_equal(st, gst) and np.array_equal(lv, glv) and np.array_equal(op, gop)
    assert np.array_equal(out, gout)
    clean = np.array([TG.clean_givens(b) for b in boards])
    assert ((st == 1) & ~clean).any() and (st == 2).any() and (st == 0).any()
    for col in (o4, o5, o6):
        assert (col[(st == 1) & ~clean] == NONE).all() and (col[st == 2] == NONE).all() and (col[st == 0] == NONE).all()
        assert np.array_equal(col == NONE, lv != 4)
    rows = np.flatnonzero(lv == 4)
    assert len(rows)
    assert np.array_equal(o6[rows], W.open6_of(boards[rows], lv[rows]))


def test_budget(engine, pool, full):
    """A budget hit is level 0, hence no count in any column; the other boards keep theirs."""
    boards, sol, level, open_, open4, open5, open6 = pool
    st, lv, op, o4, o5, o6, out = engine.wings_batch(boards, budget=2)
    hit = st == -2
    print("budget 2: hits", hit.sum(), "of", (level == 4).sum(), "level-4 boards")
    assert np.isin(st, (1, -2)).all() and hit.any()
    assert np.array_equal(lv == 0, hit) and (level[hit] == 4).all()
    for col, ref in ((o4, open4), (o5, open5), (o6, open6)):
        assert (col[hit] == NONE).all() and np.array_equal(col[~hit], ref[~hit])
    assert np.array_equal(lv[~hit], level[~hit]) and np.array_equal(out[~hit], sol[~hit])
    with pytest.raises(ValueError):
        engine.wings_batch(boards[:4], budget=-1)


def test_device_form_in_place_and_nullable_columns(engine, pool, full):
    boards = pool[0][:129]
    n = len(boards)
    bufs = [engine.alloc(boards.nbytes + 16)] + [engine.alloc(n) for _ in range(6)]
    d_io, d_st, d_lv, d_op, d_o4, d_o5, d_o6 = bufs
    u8 = lambda d: d.download(np.empty(n, dtype=np.uint8))
    try:
        d_io.upload(boards)
        engine.wings_batch_dev(d_io, d_io, d_st, d_lv, d_o6, n, d_open=d_op, d_open4=d_o4, d_open5=d_o5, budget=0)
        engine.synchronize()
        got = (d_st.download(np.empty(n, dtype=np.int8)), u8(d_lv), u8(d_op), u8(d_o4), u8(d_o5), u8(d_o6),
               d_io.download(np.empty_like(boards)))
        same(got, full, n)
        # each nullable column absent in turn, then all of them: an absent column's buffer is not written
        cols = {"d_open": (d_op, 2), "d_open4": (d_o4, 3), "d_open5": (d_o5, 4)}
        for absent in (("d_open",), ("d_open4",), ("d_open5",), ("d_open", "d_open4", "d_open5")):
            d_io.upload(boards)
            for d in (d_op, d_o4, d_o5, d_o6):
                d.upload(np.full(n, 0xEE, dtype=np.uint8))
            kw = {k: v[0] for k, v in cols.items() if k not in absent}
            engine.wings_batch_dev(d_io, d_io, d_st, d_lv, d_o6, n, budget=0, **kw)
            engine.synchronize()
            assert np.array_equal(u8(d_lv), full[1][:n]) and np.array_equal(u8(d_o6), full[5][:n]), absent
            for name, (d, at) in cols.items():
                assert (u8(d) == 0xEE).all() if name in absent else np.array_equal(u8(d), full[at][:n]), (absent, name)
        # required pointers, a misaligned input
        rc = engine.lib.sdk_wings_batch_dev(engine.ctx, d_io.ptr, d_io.ptr, d_st.ptr, d_lv.ptr, None, None, None, None, n, 0)
        assert rc == L.SDK_EINVAL
        odd = ctypes.c_void_p(d_io.ptr.value + 1)
        rc = engine.lib.sdk_wings_batch_dev(engine.ctx, odd, d_io.ptr, d_st.ptr, d_lv.ptr, None, None, None, d_o6.ptr, n, 0)
        assert rc == L.SDK_EINVAL and b"aligned" in engine.lib.sdk_last_error()
    finally:
        for d in bufs:
            d.free()


def test_host_form_with_null_columns(engine, pool, full):
    boards = np.ascontiguousarray(pool[0][:40])
    out, st = np.empty_like(boards), np.empty(40, dtype=np.int8)
    lv, o6 = np.empty(40, dtype=np.uint8), np.empty(40, dtype=np.uint8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    good = [p(boards), p(out), p(st), p(lv), None, None, None, p(o6)]
    for missing in (0, 1, 2, 3, 7):           # open6 is required, like level
        args = list(good)
        args[missing] = None
        assert engine.lib.sdk_wings_batch(engine.ctx, *args, 40, 0) == L.SDK_EINVAL
    assert engine.lib.sdk_wings_batch(engine.ctx, *good, 40, 0) == L.SDK_OK
    assert np.array_equal(lv, full[1][:40]) and np.array_equal(o6, full[5][:40]) and np.array_equal(out, full[6][:40])


def test_fish_and_subsets_are_the_same_before_and_after(engine, pool, full):
    boards = pool[0]
    fish_before, subsets_before = engine.fish_batch(boards), engine.subsets_batch(boards)
    same(engine.wings_batch(boards), full)
    for before, after in ((fish_before, engine.fish_batch(boards)), (subsets_before, engine.subsets_batch(boards))):
        assert len(before) == len(after)
        for x, y in zip(before, after):
            assert x.dtype == y.dtype and np.array_equal(x, y)


def test_one_timing_span(engine, pool):
    try:
        engine.timer_reset()
        engine.wings_batch(pool[0][:256])
        engine.synchronize()
        ms, spans = engine.timer_read()
        assert spans == 1 and ms > 0.0
    finally:
        engine.timer_stop()
