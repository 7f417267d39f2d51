"""SudokuEngine.chains_batch (sdk_chains_batch; csrc/chains_kernel.h): `open7` against the scalar model
(chains_model.py) on grade_model's pool and on make_minimal(2048), byte for byte; `open4`, `open5` and `open6`
against wings_batch and the grade outputs against grade_batch; small and odd batch shapes (the dequeue of two
entries per wave, the idle half, the list's tail); every level-4 board of the pool alone and beside a wave-mate
of each kind, which pins the waiting logic of the five tiers with all four columns; the board's position in the
batch; refusals; the device form in place and with each nullable column absent; what the call leaves behind
for wings_batch, fish_batch and subsets_batch.

Slices of 2^24 boards are not run here (see test_gpu_grade.py): the stage sits inside launch_grade's slice
loop, with the slice's own offsets, and every slice is a whole run of the path tested below."""
import ctypes

import numpy as np
import pytest

import chains_model as C
import test_gpu_grade as TG
import wings_model as W
from distributed_sudoku_solver_amd import _lib as L

pytestmark = pytest.mark.gpu

NONE = L.SDK_CHAINS_NONE


@pytest.fixture(scope="module")
def pool():
    """(boards, sol, model level, open, open4, open5, open6, open7), computed once."""
    return C.pool()


@pytest.fixture(scope="module")
def minimal():
    return C.minimal()


@pytest.fixture(scope="module")
def full(engine, pool):
    """chains_batch of the whole pool under default options."""
    return engine.chains_batch(pool[0])


def same(got, ref, n=None):
    assert len(got) == len(ref) == 8
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and np.array_equal(g, r[:n])


def against_model_wings_and_grade(engine, data, got):
    boards, sol, level, open_, open4, open5, open6, open7 = data
    st, lv, op, o4, o5, o6, o7, out = got
    assert o7.dtype == np.uint8 and np.array_equal(o7, open7), np.flatnonzero(o7 != open7)[:8]
    assert np.array_equal(o6, open6), np.flatnonzero(o6 != open6)[:8]
    assert np.array_equal(o5, open5), np.flatnonzero(o5 != open5)[:8]
    assert np.array_equal(o4, open4), np.flatnonzero(o4 != open4)[:8]
    for col in (o4, o5, o6, o7):
        assert np.array_equal(col == NONE, lv != 4)
    assert (st == 1).all() and np.array_equal(out, sol)
    assert np.array_equal(lv, level) and np.array_equal(op, open_)
    wst, wlv, wop, wo4, wo5, wo6, wout = engine.wings_batch(boards)
    assert np.array_equal(o4, wo4) and np.array_equal(o5, wo5) and np.array_equal(o6, wo6)
    gst, glv, gop, gout = engine.grade_batch(boards)
    assert np.array_equal(st, gst) and np.array_equal(lv, glv) and np.array_equal(op, gop)
    assert np.array_equal(out, gout)
    return lv, o6, o7


def line(lv, o6, o7):
    """(level-4 boards, open6 == 0, left open by F_6, changed open count, closed by chains, open7 == 0)"""
    four = lv == 4
    return (int(four.sum()), int((four & (o6 == 0)).sum()), int((four & (o6 > 0)).sum()), int((four & (o7 < o6)).sum()),
            int((four & (o6 > 0) & (o7 == 0)).sum()), int((four & (o7 == 0)).sum()))


def test_pool_matches_model_wings_and_grade(engine, pool, full):
    assert NONE == 0xFF and len(pool[0]) == 1536
    lv, o6, o7 = against_model_wings_and_grade(engine, pool, full)
    print("level-4, open6 == 0, open after F_6, fewer open cells, closed by chains, open7 == 0:", line(lv, o6, o7))
    assert line(lv, o6, o7) == (296, 122, 174, 86, 80, 202)


def test_minimal_puzzles_match_model(engine, minimal):
    lv, o6, o7 = against_model_wings_and_grade(engine, minimal, engine.chains_batch(minimal[0]))
    assert line(lv, o6, o7) == (934, 348, 586, 281, 248, 596)


def test_no_boards(engine):
    got = engine.chains_batch(np.zeros((0, 81), dtype=np.uint8))
    assert [a.shape for a in got] == [(0,)] * 7 + [(0, 81)]


@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_small_and_odd_batches(engine, pool, full, n):
    same(engine.chains_batch(pool[0][:n]), full, n)


@pytest.mark.parametrize("count", [1, 2, 3, 65])
def test_few_level4_boards(engine, pool, count):
    """The list holds `count` entries, nothing else in the batch: with 1 a half idles, with 3 and 65 the last
    wave's second half."""
    boards, sol, level, open_, open4, open5, open6, open7 = pool
    rows = np.flatnonzero(level == 4)[-count:]
    st, lv, op, o4, o5, o6, o7, out = engine.chains_batch(boards[rows])
    assert (lv == 4).all()
    assert np.array_equal(o4, open4[rows]) and np.array_equal(o5, open5[rows])
    assert np.array_equal(o6, open6[rows]) and np.array_equal(o7, open7[rows])


def mates(pool, minimal):
    """{kind: (boards, open4, open5, open6, open7)}: the wave-mates, two of each kind, with the model's counts."""
    po4, po5, po6, po7 = pool[4:8]

    def pick(data, rows):
        rows = np.asarray(rows)
        assert (data[2][rows] == 4).all()
        return (data[0][rows],) + tuple(data[k][rows] for k in (4, 5, 6, 7))

    def first(data, mask, k=2):
        rows = np.flatnonzero((data[2] == 4) & mask)[:k]
        assert len(rows) == k
        return pick(data, rows)

    kinds = {
        "open4 == 0": first(pool, po4 == 0),
        "needs fish": first(pool, (po4 > 0) & (po5 < po4)),
        "needs wings": pick(minimal, W.NEEDS_WINGS_2048),
        "needs colouring": pick(minimal, W.NEEDS_COLOUR_2048),
        "needs X-chains": pick(minimal, C.NEEDS_X_2048),
        "needs XY-chains": pick(minimal, C.NEEDS_XY_2048),
        "needs both": pick(minimal, C.NEEDS_XANDXY_2048),
        "stays open": first(pool, (po7 > 0) & (po7 == po6) & (po6 == po5) & (po5 == po4)),
    }
    for kind in ("needs wings", "needs colouring"):
        assert (kinds[kind][2] > 0).all() and (kinds[kind][3] == 0).all(), kind
    for kind in ("needs X-chains", "needs XY-chains", "needs both"):
        assert (kinds[kind][3] > 0).all() and (kinds[kind][4] == 0).all(), kind
    return kinds


def test_every_level4_board_alone_and_beside_each_kind_of_wave_mate(engine, pool, minimal):
    """A batch of level-4 boards only: the list is the batch in order, so entries 2 k and 2 k + 1 share a wave.
    Every level-4 board of the pool goes first and second beside a mate of each kind, and beside an idle half
    (a batch of one).  Each board's four counts are the model's whatever the other half of its wave needs: no
    chain removal reaches a board before its open4, open5 and open6 are stored, and no board's tiers are held
    up for good by a mate that waits."""
    boards, sol, level, open_, open4, open5, open6, open7 = pool
    rows = np.flatnonzero(level == 4)
    assert len(rows) == 296
    want = np.stack([open4[rows], open5[rows], open6[rows], open7[rows]], axis=1)
    for kind, (mb, m4, m5, m6, m7) in mates(pool, minimal).items():
        for k in range(len(mb)):
            mate = np.array([m4[k], m5[k], m6[k], m7[k]])
            for mate_first in (False, True):
                batch = np.empty((2 * len(rows), 81), dtype=np.uint8)
                batch[int(mate_first)::2] = boards[rows]
                batch[1 - int(mate_first)::2] = mb[k]
                st, lv, op, o4, o5, o6, o7, out = engine.chains_batch(batch)
                assert (lv == 4).all(), kind
                got = np.stack([o4, o5, o6, o7], axis=1)
                bad = np.flatnonzero((got[int(mate_first)::2] != want).any(axis=1))
                assert not len(bad), (kind, k, mate_first, rows[bad][:8])
                assert (got[1 - int(mate_first)::2] == mate).all(), (kind, k, mate_first)
    # alone: every one of them in a batch of one, the second half of its wave idle
    for k, i in enumerate(rows):
        st, lv, op, o4, o5, o6, o7, out = engine.chains_batch(boards[i:i + 1])
        assert lv[0] == 4 and (int(o4[0]), int(o5[0]), int(o6[0]), int(o7[0])) == tuple(int(v) for v in want[k]), i


def test_position_does_not_matter(engine, pool, full):
    boards = pool[0]
    perm = np.random.default_rng(1).permutation(len(boards))
    same(engine.chains_batch(boards[perm]), tuple(a[perm] for a in full))


def test_batches_without_work(engine, pool):
    boards, sol, level = pool[:3]
    easy = boards[level != 4][:200]
    st, lv, op, o4, o5, o6, o7, out = engine.chains_batch(easy)
    assert (st == 1).all() and (lv != 4).all() and (lv != 0).all()
    for col in (o4, o5, o6, o7):
        assert (col == NONE).all()


def test_broken_boards(engine):
    """Inert and duplicated givens, several completions, none: grade's verdicts, and no count."""
    boards = TG.mixed_pool()
    gst, glv, gop, gout = engine.grade_batch(boards)
    st, lv, op, o4, o5, o6, o7, out = engine.chains_batch(boards)
    assert np.array_equal(st, gst) and np.array_equal(lv, glv) and np.array_equal(op, gop)
    assert np.array_equal(out, gout)
    clean = np.array([TG.clean_givens(b) for b in boards])
    assert ((st == 1) & ~clean).any() and (st == 2).any() and (st == 0).any()
    for col in (o4, o5, o6, o7):
        assert (col[(st == 1) & ~clean] == NONE).all() and (col[st == 2] == NONE).all() and (col[st == 0] == NONE).all()
        assert np.array_equal(col == NONE, lv != 4)
    rows = np.flatnonzero(lv == 4)
    assert len(rows)
    assert np.array_equal(o7[rows], C.open7_of(boards[rows], lv[rows]))


def test_budget(engine, pool, full):
    """A budget hit is level 0, hence no count in any column; the other boards keep theirs."""
    boards, sol, level, open_, open4, open5, open6, open7 = pool
    st, lv, op, o4, o5, o6, o7, out = engine.chains_batch(boards, budget=2)
    hit = st == -2
    print("budget 2: hits", hit.sum(), "of", (level == 4).sum(), "level-4 boards")
    assert np.isin(st, (1, -2)).all() and hit.any()
    assert np.array_equal(lv == 0, hit) and (level[hit] == 4).all()
    for col, ref in ((o4, open4), (o5, open5), (o6, open6), (o7, open7)):
        assert (col[hit] == NONE).all() and np.array_equal(col[~hit], ref[~hit])
    assert np.array_equal(lv[~hit], level[~hit]) and np.array_equal(out[~hit], sol[~hit])
    with pytest.raises(ValueError):
        engine.chains_batch(boards[:4], budget=-1)


def test_device_form_in_place_and_nullable_columns(engine, pool, full):
    boards = pool[0][:129]
    n = len(boards)
    bufs = [engine.alloc(boards.nbytes + 16)] + [engine.alloc(n) for _ in range(7)]
    d_io, d_st, d_lv, d_op, d_o4, d_o5, d_o6, d_o7 = bufs
    u8 = lambda d: d.download(np.empty(n, dtype=np.uint8))
    try:
        d_io.upload(boards)
        engine.chains_batch_dev(d_io, d_io, d_st, d_lv, d_o7, n, d_open=d_op, d_open4=d_o4, d_open5=d_o5, d_open6=d_o6,
                                budget=0)
        engine.synchronize()
        got = (d_st.download(np.empty(n, dtype=np.int8)), u8(d_lv), u8(d_op), u8(d_o4), u8(d_o5), u8(d_o6), u8(d_o7),
               d_io.download(np.empty_like(boards)))
        same(got, full, n)
        # each nullable column absent in turn, then all of them: an absent column's buffer is not written
        cols = {"d_open": (d_op, 2), "d_open4": (d_o4, 3), "d_open5": (d_o5, 4), "d_open6": (d_o6, 5)}
        for absent in (("d_open",), ("d_open4",), ("d_open5",), ("d_open6",), tuple(cols)):
            d_io.upload(boards)
            for d in (d_op, d_o4, d_o5, d_o6, d_o7):
                d.upload(np.full(n, 0xEE, dtype=np.uint8))
            kw = {k: v[0] for k, v in cols.items() if k not in absent}
            engine.chains_batch_dev(d_io, d_io, d_st, d_lv, d_o7, n, budget=0, **kw)
            engine.synchronize()
            assert np.array_equal(u8(d_lv), full[1][:n]) and np.array_equal(u8(d_o7), full[6][:n]), absent
            for name, (d, at) in cols.items():
                assert (u8(d) == 0xEE).all() if name in absent else np.array_equal(u8(d), full[at][:n]), (absent, name)
        # required pointers, a misaligned input
        rc = engine.lib.sdk_chains_batch_dev(engine.ctx, d_io.ptr, d_io.ptr, d_st.ptr, d_lv.ptr, None, None, None, None,
                                             None, n, 0)
        assert rc == L.SDK_EINVAL
        odd = ctypes.c_void_p(d_io.ptr.value + 1)
        rc = engine.lib.sdk_chains_batch_dev(engine.ctx, odd, d_io.ptr, d_st.ptr, d_lv.ptr, None, None, None, None,
                                             d_o7.ptr, n, 0)
        assert rc == L.SDK_EINVAL and b"aligned" in engine.lib.sdk_last_error()
    finally:
        for d in bufs:
            d.free()


def test_host_form_with_null_columns(engine, pool, full):
    boards = np.ascontiguousarray(pool[0][:40])
    out, st = np.empty_like(boards), np.empty(40, dtype=np.int8)
    lv, o7 = np.empty(40, dtype=np.uint8), np.empty(40, dtype=np.uint8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    good = [p(boards), p(out), p(st), p(lv), None, None, None, None, p(o7)]
    for missing in (0, 1, 2, 3, 8):           # open7 is required, like level
        args = list(good)
        args[missing] = None
        assert engine.lib.sdk_chains_batch(engine.ctx, *args, 40, 0) == L.SDK_EINVAL
    assert engine.lib.sdk_chains_batch(engine.ctx, *good, 40, 0) == L.SDK_OK
    assert np.array_equal(lv, full[1][:40]) and np.array_equal(o7, full[6][:40]) and np.array_equal(out, full[7][:40])


def test_wings_fish_and_subsets_are_the_same_before_and_after(engine, pool, full):
    boards = pool[0]
    before = [engine.wings_batch(boards), engine.fish_batch(boards), engine.subsets_batch(boards)]
    same(engine.chains_batch(boards), full)
    after = [engine.wings_batch(boards), engine.fish_batch(boards), engine.subsets_batch(boards)]
    for b, a in zip(before, after):
        assert len(b) == len(a)
        for x, y in zip(b, a):
            assert x.dtype == y.dtype and np.array_equal(x, y)


def test_one_timing_span(engine, pool):
    try:
        engine.timer_reset()
        engine.chains_batch(pool[0][:256])
        engine.synchronize()
        ms, spans = engine.timer_read()
        assert spans == 1 and ms > 0.0
    finally:
        engine.timer_stop()
