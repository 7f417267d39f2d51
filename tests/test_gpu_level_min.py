"""Level-minimal clue removal on the GPU (csrc/reduce32_kernel.h; sdk_minimize_level_batch,
sdk_generate_level) against its model (level_min_model.py), byte for byte, puzzles and statuses."""
import ctypes
import functools

import numpy as np
import pytest

import grade_model as G
import level_min_model as M
from distributed_sudoku_solver_amd import _lib as L
from distributed_sudoku_solver_amd import synth

pytestmark = pytest.mark.gpu

LEVELS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def puzzles():
    """(512 uniqueness-minimal puzzles, their model levels); read-only."""
    p, _ = synth.make_minimal(512)
    lv, _ = G.grade(p)
    p.setflags(write=False)
    return p, lv


def same(got, want, what=""):
    out, st = got
    ref, rst = want
    bad = np.flatnonzero((out != ref).any(axis=1) | (st != rst))
    assert len(bad) == 0, (what, bad[:8].tolist(), st[bad[:8]].tolist(), rst[bad[:8]].tolist())


@pytest.mark.parametrize("L_", LEVELS)
def test_stream_rows(engine, L_):
    """Rows 0..255 in their own orders: every level among the results, 21..29 clues, four groups."""
    g, o = M.stream_rows()
    ref = M.stream_reduced(L_)
    same(engine.minimize_level_batch(g, L_, o), ref, f"L {L_}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("L_", LEVELS)
def test_ragged_groups(engine, L_, n):
    g, o = M.stream_rows()
    ref, rst = M.stream_reduced(L_)
    same(engine.minimize_level_batch(g[:n], L_, o[:n]), (ref[:n], rst[:n]), f"L {L_} n {n}")


@pytest.mark.parametrize("shift", [1, 37])
@pytest.mark.parametrize("L_", LEVELS)
def test_a_row_does_not_depend_on_its_position(engine, L_, shift):
    g, o = M.stream_rows()
    ref, rst = M.stream_reduced(L_)
    roll = lambda a: np.roll(a[:130], shift, axis=0)
    same(engine.minimize_level_batch(roll(g), L_, roll(o)), (roll(ref), roll(rst)), f"L {L_} shift {shift}")


@pytest.mark.parametrize("which", ["identity", "reversed"])
@pytest.mark.parametrize("L_", LEVELS)
def test_other_orders(engine, L_, which):
    g, _ = M.stream_rows()
    same(engine.minimize_level_batch(g, L_, M.stream_orders(which)), M.stream_reduced(L_, which), f"L {L_} {which}")


@pytest.mark.parametrize("L_", LEVELS)
def test_minimal_puzzles(engine, L_):
    """512 uniqueness-minimal puzzles: those of level <= L are L-minimal already and come back with
    status 1, the others are not eligible; all unchanged."""
    p, lv = puzzles()
    assert (lv <= L_).any() and (lv > L_).any()
    order = np.tile(M.stream_rows()[1], (2, 1))
    same(engine.minimize_level_batch(p, L_, order), (p, (lv <= L_).astype(np.int8)), f"L {L_}")


def _mixed():
    """130 boards: level-3-minimal stream puzzles and full grids (eligible) with ineligible boards
    among them -- several completions, a duplicated given, givens of 10, 128 and 255 at cells 0, 2, 3,
    78, 80 (a lane's first and last byte, a board's first and last) -- in slots 0, 31, 32, 63 of a group
    and elsewhere.  Returns (boards, orders, the ineligible rows)."""
    g, o = M.stream_rows()
    boards = M.stream_reduced(3)[0][:130].copy()
    boards[1::5] = g[1:130:5]
    bad = []
    spots = [0, 31, 32, 63, 64, 70, 95, 96, 127, 128, 129, 5, 17, 44, 50]
    kinds = [("multi", 0), ("dup", 0), (10, 0), (128, 2), (255, 3), (10, 78), (128, 80), (255, 80), ("multi", 0),
             (255, 0), ("dup", 0), (10, 80), (128, 0), ("zero", 0), (255, 78)]
    for i, (kind, cell) in zip(spots, kinds):
        b = boards[i]
        if kind == "multi":
            b[np.flatnonzero(b)[:6]] = 0
        elif kind == "zero":
            b[:] = 0
        elif kind == "dup":
            r = np.flatnonzero(b[:9] == 0)
            if len(r):
                b[r[0]] = b[np.flatnonzero(b[:9])[0]]
            else:
                b[0] = b[1]
        else:
            b[cell] = kind
        bad.append(i)
    return boards, o[:130], np.array(sorted(bad))


def test_ineligible_boards(engine):
    boards, order, bad = _mixed()
    for L_ in LEVELS:
        ref, rst = M.reduce_level(boards, order, L_)
        assert (rst[bad] == 0).all() and np.array_equal(ref[bad], boards[bad])
        if L_ == 3:
            assert rst.sum() == len(boards) - len(bad)
        same(engine.minimize_level_batch(boards, L_, order), (ref, rst), f"L {L_}")


def _dev_run(engine, boards, order, L_, guard, in_place):
    """The device form over buffers with `guard` bytes of 0xFF behind each: (out, status) with the guards."""
    n = len(boards)
    poison = np.full(guard, 0xFF, dtype=np.uint8)
    d_in, d_ord, d_st = engine.alloc(n * 81 + guard), engine.alloc(n * 81 + guard), engine.alloc(n + guard)
    d_out = d_in if in_place else engine.alloc(n * 81 + guard)
    try:
        d_ord.upload(np.concatenate([order.reshape(-1), poison]))
        if not in_place:
            d_out.upload(np.full(n * 81 + guard, 0xFF, dtype=np.uint8))
        d_in.upload(np.concatenate([boards.reshape(-1), poison]))
        d_st.upload(np.full(n + guard, 0xFF, dtype=np.uint8).view(np.int8))
        engine.minimize_level_batch_dev(d_in, d_ord, L_, d_out, d_st, n)
        engine.synchronize()
        out = d_out.download(np.empty(n * 81 + guard, dtype=np.uint8))
        st = d_st.download(np.empty(n + guard, dtype=np.int8))
        back = d_in.download(np.empty(n * 81 + guard, dtype=np.uint8))
        ordb = d_ord.download(np.empty(n * 81 + guard, dtype=np.uint8))
    finally:
        for d in {d_in, d_ord, d_st, d_out}:
            d.free()
    assert (ordb[:n * 81] == order.reshape(-1)).all() and (ordb[n * 81:] == 0xFF).all()
    assert (back[n * 81:] == 0xFF).all()
    if not in_place:
        assert (back[:n * 81] == boards.reshape(-1)).all()
    return out, st


@pytest.mark.parametrize("n", [64, 65, 127])
def test_guard_bytes(engine, n):
    """0xFF behind in, order, out and status: none is written, and none is read as data -- the last
    board is eligible, which a byte above 9 taken for one of its cells would end."""
    g, o = M.stream_rows()
    ref, rst = M.stream_reduced(3)
    out, st = _dev_run(engine, g[:n], o[:n], 3, 64, False)
    assert (out[n * 81:] == 0xFF).all() and (st[n:] == -1).all()
    assert rst[n - 1] == 1
    same((out[:n * 81].reshape(n, 81), st[:n]), (ref[:n], rst[:n]), f"n {n}")


def test_device_form_in_place(engine):
    boards, order, _ = _mixed()
    ref, rst = M.reduce_level(boards, order, 2)
    out, st = _dev_run(engine, boards, order, 2, 64, True)
    n = len(boards)
    assert (out[n * 81:] == 0xFF).all() and (st[n:] == -1).all()
    same((out[:n * 81].reshape(n, 81), st[:n]), (ref, rst))


def test_device_form_takes_a_byte_above_80_as_no_cell(engine):
    g, o = M.stream_rows()
    order = o[:67].copy()
    order[:, ::2] = 200
    order[:, 5] = 81
    ref, rst = M.reduce_level(g[:67], order, 3)
    out, st = _dev_run(engine, g[:67], order, 3, 16, False)
    same((out[:67 * 81].reshape(67, 81), st[:67]), (ref, rst))


def test_bad_arguments(engine):
    g, o = M.stream_rows()
    g, o = np.ascontiguousarray(g[:4]), np.ascontiguousarray(o[:4])
    out, grids, st = np.empty_like(g), np.empty_like(g), np.empty(4, dtype=np.int8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    lib, ctx = engine.lib, engine.ctx
    for level in (0, 4, -1):
        assert lib.sdk_minimize_level_batch(ctx, p(g), p(o), level, p(out), p(st), 4) == L.SDK_EINVAL
        assert b"level" in lib.sdk_last_error()
        assert lib.sdk_generate_level(ctx, 1, 0, 4, level, p(out), p(grids), p(st)) == L.SDK_EINVAL
        with pytest.raises(ValueError):
            engine.minimize_level_batch(g, level, o)
        with pytest.raises(ValueError):
            engine.generate_level(4, level)
    d = engine.alloc(4 * 81)
    d_st = engine.alloc(4)
    try:
        for level in (0, 4):
            assert lib.sdk_minimize_level_batch_dev(ctx, d.ptr, d.ptr, level, d.ptr, d_st.ptr, 4) == L.SDK_EINVAL
            assert lib.sdk_generate_level_dev(ctx, 1, 0, 4, level, d.ptr, d.ptr, d_st.ptr) == L.SDK_EINVAL
    finally:
        d.free()
        d_st.free()
    repeated = o.copy()
    repeated[2, 5] = repeated[2, 6]
    assert lib.sdk_minimize_level_batch(ctx, p(g), p(repeated), 2, p(out), p(st), 4) == L.SDK_EINVAL
    assert b"permutation" in lib.sdk_last_error()
    with pytest.raises(ValueError):
        engine.minimize_level_batch(g, 2, repeated)
    assert lib.sdk_minimize_level_batch(ctx, p(g), None, 2, p(out), p(st), 4) == L.SDK_EINVAL
    assert lib.sdk_minimize_level_batch(ctx, p(g), p(o), 2, p(out), p(st), 0) == L.SDK_OK


@pytest.mark.parametrize("L_", LEVELS)
def test_generate_level(engine, L_):
    """The stream call is the grids, then the minimiser in their own orders; a row depends on its
    stream index only, not on the call's slice."""
    puz, grids, st = engine.generate_level(96, L_)
    g, o, _ = engine.generate_grids(96, want_order=True)
    assert np.array_equal(grids, g) and np.array_equal(g, M.stream_rows()[0][:96])
    same((puz, st), engine.minimize_level_batch(g, L_, o), "two calls")
    ref, rst = M.stream_reduced(L_)
    same((puz, st), (ref[:96], rst[:96]), "model")
    a, b = engine.generate_level(40, L_), engine.generate_level(56, L_, lo=40)
    assert np.array_equal(np.concatenate([a[0], b[0]]), puz) and np.array_equal(np.concatenate([a[1], b[1]]), grids)
    assert np.array_equal(np.concatenate([a[2], b[2]]), st)


@pytest.mark.parametrize("L_", LEVELS)
def test_grader_agrees(engine, L_):
    g, o = M.stream_rows()
    ref, _ = M.stream_reduced(L_)
    out, _ = engine.minimize_level_batch(g, L_, o)
    st, level, _, sol = engine.grade_batch(out)
    assert (st == 1).all() and np.array_equal(sol, g)
    assert (level <= L_).all() and (level >= 1).all()
    assert np.array_equal(level, G.grade(ref)[0])
