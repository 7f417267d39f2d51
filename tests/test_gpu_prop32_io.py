"""The propagation pass's per-group input and output (csrc/prop32_kernel.h: p32_load, p32_convert,
p32_digits, p32_store_group and the staging's byte map): the boards come in as one unaligned dword per
lane and board and the answers leave through a staging of one dword per cell triad, so these tests
look where that can go wrong -- a read past the batch, a neighbour's byte taken for the lane's own,
a byte of the answers in the wrong place."""
import functools

import numpy as np
import pytest

import prop_model as M
from distributed_sudoku_solver_amd import _lib as L
from prop_inputs import DEFAULT_LC, model_of, named_set

pytestmark = pytest.mark.gpu


@pytest.fixture
def p32(engine):
    """The engine with the pass on for batches of any size; every option a test may touch is put back."""
    old_min = engine.get_option(L.SDK_OPT_PROP32_MIN)
    try:
        engine.set_option(L.SDK_OPT_SOLVER, L.SDK_SOLVER_QUAD)
        engine.set_option(L.SDK_OPT_PROP32, 1)
        engine.set_option(L.SDK_OPT_PROP32_MIN, 1)
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
          f"listed {len(listed)} (inexact {(reason == M.R_INEXACT).sum()}); kernel undecided {und} listed {count}")
    assert und == count == len(listed), what
    order = np.argsort(idx, kind="stable")
    assert np.array_equal(idx[order], listed), what
    diff = np.flatnonzero((lgrids[order] != grids[listed]).any(axis=1))
    assert len(diff) == 0, (what, listed[diff][:8].tolist())
    solved, refuted = cls == M.SOLVED, cls == M.REFUTED
    assert (st[solved] == 1).all() and np.array_equal(out[solved], grids[solved]), what
    assert (st[refuted] == 0).all() and np.array_equal(out[refuted], boards[refuted]), what
    return listed


def search_only(engine, boards):
    engine.set_option(L.SDK_OPT_PROP32, 0)
    try:
        out, st, _ = engine.solve_batch(boards)
    finally:
        engine.set_option(L.SDK_OPT_PROP32, 1)
    assert engine.debug_p32_list(1)[0] == 0 and engine.get_option(L.SDK_OPT_PROP32_UNDECIDED) == 0
    return out, st


def _pick(kind, want, k):
    """The first k boards of a named set on which the model's class / reason test `want` holds."""
    boards, m = named_set(kind)[0], model_of(kind)
    i = np.flatnonzero(want(m))[:k]
    assert len(i) == k, (kind, k)
    return boards[i], i


# ----------------------------------------------------------------------- poison behind the input
POISON = 64


def _poison_boards(n):
    """Minimal and edge boards in turn, the last board one the model solves: a byte from behind the
    batch that leaks into its > 9 test turns it into a listed board."""
    a, b = named_set("minimal")[0], named_set("edge")[0]
    mix = np.empty((n + 1, 81), dtype=np.uint8)
    mix[0::2], mix[1::2] = a[:(n + 2) // 2], b[:(n + 1) // 2]
    mix = mix[:n]
    mix[n - 1] = _pick("minimal", lambda m: m[0] == M.SOLVED, 1)[0][0]
    return mix


@pytest.mark.parametrize("n", [64, 128, 192, 65, 127])
def test_pass_reads_nothing_behind_the_batch(p32, n):
    """The input buffer ends in 64 bytes of 0xFF right behind board n - 1 (a full last group for n = 64,
    128, 192; a ragged one for 65, 127): a dword load of the last board's last three cells that reached
    one byte further would see a value above 9 and list that board."""
    boards = _poison_boards(n)
    model = M.propagate_batch(boards)
    assert model[0][n - 1] == M.SOLVED
    pad = 64
    d_in, d_out, d_st = p32.alloc(n * 81 + POISON), p32.alloc((n + pad) * 81), p32.alloc(n + pad)
    try:
        d_in.upload(np.concatenate([boards.reshape(-1), np.full(POISON, 0xFF, dtype=np.uint8)]))
        d_out.upload(np.full((n + pad) * 81, 0xA5, dtype=np.uint8))
        d_st.upload(np.full(n + pad, 0x5A, dtype=np.int8))
        p32.solve_batch_dev(d_in, d_out, d_st, n)
        out = d_out.download(np.empty((n + pad, 81), dtype=np.uint8))
        st = d_st.download(np.empty(n + pad, dtype=np.int8))
        check_pass(p32, boards, model, out[:n], st[:n], f"poison n {n}")
    finally:
        for d in (d_in, d_out, d_st):
            d.free()
    assert (out[n:] == 0xA5).all() and (st[n:] == 0x5A).all()
    o0, s0 = search_only(p32, boards)
    assert np.array_equal(st[:n], s0) and np.array_equal(out[:n], o0)


# --------------------------------------------------------- inert attribution across boundaries
BAD_CELLS = (0, 2, 3, 78, 80)
BAD_VALUES = (10, 128, 255)


def _attribution_boards():
    """256 boards, clean ones (the model solves them) and boards whose only bad cell is cell 0, 2, 3, 78
    or 80 in turn, with a clean board right before a bad-cell-0 board and a bad-cell-80 board right before
    a clean one in slots 31/32 and 63/0 of a group.  Returns (boards, bad mask)."""
    clean, _ = _pick("30clue", lambda m: m[0] == M.SOLVED, 256)
    boards = clean.copy()
    bad = np.zeros(256, dtype=bool)
    combos = [(c, v) for v in BAD_VALUES for c in BAD_CELLS]

    def spoil(i, cell, value):
        boards[i, cell] = value
        bad[i] = True

    for k, i in enumerate(range(1, 256, 2)):
        spoil(i, *combos[k % len(combos)])
    # clean, then bad cell 0: slots 31 / 32 of group 0, slots 63 / 0 of groups 0 / 1
    for i, v in ((31, 10), (63, 255)):
        boards[i], bad[i] = clean[i], False
        spoil(i + 1, 0, v)
    # bad cell 80, then clean: slots 31 / 32 of group 1, slots 63 / 0 of groups 1 / 2
    for i, v in ((64 + 31, 128), (64 + 63, 10)):
        boards[i], bad[i] = clean[i], False
        spoil(i, 80, v)
        boards[i + 1], bad[i + 1] = clean[i + 1], False
    # and the same pairs with the other values, groups 2 / 3
    for i, v in ((128 + 31, 128), (128 + 63, 10)):
        boards[i], bad[i] = clean[i], False
        spoil(i + 1, 0, v)
    for i, v in ((192 + 31, 255),):
        boards[i], bad[i] = clean[i], False
        spoil(i, 80, v)
        boards[i + 1], bad[i + 1] = clean[i + 1], False
    return boards, bad


def test_pass_attributes_an_inert_given_to_its_own_board(p32):
    """Clean boards between boards with one value above 9: the byte next to a lane's three cells belongs
    to the next lane or the next board, and must not enter the lane's > 9 test.  Exactly the bad boards
    are listed, as they came; every clean one is solved."""
    boards, bad = _attribution_boards()
    assert 100 <= bad.sum() <= 156
    assert not bad[31] and bad[32] and boards[32, 0] > 9 and not bad[63] and bad[64] and boards[64, 0] > 9
    assert bad[95] and boards[95, 80] > 9 and not bad[96] and bad[127] and boards[127, 80] > 9 and not bad[128]
    model = M.propagate_batch(boards)
    assert (model[3][bad] == M.R_INEXACT).all() and (model[0][~bad] == M.SOLVED).all()
    assert np.array_equal(model[1][bad], boards[bad])
    out, st, _ = p32.solve_batch(boards)
    listed = check_pass(p32, boards, model, out, st, "inert attribution")
    assert np.array_equal(listed, np.flatnonzero(bad))
    assert (st[~bad] == 1).all()
    o0, s0 = search_only(p32, boards)
    assert np.array_equal(st, s0) and np.array_equal(out, o0)


# ------------------------------------------------------------ every byte position of the output
@functools.lru_cache(maxsize=None)
def _symmetries():
    """64 symmetric images of one 30-clue board that propagation solves -- the digits relabelled by a
    rotation, the grid transposed and its bands and stacks rotated -- and their solutions: together
    they put every digit at every cell."""
    (p,), i = _pick("30clue", lambda m: m[0] == M.SOLVED, 1)
    s = named_set("30clue")[1][i[0]]
    ps, ss = [], []
    for k in range(64):
        shift, geo = k % 9, k // 9
        imgs = []
        for g in (p, s):
            g = g.reshape(9, 9)
            if geo & 1:
                g = g.T
            g = np.roll(g, 3 * ((geo >> 1) & 1), axis=0)
            g = np.roll(g, 3 * ((geo >> 2) & 1), axis=1)
            imgs.append(np.where(g > 0, (g.astype(np.int64) - 1 + shift) % 9 + 1, 0).astype(np.uint8).reshape(81))
        ps.append(imgs[0])
        ss.append(imgs[1])
    ps, ss = np.array(ps), np.array(ss)
    ps.setflags(write=False)
    ss.setflags(write=False)
    assert len(np.unique(ps, axis=0)) == 64
    for d in range(1, 10):
        assert (ss == d).any(axis=0).all(), d
    return ps, ss


@pytest.mark.parametrize("n", [64, 63])
def test_pass_writes_every_digit_at_every_cell(p32, n):
    """One full group, and the same boards as a ragged group of 63: the answers equal the known
    solutions, whatever the digit and the cell."""
    ps, ss = _symmetries()
    boards, sol = ps[:n], ss[:n]
    for d in range(1, 10):
        assert (sol == d).any(axis=0).all(), d
    model = M.propagate_batch(boards)
    assert (model[0] == M.SOLVED).all() and np.array_equal(model[1], sol)
    out, st, _ = p32.solve_batch(boards)
    check_pass(p32, boards, model, out, st, f"symmetries n {n}")
    assert (st == 1).all() and np.array_equal(out, sol)


@pytest.mark.parametrize("n", [64, 63])
@pytest.mark.parametrize("swap", [False, True], ids=["refuted_first", "stuck_first"])
def test_pass_copies_rows_through_the_staging_map(p32, n, swap):
    """A refuted board (its input goes back through the staging) and a stuck one (its propagated grid
    goes from the staging to the list) in slots 0, 31, 32 and 63 of the group, each kind in each slot
    over the two cases, among the solved boards."""
    ps, _ = _symmetries()
    refuted, _ = _pick("broken", lambda m: m[3] == M.R_CONTRA, 2)
    stuck, _ = _pick("hard", lambda m: m[3] == M.R_STUCK, 2)
    boards = ps.copy()
    first, second = (stuck, refuted) if swap else (refuted, stuck)
    boards[0], boards[32] = first[0], first[1]
    boards[31], boards[63] = second[0], second[1]
    boards = boards[:n]
    model = M.propagate_batch(boards)
    gone = n < 64     # slot 63 holds the second kind's second board
    assert (model[3] == M.R_CONTRA).sum() == 2 - (gone and swap)
    assert (model[3] == M.R_STUCK).sum() == 2 - (gone and not swap)
    out, st, _ = p32.solve_batch(boards)
    listed = check_pass(p32, boards, model, out, st, f"row copies n {n} swap {swap}")
    assert len(listed) == (model[3] == M.R_STUCK).sum()
    o0, s0 = search_only(p32, boards)
    assert np.array_equal(st, s0) and np.array_equal(out, o0)
