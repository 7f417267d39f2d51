"""SudokuEngine.canonical_batch (sdk_canonical_batch; csrc/canon_kernel.h): every output against the plain
model (canon_model.py), byte for byte, on 128 boards -- graded puzzles of every level, 17-clue puzzles,
complete grids, the cyclic grid with its 54 automorphisms and puzzles on it, minimal puzzles; status and
solution against classify_batch; the properties that need no model on symmetric copies; small and odd
batch shapes and the board's position; broken boards; budgets; the device form in place; refusals; what
the call leaves behind.  The model costs about 30 ms per board, so it sees at most 128 boards per test.

Slices of 2^24 boards are not run here (see test_gpu_grade.py): a slice is a whole run of the path tested
below, with its own offsets."""
import ctypes

import numpy as np
import pytest

import canon_model as CM
import subsets_model as S
import test_gpu_grade as TG
from distributed_sudoku_solver_amd import _lib as L
from distributed_sudoku_solver_amd import synth

pytestmark = pytest.mark.gpu

NAMES = ("status", "canon", "solution", "gather", "relabel", "ties")


def same(got, ref, rows=slice(None)):
    assert len(got) == len(ref) == 6
    for name, g, r in zip(NAMES, got, ref):
        assert g.dtype == r.dtype and np.array_equal(g, r[rows]), name


def identity(got, rows, boards):
    """The rows come back unchanged, with the identity symmetry and no tie count."""
    st, canon, sol, g, rl, ties = got
    assert np.array_equal(canon[rows], boards[rows])
    assert (g[rows] == CM.IDENTITY_GATHER).all() and (rl[rows] == CM.IDENTITY_RELABEL).all()
    assert (ties[rows] == 0).all()


@pytest.fixture(scope="module")
def boards128():
    """(boards, completions) of the 128 boards the model sees."""
    rng = np.random.default_rng(31)
    pb, ps, level = S.pool()[:3]
    graded = np.concatenate([np.flatnonzero(level == k)[:12] for k in (1, 2, 3, 4)])
    assert len(graded) == 48
    p17, s17 = synth.make_17clue(16)
    pm, sm = synth.make_minimal(16 + 33, lo=4096)
    cyc = CM.cyclic_grid()
    on_cyc = np.stack([cyc, CM.cyclic_puzzle(CM.CYCLIC_BLANK_54), CM.cyclic_puzzle(CM.CYCLIC_BLANK_27)])
    g, rl = synth.random_symmetries(rng, 12)
    copies = synth.apply_symmetries(np.repeat(on_cyc, 4, axis=0), g, rl)
    copies_sol = synth.apply_symmetries(np.tile(cyc, (12, 1)), g, rl)
    boards = np.concatenate([pb[graded], p17, sm[:16], on_cyc, copies, pm[16:]]).astype(np.uint8)
    sols = np.concatenate([ps[graded], s17, sm[:16], np.tile(cyc, (3, 1)), copies_sol, sm[16:]]).astype(np.uint8)
    assert boards.shape == sols.shape == (128, 81)
    return np.ascontiguousarray(boards), np.ascontiguousarray(sols)


@pytest.fixture(scope="module")
def model128(boards128):
    return CM.canonical_rows(*boards128)


@pytest.fixture(scope="module")
def full128(engine, boards128):
    return engine.canonical_batch(boards128[0])


def test_matches_model(boards128, model128, full128):
    st, canon, sol, g, rl, ties = full128
    c, m, mg, mrl, mties = model128
    assert canon.dtype == sol.dtype == g.dtype == rl.dtype == np.uint8 and ties.dtype == np.uint16
    assert (st == 1).all()
    for name, got, ref in zip(NAMES[1:], (canon, sol, g, rl, ties), (c, m, mg, mrl, mties)):
        assert np.array_equal(got, ref), (name, np.flatnonzero((got != ref).reshape(128, -1).any(axis=1))[:8])
    print("ties", np.unique(ties, return_counts=True))
    assert (ties[80:95] == 54).all() and (ties[:80] >= 1).all()


def test_status_and_solution_are_classify(engine, boards128, full128):
    boards = np.concatenate([boards128[0], TG.mixed_pool()])
    cst, cout = engine.classify_batch(boards)
    st, canon, sol, g, rl, ties = engine.canonical_batch(boards)
    assert np.array_equal(st, cst)
    eligible = ties > 0
    assert np.array_equal(sol[~eligible], cout[~eligible])
    assert (st[eligible] == 1).all() and eligible[:128].all() and (~eligible).any()
    same(tuple(a[:128] for a in (st, canon, sol, g, rl, ties)), full128)


def test_symmetric_copies(engine):
    """make_minimal_sym(4096, base=64): row j is a random symmetric copy of base puzzle j % 64."""
    p, s = synth.make_minimal_sym(4096, base=64)
    st, canon, sol, g, rl, ties = engine.canonical_batch(p)
    assert (st == 1).all() and (ties >= 1).all()
    assert np.array_equal(canon, canon[np.arange(4096) % 64])
    assert np.array_equal(sol, sol[np.arange(4096) % 64])
    base_p, base_s = synth.make_minimal(64)
    mc = CM.canonical_rows(base_p, base_s)[0]
    assert len(np.unique(canon, axis=0)) == len(np.unique(mc, axis=0))
    assert np.array_equal(np.unique(canon, axis=0), np.unique(mc, axis=0))
    assert np.array_equal(synth.apply_symmetries(p, g.astype(np.int16), rl), canon)
    assert np.array_equal(synth.apply_symmetries(s, g.astype(np.int16), rl), sol)
    st2, canon2, sol2, g2, rl2, ties2 = engine.canonical_batch(canon)
    assert (st2 == 1).all() and np.array_equal(canon2, canon) and np.array_equal(sol2, sol)
    assert (g2 == CM.IDENTITY_GATHER).all() and (rl2 == CM.IDENTITY_RELABEL).all() and np.array_equal(ties2, ties)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65])
def test_small_and_odd_batches(engine, boards128, full128, n):
    same(engine.canonical_batch(boards128[0][-n:]), full128, slice(128 - n, None))


def test_position_does_not_matter(engine, boards128, full128):
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(128)
        same(engine.canonical_batch(boards128[0][perm]), tuple(a[perm] for a in full128))


def test_one_tie_board_sixty_four_times(engine, boards128, full128):
    i = 82            # the cyclic grid without cells 0, 10, 20: 54 ties, two symmetries attain C
    assert full128[5][i] == 54
    got = engine.canonical_batch(np.tile(boards128[0][i], (64, 1)))
    same(got, tuple(np.tile(a[i], (64,) + (1,) * (a.ndim - 1)) for a in full128))


def test_broken_boards(engine):
    """Inert and duplicated givens with exactly one completion, no completion, several: the input comes
    back, with the identity symmetry and ties 0.  The first 64 eligible rows against the model."""
    boards = TG.mixed_pool()
    cst, cout = engine.classify_batch(boards)
    got = engine.canonical_batch(boards)
    st, canon, sol, g, rl, ties = got
    clean = np.array([TG.clean_givens(b) for b in boards])
    assert np.array_equal(st, cst)
    assert ((st == 1) & ~clean).any() and (st == 0).any() and (st == 2).any()
    eligible = (st == 1) & clean
    identity(got, ~eligible, boards)
    assert np.array_equal(sol[~eligible], cout[~eligible])
    assert (ties[eligible] >= 1).all()
    rows = np.flatnonzero(eligible)[:64]
    c, m, mg, mrl, mties = CM.canonical_rows(boards[rows], cout[rows])
    for name, a, b in zip(NAMES[1:], (canon, sol, g, rl, ties), (c, m, mg, mrl, mties)):
        assert np.array_equal(a[rows], b), name


def test_budget(engine):
    """A budget hit is ineligible and unchanged; the other boards keep their results.  (Which boards run
    out depends on the boards sharing their wave: no count of hits is asserted.)"""
    boards = S.pool()[0]
    full = engine.canonical_batch(boards)
    assert (full[0] == 1).all() and (full[5] >= 1).all()
    for budget in (2, 12):
        got = engine.canonical_batch(boards, budget=budget)
        st = got[0]
        hit = st == -2
        print("budget", budget, ": hits", hit.sum(), "of", len(boards))
        assert np.isin(st, (1, -2)).all() and (hit.any() or budget > 2)
        identity(got, hit, boards)
        assert np.array_equal(got[2][hit], boards[hit])
        same(tuple(a[~hit] for a in got), tuple(a[~hit] for a in full))


def test_device_form(engine, boards128, full128):
    boards = boards128[0]
    n = len(boards)
    sizes = (boards.nbytes + 16, n, boards.nbytes, boards.nbytes, 10 * n, 2 * n)
    bufs = [engine.alloc(s) for s in sizes]
    d_io, d_st, d_sol, d_g, d_rl, d_ties = bufs
    try:
        d_io.upload(boards)
        engine.canonical_batch_dev(d_io, d_io, d_st, n, d_solution=d_sol, d_gather=d_g, d_relabel=d_rl, d_ties=d_ties,
                                   budget=0)      # in place
        engine.synchronize()
        got = (d_st.download(np.empty(n, dtype=np.int8)), d_io.download(np.empty_like(boards)),
               d_sol.download(np.empty_like(boards)), d_g.download(np.empty_like(boards)),
               d_rl.download(np.empty((n, 10), dtype=np.uint8)), d_ties.download(np.empty(n, dtype=np.uint16)))
        same(got, full128)
        # every nullable output null
        d_io.upload(boards)
        d_st.upload(np.zeros(n, dtype=np.int8))
        engine.canonical_batch_dev(d_io, d_io, d_st, n, budget=0)
        engine.synchronize()
        assert np.array_equal(d_io.download(np.empty_like(boards)), full128[1])
        assert np.array_equal(d_st.download(np.empty(n, dtype=np.int8)), full128[0])
        # a misaligned input, a misaligned output
        odd = ctypes.c_void_p(d_io.ptr.value + 1)
        for args in ((odd, d_io.ptr), (d_io.ptr, odd)):
            rc = engine.lib.sdk_canonical_batch_dev(engine.ctx, *args, None, d_st.ptr, None, None, None, n, 0)
            assert rc == L.SDK_EINVAL and b"aligned" in engine.lib.sdk_last_error()
    finally:
        for d in bufs:
            d.free()


def test_arguments(engine, boards128, full128):
    got = engine.canonical_batch(np.zeros((0, 81), dtype=np.uint8))
    assert [a.shape for a in got] == [(0,), (0, 81), (0, 81), (0, 81), (0, 10), (0,)]
    assert [a.dtype for a in got] == [np.int8] + [np.uint8] * 4 + [np.uint16]
    boards = np.ascontiguousarray(boards128[0][:40])
    canon, st = np.empty_like(boards), np.empty(40, dtype=np.int8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    good = [p(boards), p(canon), None, p(st), None, None, None]
    for missing in (0, 1, 3):           # in, canon and status are required
        args = list(good)
        args[missing] = None
        assert engine.lib.sdk_canonical_batch(engine.ctx, *args, 40, 0) == L.SDK_EINVAL
    assert engine.lib.sdk_canonical_batch(None, *good, 40, 0) == L.SDK_EINVAL
    assert engine.lib.sdk_canonical_batch(engine.ctx, *good, 40, 0) == L.SDK_OK      # the others may be null
    assert np.array_equal(canon, full128[1][:40]) and np.array_equal(st, full128[0][:40])
    with pytest.raises(ValueError):
        engine.canonical_batch(boards, budget=-1)


def test_side_effects(engine, boards128, full128):
    boards = boards128[0]
    keys = (L.SDK_OPT_PROP32, L.SDK_OPT_PROP32_LC, L.SDK_OPT_NODE_BUDGET, L.SDK_OPT_SOLVER, L.SDK_OPT_ORDER,
            L.SDK_OPT_DONATE)
    options = {k: engine.get_option(k) for k in keys}
    before = engine.solve_batch(boards)
    try:
        engine.timer_reset()
        got = engine.canonical_batch(boards)
        engine.synchronize()
        ms, spans = engine.timer_read()
        assert spans == 1 and ms > 0.0
    finally:
        engine.timer_stop()
    same(got, full128)
    assert {k: engine.get_option(k) for k in keys} == options
    after = engine.solve_batch(boards)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert (after[1] == 1).all()
