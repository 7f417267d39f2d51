"""SudokuEngine.grade_batch (sdk_grade_batch; csrc/grade32_kernel.h): level and open count against
the scalar model (grade_model.py), byte for byte, on a pool whose every half-wave mixes levels; the
verdicts against classify_batch on broken boards; budgets, options, the device form and what the
call leaves behind.

Slices of 2^24 boards are not run here (a call that large does not fit a few seconds): launch_grade's
slice loop is launch_classify's and launch_minimize's (offsets b0 * 81 / b0 into every array, the
per-slice count min(n - b0, 2^24)), and every slice is a whole run of the path tested below."""
import ctypes

import numpy as np
import pytest

import grade_model as G
from distributed_sudoku_solver_amd import synth, _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool():
    """(boards, solutions, model level, model open)."""
    boards, sol = G.make_pool()
    level, open_ = G.grade(boards)
    return boards, sol, level, open_


@pytest.fixture(scope="module")
def full(engine, pool):
    """grade_batch of the whole pool under default options."""
    return engine.grade_batch(pool[0])


def test_pool_matches_model(pool, full):
    boards, sol, level, open_ = pool
    st, lv, op, out = full
    print("levels 1..4:", np.bincount(lv, minlength=5)[1:].tolist(), "open", op[lv == 4].min(), "..", op[lv == 4].max())
    assert (st == 1).all(), np.flatnonzero(st != 1)[:8]
    assert np.array_equal(out, sol)
    assert np.array_equal(lv, level), np.flatnonzero(lv != level)[:8]
    assert np.array_equal(op, open_), np.flatnonzero(op != open_)[:8]


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 129])
def test_ragged_shapes(engine, pool, full, n):
    """Half-wave and group boundaries, a lone board, one board spilling into a second group."""
    st, lv, op, out = engine.grade_batch(pool[0][:n])
    for got, ref in zip((st, lv, op, out), full):
        assert np.array_equal(got, ref[:n])


@pytest.mark.parametrize("many,one", [(1, 1), (4, 4), (1, 4), (4, 1)], ids=["all1", "all4", "one4in1", "one1in4"])
def test_uniform_groups(engine, pool, many, one):
    """64 copies of one board, and one straggler of the other kind in the group: a level-4 board keeps
    the group alive through both escalations while its neighbours are long solved, and the other way."""
    boards, sol, level, open_ = pool
    a, b = np.flatnonzero(level == many)[0], np.flatnonzero(level == one)[1]
    idx = np.full(64, a)
    idx[37] = b
    st, lv, op, out = engine.grade_batch(boards[idx])
    assert (st == 1).all()
    assert np.array_equal(out, sol[idx])
    assert np.array_equal(lv, level[idx])
    assert np.array_equal(op, open_[idx])


# ---- the mixed pool of test_gpu_classify.py, from the same recipe
def edge_pool(n, seed=5):
    rng = np.random.default_rng(seed)
    base, _ = synth.make_30clue(n, seed=seed, extra=20)
    sol, _ = synth.make_30clue(n, seed=seed + 1, extra=64)
    out = base.copy()
    for i in range(n):
        k = i % 6
        if k == 0:      # an out-of-domain given
            out[i, rng.integers(0, 81)] = rng.integers(10, 256)
        elif k == 1:    # a given repeated in its row
            r = rng.integers(0, 9)
            row = out[i, 9 * r:9 * r + 9]
            nz, z = np.flatnonzero(row), np.flatnonzero(row == 0)
            if len(nz) and len(z):
                out[i, 9 * r + z[0]] = row[nz[0]]
        elif k == 2:    # an inert given on a complete grid: still "exactly one"
            out[i] = sol[i]
            out[i, rng.integers(0, 81)] = 200
        elif k == 3:    # half a grid with one given changed
            out[i] = sol[i]
            out[i, rng.choice(81, 40, replace=False)] = 0
            nz = np.flatnonzero(out[i])
            c = nz[rng.integers(0, len(nz))]
            out[i, c] = out[i, c] % 9 + 1
        elif k == 4:    # an inert given where a clue was: usually several
            nz = np.flatnonzero(out[i])
            out[i, nz[rng.integers(0, len(nz))]] = 10
    return out


def clean_givens(board):
    """Only in-domain givens, none repeated in a unit."""
    b = board.reshape(9, 9)
    if (b > 9).any():
        return False
    units = [b[r] for r in range(9)] + [b[:, c] for c in range(9)]
    units += [b[3 * r:3 * r + 3, 3 * c:3 * c + 3].reshape(9) for r in range(3) for c in range(3)]
    return all(len(u[u > 0]) == len(set(u[u > 0].tolist())) for u in units)


def mixed_pool():
    rng = np.random.default_rng(11)
    puz, sol = synth.make_minimal(256)
    rows = np.arange(256)
    clue = np.array([rng.choice(np.flatnonzero(p)) for p in puz])
    cleared = puz.copy()
    cleared[rows, clue] = 0
    changed = puz.copy()
    changed[rows, clue] = puz[rows, clue] % 9 + 1
    broken = sol[1].copy()
    broken[40] = broken[40] % 9 + 1
    p17, _ = synth.seed_arrays()
    boards = np.concatenate([puz, cleared, changed, np.zeros((1, 81), np.uint8), sol[:1], broken[None], p17,
                             edge_pool(24)]).astype(np.uint8)
    return np.ascontiguousarray(boards[rng.permutation(len(boards))])


def test_verdicts_on_the_mixed_pool(engine):
    """Inert and duplicated givens, contradictions, the empty board, complete grids valid and not,
    cleared-clue and changed-clue puzzles: classify's verdicts, and a grade only where it is defined."""
    boards = mixed_pool()
    ref_st, ref_out = engine.classify_batch(boards)
    st, lv, op, out = engine.grade_batch(boards)
    for v in (0, 1, 2):
        assert (ref_st == v).any(), f"the pool has no board with verdict {v}"
    assert np.array_equal(st, ref_st), np.flatnonzero(st != ref_st)[:8]
    assert np.array_equal(out, ref_out)
    clean = np.array([clean_givens(b) for b in boards])
    graded = (st == 1) & clean
    print("graded", graded.sum(), "of", len(boards), "; solved with givens not clean:", ((st == 1) & ~clean).sum())
    assert ((st == 1) & ~clean).any() and graded.any()
    assert (lv[~graded] == 0).all(), np.flatnonzero(lv[~graded] != 0)[:8]
    assert (op[~graded] == 0).all()
    level, open_ = G.grade(boards[graded])
    assert np.array_equal(lv[graded], level)
    assert np.array_equal(op[graded], open_)


def test_budget(engine, pool):
    """A budget bounds the search alone: what the techniques solve keeps its level.  (Which level-4
    boards run out depends on the boards sharing their wave: no count is asserted.)"""
    boards, sol, level, open_ = pool
    st, lv, op, out = engine.grade_batch(boards, budget=2)
    print("budget 2: hits", (st == -2).sum(), "of", (level == 4).sum(), "level-4 boards")
    assert np.isin(st, (1, -2)).all()
    easy = level <= 3
    assert (st[easy] == 1).all() and np.array_equal(lv[easy], level[easy])
    hit = st == -2
    assert np.array_equal(lv == 0, hit) and (op[hit] == 0).all()
    assert np.array_equal(lv[~hit], level[~hit]) and np.array_equal(op[~hit], open_[~hit])
    assert np.array_equal(out[hit], boards[hit]) and np.array_equal(out[~hit], sol[~hit])


def test_independent_of_pass_options_and_no_residue(engine, pool, full):
    boards = pool[0]
    before = engine.solve_batch(boards)
    for key, value in ((L.SDK_OPT_PROP32, 0), (L.SDK_OPT_PROP32_LC, 1 | 1 << 8)):
        old = engine.get_option(key)
        try:
            engine.set_option(key, value)
            got = engine.grade_batch(boards)
            assert engine.get_option(key) == value
        finally:
            engine.set_option(key, old)
        for g, ref in zip(got, full):
            assert np.array_equal(g, ref), (key, value)
    after = engine.solve_batch(boards)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert (after[1] == 1).all()


def test_device_form(engine, pool, full):
    boards = pool[0][:129]
    n = len(boards)
    d_io, d_st, d_lv, d_op = engine.alloc(boards.nbytes + 16), engine.alloc(n), engine.alloc(n), engine.alloc(n)
    try:
        d_io.upload(boards)
        engine.grade_batch_dev(d_io, d_io, d_st, d_lv, n, d_open=d_op, budget=0)      # in place
        engine.synchronize()
        st = d_st.download(np.empty(n, dtype=np.int8))
        lv = d_lv.download(np.empty(n, dtype=np.uint8))
        op = d_op.download(np.empty(n, dtype=np.uint8))
        out = d_io.download(np.empty_like(boards))
        for got, ref in zip((st, lv, op, out), full):
            assert np.array_equal(got, ref[:n])
        # no open counts wanted
        d_io.upload(boards)
        engine.grade_batch_dev(d_io, d_io, d_st, d_lv, n, budget=0)
        engine.synchronize()
        assert np.array_equal(d_lv.download(np.empty(n, dtype=np.uint8)), full[1][:n])
        # a misaligned input
        odd = ctypes.c_void_p(d_io.ptr.value + 1)
        rc = engine.lib.sdk_grade_batch_dev(engine.ctx, odd, d_io.ptr, d_st.ptr, d_lv.ptr, None, n, 0)
        assert rc == L.SDK_EINVAL and engine.lib.sdk_last_error()
    finally:
        for d in (d_io, d_st, d_lv, d_op):
            d.free()


def test_arguments(engine):
    st, lv, op, out = engine.grade_batch(np.zeros((0, 81), dtype=np.uint8))
    assert st.shape == (0,) and lv.shape == (0,) and op.shape == (0,) and out.shape == (0, 81)
    boards, sol = synth.make_17clue(4, seed=1)
    out, st, lv = np.empty_like(boards), np.empty(4, dtype=np.int8), np.empty(4, dtype=np.uint8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    for args in ((None, p(out), p(st), p(lv)), (p(boards), None, p(st), p(lv)), (p(boards), p(out), None, p(lv)),
                 (p(boards), p(out), p(st), None)):
        assert engine.lib.sdk_grade_batch(engine.ctx, *args, None, 4, 0) == L.SDK_EINVAL
    # open may be null
    assert engine.lib.sdk_grade_batch(engine.ctx, p(boards), p(out), p(st), p(lv), None, 4, 0) == L.SDK_OK
    assert (st == 1).all() and np.array_equal(out, sol) and np.isin(lv, (1, 2, 3, 4)).all()
    with pytest.raises(ValueError):
        engine.grade_batch(boards, budget=-1)
