"""SudokuEngine.minimize_batch (sdk_minimize_batch): greedy clue removal on the GPU, bit for bit
against the CPU loop of tests/minimize_ref.py (the same loop over the oracle's capped count), and as
a property at the propagation pass's batch size: unique results no clue of which can go."""
import ctypes

import numpy as np
import pytest

from distributed_sudoku_solver_amd import synth, _lib as L

import minimize_ref as R

pytestmark = pytest.mark.gpu

BIG = 4096 + 37


@pytest.fixture(scope="module")
def grids():
    """512 complete grids, their seeded orders and the reference's results (computed once)."""
    _, g = synth.make_minimal(512)
    order = R.orders(512, 21)
    ref, st = R.minimize(g, order)
    assert (st == 1).all()
    return g, order, ref


@pytest.fixture
def eng(engine):
    keys = (L.SDK_OPT_PROP32, L.SDK_OPT_PROP32_MIN)
    old = {k: engine.get_option(k) for k in keys}
    yield engine
    for k, v in old.items():
        engine.set_option(k, v)


@pytest.mark.parametrize("n", [1, 5, 67, 512])
def test_grids_bit_exact(eng, grids, n):
    g, order, ref = grids
    out, st = eng.minimize_batch(g[:n], order[:n])
    assert (st == 1).all()
    clues = (out != 0).sum(axis=1)
    print("clues left:", clues.min(), "..", clues.max())
    assert (out == ref[:n]).all(), np.flatnonzero((out != ref[:n]).any(axis=1))[:8]


def test_grids_bit_exact_with_the_pass(eng, grids):
    """SDK_OPT_PROP32_MIN = 1: every round's classify runs the pass first; the same bytes."""
    g, order, ref = grids
    eng.set_option(L.SDK_OPT_PROP32_MIN, 1)
    out, st = eng.minimize_batch(g[:67], order[:67])
    assert (st == 1).all()
    assert (out == ref[:67]).all()


def test_partial_start_bit_exact(eng):
    """30-clue puzzles: most rounds meet a cell that is already empty and must leave the board alone."""
    puz, _ = synth.make_30clue(32)
    order = R.orders(32, 22)
    ref, ref_st = R.minimize(puz, order)
    out, st = eng.minimize_batch(puz, order)
    assert (st == ref_st).all() and (st == 1).all()
    assert (out == ref).all()
    assert ((out != 0).sum(axis=1) < 30).any()      # it did remove clues


def test_non_unique_inputs(eng):
    """Unique puzzles interleaved with boards that have no completion or several: those come back
    unchanged with their verdict, the others as the reference says."""
    rng = np.random.default_rng(23)
    puz, _ = synth.make_30clue(48, seed=9)
    boards = puz.copy()
    for i in range(48):
        nz = np.flatnonzero(boards[i])
        c = nz[rng.integers(0, len(nz))]
        if i % 3 == 1:
            boards[i, nz[rng.permutation(len(nz))[:14]]] = 0      # 16 clues left: several
        elif i % 3 == 2:
            boards[i, c] = boards[i, c] % 9 + 1                   # one clue changed: mostly none
    order = R.orders(48, 24)
    ref, ref_st = R.minimize(boards, order)
    for v in (0, 1, 2):
        assert (ref_st == v).any(), v
    out, st = eng.minimize_batch(boards, order)
    assert (st == ref_st).all()
    assert (out[st != 1] == boards[st != 1]).all()
    assert (out == ref).all()


def test_property_at_the_pass_size(eng):
    """4096 + 37 grids under default options (the pass runs in every round): every result is a subset
    of its grid, unique, and -- on a sample -- loses uniqueness with any one clue more removed."""
    _, g0 = synth.make_minimal(512)
    rng = np.random.default_rng(25)
    gather, relabel = synth.random_symmetries(rng, BIG)
    g = synth.apply_symmetries(g0[np.arange(BIG) % 512], gather, relabel)
    out, st = eng.minimize_batch(g, seed=26)
    assert (st == 1).all()
    assert ((out == g) | (out == 0)).all()
    clues = (out != 0).sum(axis=1)
    print("clues left:", clues.min(), "..", clues.max(), "mean", clues.mean())
    assert clues.min() >= 17 and clues.max() < 81
    status, sol = eng.classify_batch(out)
    assert (status == 1).all()
    assert (sol == g).all()
    sample = out[:: BIG // 64][:64]
    less = []
    for p in sample:
        for c in np.flatnonzero(p):
            q = p.copy()
            q[c] = 0
            less.append(q)
    less = np.array(less, dtype=np.uint8)
    status, _ = eng.classify_batch(less)
    assert (status == 2).all()
    assert (R.verdicts(sample) == 1).all()
    assert (R.verdicts(less) == 2).all()
    # the same call again gives the same bytes (seeded orders, no dependence on launch timing)
    again, _ = eng.minimize_batch(g[:256], seed=26)
    assert (again == out[:256]).all()


def test_timing_spans(eng, grids):
    """SDK_OPT_TIMING: a minimise call is one span whatever its rounds launch; a classify records what
    a plain solve of the same shape does (the pass and its fallback, or the one search launch); and a
    solve after a minimise is timed as before it."""
    g, order, _ = grids
    p17, _ = synth.make_17clue(BIG, seed=3)

    def spans(fn):
        eng.timer_reset()
        fn()
        eng.synchronize()
        ms, n = eng.timer_read()
        assert ms > 0.0
        return n

    try:
        solve_before = spans(lambda: eng.solve_batch(p17))
        assert spans(lambda: eng.minimize_batch(g[:67], order[:67])) == 1
        eng.set_option(L.SDK_OPT_PROP32_MIN, 1)
        assert spans(lambda: eng.minimize_batch(g[:67], order[:67])) == 1
        eng.set_option(L.SDK_OPT_PROP32_MIN, 4096)
        assert spans(lambda: eng.classify_batch(p17)) == 2          # the pass, then search + scatter
        assert spans(lambda: eng.classify_batch(p17[:67])) == 1     # the search launch alone
        assert spans(lambda: eng.solve_batch(p17)) == solve_before == 2
    finally:
        eng.timer_stop()


def test_bad_orders(eng):
    _, g = synth.make_minimal(4)
    good = R.orders(4, 27)
    repeated = good.copy()
    repeated[2, 5] = repeated[2, 6]
    too_big = good.copy()
    too_big[1, 80] = 81
    for bad in (repeated, too_big, good[:3], good[:, :80]):
        with pytest.raises(ValueError):
            eng.minimize_batch(g, bad)
    out = np.empty_like(g)
    st = np.empty(4, dtype=np.int8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    for bad in (repeated, too_big):
        assert eng.lib.sdk_minimize_batch(eng.ctx, p(g), p(bad), p(out), p(st), 4) == L.SDK_EINVAL
        assert b"permutation" in eng.lib.sdk_last_error()
    assert eng.lib.sdk_minimize_batch(eng.ctx, p(g), None, p(out), p(st), 4) == L.SDK_EINVAL
    assert eng.lib.sdk_minimize_batch(eng.ctx, p(g), p(good), p(out), p(st), 0) == L.SDK_OK
    e_out, e_st = eng.minimize_batch(np.zeros((0, 81), dtype=np.uint8))
    assert e_out.shape == (0, 81) and e_st.shape == (0,)


def test_device_form_tolerates_out_of_range_order_bytes(eng, grids):
    """The device path cannot validate orders: a byte >= 81 is "no cell", never an index."""
    g, order, ref = grids
    n = 67
    bad = order[:n].copy()
    bad[:, 40] = 255
    d_in, d_ord, d_out, d_st = eng.alloc(n * 81), eng.alloc(n * 81), eng.alloc(n * 81), eng.alloc(n)
    try:
        d_in.upload(g[:n])
        d_ord.upload(order[:n])
        eng.minimize_batch_dev(d_in, d_ord, d_out, d_st, n)
        eng.synchronize()
        out = d_out.download(np.empty((n, 81), dtype=np.uint8))
        st = d_st.download(np.empty(n, dtype=np.int8))
        assert (st == 1).all() and (out == ref[:n]).all()
        d_ord.upload(bad)
        eng.minimize_batch_dev(d_in, d_ord, d_out, d_st, n)
        eng.synchronize()
        out = d_out.download(np.empty((n, 81), dtype=np.uint8))
    finally:
        for d in (d_in, d_ord, d_out, d_st):
            d.free()
    # round 40 is skipped: the cell it named keeps its digit, everything else is a subset as before
    rows = np.arange(n)
    skipped = order[:n, 40]
    assert (out[rows, skipped] == g[rows, skipped]).all()
    assert ((out == g[:n]) | (out == 0)).all()
    expect = np.array([R.minimize_one(g[i], np.delete(order[i], 40))[0] for i in range(n)])
    assert (out == expect).all()
