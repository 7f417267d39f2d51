"""SudokuEngine.classify_batch (sdk_classify_batch): per-board uniqueness verdicts -- none, exactly
one, several -- against the oracle's capped count, with and without the propagation pass, under a
node budget, and without leaving anything behind for the solves that follow."""
import ctypes

import numpy as np
import pytest

from distributed_sudoku_solver_amd import synth, _lib as L
from oracle import oracle as O

import minimize_ref as R

pytestmark = pytest.mark.gpu

BIG = 4096 + 37      # the pass's default minimum batch and a ragged last group of 64


def edge_pool(n, seed=5):
    """Inert and duplicated givens, contradictions, complete grids (valid and not) and the empty board
    on 37-clue boards, so the oracle's count stays short on the broken ones."""
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
    """Only in-domain givens, none repeated in a unit: a completion is then a valid Sudoku grid."""
    b = board.reshape(9, 9)
    if (b > 9).any():
        return False
    units = [b[r] for r in range(9)] + [b[:, c] for c in range(9)]
    units += [b[3 * r:3 * r + 3, 3 * c:3 * c + 3].reshape(9) for r in range(3) for c in range(3)]
    for u in units:
        d = u[u > 0]
        if len(d) != len(set(d.tolist())):
            return False
    return True


@pytest.fixture(scope="module")
def pool():
    """(boards, oracle verdicts), every class present, families interleaved."""
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
    boards = np.ascontiguousarray(boards[rng.permutation(len(boards))])
    truth = R.verdicts(boards)
    for v in (0, 1, 2):
        assert (truth == v).any(), f"the pool has no board with verdict {v}"
    return boards, truth


@pytest.fixture(scope="module")
def solved(engine, pool):
    """engine.solve_batch of the pool under default options (pinned to the oracle elsewhere)."""
    out, st, _ = engine.solve_batch(pool[0])
    return out, st


@pytest.fixture
def eng(engine):
    keys = (L.SDK_OPT_ORDER, L.SDK_OPT_SOLVER, L.SDK_OPT_PROP32, L.SDK_OPT_PROP32_MIN, L.SDK_OPT_PROP32_HANDOVER,
            L.SDK_OPT_PROP32_TAIL, L.SDK_OPT_NODE_BUDGET)
    old = {k: engine.get_option(k) for k in keys}
    yield engine
    for k, v in old.items():
        engine.set_option(k, v)


def take(pool, n):
    boards, truth = pool
    idx = np.arange(n) % len(boards)
    return np.ascontiguousarray(boards[idx]), truth[idx], idx


def check_against_oracle(boards, truth, status, out, solved_out):
    print("verdicts none/one/several:", [(status == v).sum() for v in (0, 1, 2)], "of", len(boards))
    assert (status == truth).all(), np.flatnonzero(status != truth)[:8]
    not_one = status != 1
    assert (out[not_one] == boards[not_one]).all()
    one = np.flatnonzero(status == 1)
    given = boards[one] != 0
    assert (out[one][given] == boards[one][given]).all()
    assert (out[one] == solved_out[one]).all()
    seen = set()
    for i in one:
        key = boards[i].tobytes()
        if key in seen:
            continue
        seen.add(key)
        assert (out[i] != 0).all()
        if clean_givens(boards[i]):
            assert O.check(out[i]) & 1, i


@pytest.mark.parametrize("n", [1, 3, 5, 67])
def test_search_only_against_oracle(eng, pool, solved, n):
    """Batches below the pass's minimum: ragged quads and a ragged last wave of the search alone."""
    boards, truth, idx = take(pool, n)
    status, out = eng.classify_batch(boards)
    assert eng.get_option(L.SDK_OPT_PROP32_UNDECIDED) == 0      # the pass did not run
    check_against_oracle(boards, truth, status, out, solved[0][idx])


def test_pass_and_search_against_oracle(eng, pool, solved):
    boards, truth, idx = take(pool, BIG)
    status, out = eng.classify_batch(boards)
    check_against_oracle(boards, truth, status, out, solved[0][idx])
    und = eng.get_option(L.SDK_OPT_PROP32_UNDECIDED)
    assert 0 < und < BIG, und      # the pass ran, decided some boards itself and left the several to the search


def test_pass_on_a_small_batch(eng, pool, solved):
    """SDK_OPT_PROP32_MIN = 1: the pass on a batch smaller than one full wave of groups."""
    boards, truth, idx = take(pool, 67)
    eng.set_option(L.SDK_OPT_PROP32_MIN, 1)
    status, out = eng.classify_batch(boards)
    check_against_oracle(boards, truth, status, out, solved[0][idx])
    assert eng.get_option(L.SDK_OPT_PROP32_UNDECIDED) > 0      # the pass ran (the several are left to the search)


def test_pass_on_equals_pass_off(eng, pool):
    boards, _, _ = take(pool, BIG)
    base_st, base_out = eng.classify_batch(boards)
    for key, value in ((L.SDK_OPT_PROP32, 0), (L.SDK_OPT_PROP32_HANDOVER, 0), (L.SDK_OPT_PROP32_TAIL, 4 | 8 << 8)):
        old = eng.get_option(key)
        eng.set_option(key, value)
        st, out = eng.classify_batch(boards)
        eng.set_option(key, old)
        assert (st == base_st).all(), (key, value)
        assert (out == base_out).all(), (key, value)


def test_budget_hits(eng):
    """Every hard board branches, and a branching unique board takes at least three nodes, so a budget of
    two stops some; which ones depends on the boards sharing their wave, so that is not asserted."""
    puz, sol, _ = synth.load_hard(256)
    status, out = eng.classify_batch(puz, budget=2)
    print("budget 2: hits", (status == -2).sum(), "one", (status == 1).sum())
    assert np.isin(status, (-2, 1)).all()
    assert (status == -2).any()
    hit = status == -2
    assert (out[hit] == puz[hit]).all()
    assert (out[~hit] == sol[~hit]).all()
    status, out = eng.classify_batch(puz, budget=None)
    assert (status == 1).all()
    assert (out == sol).all()


@pytest.mark.parametrize("order", [L.SDK_ORDER_LEX, L.SDK_ORDER_MRV_UNIQUE], ids=["lex", "mrv_unique"])
def test_no_leakage_into_solves(eng, pool, order):
    eng.set_option(L.SDK_OPT_ORDER, order)
    p17, _ = synth.make_17clue(BIG, seed=3)
    hard, _, _ = synth.load_hard(512)
    p17[::9] = hard[np.arange(len(p17[::9])) % len(hard)]      # some boards the phased solve passes on
    first = eng.solve_batch(p17)
    boards, truth, _ = take(pool, BIG)
    status, _ = eng.classify_batch(boards)
    assert (status == truth).all()
    assert eng.get_option(L.SDK_OPT_ORDER) == order
    assert eng.get_option(L.SDK_OPT_SOLVER) == L.SDK_SOLVER_QUAD
    second = eng.solve_batch(p17)
    assert (first[0] == second[0]).all() and (first[1] == second[1]).all()
    assert (second[1] == 1).all()
    # and a small classify between two small solves (search only on both sides)
    a = eng.solve_batch(p17[:67])
    eng.classify_batch(boards[:5])
    b = eng.solve_batch(p17[:67])
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


def test_classify_ignores_solver_and_order_options(eng, pool):
    boards, truth, _ = take(pool, 67)
    eng.set_option(L.SDK_OPT_SOLVER, L.SDK_SOLVER_WAVE)
    eng.set_option(L.SDK_OPT_ORDER, L.SDK_ORDER_MRV_UNIQUE)
    status, _ = eng.classify_batch(boards)
    assert (status == truth).all()
    assert eng.get_option(L.SDK_OPT_SOLVER) == L.SDK_SOLVER_WAVE
    assert eng.get_option(L.SDK_OPT_ORDER) == L.SDK_ORDER_MRV_UNIQUE


def test_device_form(eng, pool):
    boards, truth, _ = take(pool, 67)
    d_in, d_out, d_st = eng.alloc(boards.nbytes), eng.alloc(boards.nbytes), eng.alloc(len(boards))
    try:
        d_in.upload(boards)
        eng.classify_batch_dev(d_in, d_out, d_st, len(boards), budget=0)
        eng.synchronize()
        st = d_st.download(np.empty(len(boards), dtype=np.int8))
        out = d_out.download(np.empty_like(boards))
    finally:
        for d in (d_in, d_out, d_st):
            d.free()
    host_st, host_out = eng.classify_batch(boards)
    assert (st == truth).all() and (st == host_st).all() and (out == host_out).all()


def test_errors(eng):
    status, out = eng.classify_batch(np.zeros((0, 81), dtype=np.uint8))
    assert status.shape == (0,) and out.shape == (0, 81)
    boards, _ = synth.make_17clue(4, seed=1)
    out = np.empty_like(boards)
    st = np.empty(4, dtype=np.int8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    for args in ((p(boards), None, p(st)), (p(boards), p(out), None), (None, p(out), p(st))):
        assert eng.lib.sdk_classify_batch(eng.ctx, *args, 4, 0) == L.SDK_EINVAL
        assert eng.lib.sdk_last_error()
    assert eng.lib.sdk_classify_batch_dev(eng.ctx, None, None, None, 4, 0) == L.SDK_EINVAL
    with pytest.raises(ValueError):
        eng.classify_batch(boards, budget=-1)
