"""The search kernels (solve_kernel, solve2_kernel, solve4_kernel) against the scalar model
(search_model.py), board by board and exactly: status, output and each of the three work[] counters
-- search nodes, propagation rounds, deepest DFS level -- in both orders, under exact node budgets,
and whatever boards share a board's wave.  Locked candidates and subtree donation are off: the
model states the plain search (solve4's EXACT rounds and donated parts count differently, by design).
No comparison here has a tolerance."""
import numpy as np
import pytest

from distributed_sudoku_solver_amd import _lib as L
import search_inputs as I
import search_model as M

pytestmark = pytest.mark.gpu

SOLVERS = {"halfwave": L.SDK_SOLVER_HALFWAVE, "wave": L.SDK_SOLVER_WAVE, "quad": L.SDK_SOLVER_QUAD}
ORDERS = {"lex": L.SDK_ORDER_LEX, "mrv_unique": L.SDK_ORDER_MRV_UNIQUE}
KINDS = {"nodes": L.SDK_WORK_NODES, "rounds": L.SDK_WORK_ROUNDS, "depth": L.SDK_WORK_DEPTH}
CASES = [pytest.param(s, o, id=f"{sn}-{on}") for sn, s in SOLVERS.items() for on, o in ORDERS.items()]


class _options:
    """Context options set for a block and put back after it."""

    def __init__(self, engine, **opts):
        self.engine, self.opts = engine, {getattr(L, k): v for k, v in opts.items()}

    def __enter__(self):
        self.old = {k: self.engine.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.engine.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.engine.set_option(k, v)


def _plain_search(engine, solver, order, **more):
    """One slot per board, no locked-candidates pass: the search the model states."""
    return _options(engine, SDK_OPT_LOCKED=0, SDK_OPT_DONATE=0, SDK_OPT_SOLVER=solver, SDK_OPT_ORDER=order, **more)


def _model(solver, order):
    """The model of a solver: solve4_kernel starts the first cell open (search_model.FIRST_CELL_OPEN)."""
    return I.model(order, first_cell_open=solver == L.SDK_SOLVER_QUAD)


def _first_difference(got, want):
    bad = np.flatnonzero(got != want) if got.ndim == 1 else np.flatnonzero((got != want).any(axis=1))
    return f"{len(bad)} boards differ, first at {bad[0]}: {got[bad[0]].tolist()} for {want[bad[0]].tolist()}"


def _compare(engine, rows, want, what, budget=None, masked=True, hit=None):
    """Solve boards `rows` (indices into the input set) once per counter: status, output and counter
    equal `want`'s rows.  hit: the boards (of rows) the budget cuts -- their work[] is not compared
    (include/sudoku_hip.h does not define it)."""
    boards, masks, _ = I.inputs()
    st_want, out_want = want.status[rows], want.out[rows]
    if hit is None:
        hit = np.zeros(len(rows), dtype=bool)
    else:
        st_want = np.where(hit, M.ST_BUDGET_HIT, st_want)
        out_want = np.where(hit[:, None], boards[rows], out_want)
    for name, kind in KINDS.items():
        with _options(engine, SDK_OPT_WORK_COUNTER=kind):
            out, st, work = engine.solve_batch(boards[rows], masks[rows] if masked else None, want_work=True,
                                               budget=budget)
        assert (st == st_want).all(), f"{what}, status: {_first_difference(st, st_want)}"
        assert (out == out_want).all(), f"{what}, output: {_first_difference(out, out_want)}"
        got, ref = work.astype(np.int64)[~hit], want.counter(kind)[rows][~hit]
        assert (got == ref).all(), f"{what}, {name}: {_first_difference(got, ref)}"


@pytest.mark.parametrize("solver,order", CASES)
def test_counters_status_and_output(engine, solver, order):
    boards, masks, fam = I.inputs()
    want = _model(solver, order)
    ends = np.flatnonzero(want.status != M.ST_BUDGET_HIT)
    assert len(boards) - len(ends) <= 4
    with _plain_search(engine, solver, order):
        _compare(engine, ends, want, "no budget")
        # the boards that carry the full range, without a mask array
        bare = np.concatenate([np.arange(fam[k].start, fam[k].stop) for k in ("17clue", "minimal", "hard", "planted")])
        assert (masks[bare] == I.FULL_MASK).all()
        _compare(engine, np.intersect1d(bare, ends), want, "no masks", masked=False)
        # every board, those that never end among them, under the per-call budget the model ran at
        everything = np.arange(len(boards))
        _compare(engine, everything, want, f"budget={I.CAP}", budget=I.CAP, hit=want.status == M.ST_BUDGET_HIT)
        b = I.BUDGETS[3]
        _compare(engine, everything, want, f"budget={b}", budget=b, hit=want.under(b)[0])


@pytest.mark.parametrize("solver,order", CASES)
def test_counters_do_not_depend_on_wave_mates(engine, solver, order):
    """The batch rotated by 1, 2 and 3 and reversed (with one board per dequeue every board meets other
    wave mates, in another slot of solve4's four and another half of solve2's two), its prefixes of 1, 2,
    3 and 5 boards (waves with empty slots), and in chunks of 7 and 64 boards per dequeue (a slot
    searches board after board: every counter starts afresh)."""
    want = _model(solver, order)
    ends = np.flatnonzero(want.status != M.ST_BUDGET_HIT)
    with _plain_search(engine, solver, order):
        for k in (1, 2, 3):
            _compare(engine, np.roll(ends, k), want, f"rotated by {k}")
        _compare(engine, ends[::-1], want, "reversed")
        for k in (1, 2, 3, 5):
            _compare(engine, ends[:k], want, f"first {k}")
            _compare(engine, ends[-k:], want, f"last {k}")
        for chunk in (7, 64):
            with _options(engine, SDK_OPT_SOLVE_CHUNK=chunk):
                _compare(engine, ends, want, f"chunks of {chunk}")
                _compare(engine, np.roll(ends, 2)[::-1], want, f"chunks of {chunk}, rotated and reversed")


@pytest.mark.parametrize("solver,order", CASES)
def test_node_budget_is_exact(engine, solver, order):
    """SDK_OPT_NODE_BUDGET = B: status -2 and the input back exactly for the boards the model needs more
    than B nodes for; every other board as without a budget, counters included."""
    boards = I.inputs()[0]
    want = _model(solver, order)
    everything = np.arange(len(boards))
    with _plain_search(engine, solver, order):
        for b in I.BUDGETS:
            hit = want.under(b)[0]
            assert hit.any() and not hit.all()
            with _options(engine, SDK_OPT_NODE_BUDGET=b):
                _compare(engine, everything, want, f"SDK_OPT_NODE_BUDGET={b}", hit=hit)
                # the call's own budget wins over the context's
                if b == I.BUDGETS[0]:
                    _compare(engine, everything, want, "budget=20 over the option", budget=20, hit=want.under(20)[0])
