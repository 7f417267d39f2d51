"""The search model (search_model.py) against everything that does not depend on the search kernels: the
golden vectors, the oracle's naive DFS, the hard filter's node counter (csrc/gen_minimal.c) -- and the
strength of the inputs the GPU comparison runs on (search_inputs.py)."""
import numpy as np
import pytest

from distributed_sudoku_solver_amd import synth
from oracle import oracle as O
import search_inputs as I
import search_model as M


@pytest.fixture(scope="module")
def lex():
    return I.model(M.ORDER_LEX)


@pytest.fixture(scope="module")
def mrv():
    return I.model(M.ORDER_MRV_UNIQUE)


def _inexact(board):
    return not all(M._Board(board, None).exact)


def test_constants_are_the_librarys():
    from distributed_sudoku_solver_amd import _lib as L
    assert (L.SDK_ORDER_LEX, L.SDK_ORDER_MRV_UNIQUE) == (M.ORDER_LEX, M.ORDER_MRV_UNIQUE)
    assert (L.SDK_SOLVED, L.SDK_UNSOLVABLE, L.SDK_BUDGET_HIT) == (M.ST_SOLVED, M.ST_UNSOLVABLE, M.ST_BUDGET_HIT)
    assert (L.SDK_WORK_NODES, L.SDK_WORK_ROUNDS, L.SDK_WORK_DEPTH) == (0, 1, 2)      # Results.counter's order


def test_golden_status_and_board(lex, mrv):
    cases = I.golden_cases()
    s = I.inputs()[2]["golden"]
    assert len(cases) == s.stop - s.start == 106
    for res in (lex, mrv):
        for c, st, out in zip(cases, res.status[s], res.out[s]):
            assert (st == 1) == c["ok"], c["name"]
            assert out.tolist() == (c["board"] if c["ok"] else c["puzzle"]), c["name"]


@pytest.mark.parametrize("family", ["sparse", "planted"])
def test_oracle_status_and_board(lex, family):
    boards, masks, fam = I.inputs()
    s = fam[family]
    ref_out, ref_st, _ = O.naive_solve_batch(boards[s], masks[s], budget=20_000_000, threads=8)
    done = (ref_st != -2) & (lex.status[s] != -2)
    assert done.mean() > 0.9, done.mean()
    assert (lex.status[s][done] == ref_st[done]).all()
    assert (lex.out[s][done] == ref_out[done]).all()
    assert (ref_st[done] == 1).sum() >= 50 and (ref_st[done] == 0).sum() >= 10


def test_mrv_unique_agrees_with_lex(lex, mrv):
    both = (lex.status != -2) & (mrv.status != -2)
    assert both.sum() >= len(both) - 4
    assert (lex.status[both] == mrv.status[both]).all()
    assert (lex.out[both] == mrv.out[both]).all()
    # a unique completion needs no re-search; the counters are those of another search all the same
    assert (lex.nodes != mrv.nodes).sum() > 100


def test_first_cell_open_changes_rounds_only():
    boards, masks, _ = I.inputs()
    one = I.one_digit_mask(boards, masks)
    assert one.sum() >= 30
    for order in I.ORDERS:
        a, b = I.model(order), I.model(order, True)
        assert (a.status == b.status).all() and (a.out == b.out).all()
        assert (a.nodes == b.nodes).all() and (a.depth == b.depth).all()
        differ = a.rounds != b.rounds
        assert differ.sum() >= 10 and not differ[~one].any()
        assert (np.abs(a.rounds - b.rounds) <= 2).all()      # one round per search of the call at most


def test_lex_nodes_equal_the_hard_filters(lex):
    """csrc/gen_minimal.c's lex_singles_nodes is a restatement of its own (a recursive scalar DFS) of
    the LEX search's node count: on the minimal stream and on the committed hard set's filter_nodes."""
    fam = I.inputs()[2]
    p, nodes = synth.minimal_nodes(200)
    assert (p == I.inputs()[0][fam["minimal"]]).all()
    assert (lex.nodes[fam["minimal"]] == nodes).all()
    with np.load(synth.HARD_SET, allow_pickle=False) as z:
        filt = z["filter_nodes"].astype(np.int64)
    assert (lex.nodes[fam["hard"]] == filt[:160]).all()
    heaviest = np.argsort(-filt, kind="stable")[:16]
    assert (lex.nodes[fam["heaviest"]] == filt[heaviest]).all()
    assert (lex.status[fam["heaviest"]] == 1).all()


def test_budget_is_exact_in_the_model():
    """A board of N nodes: budget N finishes it as no budget does, N - 1 cuts it (status -2, the input
    back, N nodes counted)."""
    boards, masks, fam = I.inputs()
    rng = np.random.default_rng(5)
    for order in I.ORDERS:
        full = I.model(order)
        pick = np.concatenate([rng.choice(np.arange(s.start, s.stop), 6, replace=False) for s in fam.values()
                               if s.stop - s.start >= 6])
        for i in pick:
            n = int(full.nodes[i])
            if full.status[i] == -2:
                continue
            at = M.solve(boards[i], masks[i], order, n)
            assert at == (full.status[i], full.out[i].tolist(), n, full.rounds[i], full.depth[i]), i
            assert M.solve(boards[i], masks[i], order, 0) == at, i
            if n > 1:
                st, out, nodes, _, _ = M.solve(boards[i], masks[i], order, n - 1)
                assert (st, nodes) == (-2, n) and out == boards[i].tolist(), i
                hit, st_u, out_u = full.under(n - 1)
                assert hit[i] and st_u[i] == -2 and (out_u[i] == boards[i]).all()


# ------------------------------------------------------------------ the inputs are strong enough
def test_inputs_go_deep(lex, mrv):
    """Deeper than solve2_kernel's ten LDS-resident levels, many times over."""
    assert (lex.depth > 10).sum() >= 50, (lex.depth > 10).sum()
    assert (mrv.depth > 10).sum() >= 50, (mrv.depth > 10).sum()
    assert lex.depth.max() >= 30


def test_inputs_take_the_double_search(mrv):
    """MRV finds two completions, LEX searches again: seen as a board whose MRV_UNIQUE call counts the
    nodes of an MRV search that stops at its second completion plus those of the LEX search."""
    boards, masks, _ = I.inputs()
    double = 0
    for i, (b, m) in enumerate(zip(boards, masks)):
        if mrv.status[i] != 1:
            continue
        bd, cnt = M._Board(b, m), M._Counters()
        if M.search(bd, M._MRV, 2, I.CAP, cnt) == 2:
            lex_nodes = I.model(M.ORDER_LEX).nodes[i]
            assert mrv.nodes[i] == cnt.nodes + lex_nodes, i
            double += 1
    assert double >= 100, double


def test_inputs_hold_inexact_boards(lex):
    boards = I.inputs()[0]
    inexact = np.array([_inexact(b) for b in boards])
    assert inexact.sum() >= 30, inexact.sum()
    assert (boards[inexact] > 9).any(axis=1).sum() >= 15 and (~(boards[inexact] > 9).any(axis=1)).sum() >= 15
    # ... that are searched, not only refuted at the root
    assert (inexact & (lex.nodes > 1) & (lex.status != -2)).sum() >= 20


def test_inputs_sit_on_both_sides_of_every_budget(lex, mrv):
    """For every budget B of the GPU test a board of exactly B nodes (`>=` for `>` would cut it) and one
    of exactly B + 1 (a budget that fires a node late would finish it), in both orders -- but for what
    an MRV_UNIQUE call cannot take: 2 nodes (a root that branches has two children at least) and, on
    these boards, 4 (a three-candidate MRV cell with one completion below it)."""
    for res, never in ((lex, ()), (mrv, (2, 4))):
        for b in I.BUDGETS:
            for n in (b, b + 1):
                assert (res.nodes == n).any() or n in never, (b, n)
        assert not any((res.nodes == n).any() for n in never)
        assert (res.status == -2).sum() <= 4 and (res.status == -2).any()
        assert res.status[I.inputs()[2]["edge"]].tolist() == [1, 1, 1, 0, 1, -2]


def test_inputs_masks():
    boards, masks, fam = I.inputs()
    real = (masks >> 1) & M.ALL
    assert (real == 0).sum() >= 20 and I.one_digit_mask(boards, masks).sum() >= 30
    assert 650 <= len(boards) <= 900
    assert len({bytes(b) + bytes(m) for b, m in zip(boards, masks)}) >= len(boards) - 20
