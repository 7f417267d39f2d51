"""The checker's case pool (check_inputs.py) and scalar model (check_model.py) against oracle.py_check, the
pure-Python reference -- and the strength of the pool: every named way in which check_board_lds could be
wrong changes a verdict of it."""
import numpy as np
import pytest

from oracle import oracle as O
import check_inputs as I
import check_model as M

MIN_VERDICTS = {0: 48000, 2: 250, 3: 120}      # boards of each verdict the pool must hold


def test_pool_shape_and_families():
    boards, tags = I.pool()
    assert boards.dtype == np.uint8 and boards.shape[1] == 81 and len(tags) == len(boards)
    assert 48620 + 1000 < len(boards) < 60000
    count = {t: int((tags == t).sum()) for t in dict.fromkeys(tags.tolist())}
    assert count["fast_multiset"] == 48620 and count["exact_pass"] == 120 and count["alias"] == 63
    assert count["single_row_col"] == 72 and count["single_box"] == 36 and count["four_boxes"] == 108
    again = I.pool.__wrapped__()[0]
    assert (again == boards).all()                                      # deterministic


def test_pool_holds_every_verdict():
    exp, tags = I.expected(), I.pool()[1]
    assert set(np.unique(exp).tolist()) == {0, 2, 3}
    for v, least in MIN_VERDICTS.items():
        assert (exp == v).sum() >= least, (v, int((exp == v).sum()))
    # the one valid multiset over 0..9, and every passing set
    assert (exp[tags == "fast_multiset"] == 3).sum() == 1
    assert (exp[tags == "exact_pass"] == 3).all()
    for t in ("near_plus1", "near_minus1", "near_merged", "alias", "byte_edge", "sum_wrap", "all_one_value",
              "single_row_col", "one_cell_off"):
        assert (exp[tags == t] == 0).all(), t
    # (on the exact path a relabelling can bring a moved box (0,0) back to sum 45)
    assert (exp[tags == "latin_box00_off"][:80] == 0).all() and (exp[tags == "latin_box00_off"] == 0).sum() >= 150
    assert (exp[tags == "latin_box00_45"] == 2).all()
    # verdict 2 on the fast path and on the exact path
    v2 = I.pool()[0][exp == 2]
    assert (v2.max(axis=1) <= 9).sum() >= 100 and (v2.max(axis=1) >= 10).sum() >= 100


def test_single_unit_boards_fail_in_one_unit():
    base = I.parse_grid(I.SINGLE_ROW)
    assert I.failing_units(base) == [0] and base.max() < 32 and base.max() > 9
    rng = np.random.default_rng(1)
    boards, units = I.single_unit_boards(rng, base)
    assert sorted(set(units.tolist())) == list(range(18))
    for b, u in zip(boards, units):
        assert I.failing_units(b) == [u]
        assert O.py_check(b.tolist()) == ("False", False)
    base = I.parse_grid(I.SINGLE_BOX)
    assert I.failing_units(base) == [18] and 9 < base.max() < 32
    boards, units = I.single_unit_boards(rng, base, box=True)
    assert sorted(set(units.tolist())) == list(range(18, 27))
    for b, u in zip(boards, units):
        assert I.failing_units(b) == [u]
        assert O.py_check(b.tolist()) == ("NameError", False)


def test_four_box_boards_fail_in_four_boxes():
    boards, which = I.four_box_boards(np.random.default_rng(2), per_pair=3)
    for b, (bi, si) in zip(boards, which):
        bands, stacks = I.BAND_PAIRS[bi], I.BAND_PAIRS[si]
        assert I.failing_units(b) == sorted(18 + 3 * x + y for x in bands for y in stacks)
        hit00 = 0 in bands and 0 in stacks
        assert O.py_check(b.tolist()) == ("False" if hit00 else "NameError", False)


def test_mix_is_drawn_from_every_family():
    m, (boards, tags), exp = I.mix(), I.pool(), I.expected()
    assert len(m) == 600
    names = list(dict.fromkeys(tags.tolist()))
    for lo in (0, 300, 600 - len(names)):
        assert set(tags[m[lo:lo + len(names)]].tolist()) == set(names)      # any short run holds all
    assert (exp[m] == 2).sum() >= 50 and (exp[m] == 3).sum() >= 30
    for t in ("single_row_col", "single_box", "alias"):
        assert (tags[m] == t).sum() >= 30, t


def test_model_equals_py_check():
    got, exp = M.verdicts(I.pool()[0]), I.expected()
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, [(I.pool()[1][i], I.pool()[0][i].tolist(), int(got[i]), int(exp[i])) for i in bad[:3]]


def test_c_oracle_equals_py_check():
    got, exp = O.check_batch(I.pool()[0], threads=8), I.expected()
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, [(I.pool()[1][i], I.pool()[0][i].tolist(), int(got[i]), int(exp[i])) for i in bad[:3]]


def test_model_on_random_boards():
    """Beyond the pool: random bytes in the ranges where the two paths meet."""
    rng = np.random.default_rng(9)
    b = np.concatenate([rng.integers(0, hi, (300, 81)) for hi in (10, 12, 20, 33, 256)]).astype(np.uint8)
    assert M.verdicts(b).tolist() == [I.py_verdict(O, c) for c in b.tolist()]


@pytest.mark.parametrize("mutation", M.MUTATIONS)
def test_every_mutation_is_caught(mutation):
    boards, tags = I.pool()
    changed = np.flatnonzero(M.verdicts(boards, mutation) != I.expected())
    assert changed.size > 0, mutation
    if mutation.startswith("skip_"):          # nothing else in the pool fails in one unit only
        assert set(tags[changed].tolist()) == {"single_box" if "box" in mutation else "single_row_col"}
