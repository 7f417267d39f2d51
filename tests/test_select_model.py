"""The selection kernels' case pool (select_inputs.py) and scalar model (select_model.py) against the plain
reference select_ref -- and the strength of the pool: what it covers is asserted, not hoped for, and every
named way in which the kernels could be wrong (select_model.MUTANTS) shows on it.  No GPU: the same pool
and reference are what test_gpu_select.py holds the kernels to."""
import functools

import numpy as np
import pytest

import select_inputs as I
import select_model as M

# the family in which a mutant must show (the rest of the pool may see it too)
KILLED_IN = {
    "no_row_guard": "partial", "no_level_guard": "table", "status_nonzero": "table",
    "clues_lo_strict": "table", "clues_hi_strict": "table", "bd_lo_strict": "table", "bd_hi_strict": "table",
    "o4_lo_strict": "table", "o4_hi_strict": "table", "bd_every_level": "table", "o4_every_level": "table",
    "bd_skipped_with_o4": "table", "o4_skipped_with_bd": "table", "clues_digits_only": "table",
    "clues_80_cells": "table",
    "scan_no_carry_in": "scan", "scan_no_run_add": "scan", "scan_before_le": "scan", "scan_inclusive": "scan",
    "scan_oob_lanes": "scan",
    "kept_unclamped": "quota", "below_le_kept": "quota", "mbcnt_lo_only": "ballot",
    "head_mod4": "quota", "in0_16_at_head0": "quota", "in1_rounded_up": "quota", "no_head_bytes": "quota",
    "no_tail_bytes": "quota", "pack_without_head": "quota",
    "grids_from_puzzles": "ballot", "gather_at_rank": "ballot", "index_without_first": "index",
    "index_32bit": "index", "last_at_rank_n": "quota", "last_is_row": "quota", "absent_source_zero": "ballot",
}


@functools.lru_cache(maxsize=None)
def refs():
    """select_ref of every case, once per module."""
    return {c.name: M.select_ref(c) for c in I.pool()}


def difference(c, got, ref):
    """What of a model result differs from the reference: outputs, total, last or the write maps."""
    diff = []
    if got.total != ref.total:
        diff.append("total")
    if got.last != ref.last:
        diff.append("last")
    for k, exp in ref.out.items():
        a = got.out[k]
        if exp is None:
            assert a is None
            continue
        fill = I.FILL64 if k == "index" else I.FILL
        if not np.array_equal(a[:c.n], exp) or not (a[c.n:] == fill).all():
            diff.append(k)
    w16, w1, per_hit = M.expected_writes(c, ref)
    for k in ("puzzles", "grids"):
        if not np.array_equal(got.w16[k], w16) or not np.array_equal(got.w1[k], w1):
            diff.append("writes:" + k)
    for k in I.NULLABLE:
        if k in got.writes and not np.array_equal(got.writes[k], per_hit):
            diff.append("writes:" + k)
    if got.misaligned:
        diff.append("misaligned")
    return diff


def test_pool_shape():
    pool = I.pool()
    names = [c.name for c in pool]
    assert len(set(names)) == len(names)
    count = {f: len(I.family(f)) for f in dict.fromkeys(c.family for c in pool)}
    print("pool", len(pool), count)
    assert count == {"table": 156, "ballot": 192, "phase": 4, "quota": 1052, "scan": 128, "partial": 24, "index": 4,
                     "rounds": count["rounds"]} and 30 <= count["rounds"] <= 60
    assert max(c.tiles for c in pool) == 3073 and max(c.m for c in pool) == 196672
    again = I.ballot_cases()                                            # deterministic
    for a, b in zip(again, I.family("ballot")):
        assert a.name == b.name and np.array_equal(a.status, b.status) and np.array_equal(a.level, b.level)
    assert np.array_equal(I.big_rows.__wrapped__()[0][:4096], I.big_rows()[0][:4096])
    for c in pool:                                                      # what sdk_select_rows_dev asks for
        assert 1 <= c.m <= 1 << 24 and c.base < c.n <= 0x7FFFFFFF and c.first + c.m <= (1 << 64) - 1
        assert c.mask in I.MASKS and c.clues[0] <= c.clues[1] <= 81
        assert c.bd[0] <= c.bd[1] <= 64 and c.o4[0] <= c.o4[1] <= 64


def as_items(rows):
    return np.ascontiguousarray(rows).view("V81").reshape(-1)


def test_rows_are_distinct():
    """Every grid row of a buffer, and every puzzle row of at least four clues, occurs once; no puzzle row is
    a grid row."""
    seen = set()
    for c in I.pool():
        for p, g in ((c.puzzles, c.grids),):
            p = p.base if p.base is not None else p
            g = g.base if g.base is not None else g
            if (id(p), id(g)) in seen:
                continue
            seen.add((id(p), id(g)))
            gi = as_items(g)
            assert len(np.unique(gi)) == len(gi), c.name
            pi = as_items(p[(p != 0).sum(axis=1) >= 4])
            assert len(np.unique(pi)) == len(pi), c.name
            assert len(np.intersect1d(as_items(p), gi)) == 0, c.name
    assert len(seen) >= 6


def test_row_bytes():
    """Every clue count 0..81, and the byte values a digit-minded copy or count would get wrong."""
    p = I.big_rows()[0]
    counts = set()
    for c in I.family("table")[:80]:
        counts |= set(np.unique((c.puzzles != 0).sum(axis=1)).tolist())
    counts |= set(np.unique((p != 0).sum(axis=1)).tolist())
    assert counts == set(range(82))
    for c in (I.family("table")[0], I.family("ballot")[0], I.family("quota")[0]):
        for a in (c.puzzles, c.grids):
            v = set(np.unique(a).tolist())
            assert {0, 9, 10, 0x80, 0xFF} <= v and len(v) > 250, c.name


def test_table_is_the_cross_product():
    lays = [I._table_layout(p) for p in range(I.TABLE_PERMS)]
    for lay in lays:
        assert len(lay) == I.TABLE_ROWS == 12740 and len(np.unique(lay, axis=0)) == len(lay)
    tab = I.family("table")
    triples = {c.tag[:3] for c in tab}
    assert len(triples) == len(I.CLUE_RANGES) * len(I.FILTER_RANGES) ** 2 == 80
    pairs = {c.tag[3:5] for c in tab}
    assert len(pairs) == 60 and {p[0] for p in pairs} == set(I.MASKS) and {p[1] for p in pairs} == set(I.PRESENCES)
    assert {c.tag[3:5] for c in tab if c.tag[:3] == ((22, 26), (3, 7), (3, 7))} == pairs
    # every range of either filter is read -- the filter given and level 4 in the mask -- alone and beside
    # the other filter
    read = {(which, c.tag[1 + which], c.tag[4][1 - which]) for c in tab for which in (0, 1)
            if c.tag[4][which] and c.tag[3] & 0x10}
    assert read == {(which, r, other) for which in (0, 1) for r in I.FILTER_RANGES for other in (False, True)}
    for which in (0, 1):                    # ... and in the dealt cases alone each range meets every presence
        assert {(c.tag[1 + which], c.tag[4]) for c in tab[:80]} == {(r, p) for r in I.FILTER_RANGES for p in I.PRESENCES}
    for c in tab[:80] + tab[140:]:
        (clo, chi), (blo, bhi), (olo, ohi) = c.tag[:3]
        m = c.m
        assert set(c.status[:m].tolist()) == set(I.STATUSES) and set(c.level[:m].tolist()) == set(I.LEVELS)
        clues = (c.puzzles[:m] != 0).sum(axis=1)
        assert set(clues.tolist()) == {v for v in (clo - 1, clo, chi, chi + 1) if 0 <= v <= 81}
        for a, (lo, hi) in ((I._table_arrays("bd", (blo, bhi), c.tag[5]), (blo, bhi)),
                            (I._table_arrays("o4", (olo, ohi), c.tag[5]), (olo, ohi))):
            assert set(a[:m].tolist()) == {v % 256 for v in (0, lo - 1, lo, hi, hi + 1, 64, 255)}
    # the rows land in every lane: every value of every column meets every lane, and over the family every
    # lane holds hits of every level
    lane = np.arange(I.TABLE_ROWS) % 64
    for lay in lays:
        for col, values in enumerate((5, 13, 4, 7, 7)):
            assert len(set(zip(lane.tolist(), lay[:, col].tolist()))) == 64 * values
    per_lane = np.zeros((5, 64), dtype=np.int64)
    for c in tab:
        hit = np.zeros(c.tiles * 64, dtype=bool)
        hit[:c.m] = M.ref_hits(c)
        assert not hit[c.m:].any() and 0 < hit.sum() < c.m / 4
        for lv in (1, 2, 3, 4):
            per_lane[lv] += np.bincount(lane[hit[:c.m] & (c.level[:c.m] == lv)], minlength=64)
    assert (per_lane[1:] > 0).all()


def test_ballot_shapes():
    fam = I.family("ballot")
    assert {(c.tag[0], c.base) for c in fam} == {(s, b) for s in I.BALLOTS for b in range(16)}
    assert {c.tiles for c in fam} == {1, 2, 3}
    want = {"lane0": 1, "lane31": 1 << 31, "lane32": 1 << 32, "lane63": 1 << 63, "lanes0_63": 1 | 1 << 63,
            "low_half": 0xFFFFFFFF, "high_half": 0xFFFFFFFF << 32, "even": 0x5555555555555555,
            "odd": 0xAAAAAAAAAAAAAAAA, "all": (1 << 64) - 1, "none": 0}
    carried = set()
    for c in fam:
        ballot = int(M.model_flag(c)[1][-1])
        hit = M.ref_hits(c)[-64:]
        assert ballot == sum(1 << i for i in np.flatnonzero(hit).tolist())
        if c.tag[0] in want:
            assert ballot == want[c.tag[0]], c.name
        if c.tag[0] == "all" and refs()[c.name].rank0[-1] > 0:
            carried.add(int(refs()[c.name].rank0[-1]) % 16)
    assert len(carried) >= 8                   # 64 of 64 behind a non-zero carry, at many phases


def test_every_phase_meets_every_length():
    """Over the steered cases every (rank0 mod 16, kept) with kept in 1..64 occurs; the two special cases are
    what they say."""
    seen = np.zeros((16, 65), dtype=bool)
    for c in I.family("phase")[:2]:
        assert c.tiles == 2049
        r = refs()[c.name]
        seen[r.rank0 % 16, r.kept] = True
    assert seen[:, 1:].all(), np.argwhere(~seen[:, 1:])[:5]
    one, full = I.family("phase")[2:]
    assert (refs()[one.name].kept == 1).all() and one.tiles == 2049
    assert (refs()[full.name].kept == 64).all() and full.tiles == 2049


def test_quota_cuts_every_length_at_every_phase():
    cut = np.zeros((16, 65), dtype=bool)
    for c in I.family("quota"):
        r = refs()[c.name]
        if c.tag[0] == "cut":
            assert r.kept.tolist() == [64, c.tag[2], 0] and c.n - r.rank0[1] == c.tag[2]
            cut[r.rank0[1] % 16, c.n - r.rank0[1]] = True
    assert cut[:, 1:].all()
    some = [c for c in I.family("quota") if c.tag[0] == "n"]
    for base in (0, 9):
        ns = {c.n for c in some if c.base == base}
        r = refs()[next(c.name for c in some if c.base == base)]
        for first in set(r.rank0[1:].tolist()):
            assert {first - 1, first, first + 1} <= ns
        assert {r.total - 1, r.total, r.total + 1, r.total + 100, base + 1} <= ns
    beyond = [c for c in some if c.n > refs()[c.name].total]
    assert beyond and all((refs()[c.name].out["puzzles"][refs()[c.name].total:] == I.FILL).all() for c in beyond)


def test_scan_partial_index_families():
    assert {c.tag for c in I.family("scan")} == {(t, p, b) for t in I.SCAN_TILES for p in I.SCAN_PATTERNS
                                                  for b in I.SCAN_BASES}
    for c in I.family("scan"):
        tiles, pattern, base = c.tag
        r = refs()[c.name]
        assert c.tiles == tiles and c.base == base
        counts = np.diff(np.append(r.rank0, r.total))
        if pattern == "last_tile":
            assert (counts[:-1] == 0).all() and counts[-1] > 0
        elif pattern == "tile_1024":
            assert counts.sum() == (counts[1024] if tiles > 1024 else 0) and (tiles <= 1024 or counts[1024] > 0)
        elif pattern == "all64":
            assert (counts == 64).all()
        else:
            assert tiles < 8 or (0 < (counts == 0).sum() < tiles and counts.max() == 64)
        assert r.total <= c.n or r.total == base
    assert sorted({c.m for c in I.family("partial")}) == sorted(I.PARTIAL_M)
    for c in I.family("partial"):
        # the rows from m on are hits in all but their row number
        whole = c.but(m=c.tiles * 64)
        assert M.ref_hits(whole).all() and len(c.status) == c.tiles * 64 and refs()[c.name].total == c.base + c.m
    assert [c.first for c in I.family("index")] == [0, (1 << 32) - 6, 1 << 32, (1 << 64) - 1 - 128]


def test_model_equals_reference():
    for c in I.pool():
        assert difference(c, M.select_model(c), refs()[c.name]) == [], c.name


def test_chained_rounds_equal_the_single_call():
    chains = I.chains()
    assert sum(len(r) == 2 for _, r, _ in chains) >= 8 and sum(len(r) == 3 for _, r, _ in chains) >= 3
    for whole, rounds, offsets in chains:
        ref = refs()[whole.name]
        out, total, scanned = M.blank(whole, whole.n), 0, None
        for c, lo in zip(rounds, offsets):
            assert c.base == (total if lo else 0) and c.n == whole.n and c.first == whole.first + lo
            r = M.select_ref(c, out)
            total = r.total
            if r.last:
                assert scanned is None
                scanned = lo + r.last
        for k, a in ref.out.items():
            assert np.array_equal(out[k], a), (whole.name, k)
        assert (scanned or 0) == ref.last
        if len(rounds) == len(offsets) and sum(c.m for c in rounds) == whole.m:
            assert total == ref.total


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_shows(mutant):
    assert set(KILLED_IN) == set(M.MUTANTS)
    for c in I.family(KILLED_IN[mutant]):
        try:
            got = M.select_model(c, mutant)
        except M.BeyondSlack:
            return
        if difference(c, got, refs()[c.name]):
            return
    raise AssertionError(f"{mutant} changes nothing in family {KILLED_IN[mutant]}")
