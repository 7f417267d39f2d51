"""The selection kernels (csrc/select_kernel.h: flag, scan, scatter) on rows of our choosing, through
SudokuEngine.select_rows_dev (sdk_select_rows_dev), against select_model.select_ref byte for byte on every
case of select_inputs.pool() -- test_select_model.py states what that pool covers and that every named way
of being wrong shows on it.

A test uploads every array of its cases once (cases share arrays), gives every output of every case a
place of its own in ONE device allocation pre-filled with the sentinel, each followed by 64 bytes of slack,
runs the calls, downloads the allocation once and compares ALL of it with the same image made from the
reference: the outputs, the rows from `total` (or n) on, the slack and the gaps between outputs alike."""
import ctypes
import time

import numpy as np
import pytest

import graded_model as G
import select_inputs as I
import select_model as M
from distributed_sudoku_solver_amd import _lib as L

pytestmark = pytest.mark.gpu

SLACK = 64
ITEM = {"puzzles": 81, "grids": 81, "level": 1, "open": 1, "index": 8, "backdoors": 1, "key": 1, "open4": 1}
SOURCES = ("puzzles", "grids", "status", "level", "open", "backdoors", "key", "open4")


def root(a):
    while isinstance(a.base, np.ndarray):
        a = a.base
    return a


def address(a):
    return a.__array_interface__["data"][0]


class Inputs:
    """The cases' source arrays in one device allocation: every distinct underlying array once."""

    def __init__(self, eng, cases):
        self.at, size, roots = {}, 0, []
        for c in cases:
            for k in SOURCES:
                a = getattr(c, k)
                if a is not None and id(root(a)) not in self.at:
                    self.at[id(root(a))] = size
                    roots.append(root(a))
                    size += (root(a).nbytes + 255) // 256 * 256
        self.buf = eng.alloc(size)
        for r in roots:
            self.buf.upload(r.reshape(-1).view(np.uint8), self.at[id(r)])

    def ptr(self, a):
        if a is None:
            return None
        return self.buf.ptr.value + self.at[id(root(a))] + address(a) - address(root(a))


class Outputs:
    """One device allocation for the outputs of `groups` (a group: calls that write the same outputs, one
    after the other -- a chain of rounds; else a single call), filled with the sentinel.  `shift` moves
    every output 16 or 32 bytes off its 256-byte place."""

    def __init__(self, eng, groups, shift=0):
        self.where, size = [], 0
        for g in groups:
            place = {}
            for k, item in ITEM.items():
                if k in ("puzzles", "grids") or k in g[0].outs:
                    place[k] = size + shift
                    size += (shift + g[0].n * item + SLACK + 255) // 256 * 256
            self.where.append(place)
        self.size = size
        self.buf = eng.alloc(size)
        self.buf.upload(np.full(size, I.FILL, dtype=np.uint8))

    def image(self, groups):
        """The allocation as the reference leaves it."""
        img = np.full(self.size, I.FILL, dtype=np.uint8)
        results = []
        for g, place in zip(groups, self.where):
            out = M.blank(g[0], g[0].n)
            for c in g:
                r = M.select_ref(c, out)
                results.append((r.total, r.last))
            for k, at in place.items():
                b = out[k].reshape(-1).view(np.uint8)
                img[at:at + len(b)] = b
        return img, results


def arguments(c, inputs, place):
    a = L.SelectRows()
    for k in SOURCES:
        setattr(a, k, inputs.ptr(getattr(c, k)))
    a.m, a.first, a.base, a.n, a.level_mask = c.m, c.first, c.base, c.n, c.mask
    (a.clues_lo, a.clues_hi), (a.backdoors_lo, a.backdoors_hi), (a.open4_lo, a.open4_hi) = c.clues, c.bd, c.o4
    for k in ITEM:
        setattr(a, "out_" + k, place.get(k))
    return a


def run(eng, groups, shift=0):
    """Every call of every group against the reference: the whole output allocation, total and last."""
    groups = [g if isinstance(g, (list, tuple)) else [g] for g in groups]
    cases = [c for g in groups for c in g]
    inputs = Inputs(eng, cases)
    outputs = Outputs(eng, groups, shift)
    try:
        got = []
        for g, place in zip(groups, outputs.where):
            dev = {k: outputs.buf.ptr.value + at for k, at in place.items()}
            for c in g:
                got.append(eng.select_rows_dev(arguments(c, inputs, dev)))
        eng.synchronize()
        mem = outputs.buf.download(np.empty(outputs.size, dtype=np.uint8))
    finally:
        inputs.buf.free()
        outputs.buf.free()
    img, exp = outputs.image(groups)
    for c, a, b in zip(cases, got, exp):
        assert a == b, (c.name, "total, last", a, b)
    if not np.array_equal(mem, img):
        at = int(np.flatnonzero(mem != img)[0])
        for g, place in zip(groups, outputs.where):
            for k, lo in place.items():
                if lo - shift <= at < lo + g[0].n * ITEM[k] + SLACK:
                    raise AssertionError((g[0].name, k, "byte", at - lo, "of", g[0].n * ITEM[k], int(mem[at]), int(img[at])))
        raise AssertionError(("a byte outside every output", at))
    return got


@pytest.mark.parametrize("family", ["table", "ballot", "phase", "quota", "partial", "index"])
def test_family(engine, family):
    t = time.perf_counter()
    cases = I.family(family)
    run(engine, cases)
    print(family, len(cases), "cases", round(time.perf_counter() - t, 2), "s")


@pytest.mark.parametrize("tiles", I.SCAN_TILES)
def test_scan(engine, tiles):
    cases = [c for c in I.family("scan") if c.tiles == tiles]
    assert len(cases) == len(I.SCAN_PATTERNS) * len(I.SCAN_BASES)
    run(engine, cases)


@pytest.mark.parametrize("shift", [16, 32])
def test_outputs_aligned_to_16_and_no_more(engine, shift):
    cases = I.family("ballot") + I.family("partial") + [c for c in I.family("quota") if c.tag[0] == "n"]
    run(engine, cases, shift=shift)


def some_cases():
    """A few cases of every small family, with and without the filter sources."""
    table = [c for c in I.family("table") if c.name.startswith("table_pair_")]
    return I.family("ballot")[::7] + I.family("partial") + table[::4] + I.family("index")


@pytest.mark.parametrize("without", list(I.NULLABLE) + ["all"])
def test_nullable_outputs(engine, without):
    """An output left out: the others are what they were (the reference knows which are given)."""
    left = I.NULLABLE if without == "all" else (without,)
    outs = [k for k in I.NULLABLE if k not in left]
    run(engine, [c.but(outs=outs) for c in some_cases()])


def test_absent_sources_give_none(engine):
    """A source left out and its output given: 0xFF, SDK_RATE_NONE / SDK_SUBSETS_NONE, at every kept rank."""
    assert L.SDK_RATE_NONE == L.SDK_SUBSETS_NONE == 0xFF
    both = [c for c in some_cases() if c.backdoors is not None and c.open4 is not None]
    assert len(both) >= 8
    cases = []
    for c in both:
        cases += [c.but(backdoors=None), c.but(key=None), c.but(open4=None), c.but(backdoors=None, key=None, open4=None)]
    for c in cases[3::4]:       # (of the reference itself: that is what it expects at every kept rank)
        r = M.select_ref(c)
        kept = slice(c.base, min(c.n, r.total))
        assert r.total > c.base
        for k in ("backdoors", "key", "open4"):
            assert (r.out[k][kept] == 0xFF).all()
    run(engine, cases)          # the kernels against it


def test_chained_rounds_equal_the_single_call(engine):
    chains = I.chains()
    got = run(engine, [[w] for w, _, _ in chains] + [r for _, r, _ in chains])
    whole, k = got[:len(chains)], len(chains)
    for (w, rounds, offsets), (total, last) in zip(chains, whole):
        mine = got[k:k + len(rounds)]
        k += len(rounds)
        scanned = [lo + la for lo, (_, la) in zip(offsets, mine) if la]
        assert scanned == ([last] if last else []), w.name
        if sum(c.m for c in rounds) == w.m:
            assert mine[-1][0] == total
        for c, (t, _) in zip(rounds[1:], mine):
            assert c.base == t                       # a round starts at the total of the one before


def test_pipeline_agreement(engine):
    """What generate_batch and grade_batch give for rows 1000..3047 of seed 7, fed to the seam: the rows
    generate_graded returns for the same window."""
    eng = engine
    puz, sol, st = eng.generate_batch(G.ROWS, seed=G.SEED, lo=G.FIRST)
    _, level, open_, _ = eng.grade_batch(puz, budget=0)
    for levels, n, clues in (((3,), 40, (0, 81)), ((1, 2, 3, 4), 300, (0, 81)), ((1, 2, 3, 4), 512, (21, 23)),
                             ((1,), 64, (0, 81))):
        mask = sum(1 << lv for lv in levels)
        c = I.Case("pipeline", "pipeline", puz, sol, st, level, open_, G.ROWS, 0, n, first=G.FIRST, mask=mask,
                   clues=clues, outs=("level", "open", "index"))
        (total, last), = run(eng, [c])
        ref = M.select_ref(c)
        res = eng.generate_graded(n, levels, seed=G.SEED, lo=G.FIRST, clues=clues, max_scan=G.ROWS)
        found = min(n, total)
        assert len(res[0]) == found and res[5] == (last if total >= n else G.ROWS)
        for a, k in zip(res[:5], ("puzzles", "grids", "level", "open", "index")):
            assert np.array_equal(a, ref.out[k][:found]), (levels, k)


def test_argument_errors(engine):
    """Each is SDK_EINVAL with a message; nothing is launched or written, total and last included."""
    eng = engine
    c = I.family("partial")[-1]
    assert c.backdoors is not None and c.m % 64 == 1
    inputs, outputs = Inputs(eng, [c]), Outputs(eng, [[c]])
    top = (1 << 64) - 1
    bad = [dict(move=("out_puzzles", 1)), dict(move=("out_grids", 8)), dict(move=("out_index", 4)),
           dict(move=("puzzles", 1)), dict(move=("grids", 15))]
    bad += [{k: None} for k in ("puzzles", "grids", "status", "level", "open", "out_puzzles", "out_grids")]
    bad += [dict(m=0), dict(m=(1 << 24) + 1), dict(n=0), dict(n=1 << 31), dict(base=c.n), dict(base=c.n + 1),
            dict(level_mask=0), dict(level_mask=1), dict(level_mask=0x20), dict(level_mask=0x1F),
            dict(clues_lo=30, clues_hi=29), dict(clues_hi=82), dict(backdoors_lo=5, backdoors_hi=4),
            dict(backdoors_hi=65), dict(open4_lo=5, open4_hi=4), dict(open4_hi=65), dict(first=top - c.m + 1),
            dict(first=top)]
    try:
        dev = {k: outputs.buf.ptr.value + at for k, at in outputs.where[0].items()}
        for kw in bad:
            a = arguments(c, inputs, dev)
            for k, v in kw.items():
                if k == "move":                     # a pointer off its alignment
                    setattr(a, v[0], getattr(a, v[0]) + v[1])
                else:
                    setattr(a, k, v)
            total, last = ctypes.c_uint64(12345), ctypes.c_uint64(12345)
            rc = eng.lib.sdk_select_rows_dev(eng.ctx, ctypes.byref(a), ctypes.byref(total), ctypes.byref(last))
            assert rc == L.SDK_EINVAL, kw
            assert eng.lib.sdk_last_error(), kw
            assert (total.value, last.value) == (12345, 12345), kw
        a = arguments(c, inputs, dev)
        one = ctypes.c_uint64(12345)
        for args in ((None, ctypes.byref(one), ctypes.byref(one)), (ctypes.byref(a), None, ctypes.byref(one)),
                     (ctypes.byref(a), ctypes.byref(one), None)):
            assert eng.lib.sdk_select_rows_dev(eng.ctx, *args) == L.SDK_EINVAL and one.value == 12345
        eng.synchronize()
        mem = outputs.buf.download(np.empty(outputs.size, dtype=np.uint8))
        assert (mem == I.FILL).all()
        # the last indices of the stream are a valid round
        a = arguments(c, inputs, dev)
        a.first = top - c.m
        total, last = eng.select_rows_dev(a)
        assert total == c.base + c.m
    finally:
        inputs.buf.free()
        outputs.buf.free()


def test_one_timing_span(engine):
    eng = engine
    c = I.family("quota")[100]
    inputs, outputs = Inputs(eng, [c]), Outputs(eng, [[c]])
    try:
        dev = {k: outputs.buf.ptr.value + at for k, at in outputs.where[0].items()}
        eng.timer_reset()
        got = eng.select_rows_dev(arguments(c, inputs, dev))
        eng.synchronize()
        ms, spans = eng.timer_read()
        assert got == (M.select_ref(c).total, M.select_ref(c).last) and spans == 1 and ms > 0.0
    finally:
        eng.timer_stop()
        inputs.buf.free()
        outputs.buf.free()
