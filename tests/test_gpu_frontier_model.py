"""The frontier kernels against the scalar model (frontier_model.py), byte for byte: one expansion
level at exact parent counts, multi-level builds in both modes, the refinements, record loads and
the first-solution scan.  Every comparison covers the size, the leaves and every record byte."""
import ctypes
import functools

import numpy as np
import pytest

from distributed_sudoku_solver_amd import synth, _lib as L
from oracle import oracle as O
import frontier_inputs as I
import frontier_model as M

pytestmark = pytest.mark.gpu

SOLVERS = [L.SDK_SOLVER_QUAD, L.SDK_SOLVER_HALFWAVE]          # expand4_kernel, expand_kernel
LEVEL_COUNTS = [1, 2, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, 8193]
INT64_MAX = 2 ** 63 - 1
END = 2 ** 64 - 1


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


def _records(e, lo=0, hi=None):
    """Records [lo, hi) of the context's frontier, downloaded."""
    size = e.frontier_boards()[1]
    hi = size if hi is None else hi
    if hi <= lo:
        return np.empty((0, 81), np.uint8)
    ptr, nbytes = e.frontier_records(lo, hi)
    host = np.empty(nbytes, np.uint8)
    if nbytes:
        L.check(e.lib.sdk_memcpy_d2h(e.ctx, host.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), nbytes))
    return host.reshape(-1, 81)


def _same_records(got, want, what):
    if got.shape == want.shape and (got == want).all():
        return
    k = min(len(got), len(want))
    diff = np.argwhere(got[:k] != want[:k])
    where = f"first difference at record {diff[0][0]}, cell {diff[0][1]}: {got[tuple(diff[0])]} for " \
            f"{want[tuple(diff[0])]}" if len(diff) else "the common records agree"
    raise AssertionError(f"{what}: {len(got)} records for the model's {len(want)}; {where}")


def _same(e, size_leaves, want, what):
    """The context's frontier and the (size, leaves) its call returned against a model Frontier."""
    size, leaves = size_leaves
    got = _records(e)
    assert size == len(got), what
    _same_records(got, want.records, what)
    assert leaves == want.leaves, (what, leaves, want.leaves)


# ------------------------------------------------------------------ one level
@functools.lru_cache(maxsize=None)
def _model_level(n, masked):
    out = M.level(I.seed_pool()[:n], I.seed_masks()[:n] if masked else None, M.FIRST)[0]
    out.setflags(write=False)
    return out


def _level_case(engine, n):
    pool, masks = I.seed_pool(), I.seed_masks()
    for masked in (True, False):
        got = engine.expand(pool[:n], masks[:n] if masked else None, target=1)
        _same_records(got, _model_level(n, masked), f"{n} parents, masks {masked}")


def test_pool_holds_every_edge():
    pool, masks = I.seed_pool()[:8193], I.seed_masks()[:8193]
    first = np.where((pool == 0).any(axis=1), np.argmax(pool == 0, axis=1), 81)
    for lo, hi in ((0, 27), (27, 54), (54, 64), (64, 81), (81, 82)):
        assert ((first >= lo) & (first < hi)).any(), (lo, hi)
    assert (pool == 255).any() and ((pool > 9) & (pool < 255)).any()
    assert (pool == 0).all(axis=1).any() and ((pool == 0).sum(axis=1) == 1).any()
    real = (masks >> 1) & 0x1FF
    assert (real == 0).any() and (real == 0x1FF).any() and (M._POP[real] == 1).any()
    assert ((masks & 0xFC01) != 0).any()
    # an empty and a one-digit mask on a board whose lowest empty cell is cell 64..80
    late = first >= 64
    assert (late & (first < 81) & (real == 0)).any() and (late & (first < 81) & (M._POP[real] == 1)).any()
    verdict = M.propagate_batch(pool, masks)[0]
    assert set(verdict.tolist()) == {M.CONTRA, M.SOLVED, M.OPEN}


@pytest.mark.parametrize("n", LEVEL_COUNTS)
@pytest.mark.parametrize("solver", SOLVERS)
def test_one_level_at_exact_parent_counts(engine, solver, n):
    with _options(engine, SDK_OPT_SOLVER=solver):
        _level_case(engine, n)


def test_one_level_wave_solver_dispatch(engine):
    with _options(engine, SDK_OPT_SOLVER=L.SDK_SOLVER_WAVE):
        _level_case(engine, 65)


@pytest.mark.parametrize("solver", SOLVERS)
def test_one_level_grid_stride_second_pass(engine, solver):
    """One wave per CU: at 4 * CUs + 3 parents expand4_kernel's grid-stride loop runs a second pass."""
    n = 4 * engine.get_option(L.SDK_OPT_DEVICE_CUS) + 3
    assert n <= I.seed_pool().shape[0]
    with _options(engine, SDK_OPT_SOLVER=solver, SDK_OPT_WAVES_PER_CU2=1, SDK_OPT_WAVES_PER_CU=1):
        _level_case(engine, n)


# ------------------------------------------------------------------ multi-level builds
@functools.lru_cache(maxsize=None)
def _build_boards():
    inert = synth.parse(I.C5_16).copy()
    inert[int(np.flatnonzero(inert)[3])] = 255
    dup = I.with_duplicate(synth.parse(I.C5_16)[None], 3)[0]
    named = [synth.parse(I.C5_16), synth.parse(I.C5_15), synth.parse(I.DEMO), synth.parse(synth.WIKI), I.dead_wiki(),
             inert, dup]
    return named + list(I.sparse_boards(10, 51, 20, 30))


def _build_masks(k, mode):
    """The first-cell masks board k is built with: none; in first mode also one digit and a range
    (empty ones among them); in count mode a range for every third board."""
    ranges = I.range_masks(len(_build_boards()), 52)
    if mode == M.FIRST:
        return [None, 1 << (1 + k % 9), int(ranges[k])]
    return [None, int(ranges[k])] if k % 3 == 0 else [None]


@functools.lru_cache(maxsize=None)
def _model_build(k, mask, mode, target):
    return M.build(_build_boards()[k], mask, mode, target)


@pytest.mark.parametrize("target", [1, 2, 64, 5000])
@pytest.mark.parametrize("mode", [M.COUNT, M.FIRST])
@pytest.mark.parametrize("solver", SOLVERS)
def test_builds(engine, solver, mode, target):
    with _options(engine, SDK_OPT_SOLVER=solver):
        for k, b in enumerate(_build_boards()):
            for mask in _build_masks(k, mode):
                got = engine.frontier_build(b, mask, mode=mode, target=target)
                _same(engine, got, _model_build(k, mask, mode, target), f"board {k}, mask {mask}")


@pytest.mark.parametrize("mode", [M.COUNT, M.FIRST])
@pytest.mark.parametrize("solver", SOLVERS)
def test_build_crosses_the_scan_tile(engine, solver, mode):
    want = _model_build(1, None, mode, 20_000)
    assert max(want.parents) > 4096 and want.size >= 20_000
    with _options(engine, SDK_OPT_SOLVER=solver):
        got = engine.frontier_build(_build_boards()[1], None, mode=mode, target=20_000)
        _same(engine, got, want, "15-clue board at 20,000")


@functools.lru_cache(maxsize=None)
def _model_expand_seeds():
    seeds, masks = I.sparse_boards(40, 53, 20, 30), I.range_masks(40, 54)
    out = M.expand_boards(seeds, masks, 3000)
    out.setflags(write=False)
    return seeds, masks, out


@pytest.mark.parametrize("solver", SOLVERS)
def test_expand_several_seeds_several_levels(engine, solver):
    seeds, masks, want = _model_expand_seeds()
    assert len(want) >= 3000
    with _options(engine, SDK_OPT_SOLVER=solver):
        _same_records(engine.expand(seeds, masks, target=3000), want, "40 seeds at 3000")


# ------------------------------------------------------------------ refinement
@functools.lru_cache(maxsize=None)
def _base(mode):
    f = M.build(synth.parse(I.C5_16), None, mode, 600)
    assert 600 <= f.size < 1000
    return f


def _rebuild(engine, mode):
    got = engine.frontier_build(synth.parse(I.C5_16), None, mode=mode, target=600)
    assert got[0] == _base(mode).size
    return _base(mode)


@pytest.mark.parametrize("mode", [M.COUNT, M.FIRST])
@pytest.mark.parametrize("solver", SOLVERS)
def test_refine_strided_and_range(engine, solver, mode):
    with _options(engine, SDK_OPT_SOLVER=solver):
        for r in range(3):
            for target in (0, 2000):
                f = _rebuild(engine, mode)
                _same(engine, engine.frontier_refine(r, 3, target), f.refine(r, 3, END, target), f"refine {r}/3 {target}")
        size = _base(mode).size
        # an inner range; lo >= hi; hi beyond the size; T <= n: the gathered records, nothing expanded
        for lo, hi, target in ((100, 130, 900), (50, 50, 64), (70, 30, 64), (size - 9, size + 100, 300), (size, END, 64),
                               (10, 200, 50), (10, 200, 190)):
            f = _rebuild(engine, mode)
            want = f.refine(lo, 1, hi, target)
            _same(engine, engine.frontier_refine_range(lo, hi, target), want, f"range [{lo}, {hi}) {target}")
            if target <= max(0, min(hi, size) - lo):
                assert want.levels == 0 and (want.records == f.records[lo:hi]).all()


@pytest.mark.parametrize("mode", [M.COUNT, M.FIRST])
@pytest.mark.parametrize("solver", SOLVERS)
def test_refine_head(engine, solver, mode):
    size = _base(mode).size
    with _options(engine, SDK_OPT_SOLVER=solver):
        # no tail; mid < lo; hi beyond the size; mid = lo + 1 with a long tail; everything beyond the size
        for lo, mid, hi, target in ((20, 60, 60, 400), (40, 10, 90, 64), (size - 30, size - 20, size + 7, 200),
                                    (3, 4, size, 64), (size + 1, size + 2, size + 3, 64), (0, 5, 5, 0)):
            f = _rebuild(engine, mode)
            _same(engine, engine.frontier_refine_head(lo, mid, hi, target), f.refine_head(lo, mid, hi, target),
                  f"head [{lo}, {mid}, {hi}) {target}")


@pytest.mark.parametrize("mode", [M.COUNT, M.FIRST])
def test_refine_head_regrows_and_load_then_refine(engine, mode):
    """Records loaded from another context, then refined: refine_head(0, 1, 5000, 64) on a fresh
    context leaves a head and a tail that no longer fit the swapped buffer (the path that allocates a
    new one and copies); a loaded range refines as the model's load + refine."""
    src_model = _model_build(1, None, mode, 5000)
    assert src_model.size >= 5000
    a, b = engine.fork(), engine.fork()
    try:
        assert b.frontier_build(_build_boards()[1], None, mode=mode, target=5000)[0] == src_model.size
        a.frontier_build(synth.parse(synth.WIKI), None, mode=mode, target=1)        # the mode of the loads
        small = M.build(synth.parse(synth.WIKI), None, mode, 1)
        ptr, _ = b.frontier_records(0, 5000)
        a.frontier_load(ptr, 5000)
        loaded = small.load(src_model.records[:5000])
        _same(a, (a.frontier_boards()[1], 0), loaded, "load 5000")
        want = loaded.refine_head(0, 1, 5000, 64)
        assert want.size > 5000
        _same(a, a.frontier_refine_head(0, 1, 5000, 64), want, "regrow")
        # a range of another context's records, then each kind of refinement
        ptr, _ = b.frontier_records(1000, 1300)
        loaded = small.load(src_model.records[1000:1300])
        for call, model in ((lambda: a.frontier_refine(1, 4, 500), lambda f: f.refine(1, 4, END, 500)),
                            (lambda: a.frontier_refine_range(17, 90, 0), lambda f: f.refine(17, 1, 90, 0)),
                            (lambda: a.frontier_refine_head(5, 9, 400, 100), lambda f: f.refine_head(5, 9, 400, 100))):
            a.frontier_load(ptr, 300)
            _same(a, call(), model(loaded), "load 300 + refine")
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ the first-solution scan
def test_frontier_first_ranges(engine):
    f = _rebuild(engine, M.FIRST)
    rec = _records(engine)
    _same_records(rec, f.records, "first-mode base")
    status_all = engine.solve_batch(rec)[1]
    dead = np.flatnonzero(status_all == 0)
    assert len(dead) and status_all[0] != 0
    d0 = int(dead[0])
    run = d0 + 1
    while run < len(rec) and status_all[run] == 0:
        run += 1
    found_buf, best_buf = engine.result_buffer(1, np.int64), engine.alloc(128)
    seen = set()
    try:
        # empty; no hit; hi beyond the size; above the first hit; dead records, then a hit
        for lo, hi in ((10, 10), (30, 12), (d0, run), (len(rec) - 6, len(rec) + 50), (5, 40), (d0, min(run + 3, len(rec))),
                       (len(rec), END)):
            engine.frontier_first(lo, hi, found_buf, best_buf)
            found = int(engine.read(found_buf, 1, np.int64)[0])
            best = engine.read(best_buf, 128, np.uint8)
            part = rec[lo:min(hi, len(rec))] if lo < min(hi, len(rec)) else rec[:0]
            out, st, _ = engine.solve_batch(part) if len(part) else (part, np.zeros(0, np.int8), None)
            hits = np.flatnonzero(st != 0)
            if len(hits) == 0:
                assert found == INT64_MAX, (lo, hi, found)
                seen.add("none")
            else:
                k = int(hits[0])
                assert found == lo + k, (lo, hi, found, lo + k)
                assert (best[:81] == out[k]).all() and best[81].astype(np.int8) == st[k], (lo, hi)
                ref = O.naive_solve(part[k])
                assert ref[0] == 1 and (ref[1] == out[k]).all()
                seen.add("first" if k == 0 else "later")
    finally:
        found_buf.free()
        best_buf.free()
    assert seen == {"none", "first", "later"}


# ------------------------------------------------------------------ an empty range in a batched solve
@pytest.mark.parametrize("solver", [L.SDK_SOLVER_QUAD, L.SDK_SOLVER_HALFWAVE, L.SDK_SOLVER_WAVE])
def test_solve_batch_empty_mask_under_a_budget(engine, solver):
    """TASK range(5, 5): no digit may be tried at the first empty cell, so the reference returns False
    with the board as it was -- at its first node, so a budget of 64 nodes is never the answer."""
    boards = np.concatenate([synth.parse(synth.WIKI)[None], synth.parse(I.C5_16)[None], I.sparse_boards(6, 61, 20, 30)])
    masks = np.full(len(boards), O.range_mask(5, 5), np.uint16)
    assert (masks == 0).all()
    for b in boards:
        ref = O.naive_solve(b, 0)
        assert ref[0] == 0 and (ref[1] == b).all()
    with _options(engine, SDK_OPT_SOLVER=solver):
        out, st, _ = engine.solve_batch(boards, masks, budget=64)
        assert (st == 0).all(), st
        assert (out == boards).all()
