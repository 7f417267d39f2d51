"""The checker kernels (csrc/check_kernel.h: seven tile pipelines and the int64 kernel) against
oracle.py_check on the case pool of check_inputs.py: every 9-multiset over 0..9, every passing set, the
near misses at the kernel's bit tricks, boards that fail in one row, one column or one box only, boards
whose rows and columns pass while boxes fail -- in every pipeline, in every thread slot of a tile and in ragged tails.

The expected verdict is always py_check's, computed once per process (check_inputs.expected)."""
import ctypes

import numpy as np
import pytest

from distributed_sudoku_solver_amd import _lib as L
from oracle import oracle as O
import check_inputs as I

pytestmark = pytest.mark.gpu

VARIANTS = {"REG1": L.SDK_CHECK_REG1, "REG2": L.SDK_CHECK_REG2, "GLDS2": L.SDK_CHECK_GLDS2,
            "GLDS3": L.SDK_CHECK_GLDS3, "GLDS4": L.SDK_CHECK_GLDS4, "WAVE1": L.SDK_CHECK_WAVE1,
            "WAVE2": L.SDK_CHECK_WAVE2}
TAILS = (0, 1, 63, 64, 65, 255)
RING = 768      # the 600-board mix, continued with its own head to three tiles: rotating by o moves every
                # case through (its place - o) mod 256, i.e. through every thread slot of a full tile


class _options:
    """Set checker options on the shared engine and put back what was there."""

    def __init__(self, engine, **opts):
        self.engine, self.opts = engine, {getattr(L, "SDK_OPT_" + k): v for k, v in opts.items()}

    def __enter__(self):
        self.old = {k: self.engine.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.engine.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.engine.set_option(k, v)


def _assert_equal(got, exp, index, what):
    bad = np.flatnonzero(got != exp)
    if bad.size:
        boards, tags = I.pool()
        i = bad[0]
        pytest.fail(f"{what}: {bad.size} verdicts differ; first at {i}: tag {tags[index[i]]}, got {got[i]}, "
                    f"py_check {exp[i]}, board {boards[index[i]].tolist()}")


def _ring():
    m = I.mix()
    return np.concatenate([m, m[:RING - len(m)]])


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_whole_pool_every_variant(engine, variant):
    boards, exp = I.pool()[0], I.expected()
    with _options(engine, CHECK_VARIANT=VARIANTS[variant]):
        _assert_equal(engine.check_batch(boards), exp, np.arange(len(boards)), variant)


@pytest.mark.parametrize("variant", ["REG1", "GLDS3", "WAVE2"])
def test_every_case_in_every_thread_slot(engine, variant):
    """Batches of 768 + r boards (three full tiles and a ragged tail of r), the mix rotated by every offset
    0..255: each case sits in every thread slot t (every phase 81t & 3 and first dword d0 of the LDS
    re-alignment) of a full tile, and the head of the mix, which holds every family, runs through the tail."""
    boards, exp, ring = I.pool()[0], I.expected(), _ring()
    assert all(len({(j - o) % RING % 256 for o in range(256)}) == 256 for j in (0, 255, 599))
    with _options(engine, CHECK_VARIANT=VARIANTS[variant]):
        for r in TAILS:
            pos = np.arange(RING + r)
            for o in range(256):
                idx = ring[(pos + o) % RING]
                _assert_equal(engine.check_batch(boards[idx]), exp[idx], idx, (variant, r, o))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_two_tiles_per_workgroup_and_more(engine, variant):
    """One workgroup per CU and 2 * CUs + 1 tiles (the last ragged): REG2 runs check_kernel_rr2 instead of
    falling back to REG1, every ring slot of the other pipelines is used, and the workgroups that get a
    third tile wrap their ring."""
    boards, exp, ring = I.pool()[0], I.expected(), _ring()
    cus = engine.get_option(L.SDK_OPT_DEVICE_CUS)
    n = 256 * cus * 2 + 17
    idx = ring[(np.arange(n) + 101) % RING]
    with _options(engine, CHECK_VARIANT=VARIANTS[variant], CHECK_BLOCKS_PER_CU=1):
        _assert_equal(engine.check_batch(boards[idx]), exp[idx], idx, (variant, n))


def test_int64_kernel_on_the_pool(engine):
    boards, exp = I.pool()[0], I.expected()
    got = engine.check_batch(boards.astype(np.int64))
    _assert_equal(got, exp, np.arange(len(boards)), "int64")
    tags = I.pool()[1]
    for t in ("single_row_col", "single_box", "four_boxes", "four_boxes_exact", "latin_box00_45"):
        assert (got[tags == t] == exp[tags == t]).all()
    assert (got == 2).sum() == (exp == 2).sum() >= 250


def test_int64_kernel_wide_values(engine):
    wide = I.wide_cases()
    exp = np.array([I.py_verdict(O, b) for b in wide.tolist()], dtype=np.uint8)
    assert exp[:3].tolist() == [3, 3, 3] and (exp[3:] == 0).sum() >= 60 and int(np.abs(wide).max()) == (1 << 59) - 1
    got = engine.check_batch(wide)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (wide[bad[0]].tolist(), int(got[bad[0]]), int(exp[bad[0]]))


def test_device_form_equals_host_form(engine):
    boards, exp = I.pool()[0], I.expected()
    n = len(boards)
    assert n % 256 not in (0, 1)
    guard = 300
    d_b, d_v = engine.alloc(n * 81 + 16), engine.alloc(n + guard)
    try:
        d_b.upload(boards)
        for name, variant in VARIANTS.items():
            with _options(engine, CHECK_VARIANT=variant):
                for m in (n, 256 * 3 + 1, 255):
                    d_v.upload(np.full(n + guard, 0xAB, dtype=np.uint8))
                    engine.check_batch_dev(d_b, d_v, m)
                    engine.synchronize()
                    out = d_v.download(np.empty(n + guard, dtype=np.uint8))
                    _assert_equal(out[:m], exp[:m], np.arange(m), (name, m))
                    assert (out[m:] == 0xAB).all(), (name, m)          # nothing written behind row m
    finally:
        d_b.free()
        d_v.free()


def test_device_form_argument_checks(engine):
    lib, ctx = engine.lib, engine.ctx
    n = 300
    d_b, d_v = engine.alloc(n * 81 + 16), engine.alloc(n)
    try:
        d_b.upload(np.ascontiguousarray(I.pool()[0][:n]))
        d_v.upload(np.full(n, 0xAB, dtype=np.uint8))
        off = ctypes.c_void_p(d_b.ptr.value + 1)
        assert lib.sdk_check_batch_dev(ctx, off, d_v.ptr, n - 1) == L.SDK_EINVAL
        assert b"aligned" in lib.sdk_last_error()
        assert lib.sdk_check_batch_dev(ctx, None, d_v.ptr, n) == L.SDK_EINVAL
        assert b"NULL" in lib.sdk_last_error()
        assert lib.sdk_check_batch_dev(ctx, d_b.ptr, None, n) == L.SDK_EINVAL
        assert b"NULL" in lib.sdk_last_error()
        assert lib.sdk_check_batch_dev(None, d_b.ptr, d_v.ptr, n) == L.SDK_EINVAL
        assert lib.sdk_check_batch_dev(ctx, None, None, 0) == L.SDK_OK
        assert lib.sdk_check_batch_dev(ctx, off, d_v.ptr, 0) == L.SDK_OK
        engine.synchronize()
        assert (d_v.download(np.empty(n, dtype=np.uint8)) == 0xAB).all()      # no refused call wrote
    finally:
        d_b.free()
        d_v.free()
