"""sdk_set_option / sdk_get_option over every SDK_OPT_* key of include/sudoku_hip.h: defaults of a fresh
context, accepted ranges (their edges round-trip, the first value outside is SDK_EINVAL with a message
and changes nothing), read-only and unknown keys.  One context of its own, no kernel launch."""
import ctypes
import re

import pytest

from distributed_sudoku_solver_amd import SudokuEngine, _lib as L

pytestmark = pytest.mark.gpu

I64_MAX = (1 << 63) - 1

# key name -> (default, lowest accepted, highest accepted); a highest of I64_MAX has no value above it
WRITABLE = {
    "SDK_OPT_ORDER": (L.SDK_ORDER_LEX, 0, 1),
    "SDK_OPT_NODE_BUDGET": (0, 0, I64_MAX),
    "SDK_OPT_WAVES_PER_CU": (32, 1, 32),
    "SDK_OPT_CHECK_BLOCKS_PER_CU": (3, 1, 16),
    "SDK_OPT_WORK_COUNTER": (L.SDK_WORK_NODES, 0, 2),
    "SDK_OPT_SOLVER": (L.SDK_SOLVER_QUAD, 0, 3),
    "SDK_OPT_WAVES_PER_CU2": (28, 1, 32),
    "SDK_OPT_CHECK_VARIANT": (L.SDK_CHECK_REG1, 0, 6),
    "SDK_OPT_SOLVE_CHUNK": (0, 0, 4096),
    "SDK_OPT_TIMING": (0, 0, 1),
    "SDK_OPT_LOCKED": (1, 0, 2),
    "SDK_OPT_XCD_HEADS": (1, 0, 1),
    "SDK_OPT_DONATE": (1, 0, 1 << 30),
    "SDK_OPT_DONATE_MODE": (1, 0, 1),
    "SDK_OPT_DONATE_MAX": (1 << 19, 0, I64_MAX),
    "SDK_OPT_DN_FAULT": (0, 0, 1),
    "SDK_OPT_DONATE_HELPERS": (2, 1, 4096),
    "SDK_OPT_DONATE_RESUME": (1, 0, 1),
    "SDK_OPT_PROP32": (1, 0, 1),
    "SDK_OPT_PROP32_MIN": (4096, 1, I64_MAX),
    "SDK_OPT_PROP32_HANDOVER": (1, 0, 1),
    "SDK_OPT_GEN_CAP": (1 << 20, 81, (1 << 31) - 1),
}

# packed keys: (default, accepted values at the packed edges, the first values outside them)
PACKED = {
    # period 1..64 (low byte) | first step 0..64 << 8
    "SDK_OPT_PROP32_LC": (5 | 3 << 8, [1, 64, 1 | 64 << 8, 64 | 64 << 8], [-1, 0, 65, 3 << 8, 1 | 65 << 8]),
    # live 0..64 (low byte) | step 0..96 << 8
    "SDK_OPT_PROP32_TAIL": (24 << 8, [0, 64, 96 << 8, 64 | 96 << 8], [-1, 65, 97 << 8, 64 | 97 << 8]),
}

# read-only keys: the five that read device memory are 0 before any solve
READ_ONLY = {
    "SDK_OPT_DEVICE_CUS": None,
    "SDK_OPT_TIMER_EVENTS": 0,
    "SDK_OPT_DONATED": 0,
    "SDK_OPT_SPLIT_BOARDS": 0,
    "SDK_OPT_LEX_BOARDS": 0,
    "SDK_OPT_RESUMED": 0,
    "SDK_OPT_PROP32_UNDECIDED": 0,
}


def header_keys():
    with open(L.HEADER) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(SDK_OPT_\w+)\s+(\d+)\b", f.read())}


KEYS = header_keys()


@pytest.fixture(scope="module")
def ctx():
    with SudokuEngine(0) as eng:
        yield eng


def set_raw(eng, key, value):
    """(return code, sdk_last_error) of one sdk_set_option."""
    rc = eng.lib.sdk_set_option(eng.ctx, key, value)
    return rc, (eng.lib.sdk_last_error() or b"").decode()


def test_every_header_key_is_bound_and_covered():
    assert len(KEYS) == 31 and sorted(KEYS.values()) == list(range(1, 32))
    for name, key in KEYS.items():
        assert getattr(L, name) == key, name
    assert set(KEYS) == set(WRITABLE) | set(PACKED) | set(READ_ONLY)
    assert len(KEYS) == len(WRITABLE) + len(PACKED) + len(READ_ONLY)


def test_defaults_of_a_fresh_context():
    with SudokuEngine(0) as eng:
        for name, (default, _, _) in WRITABLE.items():
            assert eng.get_option(KEYS[name]) == default, name
        for name, (default, _, _) in PACKED.items():
            assert eng.get_option(KEYS[name]) == default, name
        for name, default in READ_ONLY.items():
            if default is not None:
                assert eng.get_option(KEYS[name]) == default, name
        assert eng.get_option(L.SDK_OPT_DEVICE_CUS) > 0


@pytest.mark.parametrize("name", sorted(WRITABLE))
def test_writable_range(ctx, name):
    key = KEYS[name]
    default, lo, hi = WRITABLE[name]
    try:
        for v in (lo, hi):
            assert set_raw(ctx, key, v)[0] == L.SDK_OK, (name, v)
            assert ctx.get_option(key) == v, (name, v)
            for bad in (lo - 1,) + ((hi + 1,) if hi < I64_MAX else ()):
                rc, msg = set_raw(ctx, key, bad)
                assert rc == L.SDK_EINVAL and msg, (name, bad)
                assert ctx.get_option(key) == v, (name, bad)
    finally:
        ctx.set_option(key, default)


@pytest.mark.parametrize("name", sorted(PACKED))
def test_packed_edges(ctx, name):
    key = KEYS[name]
    default, good, bad = PACKED[name]
    try:
        for v in good:
            assert set_raw(ctx, key, v)[0] == L.SDK_OK, (name, v)
            assert ctx.get_option(key) == v, (name, v)
            for b in bad:
                rc, msg = set_raw(ctx, key, b)
                assert rc == L.SDK_EINVAL and msg, (name, b)
                assert ctx.get_option(key) == v, (name, b)
    finally:
        ctx.set_option(key, default)


@pytest.mark.parametrize("name", sorted(READ_ONLY))
def test_read_only_keys_refuse_every_set(ctx, name):
    key = KEYS[name]
    before = ctx.get_option(key)
    for v in (-1, 0, 1, before, I64_MAX):
        rc, msg = set_raw(ctx, key, v)
        assert rc == L.SDK_EINVAL and msg, (name, v)
    assert ctx.get_option(key) == before


@pytest.mark.parametrize("key", [0, 32])
def test_unknown_keys(ctx, key):
    assert key not in KEYS.values()
    rc, msg = set_raw(ctx, key, 0)
    assert rc == L.SDK_EINVAL and msg
    v = ctypes.c_int64(-7)
    assert ctx.lib.sdk_get_option(ctx.ctx, key, ctypes.byref(v)) == L.SDK_EINVAL
    assert (ctx.lib.sdk_last_error() or b"")
