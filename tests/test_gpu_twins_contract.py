"""The twelve twin entry points -- sdk_{grade,rate,subsets}_batch[_dev] and
sdk_generate_{graded,rated,subsets}[_dev] -- through raw ctypes, so that engine.py's own argument checks
do not mask the library's: which pointers are required, what n == 0 does, the text and the ORDER of the
argument errors, and the host form against the device form byte for byte, sentinels behind the rows
included.  A pin of the ABI's behaviour: it passed unchanged on the library before the entry points
were folded onto one body per family.

Generation runs on graded_model's window (seed 7, rows from 1000) with the level-3 mask of
test_gpu_generate_graded.py's device-form test: chunk = offset of the first hit + 1 and max_scan =
offset of the second hit + 1 are the smallest round and window with hits in more than one round."""
import ctypes

import numpy as np
import pytest

import grade_model as G
import graded_model as M
from distributed_sudoku_solver_amd import _lib as L

pytestmark = pytest.mark.gpu

FILL = 0xEE
PAD = 3             # sentinel rows behind the rows a call may write
N = 65              # one full group of 64 boards and a ragged group of one
MARK = 12345        # what *found and *scanned hold before a call

NULL_TEXT = b"NULL argument"
ALIGN_TEXT = b"device boards must be 16-byte aligned"
COUNT_TEXT = b"at most 2^31-1 boards per call"
MASK_TEXT = b"level_mask must be a non-empty set of bits 1..4"
CLUES_TEXT = b"clue range must be clues_lo <= clues_hi <= 81"
SCAN_TEXT = b"max_scan must be at least 1"
CHUNK_TEXT = b"chunk must be 0 (automatic) or 1..2^24"
RANGE_TEXT = {"rated": b"backdoor range must be backdoors_lo <= backdoors_hi <= 64",
              "subsets": b"open4 range must be open4_lo <= open4_hi <= 64"}

# the columns of a family after in / out / status / level / open (batch) or puzzles / grids / level / open
# (generation), and which of them a caller must give
EXTRA = {"grade": (), "graded": (), "rate": ("backdoors", "key"), "rated": ("backdoors", "key"),
         "subsets": ("open4",)}
BATCH_COLS = ("in", "out", "status", "level", "open")
BATCH_REQUIRED = {"in", "out", "status", "level", "backdoors", "open4"}
GEN_COLS = ("puzzles", "grids", "level", "open")
GEN_REQUIRED = {"puzzles", "grids"}
WIDTH = {"in": 81, "out": 81, "puzzles": 81, "grids": 81, "index": 8}     # bytes per row; every other column 1

FORMS = pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
BATCH = pytest.mark.parametrize("fam", ["grade", "rate", "subsets"])
GEN = pytest.mark.parametrize("fam", ["graded", "rated", "subsets"])


class Cols:
    """FILL-filled byte columns of `rows` rows, in host memory or (dev) in device buffers."""

    def __init__(self, eng, names, rows, dev):
        self.dev = dev
        self.host = {k: np.full(rows * WIDTH.get(k, 1), FILL, dtype=np.uint8) for k in names}
        self.bufs = {}
        if dev:
            for k, a in self.host.items():
                self.bufs[k] = eng.alloc(a.nbytes)
                self.bufs[k].upload(a)

    def put(self, name, data):
        flat = np.ascontiguousarray(data).view(np.uint8).ravel()
        self.host[name][:flat.size] = flat
        if self.dev:
            self.bufs[name].upload(self.host[name])

    def ptrs(self, skip=()):
        return {k: None if k in skip else (self.bufs[k].ptr if self.dev else ctypes.c_void_p(a.ctypes.data))
                for k, a in self.host.items()}

    def read(self):
        """name -> bytes (a device column is downloaded, which waits for the stream)"""
        for k, b in self.bufs.items():
            b.download(self.host[k])
        return self.host

    def untouched(self, names=None, start=0):
        got = self.read()
        return all((got[k][start * WIDTH.get(k, 1):] == FILL).all() for k in (names or got) if k != "in")

    def free(self):
        for b in self.bufs.values():
            b.free()


@pytest.fixture
def cols(engine):
    made = []

    def make(names, rows, dev):
        made.append(Cols(engine, names, rows, dev))
        return made[-1]
    yield make
    for c in made:
        c.free()


def off(p, k):
    return ctypes.c_void_p(p.value + k)


# ------------------------------------------------------------------ grade / rate / subsets
def batch_names(fam):
    return BATCH_COLS + EXTRA[fam]


def batch_call(engine, fam, dev, p, n, budget=L.SDK_BUDGET_CONTEXT, ctx=True):
    fn = getattr(engine.lib, "sdk_%s_batch%s" % (fam, "_dev" if dev else ""))
    return fn(engine.ctx if ctx else None, *[p[k] for k in batch_names(fam)], n, budget)


def err(engine):
    return engine.lib.sdk_last_error()


@pytest.fixture(scope="module")
def boards():
    return np.ascontiguousarray(G.make_pool()[0][:N])


@pytest.fixture(scope="module")
def graded_ref(engine, boards):
    """sdk_grade_batch of the 65 boards: out, status, level, open as bytes."""
    c = Cols(engine, batch_names("grade"), N, False)
    c.put("in", boards)
    assert batch_call(engine, "grade", False, c.ptrs(), N) == L.SDK_OK
    return {k: c.host[k].copy() for k in ("out", "status", "level", "open")}


@BATCH
@FORMS
def test_batch_required_and_optional_pointers(engine, cols, boards, fam, dev):
    names = batch_names(fam)
    c = cols(names, 1 + PAD, dev)
    c.put("in", boards[:1])
    assert batch_call(engine, fam, dev, c.ptrs(), 1, ctx=False) == L.SDK_EINVAL and err(engine) == NULL_TEXT
    for k in names:
        if k in BATCH_REQUIRED:
            assert batch_call(engine, fam, dev, c.ptrs(skip=(k,)), 1) == L.SDK_EINVAL, k
            assert err(engine) == NULL_TEXT, k
    assert c.untouched()
    for k in names:
        if k not in BATCH_REQUIRED:
            c = cols(names, 1 + PAD, dev)
            c.put("in", boards[:1])
            assert batch_call(engine, fam, dev, c.ptrs(skip=(k,)), 1) == L.SDK_OK, (k, err(engine))
            assert c.untouched((k,)) and c.untouched(start=1), k
            assert (c.host["level"][0] != FILL), k


@BATCH
@FORMS
def test_batch_n_zero(engine, cols, fam, dev):
    c = cols(batch_names(fam), 4, dev)
    assert batch_call(engine, fam, dev, c.ptrs(), 0) == L.SDK_OK
    assert batch_call(engine, fam, dev, c.ptrs(skip=batch_names(fam)), 0) == L.SDK_OK     # no pointer is needed
    assert c.untouched()


@BATCH
@FORMS
def test_batch_bad_arguments(engine, cols, fam, dev):
    c = cols(batch_names(fam), 4, dev)
    big = 1 << 63                                  # above INT64_MAX, and not SDK_BUDGET_CONTEXT
    text = b"node budget out of range"
    for p, n, budget, want in [(c.ptrs(), 1, big, text),
                               (c.ptrs(), 0, big, text),                  # the budget before n == 0
                               (c.ptrs(skip=("in",)), 1, big, NULL_TEXT),     # the pointers before the budget
                               (c.ptrs(), 1 << 31, L.SDK_BUDGET_CONTEXT, COUNT_TEXT),
                               (c.ptrs(), 1 << 31, big, text)]:           # the budget before the count
        assert batch_call(engine, fam, dev, p, n, budget) == L.SDK_EINVAL
        assert err(engine) == want
        assert c.untouched()
    if dev:
        p = c.ptrs()
        odd_in, odd_out = {**p, "in": off(p["in"], 1)}, {**p, "out": off(p["out"], 16 - 1)}
        for q, n, budget, want in [(odd_in, 1, 0, ALIGN_TEXT), (odd_out, 1, 0, ALIGN_TEXT),
                                   (odd_in, 1, big, text),                    # the budget before the alignment
                                   (odd_in, 1 << 31, 0, COUNT_TEXT)]:         # and the count
            assert batch_call(engine, fam, dev, q, n, budget) == L.SDK_EINVAL
            assert err(engine) == want
        assert batch_call(engine, fam, dev, odd_in, 0) == L.SDK_OK            # n == 0 before the alignment
        assert c.untouched()


@BATCH
def test_batch_host_against_device(engine, cols, boards, graded_ref, fam):
    names = batch_names(fam)
    optional = tuple(k for k in names if k not in BATCH_REQUIRED)
    full = {}
    for skip in ((), optional):
        got = []
        for dev in (False, True):
            c = cols(names, N + PAD, dev)
            c.put("in", boards)
            assert batch_call(engine, fam, dev, c.ptrs(skip=skip), N) == L.SDK_OK, err(engine)
            got.append({k: v.copy() for k, v in c.read().items()})
        host, device = got
        for k in names:
            assert np.array_equal(host[k], device[k]), k           # the rows and the sentinels behind them
            if k != "in":
                assert (host[k][N * WIDTH.get(k, 1):] == FILL).all(), k
        for k in skip:
            assert (host[k] == FILL).all(), k
        for k in ("out", "status", "level", "open"):
            if k not in skip:
                assert np.array_equal(host[k][:N * WIDTH.get(k, 1)], graded_ref[k][:N * WIDTH.get(k, 1)]), k
        if not skip:
            full = host
        else:
            for k in names:
                if k not in skip:
                    assert np.array_equal(host[k], full[k]), k
    assert (full["status"][:N].view(np.int8) == L.SDK_SOLVED).all()
    assert (full["level"][:N] == L.SDK_GRADE_SEARCH).any() and (full["level"][:N] < L.SDK_GRADE_SEARCH).any()


# ------------------------------------------------------------------ graded / rated / subsets generation
def gen_names(fam):
    return GEN_COLS + EXTRA[fam] + ("index",)


def gen_mask(fam):
    """the device-form test's level 3; the families with a stage over level 4 select that level too"""
    return 1 << 3 if fam == "graded" else (1 << 3) | (1 << 4)


def gen_call(engine, fam, dev, p, n, mask=None, clues=(0, 81), rng=(0, 64), max_scan=M.ROWS, chunk=0,
             first=M.FIRST, ctx=True, found=True, scanned=True):
    """-> (rc, *found, *scanned): both start as MARK; found / scanned False pass NULL"""
    fn = getattr(engine.lib, "sdk_generate_%s%s" % (fam, "_dev" if dev else ""))
    args = [engine.ctx if ctx else None, M.SEED, first, n, gen_mask(fam) if mask is None else mask, *clues]
    if fam != "graded":
        args += list(rng)
    args += [max_scan, chunk] + [p[k] for k in gen_names(fam)]
    f, s = ctypes.c_uint64(MARK), ctypes.c_uint64(MARK)
    rc = fn(*args, ctypes.byref(f) if found else None, ctypes.byref(s) if scanned else None)
    return rc, f.value, s.value


def two_rounds(fam):
    """(chunk, max_scan, stream indices of the first two hits)"""
    p = np.flatnonzero(M.hits(M.window(), gen_mask(fam)))
    chunk, max_scan = int(p[0]) + 1, int(p[1]) + 1
    assert chunk < max_scan           # the second hit lies behind the first round
    return chunk, max_scan, (p[:2] + M.FIRST).astype(np.uint64)


@GEN
@FORMS
def test_gen_required_and_optional_pointers(engine, cols, fam, dev):
    names = gen_names(fam)
    chunk, max_scan, index = two_rounds(fam)
    c = cols(names, 2 + PAD, dev)
    kw = dict(max_scan=max_scan, chunk=chunk)
    assert gen_call(engine, fam, dev, c.ptrs(), 2, ctx=False, **kw) == (L.SDK_EINVAL, MARK, MARK)
    assert err(engine) == NULL_TEXT
    assert gen_call(engine, fam, dev, c.ptrs(), 2, found=False, **kw) == (L.SDK_EINVAL, MARK, MARK)
    assert err(engine) == NULL_TEXT
    for k in GEN_REQUIRED:
        assert gen_call(engine, fam, dev, c.ptrs(skip=(k,)), 2, **kw) == (L.SDK_EINVAL, MARK, MARK), k
        assert err(engine) == NULL_TEXT
    assert c.untouched()
    for k in names:
        if k in GEN_REQUIRED:
            continue
        c = cols(names, 2 + PAD, dev)
        assert gen_call(engine, fam, dev, c.ptrs(skip=(k,)), 2, **kw) == (L.SDK_OK, 2, max_scan), (k, err(engine))
        assert c.untouched((k,)) and c.untouched(start=2), k
        if k != "index":
            assert np.array_equal(c.host["index"][:16].view(np.uint64), index)
    assert gen_call(engine, fam, dev, c.ptrs(), 2, scanned=False, **kw) == (L.SDK_OK, 2, MARK)


@GEN
@FORMS
def test_gen_n_zero(engine, cols, fam, dev):
    c = cols(gen_names(fam), 4, dev)
    assert gen_call(engine, fam, dev, c.ptrs(), 0) == (L.SDK_OK, 0, 0)
    assert gen_call(engine, fam, dev, c.ptrs(skip=gen_names(fam)), 0) == (L.SDK_OK, 0, 0)
    assert c.untouched()


@GEN
@FORMS
def test_gen_bad_arguments(engine, cols, fam, dev):
    c = cols(gen_names(fam), 4, dev)
    p = c.ptrs()
    top = (1 << 64) - 1
    bad_chunk = (1 << 24) + 1
    cases = [(dict(mask=0), MASK_TEXT), (dict(mask=1), MASK_TEXT), (dict(mask=1 << 5), MASK_TEXT),
             (dict(clues=(30, 29)), CLUES_TEXT), (dict(clues=(0, 82)), CLUES_TEXT),
             (dict(max_scan=0), SCAN_TEXT), (dict(chunk=bad_chunk), CHUNK_TEXT),
             (dict(first=top - 9, max_scan=10), b"first + max_scan overflows the stream index"),
             (dict(n=1 << 31), COUNT_TEXT),
             # two bad arguments: the one checked first
             (dict(n=1 << 31, mask=0), COUNT_TEXT),
             (dict(p=c.ptrs(skip=("puzzles",)), mask=0), NULL_TEXT),
             (dict(mask=0, clues=(30, 29)), MASK_TEXT),
             (dict(clues=(30, 29), max_scan=0), CLUES_TEXT),
             (dict(max_scan=0, chunk=bad_chunk), SCAN_TEXT)]
    if fam != "graded":
        cases += [(dict(rng=(5, 4)), RANGE_TEXT[fam]), (dict(rng=(0, 65)), RANGE_TEXT[fam]),
                  (dict(chunk=bad_chunk, rng=(5, 4)), CHUNK_TEXT)]
    if dev:
        odd_puz, odd_grid, odd_index = ({**p, k: off(p[k], d)} for k, d in (("puzzles", 1), ("grids", 16 - 1),
                                                                             ("index", 4)))
        cases += [(dict(p=odd_puz), ALIGN_TEXT), (dict(p=odd_grid), ALIGN_TEXT),
                  (dict(p=odd_index), b"d_index must be 8-byte aligned"),
                  (dict(p={**odd_puz, "index": odd_index["index"]}), ALIGN_TEXT),
                  (dict(p=odd_puz, chunk=bad_chunk), CHUNK_TEXT),
                  (dict(p=odd_puz, n=0), ALIGN_TEXT)]               # the alignment before n == 0
        if fam != "graded":
            cases += [(dict(p=odd_puz, rng=(5, 4)), RANGE_TEXT[fam])]
    for kw, want in cases:
        kw = dict(kw)
        rc = gen_call(engine, fam, dev, kw.pop("p", p), kw.pop("n", 4), **kw)
        assert rc == (L.SDK_EINVAL, MARK, MARK), kw
        assert err(engine) == want, kw
    assert c.untouched()


@GEN
def test_gen_host_against_device(engine, cols, fam):
    names = gen_names(fam)
    optional = tuple(k for k in names if k not in GEN_REQUIRED)
    chunk, max_scan, index = two_rounds(fam)
    full = None
    # n = 2: the quota is met by the last row of the window; n = 3: the window ends with two rows found
    for n, skip in ((2, ()), (3, ()), (2, optional)):
        got = []
        for dev in (False, True):
            c = cols(names, n + PAD, dev)
            rc = gen_call(engine, fam, dev, c.ptrs(skip=skip), n, max_scan=max_scan, chunk=chunk)
            assert rc == (L.SDK_OK, 2, max_scan), err(engine)
            got.append({k: v.copy() for k, v in c.read().items()})
        host, device = got
        for k in names:
            assert np.array_equal(host[k], device[k]), k
            assert (host[k][2 * WIDTH.get(k, 1):] == FILL).all(), k     # exactly `found` rows were written
        for k in skip:
            assert (host[k] == FILL).all(), k
        if not skip:
            assert np.array_equal(host["index"][:16].view(np.uint64), index)
            assert (host["level"][:2] >= 3).all()
            if full is not None:
                for k in names:
                    assert np.array_equal(host[k][:2 * WIDTH.get(k, 1)], full[k][:2 * WIDTH.get(k, 1)]), k
            full = host
        else:
            for k in GEN_REQUIRED:
                assert np.array_equal(host[k], full[k][:host[k].size]), k
