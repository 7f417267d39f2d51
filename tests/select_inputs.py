"""The case pool of the selection kernels (csrc/select_kernel.h through sdk_select_rows_dev): rows of our
choosing, built from fixed seeds and from nothing the generator or the grader makes.

A Case is one call: the row buffers (puzzles and grids in whole tiles of 64 rows, the per-row arrays, the
nullable sources), the scalars (m, base, n, first, mask, the three ranges) and which nullable outputs are
given.  Cases share arrays: the large families are prefixes of ONE pair of random row buffers (big_rows),
and a sweep over `n` or `base` reuses its rows, so a GPU test uploads an array once (it keys on the array's
base object).

Row bytes are random over 0..255, puzzles with a prescribed number of non-zero bytes.  Rows of a buffer are
pairwise different wherever that is possible: every grid row, and every puzzle row of at least four clues
(two rows of no clue are the same 81 zeros, and the predicate table needs hundreds of those); no puzzle row
equals a grid row.  test_select_model.py asserts it.

Families (Case.family):
  table    the predicate cross product: status x level x clues x backdoors x open4, one row each, shuffled
           over the lanes.  The (clue, backdoor, open4) range triples are NOT crossed with the 15 masks and
           the 4 filter presences but dealt over them: one case per triple, the presence turning with the
           sum of the three range indices; one triple under all 60 (mask, presence) pairs; and for each
           filter and each of its ranges one case with the filter given alone and one beside the other
           filter, level 4 in the mask -- so every range of every filter is read in both settings
  ballot   one to three tiles, the ballot shapes of BALLOTS in the last tile, at every base 0..15
  phase    2,049 tiles, per-tile hit counts steered so that every (rank0 mod 16, kept) occurs; one hit in
           every tile; 64 hits in every tile
  quota    the cut inside a tile at every (phase, n - rank0); n around a tile's first rank; n beyond the
           total; n = base + 1
  scan     SCAN_TILES x SCAN_BASES x SCAN_PATTERNS
  partial  m in PARTIAL_M, rows m.. of the last tile (and of every per-row array) would-be hits
  index    `first` in FIRSTS
  rounds   chains(): a stream as one call and as two or three chained calls
"""
import functools
import itertools

import numpy as np

TILE = 64
MASK_ALL = 0x1E
FILL = 0xEE                                  # what an untouched output byte holds
FILL64 = 0xEEEEEEEEEEEEEEEE
NULLABLE = ("level", "open", "index", "backdoors", "key", "open4")      # the nullable outputs
BIG_TILES = 3073

STATUSES = (1, 0, -1, 2, -128)
LEVELS = (0, 1, 2, 3, 4, 5, 31, 32, 33, 34, 35, 36, 255)
CLUE_RANGES = ((0, 81), (17, 17), (0, 0), (81, 81), (22, 26))
FILTER_RANGES = ((0, 64), (0, 0), (3, 7), (64, 64))
MASKS = tuple(range(2, 0x20, 2))             # the 15 non-empty sets of bits 1..4
PRESENCES = ((False, False), (True, False), (False, True), (True, True))     # (backdoors, open4) given
BALLOTS = ("lane0", "lane31", "lane32", "lane63", "lanes0_63", "low_half", "high_half", "even", "odd", "all",
           "none", "random")
SCAN_TILES = (1, 2, 1023, 1024, 1025, 2048, 2049, 3073)
SCAN_BASES = (0, 1, 15, 1000)
SCAN_PATTERNS = ("last_tile", "tile_1024", "random", "all64")
PARTIAL_M = (1, 63, 64, 65, 127, 64 * 5 + 1)
FIRSTS = ("zero", "below_2_32", "at_2_32", "top")


class Case:
    """One call of sdk_select_rows_dev.  Arrays are read-only; `outs` names the nullable outputs given."""

    def __init__(self, name, family, puzzles, grids, status, level, open_, m, base, n, first=0, mask=MASK_ALL,
                 clues=(0, 81), bd=(0, 64), o4=(0, 64), backdoors=None, key=None, open4=None, outs=NULLABLE, tag=None):
        assert puzzles.shape == grids.shape and puzzles.shape[0] % TILE == 0 and puzzles.shape[1] == 81
        assert 1 <= m <= puzzles.shape[0] and puzzles.shape[0] - m < TILE
        assert min(len(status), len(level), len(open_)) >= m and 0 <= base < n
        self.name, self.family, self.tag = name, family, tag
        self.puzzles, self.grids, self.status, self.level, self.open = puzzles, grids, status, level, open_
        self.backdoors, self.key, self.open4 = backdoors, key, open4
        self.m, self.base, self.n, self.first, self.mask = int(m), int(base), int(n), int(first), int(mask)
        self.clues, self.bd, self.o4 = tuple(clues), tuple(bd), tuple(o4)
        self.outs = frozenset(outs)

    @property
    def tiles(self):
        return self.puzzles.shape[0] // TILE

    def but(self, **kw):
        """The same call with some fields replaced (the arrays stay shared)."""
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        for k, v in kw.items():
            assert k in c.__dict__, k
            setattr(c, k, frozenset(v) if k == "outs" else v)
        return c

    def __repr__(self):
        return f"<Case {self.name} m={self.m} base={self.base} n={self.n}>"


def _frozen(a):
    a.setflags(write=False)
    return a


def make_puzzles(rng, counts):
    """uint8[len(counts), 81]: row i has counts[i] non-zero bytes, at positions spread by a per-row stride,
    with random values 1..255; every row's first non-zero bytes are 10, 0x80 and 0xFF in turn."""
    counts = np.asarray(counts, dtype=np.int64)
    r = len(counts)
    stride = np.array([s for s in range(1, 81) if s % 3])[rng.integers(0, 54, r)]
    shift = rng.integers(0, 81, r)
    order = (np.arange(81)[None, :] * stride[:, None] + shift[:, None]) % 81     # a permutation of 0..80 per row
    vals = rng.integers(1, 256, (r, 81), dtype=np.uint8)
    special = np.array([10, 0x80, 0xFF], dtype=np.uint8)
    first = order == 0
    vals[first] = special[np.arange(r) % 3]
    return np.where(order < counts[:, None], vals, 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def big_rows():
    """(puzzles, grids) of BIG_TILES tiles, shared by the large families.  Clue counts 17..81 in turn, and
    every 1,021st row one of 0..16."""
    rng = np.random.default_rng(20240611)
    rows = BIG_TILES * TILE
    i = np.arange(rows)
    counts = np.where(i % 1021 == 0, (i // 1021) % 17, 81 - i % 65)
    return _frozen(make_puzzles(rng, counts)), _frozen(rng.integers(0, 256, (rows, 81), dtype=np.uint8))


def _rows(t0, tiles):
    p, g = big_rows()
    return p[t0 * TILE:(t0 + tiles) * TILE], g[t0 * TILE:(t0 + tiles) * TILE]


def _status_case(name, family, hit, t0=0, base=0, n=None, m=None, rng=None, **kw):
    """A case over big_rows whose hits are `hit` (bool[tiles * 64]): status 1 or, for the others, one of
    the other status values; levels 1..4 and open bytes random."""
    rng = rng or np.random.default_rng(len(hit) * 7 + base)
    tiles = len(hit) // TILE
    p, g = _rows(t0, tiles)
    status = np.where(hit, 1, rng.choice(np.array(STATUSES[1:], dtype=np.int8), len(hit))).astype(np.int8)
    level = rng.integers(1, 5, len(hit), dtype=np.uint8)
    open_ = rng.integers(0, 256, len(hit), dtype=np.uint8)
    m = len(hit) if m is None else m
    total = base + int(hit[:m].sum())
    n = max(total, base + 1) if n is None else n
    return Case(name, family, p, g, _frozen(status), _frozen(level), _frozen(open_), m, base, n, **kw)


# ------------------------------------------------------------------------------------------- table
def _around(lo, hi, top):
    """{lo-1, lo, hi, hi+1} as values 0..top; an impossible one is replaced by lo."""
    return tuple(v if 0 <= v <= top else lo for v in (lo - 1, lo, hi, hi + 1))


def _filter_values(lo, hi):
    return tuple(v % 256 for v in (0, lo - 1, lo, hi, hi + 1, 64, 255))


@functools.lru_cache(maxsize=None)
def _table_layout(perm=0):
    """The cross product's index columns (status, level, clue position, backdoor position, open4 position),
    one row per combination, shuffled so that every lane sees every kind of row.  TABLE_PERMS shuffles:
    one alone leaves a lane or two without, say, a level-1 row of status 1."""
    grid = np.array(list(itertools.product(range(len(STATUSES)), range(len(LEVELS)), range(4), range(7), range(7))))
    return _frozen(grid[np.random.default_rng(5 + perm).permutation(len(grid))])


TABLE_PERMS = 4
TABLE_ROWS = len(STATUSES) * len(LEVELS) * 4 * 7 * 7          # 12,740: 199 tiles and 4 rows


@functools.lru_cache(maxsize=None)
def _table_arrays(kind, span, perm=0):
    """The table's arrays that depend on one range only (built once per range)."""
    lay = _table_layout(perm)
    rows = (TABLE_ROWS + TILE - 1) // TILE * TILE
    rng = np.random.default_rng({"puzzles": 11, "bd": 12, "o4": 13, "common": 14}[kind] * 1000
                                + span[0] * 100 + span[1] + 100000 * perm)
    if kind == "puzzles":
        lo, hi = span
        counts = np.full(rows, hi)                                    # the tile's tail: would-be hits
        counts[:TABLE_ROWS] = np.array(_around(lo, hi, 81))[lay[:, 2]]
        return _frozen(make_puzzles(rng, counts))
    if kind in ("bd", "o4"):
        lo, hi = span
        a = np.full(rows, lo, dtype=np.uint8)
        a[:TABLE_ROWS] = np.array(_filter_values(lo, hi), dtype=np.uint8)[lay[:, 3 if kind == "bd" else 4]]
        return _frozen(a)
    status = np.ones(rows, dtype=np.int8)
    status[:TABLE_ROWS] = np.array(STATUSES, dtype=np.int8)[lay[:, 0]]
    level = np.full(rows, 4, dtype=np.uint8)
    level[:TABLE_ROWS] = np.array(LEVELS, dtype=np.uint8)[lay[:, 1]]
    return (_frozen(status), _frozen(level), _frozen(rng.integers(0, 256, rows, dtype=np.uint8)),
            _frozen(rng.integers(0, 256, rows, dtype=np.uint8)),
            _frozen(rng.integers(0, 256, (rows, 81), dtype=np.uint8)))


def _table_case(name, cr, br, orr, mask, presence, base, perm):
    status, level, open_, key, grids = _table_arrays("common", (0, 0), perm)
    has_bd, has_o4 = presence
    return Case(name, "table", _table_arrays("puzzles", cr, perm), grids, status, level, open_, TABLE_ROWS, base,
                base + TABLE_ROWS // 4, mask=mask, clues=cr, bd=br, o4=orr,
                backdoors=_table_arrays("bd", br, perm) if has_bd else None, key=key if has_bd else None,
                open4=_table_arrays("o4", orr, perm) if has_o4 else None, tag=(cr, br, orr, mask, presence, perm))


def table_cases():
    out = []
    triples = list(itertools.product(CLUE_RANGES, FILTER_RANGES, FILTER_RANGES))
    pairs = list(itertools.product(MASKS, PRESENCES))
    for k, (cr, br, orr) in enumerate(triples):
        # the presence turns with the SUM of the three range indices, so each backdoor range and each open4
        # range meets every presence (a presence tied to k alone would tie it to the open4 range, k % 4)
        ci, bi, oi = k // 16, k // 4 % 4, k % 4
        out.append(_table_case(f"table_{k}", cr, br, orr, MASKS[k * 7 % 15], PRESENCES[(ci + bi + oi) % 4], k % 16,
                               k % TABLE_PERMS))
    for j, (mask, presence) in enumerate(pairs):
        out.append(_table_case(f"table_pair_{j}", (22, 26), (3, 7), (3, 7), mask, presence, (j * 5) % 16, j % TABLE_PERMS))
    # every range of each filter READ: level 4 asked for, the filter given alone and beside the other one
    j = 0
    for which in (0, 1):
        for ri, rng in enumerate(FILTER_RANGES):
            for both in (False, True):
                other = FILTER_RANGES[(ri + 1 + j) % 4]
                br, orr = (rng, other) if which == 0 else (other, rng)
                presence = (True, True) if both else (which == 0, which == 1)
                out.append(_table_case(f"table_filter_{j}", CLUE_RANGES[j % 5], br, orr, (0x10, 0x1E, 0x18, 0x14)[j % 4],
                                       presence, (j * 3) % 16, j % TABLE_PERMS))
                j += 1
    return out


# ------------------------------------------------------------------------------------------ ballot
def ballot_bits(shape, rng):
    b = np.zeros(TILE, dtype=bool)
    lanes = {"lane0": [0], "lane31": [31], "lane32": [32], "lane63": [63], "lanes0_63": [0, 63],
             "low_half": range(32), "high_half": range(32, 64), "even": range(0, 64, 2), "odd": range(1, 64, 2),
             "all": range(64), "none": []}
    if shape == "random":
        return rng.random(TILE) < 0.5
    b[list(lanes[shape])] = True
    return b


def ballot_cases():
    """The shape in the LAST of 1..3 tiles; the tiles before it random, or full (a carry that is a multiple
    of 64 on top of `base`).  A row that is no hit fails by its status or by its level (mask 0x0E)."""
    out = []
    rng = np.random.default_rng(77)
    for si, shape in enumerate(BALLOTS):
        for base in range(16):
            tiles = 1 + (base + si) % 3
            hit = np.concatenate([np.ones(TILE, dtype=bool) if (base + t) % 2 else rng.random(TILE) < 0.4
                                  for t in range(tiles - 1)] + [ballot_bits(shape, rng)])
            p, g = _rows((si * 16 + base) * 3, tiles)
            rows = tiles * TILE
            by_status = rng.random(rows) < 0.5
            status = np.where(hit | ~by_status, 1, rng.choice(np.array(STATUSES[1:]), rows)).astype(np.int8)
            level = np.where(hit | by_status, rng.integers(1, 4, rows), rng.choice([0, 4, 5, 32, 33], rows))
            total = base + int(hit.sum())
            n = (total if base % 2 else total + 3) if total > base else base + 1
            out.append(Case(f"ballot_{shape}_{base}", "ballot", p, g, _frozen(status), _frozen(level.astype(np.uint8)),
                            _frozen(rng.integers(0, 256, rows, dtype=np.uint8)), rows, base, n, mask=0x0E,
                            first=1000 + base, tag=(shape, hit[-TILE:].copy())))
    return out


# ------------------------------------------------------------------------------------------- phase
PHASE_TILES = 2049


def steered_counts(rng, tiles, base, seen):
    """Per-tile hit counts 0..64: at each tile, a count not yet seen at the tile's phase (rank0 mod 16) if
    there is one, else a random one.  `seen` [16][65] is updated."""
    counts = np.zeros(tiles, dtype=np.int64)
    rank = base
    for t in range(tiles):
        todo = np.flatnonzero(~seen[rank % 16, 1:]) + 1
        c = int(rng.choice(todo)) if len(todo) else int(rng.integers(0, 65))
        seen[rank % 16, c] = True
        counts[t] = c
        rank += c
    return counts


def hits_from_counts(rng, counts):
    """bool[tiles * 64] with counts[t] hits in tile t, in random lanes."""
    keys = rng.random((len(counts), TILE))
    return (np.argsort(np.argsort(keys, axis=1), axis=1) < counts[:, None]).reshape(-1)


def phase_cases():
    out = []
    seen = np.zeros((16, 65), dtype=bool)
    for k, base in enumerate((0, 5)):
        rng = np.random.default_rng(300 + k)
        counts = steered_counts(rng, PHASE_TILES, base, seen)
        out.append(_status_case(f"phase_steered_{k}", "phase", hits_from_counts(rng, counts), base=base, rng=rng,
                                first=(1 << 40) + k))
    rng = np.random.default_rng(310)
    out.append(_status_case("phase_one_per_tile", "phase", hits_from_counts(rng, np.ones(PHASE_TILES, dtype=np.int64)),
                            base=3, rng=rng))
    out.append(_status_case("phase_all64", "phase", np.ones(PHASE_TILES * TILE, dtype=bool), base=7, rng=rng))
    return out


# ------------------------------------------------------------------------------------------- quota
def quota_cases():
    out = []
    rng = np.random.default_rng(400)
    dense = _status_case("quota_dense", "quota", np.ones(3 * TILE, dtype=bool), t0=700, rng=rng)
    for base in range(16):                    # the cut in tile 1 (rank0 = base + 64, phase = base mod 16)
        for k in range(1, 65):
            out.append(dense.but(name=f"quota_cut_{base}_{k}", base=base, n=base + 64 + k, tag=("cut", base % 16, k)))
    hit = hits_from_counts(rng, np.array([37, 0, 50, 21, 64]))
    some = _status_case("quota_some", "quota", hit, t0=710, rng=rng)
    for base in (0, 9):
        firsts = base + np.concatenate([[0], np.cumsum([37, 0, 50, 21])])       # the tiles' first ranks
        total = base + int(hit.sum())
        for n in sorted({int(r) + d for r in firsts[1:] for d in (-1, 0, 1)} | {total - 1, total, total + 1,
                                                                               total + 100, base + 1}):
            out.append(some.but(name=f"quota_n_{base}_{n}", base=base, n=n, tag=("n", base, n)))
    return out


# -------------------------------------------------------------------------------------------- scan
def scan_hits(pattern, tiles, rng):
    hit = np.zeros((tiles, TILE), dtype=bool)
    if pattern == "last_tile":
        hit[-1] = rng.random(TILE) < 0.5
        hit[-1, 17] = True
    elif pattern == "tile_1024":
        if tiles > 1024:
            hit[1024] = rng.random(TILE) < 0.5
            hit[1024, 40] = True
    elif pattern == "random":                 # half of the tiles empty, the others 1..64 hits
        counts = np.where(rng.random(tiles) < 0.5, 0, rng.integers(1, 65, tiles))
        hit = hits_from_counts(rng, counts).reshape(tiles, TILE)
    else:
        hit[:] = True
    return hit.reshape(-1)


def scan_cases():
    out = []
    for tiles in SCAN_TILES:
        for pi, pattern in enumerate(SCAN_PATTERNS):
            rng = np.random.default_rng(500 + tiles * 4 + pi)
            one = _status_case("scan", "scan", scan_hits(pattern, tiles, rng), rng=rng)
            hits = one.n                       # (base 0: n = the hits, or 1)
            for base in SCAN_BASES:
                out.append(one.but(name=f"scan_{tiles}_{pattern}_{base}", base=base, n=max(base + hits, base + 1),
                                   tag=(tiles, pattern, base)))
    return out


# ----------------------------------------------------------------------------------------- partial
def partial_cases():
    """Every row of every buffer a hit -- the rows from m on as well, in the row bytes and in the per-row
    arrays, which are allocated to the end of the tile: only `row < m` keeps them out."""
    out = []
    for k, m in enumerate(PARTIAL_M):
        tiles = (m + TILE - 1) // TILE
        rows = tiles * TILE
        rng = np.random.default_rng(600 + k)
        p, g = _rows(900 + 8 * k, tiles)
        ones = _frozen(np.ones(rows, dtype=np.int8))
        level = _frozen(np.full(rows, 4, dtype=np.uint8))
        byte = [_frozen(rng.integers(0, 256, rows, dtype=np.uint8)) for _ in range(2)]
        filt = [_frozen(rng.integers(2, 6, rows, dtype=np.uint8)) for _ in range(2)]
        for base in (0, 11):
            for with_filters in (False, True):
                out.append(Case(f"partial_{m}_{base}_{int(with_filters)}", "partial", p, g, ones, level, byte[0], m,
                                base, base + rows + 8, bd=(2, 5), o4=(2, 5),
                                backdoors=filt[0] if with_filters else None, key=byte[1] if with_filters else None,
                                open4=filt[1] if with_filters else None, tag=m))
    return out


# ------------------------------------------------------------------------------------------- index
def first_value(kind, m):
    return {"zero": 0, "below_2_32": (1 << 32) - 1 - 5, "at_2_32": 1 << 32, "top": (1 << 64) - 1 - m}[kind]


def index_cases():
    rng = np.random.default_rng(700)
    one = _status_case("index", "index", rng.random(2 * TILE) < 0.6, t0=960, base=2, rng=rng)
    return [one.but(name=f"index_{kind}", first=first_value(kind, one.m), tag=kind) for kind in FIRSTS]


# ------------------------------------------------------------------------------------------ rounds
ROUNDS_M = 300


def _round(stream, lo, hi, base, n, name):
    """Rows [lo, hi) of the stream as a round of their own: copied to the start of whole tiles (a round's
    buffers start at a row 0), the rest of the last tile filled with would-be hits."""
    m = hi - lo
    rows = (m + TILE - 1) // TILE * TILE
    pad_p, pad_g = _rows(1000, 1)

    def tiled(a, pad):
        b = np.concatenate([a[lo:hi], pad[:rows - m]])
        return _frozen(b)

    return Case(name, "rounds", tiled(stream.puzzles, pad_p), tiled(stream.grids, pad_g),
                tiled(stream.status, np.ones(TILE, dtype=np.int8)), tiled(stream.level, np.ones(TILE, dtype=np.uint8)),
                tiled(stream.open, np.zeros(TILE, dtype=np.uint8)), m, base, n, first=stream.first + lo)


@functools.lru_cache(maxsize=None)
def chains():
    """[(whole, [round, ...], offsets)]: a stream of ROUNDS_M rows as one call and cut into two or three
    rounds, each with base = the hits before it.  A round that would start at or above the quota is not
    run (the driver stops there), so a chain may be shorter than its cuts."""
    rng = np.random.default_rng(800)
    hit = rng.random(ROUNDS_M) < 0.45
    hit[[0, ROUNDS_M - 1]] = True
    full = np.concatenate([hit, np.zeros(20, dtype=bool)])
    out = []
    total = int(hit.sum())
    for n in (total - 2, total + 5):
        whole = _status_case(f"rounds_whole_{n}", "rounds", full, t0=1010, m=ROUNDS_M, n=n, first=12345,
                             rng=np.random.default_rng(801))
        last_row = int(np.flatnonzero(hit)[min(n, total) - 1])
        cuts = [(1,), (63,), (64,), (65,), (ROUNDS_M - 1,), (last_row,), (last_row + 1,), (63, 65), (64, 128),
                (1, ROUNDS_M - 1), (last_row, last_row + 1)]
        for cut in cuts:
            edges = [0, *[c for c in cut if 0 < c < ROUNDS_M], ROUNDS_M]
            rounds, offsets = [], []
            for lo, hi in zip(edges[:-1], edges[1:]):
                base = int(hit[:lo].sum())
                if base >= n:
                    break
                rounds.append(_round(whole, lo, hi, base, n, f"rounds_{n}_{'_'.join(map(str, cut))}_{lo}"))
                offsets.append(lo)
            out.append((whole, rounds, offsets))
    return out


def rounds_cases():
    seen, out = set(), []
    for whole, rounds, _ in chains():
        for c in [whole, *rounds]:
            if c.name not in seen:
                seen.add(c.name)
                out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def pool():
    """Every case, in a fixed order."""
    return tuple(table_cases() + ballot_cases() + phase_cases() + quota_cases() + scan_cases() + partial_cases()
                 + index_cases() + rounds_cases())


def family(name):
    return [c for c in pool() if c.family == name]
