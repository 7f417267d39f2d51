"""The boards the checker's tests share (test_check_model.py on the CPU, test_gpu_check_units.py against
the kernels): a deterministic pool that reaches every branch of the unit rule `sum == 45 and 9 distinct`.

Pure numpy; everything derives from synth.seed_arrays() solutions under synth.random_symmetries.  A
RELABELLED board is a symmetric copy of a valid grid whose digit i is replaced by M[i]: each of its 27
units then holds the multiset M, so its verdict is the rule applied to M (3 if sum(M) == 45 and the
values are distinct, else 0).  pool() returns (boards uint8[n,81], tags): tags[i] names the family of
board i.  The expected verdicts are never taken from the construction: the tests ask oracle.py_check."""
import functools
import itertools

import numpy as np

from distributed_sudoku_solver_amd import synth

SEED = 20251021

# Exactly one of the 27 units fails: row 0 holds 5 twice (sum 45); every other row, every column and
# every box holds nine distinct values of sum 45 (failing_units() says so, test_check_model.py asks).
# Every byte is below 32 and some are above 9: the fast path's sums, then the exact path.
SINGLE_ROW = (
    "15 5 2 10 5 3 4 0 1 / 3 8 7 4 0 1 14 2 6 / 0 1 4 11 9 2 8 7 3 / "
    "5 11 1 6 4 0 3 8 7 / 4 6 8 1 3 7 2 14 0 / 7 3 0 2 14 8 6 1 4 / "
    "2 0 14 3 7 4 1 6 8 / 8 4 6 0 1 14 7 3 2 / 1 7 3 8 2 6 0 4 14")
# No such board holds a byte >= 18 (so none takes the exact path directly, and tools/find_check_cases.py
# has nothing to search there): every cell lies in a row, a column and a box, two of which pass, and a
# passing unit's largest value is 17 (eight distinct values sum to >= 28).
# The same for a BOX: only box (0,0) fails, it holds 3 twice (sum 45).  Found by tools/find_check_cases.py
# (an integer program, DESIGN.md "checker pin"); failing_units() is what vouches for it.
SINGLE_BOX = (
    "3 10 1 12 2 4 0 6 7 / 4 3 16 6 8 0 2 1 5 / 0 6 2 1 5 7 4 3 17 / "
    "1 4 5 2 6 14 3 10 0 / 6 14 0 4 3 8 1 7 2 / 10 2 3 7 0 1 5 11 6 / "
    "2 1 6 0 16 3 8 5 4 / 7 5 4 8 1 2 15 0 3 / 12 0 8 5 4 6 7 2 1")

UNIT_NAMES = [f"row{r}" for r in range(9)] + [f"col{c}" for c in range(9)] + [f"box{b}" for b in range(9)]


def unit_cells():
    """int[27,9]: the cells of row 0..8, column 0..8, box 0..8 (box b = 3 * band + stack)."""
    k = np.arange(81).reshape(9, 9)
    boxes = [k[3 * (b // 3):3 * (b // 3) + 3, 3 * (b % 3):3 * (b % 3) + 3].ravel() for b in range(9)]
    return np.stack(list(k) + list(k.T) + boxes)


def failing_units(board):
    """The units (indices into UNIT_NAMES) of one board that miss the literal rule; plain Python ints."""
    cells = [int(v) for v in board]
    out = []
    for u, idx in enumerate(unit_cells()):
        vals = [cells[i] for i in idx]
        if not (sum(vals) == 45 and len(set(vals)) == 9):
            out.append(u)
    return out


def parse_grid(text):
    return np.array([int(t) for t in text.replace("/", " ").split()], dtype=np.int64)


# ------------------------------------------------------------------------------------------ multisets
def multisets_0_9():
    """Every 9-multiset over 0..9, repeated values included: uint8[48620, 9]."""
    m = np.array(list(itertools.combinations_with_replacement(range(10), 9)), dtype=np.uint8)
    assert m.shape == (48620, 9)
    return m


def passing_sets():
    """Every set of nine distinct non-negative integers of sum 45: {0..8} plus a partition of 9, so 30
    sets, the largest value 17."""
    s = [c for c in itertools.combinations(range(18), 9) if sum(c) == 45]
    assert len(s) == 30 and max(map(max, s)) == 17
    return np.array(s, dtype=np.int64)


def near_misses():
    """Multisets one step off a passing set, and the bytes at which the kernel's bit tricks change
    behaviour.  Returns [(tag, int64[m,9])]."""
    sets = passing_sets()
    plus, minus, merged = [], [], []
    for s in sets:
        for i in range(9):
            t = s.copy(); t[i] += 1; plus.append(t)                 # sum 46 (sometimes a duplicate too)
            if s[i] > 0:
                t = s.copy(); t[i] -= 1; minus.append(t)            # sum 44
        for i, j in itertools.combinations(range(9), 2):            # a + b = 2m: {a, b} -> {m, m}, sum kept
            if (s[i] + s[j]) % 2 == 0:
                t = s.copy(); t[i] = t[j] = (s[i] + s[j]) // 2; merged.append(t)
    # the clamp at 18 and the fast path's entry mask at 32: one large value over {0..7}, and over
    # {0..6, 6} where the sum can stay 45 (x = 18) with a duplicate
    edge = [[0, 1, 2, 3, 4, 5, 6, 7, x] for x in (17, 18, 19, 31, 32, 33)]
    edge += [[0, 1, 2, 3, 4, 5, 6, 6, 18], [0, 1, 2, 3, 4, 5, 5, 6, 19], [0, 1, 2, 3, 4, 5, 6, 18, 19],
             [0, 1, 2, 3, 4, 18, 18, 18, 18], [0, 0, 0, 0, 0, 0, 0, 14, 31], [0, 0, 0, 0, 0, 0, 0, 13, 32],
             [0, 0, 0, 0, 0, 0, 0, 12, 33], [1, 2, 3, 4, 5, 6, 7, 8, 41], [1, 2, 3, 4, 5, 6, 7, 8, 73]]
    # 1u << v takes v mod 32: digit d as d + 32k with the other eight digits in place
    alias = []
    for d in range(1, 10):
        for k in range(1, 8):
            t = np.arange(1, 10); t[d - 1] = d + 32 * k; alias.append(t)
    # {0, 2..8, 10} passes; 0 as 32 or 64 and 10 as 42 or 74 must not
    alias0 = [[z, 2, 3, 4, 5, 6, 7, 8, t] for z, t in ((0, 10), (32, 10), (64, 10), (0, 42), (0, 74), (32, 42))]
    byte = [[1, 2, 3, 4, 5, 6, 7, 8, x] for x in (127, 128, 255)]
    byte += [[0, 1, 2, 3, 4, 5, 6, 7, x] for x in (127, 128, 255)]
    # sums that equal 45 only in an 8-bit or a 10-bit field
    wrap = [[0, 1, 2, 3, 4, 5, 6, 100, 180], [0, 1, 2, 3, 4, 5, 6, 25, 255],                # 301 = 45 + 256
            [0, 1, 2, 3, 4, 5, 37, 250, 255], [10, 11, 12, 13, 14, 15, 16, 211, 255],       # 557 = 45 + 512
            [255, 255, 255, 255, 49, 0, 0, 0, 0], [255, 254, 253, 252, 49, 0, 1, 2, 3]]     # 1069 = 45 + 1024
    assert [sum(w) for w in wrap] == [301, 301, 557, 557, 1069, 1069]
    return [("near_plus1", np.array(plus)), ("near_minus1", np.array(minus)), ("near_merged", np.array(merged)),
            ("clamp_edge", np.array(edge)), ("alias", np.array(alias)), ("alias_0_10", np.array(alias0)),
            ("byte_edge", np.array(byte)), ("sum_wrap", np.array(wrap))]


# --------------------------------------------------------------------------------------------- boards
def valid_grids(rng, n):
    """n valid grids (digits 1..9): seed solutions under random symmetries, digits shuffled."""
    _, sol = synth.seed_arrays()
    sol = np.concatenate([sol, synth.parse(synth.WIKI_SOLUTION)[None]])
    g, rl = synth.random_symmetries(rng, n)
    return synth.apply_symmetries(sol[rng.integers(0, len(sol), n)], g, rl)


def relabelled(rng, multisets, dtype=np.uint8):
    """One relabelled board per row of multisets[m,9]: digit i of a valid grid becomes multisets[., i-1]
    (valid_grids has shuffled which digit that is)."""
    ms = np.asarray(multisets)
    lut = np.zeros((len(ms), 10), dtype=dtype)
    lut[:, 1:] = ms
    return lut[np.arange(len(ms))[:, None], valid_grids(rng, len(ms))]


def _move_line(rng, target):
    """A band-keeping permutation p of 0..8 (new line i = old line p[i]) with p[target] = 0."""
    tb, ti = divmod(target, 3)
    bands = rng.permutation(3).tolist()
    j = bands.index(0)
    bands[j], bands[tb] = bands[tb], bands[j]
    p = []
    for pos, b in enumerate(bands):
        inner = rng.permutation(3).tolist()
        if pos == tb:
            j = inner.index(0)
            inner[j], inner[ti] = inner[ti], inner[j]
        p += [3 * b + i for i in inner]
    return np.array(p)


def single_unit_boards(rng, base, box=False, copies=4):
    """`base` has one failing unit, row 0 (or box 0 with box=True).  Returns the boards that move it to
    each of the 9 rows and, transposed, each of the 9 columns (or to each of the 9 boxes), `copies` of
    each under random band-keeping permutations of the other lines, and the unit each board fails in."""
    g = np.asarray(base).reshape(9, 9)
    out, units = [], []
    for target in range(9):
        for _ in range(copies):
            if box:
                rp, cp = _move_line(rng, 3 * (target // 3)), _move_line(rng, 3 * (target % 3))
                out.append(g[rp][:, cp].ravel()); units.append(18 + target)
                continue
            rp = _move_line(rng, target)
            cp = synth._line_perms(rng, 1)[0]
            m = g[rp][:, cp]
            out.append(m.ravel()); units.append(target)
            out.append(m.T.ravel()); units.append(9 + target)
    return np.array(out), np.array(units)


BAND_PAIRS = [(0, 1), (0, 2), (1, 2)]


def four_box_boards(rng, per_pair=12):
    """Rows and columns pass, exactly four boxes fail (the fewest an in-domain board can have: failing
    boxes number 0 or >= 2 in every band and every stack).  In a valid grid, cells (r1,c1) and (r2,c2)
    hold a, (r1,c2) and (r2,c1) hold b, rows in two bands, columns in two stacks: a and b exchanged.
    per_pair boards for each of the 9 (band pair, stack pair); box (0,0) is among the four, and its sum
    moves, when both pairs hold 0.  Returns (boards, int[n,2] indices into BAND_PAIRS)."""
    out, which = [], []
    for bi, (ba, bb) in enumerate(BAND_PAIRS):
        for si, (sa, sb) in enumerate(BAND_PAIRS):
            have = 0
            while have < per_pair:
                g = valid_grids(rng, 1)[0].reshape(9, 9)
                rect = [(r1, r2, c1, c2)
                        for r1 in range(3 * ba, 3 * ba + 3) for r2 in range(3 * bb, 3 * bb + 3)
                        for c1 in range(3 * sa, 3 * sa + 3) for c2 in range(3 * sb, 3 * sb + 3)
                        if g[r1, c1] == g[r2, c2] and g[r1, c2] == g[r2, c1]]
                if not rect:
                    continue
                r1, r2, c1, c2 = rect[rng.integers(len(rect))]
                g = g.copy()
                g[r1, c1], g[r1, c2] = g[r1, c2], g[r1, c1]
                g[r2, c1], g[r2, c2] = g[r2, c2], g[r2, c1]
                out.append(g.ravel()); which.append((bi, si)); have += 1
    return np.array(out, dtype=np.uint8), np.array(which)


def latin_boards(rng, n, keep_box00):
    """Valid grids with their rows and columns permuted across bands and stacks: every row and column
    still passes, boxes fail.  keep_box00: only rows 3..8 and columns 3..8 move, so box (0,0) keeps its
    cells (sum 45: verdict 2); else only boards whose box (0,0) sum left 45 are kept (verdict 0)."""
    out = []
    while len(out) < n:
        g = valid_grids(rng, 1)[0].reshape(9, 9)
        if keep_box00:
            rp = np.concatenate([np.arange(3), 3 + rng.permutation(6)])
            cp = np.concatenate([np.arange(3), 3 + rng.permutation(6)])
        else:
            rp, cp = rng.permutation(9), rng.permutation(9)
        m = g[rp][:, cp]
        boxes_fail = any(len(set(m[3 * i:3 * i + 3, 3 * j:3 * j + 3].ravel().tolist())) != 9
                         for i in range(3) for j in range(3))
        if boxes_fail and (keep_box00 or m[:3, :3].sum() != 45):
            out.append(m.ravel())
    return np.array(out, dtype=np.uint8)


def _lut(mapping):
    lut = np.arange(256, dtype=np.uint8)
    for k, v in mapping.items():
        lut[k] = v
    return lut


# {1..9} -> a passing set with values >= 10: the same unit structure on the exact path
EXACT_LUTS = [{1: 0, 9: 10}, {1: 0, 2: 1, 3: 2, 4: 3, 5: 4, 6: 5, 7: 6, 8: 7, 9: 17},
              {1: 0, 2: 1, 3: 2, 4: 3, 5: 4, 6: 5, 7: 6, 8: 9, 9: 15}]


def _on_exact_path(boards, rng):
    luts = np.stack([_lut(m) for m in EXACT_LUTS])
    return luts[rng.integers(0, len(luts), len(boards))[:, None], boards]


@functools.lru_cache(maxsize=None)
def pool():
    """(boards uint8[n,81], tags str[n]); read-only arrays, built once per process."""
    rng = np.random.default_rng(SEED)
    fam = [("fast_multiset", relabelled(rng, multisets_0_9()))]
    fam.append(("exact_pass", relabelled(rng, np.repeat(passing_sets(), 4, axis=0))))
    for tag, ms in near_misses():
        fam.append((tag, relabelled(rng, ms)))
    fam.append(("all_one_value", np.repeat(np.array([0, 5, 9, 10, 31, 32, 255], dtype=np.uint8)[:, None], 81, axis=1)))
    rows_cols, _ = single_unit_boards(rng, parse_grid(SINGLE_ROW))
    fam.append(("single_row_col", rows_cols.astype(np.uint8)))
    fam.append(("single_box", single_unit_boards(rng, parse_grid(SINGLE_BOX), box=True)[0].astype(np.uint8)))
    four, _ = four_box_boards(rng)
    fam.append(("four_boxes", four))
    fam.append(("four_boxes_exact", _on_exact_path(four, rng)))
    keep, move = latin_boards(rng, 160, True), latin_boards(rng, 160, False)
    fam.append(("latin_box00_45", np.concatenate([keep[:80], _on_exact_path(keep[80:], rng)])))
    fam.append(("latin_box00_off", np.concatenate([move[:80], _on_exact_path(move[80:], rng)])))
    # a valid grid with one cell out of domain: its row, column and box fail, on the direct exact route
    one = valid_grids(rng, 81)
    one[np.arange(81), np.arange(81)] = np.tile(np.array([32, 33, 64, 41, 128, 255, 10, 18, 0], dtype=np.uint8), 9)
    fam.append(("one_cell_off", one))
    boards = np.ascontiguousarray(np.concatenate([b for _, b in fam]), dtype=np.uint8)
    tags = np.concatenate([np.full(len(b), t) for t, b in fam])
    boards.setflags(write=False)
    tags.setflags(write=False)
    return boards, tags


@functools.lru_cache(maxsize=None)
def expected():
    """oracle.py_check's verdict byte for every board of pool(): bit 0 intended, bit 1 raw NameError."""
    from oracle import oracle as O
    v = np.array([py_verdict(O, b) for b in pool()[0].tolist()], dtype=np.uint8)
    v.setflags(write=False)
    return v


def py_verdict(O, cells):
    raw, intended = O.py_check(cells)
    return int(intended) | (2 if raw == "NameError" else 0)


@functools.lru_cache(maxsize=None)
def mix(n=600):
    """Indices into pool() of an n-board mix drawn evenly from the tags, tag after tag in turn (so any
    short run of it holds every family); the verdict-2 boards, the single-unit boards and the aliases
    are in it because their families are."""
    boards, tags = pool()
    rng = np.random.default_rng(SEED + 1)
    names = list(dict.fromkeys(tags.tolist()))
    per = -(-n // len(names))
    cols = []
    for t in names:
        idx = np.flatnonzero(tags == t)
        pick = rng.permutation(idx)[:per] if len(idx) >= per else idx[np.arange(per) % len(idx)]
        cols.append(pick)
    m = np.stack(cols, axis=1).ravel()[:n]
    m.setflags(write=False)
    return m


# ---------------------------------------------------------------------------------- int64 (wide) cases
def wide_cases():
    """int64[n,81] boards for check_kernel_i64 beyond the uint8 pool: relabelled boards whose units hold
    {x, -x, 1, 2, 3, 4, 5, 6, 24} with x = 2^59 - 1 (passes: distinct, the sum is exact), one digit as
    d + 2^32 or d - 2^32 (fails; equal to d in 32 bits), and negative near misses."""
    rng = np.random.default_rng(SEED + 2)
    x = (1 << 59) - 1
    ms = [[x, -x, 1, 2, 3, 4, 5, 6, 24], [x, -x, 1, 2, 3, 4, 5, 6, 25], [x, -x, 1, 2, 3, 4, 5, 5, 25],
          [x, 1 - x, 0, 2, 3, 4, 5, 6, 24], [-1, 1, 2, 3, 4, 5, 6, 7, 18], [-1, -2, 3, 4, 5, 6, 7, 8, 15],
          [-36, 0, 1, 2, 3, 4, 5, 6, 60], [-1, -1, 2, 3, 4, 5, 6, 7, 20]]
    for d in range(1, 10):
        for off in (1 << 32, -(1 << 32)):
            t = list(range(1, 10)); t[d - 1] = d + off; ms.append(t)
    ms = np.repeat(np.array(ms, dtype=np.int64), 3, axis=0)
    return relabelled(rng, ms, dtype=np.int64)
