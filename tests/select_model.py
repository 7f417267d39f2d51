"""Two statements of one round of the graded selection (sdk_select_rows_dev, include/sudoku_hip.h).

select_ref(case)    the plain reference: the predicate of the header's text on every row (status == 1;
                    level < 32 and its mask bit set; clues in range; a level-4 row also held to each filter
                    that is given), the first n - base hits in row order written at ranks base, base + 1, ...
select_model(case)  the three kernels of csrc/select_kernel.h restated tile by tile in uint32 / uint64:
                    flag (clue count, ballot, popcount), scan (steps of 1,024 tiles with wsum, before, run),
                    scatter (kept, below, head, in0, in1, the pack buffer at the output's 16-byte phase,
                    then the 16-byte pieces, the head bytes and the tail bytes).  It records for every byte
                    of every output how often it was written, the row outputs apart by 16-byte stores (w16)
                    and single-byte stores (w1), and how many 16-byte stores were not 16-byte aligned.
                    `mutant` names one way of being wrong (MUTANTS).

Both return a Result: `out`, a dict of the output arrays pre-filled with the sentinel (None for an output
that is not given), `total` and `last`; the reference adds the tiles' (rank0, kept), the model its write maps.
The model's arrays are SLACK rows longer than n, so that a mutant that stores past the end is counted
instead of raising.  test_select_model.py pins the model to the reference on select_inputs.pool() and asks
that every mutant shows on that pool: what a mutant survives, the pool cannot see in the kernels either.
"""
from collections import namedtuple

import numpy as np

import select_inputs as I

TILE = I.TILE
SLACK = 66                        # rows behind n in the model's arrays
SCAN = 1024
PACK = TILE * 81 + 16
POISON = 0xA5                     # what the pack buffer holds where no row was packed

MUTANTS = (
    "no_row_guard", "no_level_guard", "status_nonzero",
    "clues_lo_strict", "clues_hi_strict", "bd_lo_strict", "bd_hi_strict", "o4_lo_strict", "o4_hi_strict",
    "bd_every_level", "o4_every_level", "bd_skipped_with_o4", "o4_skipped_with_bd",
    "clues_digits_only", "clues_80_cells",
    "scan_no_carry_in", "scan_no_run_add", "scan_before_le", "scan_inclusive", "scan_oob_lanes",
    "kept_unclamped", "below_le_kept", "mbcnt_lo_only",
    "head_mod4", "in0_16_at_head0", "in1_rounded_up", "no_head_bytes", "no_tail_bytes", "pack_without_head",
    "grids_from_puzzles", "gather_at_rank", "index_without_first", "index_32bit", "last_at_rank_n", "last_is_row",
    "absent_source_zero",
)

class BeyondSlack(Exception):
    """A mutant of select_model stored beyond the SLACK rows behind n."""


Ref = namedtuple("Ref", "out total last rank0 kept")
Model = namedtuple("Model", "out total last writes w16 w1 misaligned ballot offset")

DTYPES = {"puzzles": np.uint8, "grids": np.uint8, "level": np.uint8, "open": np.uint8, "index": np.uint64,
          "backdoors": np.uint8, "key": np.uint8, "open4": np.uint8}


def blank(case, rows):
    """The outputs before the call: `rows` rows of the sentinel each, None where the output is not given."""
    out = {}
    for k, dt in DTYPES.items():
        if k in ("puzzles", "grids"):
            out[k] = np.full((rows, 81), I.FILL, dtype=np.uint8)
        elif k in case.outs:
            out[k] = np.full(rows, I.FILL64 if dt is np.uint64 else I.FILL, dtype=dt)
        else:
            out[k] = None
    return out


# ------------------------------------------------------------------------------------ the reference
def ref_hits(c):
    """bool[m]: the predicate on every row, in plain signed integers."""
    m = c.m
    clues = (np.asarray(c.puzzles[:m]) != 0).sum(axis=1)
    level = c.level[:m].astype(np.int64)
    in_mask = np.zeros(m, dtype=bool)
    small = level < 32
    in_mask[small] = (c.mask >> level[small]) & 1 == 1
    hit = (c.status[:m] == 1) & in_mask & (c.clues[0] <= clues) & (clues <= c.clues[1])
    for src, (lo, hi) in ((c.backdoors, c.bd), (c.open4, c.o4)):
        if src is not None:
            v = src[:m].astype(np.int64)
            hit &= (level != 4) | ((lo <= v) & (v <= hi))
    return hit


def select_ref(c, out=None):
    """`out`: the outputs of the rounds before (a chain writes into the same arrays), default blank."""
    hit = ref_hits(c)
    where = np.flatnonzero(hit)
    take = where[:max(0, c.n - c.base)]
    ranks = c.base + np.arange(len(take))
    out = blank(c, c.n) if out is None else out
    out["puzzles"][ranks] = c.puzzles[take]
    out["grids"][ranks] = c.grids[take]
    src = {"level": c.level, "open": c.open, "backdoors": c.backdoors, "key": c.key, "open4": c.open4}
    for k, a in src.items():
        if out[k] is not None:
            out[k][ranks] = a[take] if a is not None else 0xFF
    if out["index"] is not None:
        out["index"][ranks] = [c.first + int(r) for r in take]
    total = c.base + len(where)
    last = int(where[c.n - 1 - c.base]) + 1 if c.n - 1 - c.base < len(where) else 0
    # the tiles: a tile's kept rows are ranks [rank0, rank0 + kept)
    padded = np.zeros(c.tiles * TILE, dtype=np.int64)
    padded[:c.m] = hit
    counts = padded.reshape(-1, TILE).sum(axis=1)
    rank0 = c.base + np.concatenate([[0], np.cumsum(counts)[:-1]])
    kept = np.clip(np.minimum(counts, c.n - rank0), 0, None)
    return Ref(out, total, last, rank0, kept)


# ------------------------------------------------------------------------------------------ the model
u32, u64 = np.uint32, np.uint64


def _popc64(b):
    b = b - ((b >> u64(1)) & u64(0x5555555555555555))
    b = (b & u64(0x3333333333333333)) + ((b >> u64(2)) & u64(0x3333333333333333))
    b = (b + (b >> u64(4))) & u64(0x0F0F0F0F0F0F0F0F)
    return ((b * u64(0x0101010101010101)) >> u64(56)).astype(u32)


def _padded(a, rows, fill):
    """A per-row array as the kernel would find it beyond its end: `fill` (a would-be hit)."""
    a = np.asarray(a)
    if len(a) >= rows:
        return a[:rows]
    return np.concatenate([a, np.full(rows - len(a), fill, dtype=a.dtype)])


def model_flag(c, mut=None):
    """-> (hit bool[tiles, 64], ballot uint64[tiles], count uint32[tiles])."""
    tiles, rows = c.tiles, c.tiles * TILE
    p = np.asarray(c.puzzles)
    nz = p != 0
    if mut == "clues_digits_only":
        nz &= p <= 9
    if mut == "clues_80_cells":
        nz = nz[:, :80]
    clues = nz.sum(axis=1, dtype=u32)
    row = np.arange(rows, dtype=u32)
    live = np.ones(rows, dtype=bool) if mut == "no_row_guard" else row < u32(c.m)
    status = _padded(c.status, rows, 1)
    lv = _padded(c.level, rows, 1).astype(u32)
    hit = live & ((status != 0) if mut == "status_nonzero" else (status == 1))
    if mut != "no_level_guard":
        hit &= lv < u32(32)
    hit &= ((u32(c.mask) >> (lv & u32(31))) & u32(1)) == 1            # the shift count as the hardware takes it
    hit &= (clues > u32(c.clues[0])) if mut == "clues_lo_strict" else (clues >= u32(c.clues[0]))
    hit &= (clues < u32(c.clues[1])) if mut == "clues_hi_strict" else (clues <= u32(c.clues[1]))
    for name, src, rng, other in (("bd", c.backdoors, c.bd, c.open4), ("o4", c.open4, c.o4, c.backdoors)):
        if src is None or (other is not None and mut == f"{name}_skipped_with_{'o4' if name == 'bd' else 'bd'}"):
            continue
        v = _padded(src, rows, rng[0]).astype(u32)
        ok = (v > u32(rng[0])) if mut == f"{name}_lo_strict" else (v >= u32(rng[0]))
        ok &= (v < u32(rng[1])) if mut == f"{name}_hi_strict" else (v <= u32(rng[1]))
        held = np.ones(rows, dtype=bool) if mut == f"{name}_every_level" else lv == u32(4)
        hit &= ~held | ok
    hit = hit.reshape(tiles, TILE)
    ballot = (hit.astype(u64) << np.arange(TILE, dtype=u64)[None, :]).sum(axis=1, dtype=u64)
    return hit, ballot, _popc64(ballot)


def model_scan(count, base, mut=None):
    """-> (offset uint32[tiles], total): the one workgroup's loop, 1,024 tiles a step."""
    tiles = len(count)
    offset = np.zeros(tiles, dtype=u32)
    run = u32(0 if mut == "scan_no_carry_in" else base)
    with np.errstate(over="ignore"):
        for s in range(0, tiles, SCAN):
            live = min(SCAN, tiles - s)
            v = np.full(SCAN, 64 if mut == "scan_oob_lanes" else 0, dtype=u32)     # (a stale count of an older round)
            v[:live] = count[s:s + live]
            x = np.cumsum(v.reshape(SCAN // 64, 64), axis=1, dtype=u32)          # inclusive inside the wave
            wsum = x[:, 63]
            incl = np.cumsum(wsum, dtype=u32)
            before = incl if mut == "scan_before_le" else incl - wsum
            inside = x if mut == "scan_inclusive" else x - v.reshape(x.shape)
            off = (run + before[:, None] + inside).astype(u32).reshape(-1)
            offset[s:s + live] = off[:live]
            if mut != "scan_no_run_add":
                run = u32(run + wsum.sum(dtype=u32))
    return offset, int(run)


def select_model(c, mutant=None):
    assert mutant is None or mutant in MUTANTS, mutant
    mut = mutant
    hit, ballot, count = model_flag(c, mut)
    offset, total = model_scan(count, c.base, mut)
    n, tiles = c.n, c.tiles
    rows = n + SLACK
    out = blank(c, rows)
    writes = {k: np.zeros(rows * (81 if k in ("puzzles", "grids") else 1), dtype=np.int8)
              for k, a in out.items() if a is not None}
    w16 = {k: np.zeros(rows * 81, dtype=np.int8) for k in ("puzzles", "grids")}
    w1 = {k: np.zeros(rows * 81, dtype=np.int8) for k in ("puzzles", "grids")}
    flat = {k: out[k].reshape(-1) for k in ("puzzles", "grids")}

    # ---- scatter, the per-hit part: every tile at once
    active = (ballot != 0) & (offset < u32(n))
    with np.errstate(over="ignore"):
        room = (u32(n) - offset).astype(u32)
    kept = count.copy() if mut == "kept_unclamped" else np.minimum(count, room)
    hits_i = hit.astype(u32)
    below = np.cumsum(hits_i, axis=1, dtype=u32) - hits_i                # v_mbcnt lo, then hi
    if mut == "mbcnt_lo_only":
        below[:, 32:] = below[:, 32:33]                                  # the low half's count for every high lane
    keep = hit & ((below <= kept[:, None]) if mut == "below_le_kept" else (below < kept[:, None])) & active[:, None]
    t_idx, lane = np.nonzero(keep)
    row = (t_idx * TILE + lane).astype(np.int64)
    rank = (offset[t_idx] + below[t_idx, lane]).astype(np.int64)
    if not (rank < rows).all():
        raise BeyondSlack(mutant)
    src_rows = rank if mut == "gather_at_rank" else row

    def gathered(a):
        a = np.asarray(a)
        return a[np.minimum(src_rows, len(a) - 1)]

    none = 0 if mut == "absent_source_zero" else 0xFF
    per_hit = {"level": gathered(c.level), "open": gathered(c.open),
               "backdoors": gathered(c.backdoors) if c.backdoors is not None else none,
               "key": gathered(c.key) if c.key is not None else none,
               "open4": gathered(c.open4) if c.open4 is not None else none}
    if mut == "index_without_first":
        per_hit["index"] = row.astype(u64)
    elif mut == "index_32bit":
        per_hit["index"] = ((row + (c.first & 0xFFFFFFFF)) & 0xFFFFFFFF).astype(u64)
    else:
        with np.errstate(over="ignore"):
            per_hit["index"] = u64(c.first) + row.astype(u64)
    for k, v in per_hit.items():
        if out[k] is not None:
            out[k][rank] = v
            writes[k] += np.bincount(rank, minlength=rows).astype(np.int8)
    at = rank == (n if mut == "last_at_rank_n" else n - 1)
    last = int(row[at][-1]) + (0 if mut == "last_is_row" else 1) if at.any() else 0

    # ---- scatter, the rows: tile by tile through the pack buffer
    misaligned = 0
    ar81 = np.arange(81)
    pack = np.full(PACK + 128, POISON, dtype=np.uint8)       # (+128: a mutant's reads past the buffer)
    act = np.flatnonzero(active)
    srcs = (np.asarray(c.puzzles).reshape(tiles, TILE, 81),
            np.asarray(c.puzzles if mut == "grids_from_puzzles" else c.grids).reshape(tiles, TILE, 81))
    for t, rank0, kp in zip(act.tolist(), offset[act].tolist(), kept[act].tolist()):
        byte0 = 81 * rank0
        head = byte0 & (3 if mut == "head_mod4" else 15)
        end = head + 81 * kp
        in0 = 16 if (mut == "in0_16_at_head0" and head == 0) else (head + 15) & ~15
        in1 = (end + 15) & ~15 if mut == "in1_rounded_up" else end & ~15
        lanes = np.flatnonzero(keep[t])
        where = ((0 if mut == "pack_without_head" else head) + 81 * below[t, lanes].astype(np.int64))[:, None] + ar81
        base = byte0 - head
        n_head = 0 if mut == "no_head_bytes" else min(TILE, (in0 - head) & 0xFFFFFFFF)
        n_tail = 0 if mut == "no_tail_bytes" else min(TILE, (end - in1) & 0xFFFFFFFF)
        for k, src in zip(("puzzles", "grids"), srcs):
            pack[where] = src[t, lanes]
            o, wv, wb = flat[k], w16[k], w1[k]
            if in1 > in0:
                o[base + in0:base + in1] = pack[in0:in1]
                wv[base + in0:base + in1] += 1
            o[base + head:base + head + n_head] = pack[head:head + n_head]
            wb[base + head:base + head + n_head] += 1
            o[base + in1:base + in1 + n_tail] = pack[in1:in1 + n_tail]
            wb[base + in1:base + in1 + n_tail] += 1
        if in1 > in0 and (base + in0) % 16:
            misaligned += 2 * ((in1 - in0) // 16)
    for k in ("puzzles", "grids"):
        writes[k] = w16[k] + w1[k]
    return Model(out, total, last, writes, w16, w1, misaligned, ballot, offset)


def expected_writes(c, ref):
    """What the write maps must be, from the reference's tiles: every byte of a tile's range
    [81 rank0, 81 (rank0 + kept)) once -- by a 16-byte store where the 16-byte piece around it lies inside the
    range, else by a single-byte store -- and no byte outside; every per-hit entry of a kept rank once."""
    rows = c.n + SLACK
    w16 = np.zeros(rows * 81, dtype=np.int8)
    w1 = np.zeros(rows * 81, dtype=np.int8)
    for r0, k in zip(ref.rank0.tolist(), ref.kept.tolist()):
        if k == 0:
            continue
        lo, hi = 81 * r0, 81 * (r0 + k)
        a, b = (lo + 15) // 16 * 16, hi // 16 * 16
        w16[a:b] += 1
        w1[lo:a] += 1
        w1[b:hi] += 1
    per_hit = np.zeros(rows, dtype=np.int8)
    per_hit[c.base:min(c.n, ref.total)] = 1
    return w16, w1, per_hit
