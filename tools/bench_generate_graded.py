"""Graded generation rates (measuring tool; prints one JSON line).

levels:    for each level 1..4, sdk_generate_graded_dev for `--n` puzzles of that level from row `--lo`
           of the stream (automatic rounds, device-resident outputs): the rate of delivered puzzles
           and of candidates scanned (`scanned` of the result) per second of the HIP-event span
           (SDK_OPT_TIMING: one span per call) and of the host wall time.
           Beside it, what a caller does without the call over the same window [lo, lo + scanned):
           generate_batch, then grade_batch, then a numpy filter on the host -- wall time, all three
           included; its keepers must be the call's.
overhead:  what the selection launches and the per-round readback add to generate plus grade: the
           same `--rows` rows in rounds of `--chunk`, once as ONE graded call that cannot end early
           (quota = the rows; every level = every row is kept and copied, and level 1 alone = about
           one row in a hundred), once as generate_batch_dev + grade_batch_dev per round.  HIP-event
           spans (summed over the rounds' calls) and wall; the ratio is graded / (generate + grade).
Each leg: `--repeats` timed passes after `--warmup`, median and spread.

No oracle and no reference data are read.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_sudoku_solver_amd import SudokuEngine, synth  # noqa: E402

from bench_classify import sclk, stats, timed  # noqa: E402


def leg(eng, fn, warmup, repeats):
    ev, wall = [], []
    for r in range(warmup + repeats):
        ms, w, spans = timed(eng, fn)
        if r >= warmup:
            ev.append(ms)
            wall.append(w)
    return {"events": stats(ev), "wall": stats(wall), "timed_spans": spans}


def wall_leg(fn, warmup, repeats):
    w = []
    for r in range(warmup + repeats):
        t = time.perf_counter()
        out = fn()
        if r >= warmup:
            w.append((time.perf_counter() - t) * 1e3)
    return stats(w), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--lo", type=int, default=0)
    ap.add_argument("--rows", type=int, default=1 << 18)
    ap.add_argument("--chunk", type=int, default=1 << 16)
    ap.add_argument("--seed", type=int, default=synth.DEFAULT_SEED + 3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if a.rows % a.chunk:
        ap.error("--rows must be a multiple of --chunk")
    res = {"tool": "bench_generate_graded", "seed": a.seed, "lo": a.lo, "n": a.n, "warmup": a.warmup,
           "repeats": a.repeats, "sclk_before": sclk(), "levels": {}, "overhead": {}}
    ok = True
    n, rows, chunk = a.n, a.rows, a.chunk
    cap = max(n, rows)
    with SudokuEngine(0) as eng:
        d_puz, d_grid, d_sol = eng.alloc(cap * 81), eng.alloc(cap * 81), eng.alloc(cap * 81)
        d_level, d_open, d_st, d_index = eng.alloc(cap), eng.alloc(cap), eng.alloc(cap), eng.alloc(cap * 8)
        for level in (1, 2, 3, 4):
            got = []

            def graded():
                got[:] = eng.generate_graded_dev(d_puz, d_grid, n, (level,), seed=a.seed, lo=a.lo, d_level=d_level,
                                                 d_open=d_open, d_index=d_index)

            r = leg(eng, graded, a.warmup, a.repeats)
            found, scanned = got
            index = d_index.download(np.empty(n, dtype=np.uint64))[:found]
            puz = d_puz.download(np.empty((n, 81), dtype=np.uint8))[:found]
            ms = r["events"]["median_ms"]
            r.update(found=found, scanned=scanned, delivered_per_s=round(found / ms * 1e3),
                     scanned_per_s=round(scanned / ms * 1e3),
                     delivered_per_s_wall=round(found / r["wall"]["median_ms"] * 1e3))

            def by_hand():
                p, s, st = eng.generate_batch(scanned, seed=a.seed, lo=a.lo)
                _, lv, op, _ = eng.grade_batch(p, budget=0)
                keep = np.flatnonzero((st == 1) & (lv == level))[:n]
                return p[keep], s[keep], lv[keep], op[keep], keep + a.lo

            hand, out = wall_leg(by_hand, 1, max(3, a.repeats // 2))
            same = bool(len(out[4]) == found and (out[4] == index).all() and (out[0] == puz).all())
            ok = ok and same
            r["by_hand"] = {"rows": scanned, "wall": hand, "same_keepers": same,
                            "wall_over_graded_wall": round(hand["median_ms"] / r["wall"]["median_ms"], 3)}
            res["levels"][str(level)] = r
            print("level", level, json.dumps(r), file=sys.stderr, flush=True)

        def parts():
            for c0 in range(0, rows, chunk):
                eng.generate_batch_dev(d_puz, d_grid, d_st, chunk, seed=a.seed, lo=a.lo + c0)
                eng.grade_batch_dev(d_puz, d_sol, d_st, d_level, chunk, d_open=d_open, budget=0)

        base = leg(eng, parts, a.warmup, a.repeats)
        res["overhead"] = {"rows": rows, "chunk": chunk, "generate_plus_grade": base}
        for name, levels in (("every_level", (1, 2, 3, 4)), ("level_1", (1,))):
            got = []

            def graded():
                got[:] = eng.generate_graded_dev(d_puz, d_grid, rows, levels, seed=a.seed, lo=a.lo, max_scan=rows,
                                                 chunk=chunk, d_level=d_level, d_open=d_open, d_index=d_index)

            r = leg(eng, graded, a.warmup, a.repeats)
            r.update(found=got[0], scanned=got[1],
                     events_ratio=round(r["events"]["median_ms"] / base["events"]["median_ms"], 4),
                     wall_ratio=round(r["wall"]["median_ms"] / base["wall"]["median_ms"], 4))
            res["overhead"][name] = r
        print("overhead", json.dumps(res["overhead"]), file=sys.stderr, flush=True)
        for b in (d_puz, d_grid, d_sol, d_level, d_open, d_st, d_index):
            b.free()
    res["ok"] = ok
    res["sclk_after"] = sclk()
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
