"""Level-minimal generation rates (measuring tool; prints one JSON line).

rows:      `--rows` rows of the stream from row `--lo`: sdk_generate_level_dev at level 1, 2, 3 beside
           sdk_generate_puzzles_dev (the uniqueness minimiser: unchanged code, the yardstick) --
           rows per second of the HIP-event span (SDK_OPT_TIMING: one span per call).  With it the
           level mix (sdk_grade_batch_dev of the results) and the clue histogram of each level's rows.
delivered: puzzles of exactly level L per second, two ways, for about `--n` delivered puzzles each:
           generate_level_dev(L) over as many rows as its level-L share of the `rows` leg asks for,
           followed by grade_batch_dev (the count of level == L is what was delivered), beside
           generate_graded_dev(n, levels=(L,)) over the uniqueness-minimal stream.  The puzzles differ
           (the two streams share grids, not clue sets); the ratio of the two rates is the figure.
Every leg is resident on the device; the legs of a section are interleaved in one process, each round
running every leg once: `--warmup` rounds, then `--repeats` timed ones, median (min..max).

No oracle and no reference data are read.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_sudoku_solver_amd import SudokuEngine, synth  # noqa: E402

from bench_classify import sclk, stats, timed  # noqa: E402

LEVELS = (1, 2, 3)


def interleaved(eng, legs, warmup, repeats):
    """legs {name: fn} -> {name: {"events": stats, "wall": stats, "timed_spans": k}}."""
    ev = {k: [] for k in legs}
    wall = {k: [] for k in legs}
    spans = {}
    for r in range(warmup + repeats):
        for k, fn in legs.items():
            ms, w, spans[k] = timed(eng, fn)
            if r >= warmup:
                ev[k].append(ms)
                wall[k].append(w)
    return {k: {"events": stats(ev[k]), "wall": stats(wall[k]), "timed_spans": spans[k]} for k in legs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 16)
    ap.add_argument("--n", type=int, default=1 << 14)
    ap.add_argument("--lo", type=int, default=0)
    ap.add_argument("--seed", type=int, default=synth.DEFAULT_SEED + 3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    rows, n = a.rows, a.n
    res = {"tool": "bench_generate_level", "seed": a.seed, "lo": a.lo, "rows": rows, "n": n, "warmup": a.warmup,
           "repeats": a.repeats, "sclk_before": sclk(), "rows_leg": {}, "delivered": {}}
    ok = True
    with SudokuEngine(0) as eng:
        d_puz, d_grid, d_sol = eng.alloc(rows * 81), eng.alloc(rows * 81), eng.alloc(rows * 81)
        d_st, d_level, d_open = eng.alloc(rows), eng.alloc(rows), eng.alloc(rows)
        d_index = eng.alloc(rows * 8)

        # ---- rows per second
        legs = {"generate_batch": lambda: eng.generate_batch_dev(d_puz, d_grid, d_st, rows, seed=a.seed, lo=a.lo)}
        for lv in LEVELS:
            legs[f"generate_level_{lv}"] = (lambda lv=lv: eng.generate_level_dev(d_puz, d_grid, d_st, rows, lv,
                                                                                 seed=a.seed, lo=a.lo))
        r = interleaved(eng, legs, a.warmup, a.repeats)
        base = r["generate_batch"]["events"]["median_ms"]
        for k, v in r.items():
            v["rows_per_s"] = round(rows / v["events"]["median_ms"] * 1e3)
            v["events_over_generate_batch"] = round(v["events"]["median_ms"] / base, 4)
        share = {}
        for lv in LEVELS:
            legs[f"generate_level_{lv}"]()
            eng.grade_batch_dev(d_puz, d_sol, d_st, d_level, rows, d_open=d_open, budget=0)
            eng.synchronize()
            puz = d_puz.download(np.empty((rows, 81), dtype=np.uint8))
            level = d_level.download(np.empty(rows, dtype=np.uint8))
            grid = d_grid.download(np.empty((rows, 81), dtype=np.uint8))
            sol = d_sol.download(np.empty((rows, 81), dtype=np.uint8))
            kept = (grid != 0).any(axis=1)
            good = bool(((level >= 1) & (level <= lv))[kept].all() and (sol[kept] == grid[kept]).all()
                        and ((puz == 0) | (puz == grid)).all())
            ok = ok and good
            clues = (puz[kept] != 0).sum(axis=1)
            share[lv] = float((level == lv).sum()) / rows
            r[f"generate_level_{lv}"].update(
                level_mix={str(k): int((level == k).sum()) for k in range(5)},
                clue_histogram={str(k): int(c) for k, c in enumerate(np.bincount(clues)) if c},
                clues_mean=round(float(clues.mean()), 3), grids_kept=int(kept.sum()), results_ok=good)
        res["rows_leg"] = r
        print("rows", json.dumps(r), file=sys.stderr, flush=True)

        # ---- delivered level-L puzzles per second
        for lv in LEVELS:
            need = min(rows, -(-int(n / max(share[lv], 1e-6)) // 64) * 64)
            want = min(n, rows)
            got = []

            def level_then_grade():
                eng.generate_level_dev(d_puz, d_grid, d_st, need, lv, seed=a.seed, lo=a.lo)
                eng.grade_batch_dev(d_puz, d_sol, d_st, d_level, need, d_open=d_open, budget=0)

            def graded():
                got[:] = eng.generate_graded_dev(d_puz, d_grid, want, (lv,), seed=a.seed, lo=a.lo, d_level=d_level,
                                                 d_open=d_open, d_index=d_index)

            r = interleaved(eng, {"generate_level_then_grade": level_then_grade, "generate_graded": graded},
                            a.warmup, a.repeats)
            level_then_grade()
            eng.synchronize()
            delivered = int((d_level.download(np.empty(rows, dtype=np.uint8))[:need] == lv).sum())
            found, scanned = got
            x, y = r["generate_level_then_grade"], r["generate_graded"]
            x.update(rows=need, delivered=delivered, delivered_per_s=round(delivered / x["events"]["median_ms"] * 1e3))
            y.update(rows=scanned, delivered=found, delivered_per_s=round(found / y["events"]["median_ms"] * 1e3))
            r["delivered_per_s_ratio"] = round(x["delivered_per_s"] / max(y["delivered_per_s"], 1), 3)
            ok = ok and delivered > 0 and found == want
            res["delivered"][str(lv)] = r
            print("delivered", lv, json.dumps(r), file=sys.stderr, flush=True)
        for b in (d_puz, d_grid, d_sol, d_st, d_level, d_open, d_index):
            b.free()
    res["ok"] = ok
    res["sclk_after"] = sclk()
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
