"""Subsets generation rates (measuring tool; prints one JSON line and, with --out, writes it to a file).

subsets:   sdk_generate_subsets_dev for `--n` puzzles of level 4 with open4 in `--open4` (default 0..0:
           the hard puzzles that need no guess) from row `--lo` of the stream (automatic rounds,
           device-resident outputs): delivered puzzles and candidates scanned per second of the
           HIP-event span (SDK_OPT_TIMING: one span per call) and of the host wall time.
           Beside it, what a caller does without the call over the same window [lo, lo + scanned):
           generate_batch, then subsets_batch, then a numpy filter on the host -- wall time, all three
           included; its keepers and their counts must be the call's.  The window's open4 histogram
           and the share of its level-4 puzzles with open4 == 0 come from that leg.
graded:    the same call with the range 0..64 beside sdk_generate_graded_dev for the same quota: what
           the subsets stage adds to a round when it filters nothing.
Each leg: `--repeats` timed passes after `--warmup`, median and spread.

No oracle and no reference data are read.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_sudoku_solver_amd import SudokuEngine, synth  # noqa: E402

from bench_classify import sclk  # noqa: E402
from bench_generate_graded import leg, wall_leg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--lo", type=int, default=0)
    ap.add_argument("--open4", type=int, nargs=2, default=(0, 0))
    ap.add_argument("--seed", type=int, default=synth.DEFAULT_SEED + 3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    n, rng = a.n, tuple(a.open4)
    res = {"tool": "bench_generate_subsets", "seed": a.seed, "lo": a.lo, "n": n, "open4": list(rng),
           "warmup": a.warmup, "repeats": a.repeats, "sclk_before": sclk()}
    with SudokuEngine(0) as eng:
        d_puz, d_grid = eng.alloc(n * 81), eng.alloc(n * 81)
        d_level, d_open, d_o4, d_index = eng.alloc(n), eng.alloc(n), eng.alloc(n), eng.alloc(n * 8)
        got = []

        def subsets():
            got[:] = eng.generate_subsets_dev(d_puz, d_grid, n, (4,), seed=a.seed, lo=a.lo, open4=rng, d_level=d_level,
                                              d_open=d_open, d_open4=d_o4, d_index=d_index)

        r = leg(eng, subsets, a.warmup, a.repeats)
        found, scanned = got
        index = d_index.download(np.empty(n, dtype=np.uint64))[:found]
        puz = d_puz.download(np.empty((n, 81), dtype=np.uint8))[:found]
        o4 = d_o4.download(np.empty(n, dtype=np.uint8))[:found]
        ms = r["events"]["median_ms"]
        r.update(found=found, scanned=scanned, delivered_per_s=round(found / ms * 1e3),
                 scanned_per_s=round(scanned / ms * 1e3),
                 delivered_per_s_wall=round(found / r["wall"]["median_ms"] * 1e3),
                 open4_of_the_hits=np.bincount(o4, minlength=rng[1] + 1).tolist())

        def by_hand():
            p, s, st = eng.generate_batch(scanned, seed=a.seed, lo=a.lo)
            _, lv, op, v, _ = eng.subsets_batch(p, budget=0)
            keep = np.flatnonzero((st == 1) & (lv == 4) & (v >= rng[0]) & (v <= rng[1]))[:n]
            return p[keep], v[keep], keep + a.lo, v[lv == 4]

        hand, out = wall_leg(by_hand, 1, max(3, a.repeats // 2))
        same = bool(len(out[2]) == found and (out[2] == index).all() and (out[0] == puz).all() and (out[1] == o4).all())
        hist = np.bincount(out[3], minlength=65)
        r["by_hand"] = {"rows": scanned, "wall": hand, "same_keepers": same,
                        "wall_over_subsets_wall": round(hand["median_ms"] / r["wall"]["median_ms"], 3),
                        "level4": int(len(out[3])), "open4_zero": int(hist[0]),
                        "open4_zero_share": round(float(hist[0] / max(1, len(out[3]))), 4),
                        "open4_hist": {int(k): int(hist[k]) for k in np.flatnonzero(hist)}}
        res["subsets"] = r
        print("subsets", json.dumps(r), file=sys.stderr, flush=True)

        q = 4096
        d_puz4, d_grid4 = eng.alloc(q * 81), eng.alloc(q * 81)

        def graded():
            got[:] = eng.generate_graded_dev(d_puz4, d_grid4, q, (4,), seed=a.seed, lo=a.lo)

        def full_range():
            got[:] = eng.generate_subsets_dev(d_puz4, d_grid4, q, (4,), seed=a.seed, lo=a.lo, open4=(0, 64))

        g = leg(eng, graded, a.warmup, a.repeats)
        g.update(found=got[0], scanned=got[1])
        f = leg(eng, full_range, a.warmup, a.repeats)
        f.update(found=got[0], scanned=got[1],
                 events_over_graded=round(f["events"]["median_ms"] / g["events"]["median_ms"], 3))
        same = same and (f["found"], f["scanned"]) == (g["found"], g["scanned"])
        res["full_range"] = {"n": q, "graded": g, "subsets": f}
        print("full_range", json.dumps(res["full_range"]), file=sys.stderr, flush=True)
        for b in (d_puz, d_grid, d_level, d_open, d_o4, d_index, d_puz4, d_grid4):
            b.free()
    res["ok"] = same
    res["sclk_after"] = sclk()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
