"""Subsets rate beside grading and rating on resident batches (measuring tool; prints one JSON line and,
with --out, writes it to a file).

subsets: sdk_subsets_batch_dev, sdk_grade_batch_dev and sdk_rate_batch_dev on the same boards in the
  same process, interleaved, `--repeats` rounds after `--warmup`: median, min and max of the HIP-event
  spans (SDK_OPT_TIMING) and of the host wall time around call + synchronise, the ratios, the number of
  level-4 boards (the stage's work items), the `open4` histogram and the share with open4 == 0.
  grade is the yardstick: the same call without the stage, on the same input in the same run.
generated: sdk_generate_puzzles_dev of `--n-generated` puzzles, then the three calls on the
  device-resident puzzles: the histogram of what the generator makes.

Every leg runs under a watchdog (`--leg-timeout` seconds): a leg that does not come back ends the
process with status 124, so nothing is started on the device after it.
No oracle and no reference data are read: inputs come from synth's seeded generators.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_sudoku_solver_amd import SudokuEngine, synth, _lib as L  # noqa: E402
from bench_classify import sclk, timed  # noqa: E402
from bench_grade import Watchdog, stats  # noqa: E402


def counts_of(lv, op, o4):
    four = lv == L.SDK_GRADE_SEARCH
    res = {"levels_0_to_4": np.bincount(lv, minlength=5)[:5].tolist(), "level4": int(four.sum())}
    if not (o4[~four] == L.SDK_SUBSETS_NONE).all():
        raise SystemExit("a board that is not of level 4 has a subsets count")
    if four.any():
        v = o4[four]
        if v.max() > 64 or (v > op[four]).any():
            raise SystemExit("inconsistent subsets counts")
        hist = np.bincount(v, minlength=65)
        res.update(open4_hist={int(k): int(hist[k]) for k in np.flatnonzero(hist)},
                   open4_zero=int((v == 0).sum()), open4_zero_share=round(float((v == 0).mean()), 4),
                   open4_below_open=int((v < op[four]).sum()), open4_mean=round(float(v.mean()), 2))
    return res


def bench_subsets(eng, name, d_in, n, sols, warmup, repeats):
    """d_in: the resident boards (left as they are); sols: their completions, or None."""
    d_out, d_st, d_lv, d_op, d_o4, d_bd = [eng.alloc(n * 81)] + [eng.alloc(n) for _ in range(5)]

    def subsets():
        eng.subsets_batch_dev(d_in, d_out, d_st, d_lv, d_o4, n, d_open=d_op, budget=0)

    def grade():
        eng.grade_batch_dev(d_in, d_out, d_st, d_lv, n, d_open=d_op, budget=0)

    def rate():
        eng.rate_batch_dev(d_in, d_out, d_st, d_lv, d_bd, n, d_open=d_op, budget=0)

    legs = (("subsets", subsets), ("grade", grade), ("rate", rate))
    ev = {k: [] for k, _ in legs}
    wall = {k: [] for k, _ in legs}
    spans, first = {}, {}
    res = {"n": n}
    u8 = lambda d: d.download(np.empty(n, dtype=np.uint8))
    for r in range(warmup + repeats):
        for k, fn in legs:
            ms, w, spans[k] = timed(eng, fn)
            if r >= warmup:
                ev[k].append(ms)
                wall[k].append(w)
            if r == 0:      # every leg's answers, once
                st = d_st.download(np.empty(n, dtype=np.int8))
                out = d_out.download(np.empty((n, 81), dtype=np.uint8))
                if sols is not None and not ((st == 1).all() and (out == sols).all()):
                    raise SystemExit(f"{name}/{k}: wrong answers")
                first[k] = (st, u8(d_lv), u8(d_op), out)
                if k == "subsets":
                    res.update(counts_of(first[k][1], first[k][2], u8(d_o4)))
    for b in (d_out, d_st, d_lv, d_op, d_o4, d_bd):
        b.free()
    for k in ("grade", "rate"):
        if not all((x == y).all() for x, y in zip(first["subsets"], first[k])):
            raise SystemExit(f"{name}: subsets and {k} disagree on the shared outputs")
    for k, _ in legs:
        e = stats(ev[k])
        res[k] = {"events": e, "wall": stats(wall[k]), "boards_per_s": round(n / e["median_ms"] * 1e3),
                  "timed_spans": spans[k]}
    med = {k: res[k]["events"]["median_ms"] for k, _ in legs}
    extra = med["subsets"] - med["grade"]
    res["subsets_over_grade"] = round(med["subsets"] / med["grade"], 3)
    res["subsets_over_rate"] = round(med["subsets"] / med["rate"], 3)
    res["subsets_stage_ms"] = round(extra, 4)
    res["rate_stage_ms"] = round(med["rate"] - med["grade"], 4)
    res["level4_per_s_of_stage"] = round(res["level4"] / extra * 1e3) if extra > 0 and res["level4"] else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="hard,minimal")
    ap.add_argument("--n-minimal", type=int, default=1_000_000)
    ap.add_argument("--n-generated", type=int, default=1 << 16, help="0 = skip")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--leg-timeout", type=float, default=120.0, help="seconds per GPU leg")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    res = {"tool": "bench_subsets", "warmup": a.warmup, "repeats": a.repeats, "sclk_before": sclk(), "subsets": {}}
    with SudokuEngine(0) as eng:
        for name in filter(None, a.sets.split(",")):
            if name == "hard":
                p, s, _ = synth.load_hard(threads=16)
            elif name == "minimal":
                p, s = synth.make_minimal_sym(a.n_minimal, threads=16)
            else:
                raise SystemExit(f"unknown set {name}")
            d_in = eng.alloc(len(p) * 81)
            d_in.upload(p)
            with Watchdog(name, a.leg_timeout):
                res["subsets"][name] = bench_subsets(eng, name, d_in, len(p), s, a.warmup, a.repeats)
            d_in.free()
            print(name, json.dumps(res["subsets"][name]), file=sys.stderr, flush=True)
        if a.n_generated:
            n = a.n_generated
            d_p, d_g, d_st = eng.alloc(n * 81), eng.alloc(n * 81), eng.alloc(n)
            with Watchdog("generated", a.leg_timeout):
                eng.generate_batch_dev(d_p, d_g, d_st, n)
                eng.synchronize()
                kept = d_st.download(np.empty(n, dtype=np.int8)) == 1
                sols = d_g.download(np.empty((n, 81), dtype=np.uint8)) if kept.all() else None
                res["generated"] = bench_subsets(eng, "generated", d_p, n, sols, a.warmup, a.repeats)
                res["generated"]["kept"] = int(kept.sum())
            for b in (d_p, d_g, d_st):
                b.free()
            print("generated", json.dumps(res["generated"]), file=sys.stderr, flush=True)
    res["sclk_after"] = sclk()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
