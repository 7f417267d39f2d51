"""Grade rate beside classify on resident batches (measuring tool; prints one JSON line).

grade: sdk_grade_batch_dev and sdk_classify_batch_dev on the same boards in the same process,
  interleaved, `--repeats` rounds after `--warmup`: median, min and max of the HIP-event spans
  (SDK_OPT_TIMING) and of the host wall time around call + synchronise, their ratio, the level
  histogram and the mean open count of the level-4 boards.  classify is the yardstick: unchanged
  code on the same input in the same run.
generated: sdk_generate_puzzles_dev of `--n-generated` puzzles, then sdk_grade_batch_dev on the
  device-resident puzzles: the level mix of what the generator makes.
--stats (a -DSDK_GRADE32_STATS=1 build, tools/build_variant.sh, named by SDK_LIB_PATH): the
  grader's unit/cells steps and locked passes per group of 64 boards, per input.

Every leg runs under a watchdog (`--leg-timeout` seconds): a leg that does not come back ends the
process with status 124, so nothing is started on the device after it.
No oracle and no reference data are read: inputs come from synth's seeded generators.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_sudoku_solver_amd import SudokuEngine, synth, _lib as L  # noqa: E402
from bench_classify import sclk, timed  # noqa: E402


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


class Watchdog:
    """Ends the process (status 124) if the block takes longer than `seconds`."""

    def __init__(self, what, seconds):
        self.timer = threading.Timer(seconds, self.fire)
        self.timer.daemon = True
        self.what = what

    def fire(self):
        print(f"bench_grade: {self.what} exceeded its time limit", file=sys.stderr, flush=True)
        os._exit(124)

    def __enter__(self):
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()


def read_stats(eng):
    fn = getattr(eng.lib, "sdk_debug_g32_stats", None)
    if fn is None:
        raise SystemExit("--stats needs a -DSDK_GRADE32_STATS=1 build (SDK_LIB_PATH)")
    h = np.zeros((2, 128), dtype=np.uint64)
    if fn(ctypes.c_void_p(h.ctypes.data)) != 0:
        raise SystemExit("sdk_debug_g32_stats failed")
    return h


def histogram(h):
    """{value: groups} of one statistics row, and its mean."""
    nz = np.flatnonzero(h)
    return {"groups": {int(v): int(h[v]) for v in nz}, "mean": round(float((h * np.arange(128)).sum() / max(1, h.sum())), 2)}


def levels_of(lv, op):
    hist = np.bincount(lv, minlength=5)[:5]
    four = lv == L.SDK_GRADE_SEARCH
    return {"levels_0_to_4": hist.tolist(), "share_1_to_4": [round(float(x) / max(1, len(lv)), 4) for x in hist[1:]],
            "open_mean": round(float(op[four].mean()), 2) if four.any() else None,
            "open_min": int(op[four].min()) if four.any() else None,
            "open_max": int(op[four].max()) if four.any() else None}


def bench_grade(eng, name, boards, sols, warmup, repeats, want_stats):
    n = len(boards)
    d_in, d_out, d_st, d_lv, d_op = eng.alloc(n * 81), eng.alloc(n * 81), eng.alloc(n), eng.alloc(n), eng.alloc(n)
    d_in.upload(boards)

    def grade():
        eng.grade_batch_dev(d_in, d_out, d_st, d_lv, n, d_open=d_op, budget=0)

    def classify():
        eng.classify_batch_dev(d_in, d_out, d_st, n, budget=0)

    legs = (("grade", grade), ("classify", classify))
    ev = {k: [] for k, _ in legs}
    wall = {k: [] for k, _ in legs}
    und, spans = {}, {}
    res = {"n": n}
    if want_stats:
        read_stats(eng)      # (clears them)
    for r in range(warmup + repeats):
        for k, fn in legs:
            ms, w, spans[k] = timed(eng, fn)
            if r >= warmup:
                ev[k].append(ms)
                wall[k].append(w)
            und[k] = eng.get_option(L.SDK_OPT_PROP32_UNDECIDED)
            if r == 0:      # every leg's answers, once
                st = d_st.download(np.empty(n, dtype=np.int8))
                out = d_out.download(np.empty((n, 81), dtype=np.uint8))
                if not ((st == 1).all() and (out == sols).all()):
                    raise SystemExit(f"{name}/{k}: wrong answers")
                if k == "grade":
                    lv = d_lv.download(np.empty(n, dtype=np.uint8))
                    op = d_op.download(np.empty(n, dtype=np.uint8))
                    res.update(levels_of(lv, op))
                    if want_stats:
                        h = read_stats(eng)
                        res["steps_per_group"] = histogram(h[0])
                        res["locked_passes_per_group"] = histogram(h[1])
    for b in (d_in, d_out, d_st, d_lv, d_op):
        b.free()
    for k, _ in legs:
        e = stats(ev[k])
        res[k] = {"events": e, "wall": stats(wall[k]), "boards_per_s": round(n / e["median_ms"] * 1e3),
                  "listed_by_pass": und[k], "timed_spans": spans[k]}
    res["grade_over_classify"] = round(res["grade"]["events"]["median_ms"] / res["classify"]["events"]["median_ms"], 3)
    return res


def bench_generated(eng, n, warmup, repeats):
    d_p, d_g, d_st, d_lv, d_op = eng.alloc(n * 81), eng.alloc(n * 81), eng.alloc(n), eng.alloc(n), eng.alloc(n)
    eng.generate_batch_dev(d_p, d_g, d_st, n)
    eng.synchronize()
    gen_st = d_st.download(np.empty(n, dtype=np.int8))
    ev = []
    for r in range(warmup + repeats):
        ms, _, _ = timed(eng, lambda: eng.grade_batch_dev(d_p, d_g, d_st, d_lv, n, d_open=d_op, budget=0))
        if r >= warmup:
            ev.append(ms)
    st = d_st.download(np.empty(n, dtype=np.int8))
    lv = d_lv.download(np.empty(n, dtype=np.uint8))
    op = d_op.download(np.empty(n, dtype=np.uint8))
    for b in (d_p, d_g, d_st, d_lv, d_op):
        b.free()
    if not (st == gen_st).all():
        raise SystemExit("generated: the grader's verdicts differ from the minimiser's")
    res = {"n": n, "kept": int((gen_st == 1).sum()), "grade_events": stats(ev)}
    keep = gen_st == 1
    res.update(levels_of(lv[keep], op[keep]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="hard,minimal,17clue")
    ap.add_argument("--n-minimal", type=int, default=1_000_000)
    ap.add_argument("--n-17clue", type=int, default=10_000_000)
    ap.add_argument("--n-generated", type=int, default=1 << 16, help="0 = skip")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--leg-timeout", type=float, default=120.0, help="seconds per GPU leg")
    ap.add_argument("--stats", action="store_true")
    a = ap.parse_args()
    res = {"tool": "bench_grade", "warmup": a.warmup, "repeats": a.repeats, "sclk_before": sclk()}
    with SudokuEngine(0) as eng:
        res["grade"] = {}
        for name in filter(None, a.sets.split(",")):
            if name == "hard":
                p, s, _ = synth.load_hard(threads=16)
            elif name == "minimal":
                p, s = synth.make_minimal_sym(a.n_minimal, threads=16)
            elif name == "17clue":
                p, s = synth.make_17clue(a.n_17clue)
            else:
                raise SystemExit(f"unknown set {name}")
            with Watchdog(name, a.leg_timeout):
                res["grade"][name] = bench_grade(eng, name, p, s, a.warmup, a.repeats, a.stats)
            print(name, json.dumps(res["grade"][name]), file=sys.stderr, flush=True)
        if a.n_generated:
            with Watchdog("generated", a.leg_timeout):
                res["generated"] = bench_generated(eng, a.n_generated, a.warmup, a.repeats)
            print("generated", json.dumps(res["generated"]), file=sys.stderr, flush=True)
    res["sclk_after"] = sclk()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
