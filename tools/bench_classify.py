"""Classify and minimise rates on resident batches (measuring tool; prints one JSON line).

classify: sdk_classify_batch_dev beside two solves of the same boards in the same process --
  SDK_ORDER_MRV_UNIQUE with donate 0 (one launch; on all-unique boards the same search as the
  classify launch) and the default phased LEX solve -- interleaved, `--repeats` rounds after
  `--warmup`, median and spread (max - min) of the HIP-event kernel spans (SDK_OPT_TIMING) and the
  host wall time around call + synchronise.
minimise: sdk_minimize_batch_dev on complete grids (grids per second), beside synth.make_minimal on
  16 CPU threads (which also generates its grids).
--profile-rounds N: a diagnostic minimise of N grids driven from the host, round by round, reading
  SDK_OPT_PROP32_UNDECIDED after every round's classify: the share of boards the propagation pass
  decides per round.

No oracle and no reference data are read: inputs come from synth's seeded generators.
"""
import argparse
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_sudoku_solver_amd import SudokuEngine, synth, _lib as L  # noqa: E402


def sclk():
    """The shader clock the driver reports as current (best effort, read-only)."""
    for path in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            for line in open(path):
                if "*" in line:
                    return line.split(":", 1)[1].replace("*", "").strip()
        except OSError:
            pass
    return None


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "spread_ms": round(max(v) - min(v), 4)}


def timed(eng, fn):
    eng.timer_reset()
    t = time.perf_counter()
    fn()
    eng.synchronize()
    wall = (time.perf_counter() - t) * 1e3
    ms, launches = eng.timer_read()
    eng.timer_stop()
    return ms, wall, launches


def bench_classify(eng, name, boards, sols, warmup, repeats):
    n = len(boards)
    d_in, d_out, d_st = eng.alloc(n * 81), eng.alloc(n * 81), eng.alloc(n)
    d_in.upload(boards)

    def classify():
        eng.classify_batch_dev(d_in, d_out, d_st, n, budget=0)

    def mrv():
        eng.set_option(L.SDK_OPT_ORDER, L.SDK_ORDER_MRV_UNIQUE)
        eng.set_option(L.SDK_OPT_DONATE, 0)
        eng.solve_batch_dev(d_in, d_out, d_st, n)

    def lex():
        eng.set_option(L.SDK_OPT_ORDER, L.SDK_ORDER_LEX)
        eng.set_option(L.SDK_OPT_DONATE, 1)
        eng.solve_batch_dev(d_in, d_out, d_st, n)

    legs = (("classify", classify), ("solve_mrv_unique_donate0", mrv), ("solve_lex_phased", lex))
    ev = {k: [] for k, _ in legs}
    wall = {k: [] for k, _ in legs}
    und = {}
    for r in range(warmup + repeats):
        for k, fn in legs:
            ms, w, _ = timed(eng, fn)
            if r >= warmup:
                ev[k].append(ms)
                wall[k].append(w)
            und[k] = eng.get_option(L.SDK_OPT_PROP32_UNDECIDED)
            if r == 0:      # every leg's answers, once
                st = d_st.download(np.empty(n, dtype=np.int8))
                out = d_out.download(np.empty((n, 81), dtype=np.uint8))
                if not ((st == 1).all() and (out == sols).all()):
                    raise SystemExit(f"{name}/{k}: wrong answers")
    eng.set_option(L.SDK_OPT_ORDER, L.SDK_ORDER_LEX)
    eng.set_option(L.SDK_OPT_DONATE, 1)
    for b in (d_in, d_out, d_st):
        b.free()
    res = {"n": n}
    for k, _ in legs:
        e = stats(ev[k])
        res[k] = {"events": e, "wall": stats(wall[k]), "boards_per_s": round(n / e["median_ms"] * 1e3),
                  "undecided_by_pass": und[k]}
    return res


def bench_minimize(eng, grids, warmup, repeats):
    n = len(grids)
    order = np.random.default_rng(1).permuted(np.tile(np.arange(81, dtype=np.uint8), (n, 1)), axis=1)
    d_in, d_ord, d_out, d_st = eng.alloc(n * 81), eng.alloc(n * 81), eng.alloc(n * 81), eng.alloc(n)
    d_in.upload(grids)
    d_ord.upload(order)
    ev, wall = [], []
    for r in range(warmup + repeats):
        ms, w, launches = timed(eng, lambda: eng.minimize_batch_dev(d_in, d_ord, d_out, d_st, n))
        if r >= warmup:
            ev.append(ms)
            wall.append(w)
    out = d_out.download(np.empty((n, 81), dtype=np.uint8))
    st = d_st.download(np.empty(n, dtype=np.int8))
    for b in (d_in, d_ord, d_out, d_st):
        b.free()
    if not ((st == 1).all() and ((out == grids) | (out == 0)).all()):
        raise SystemExit("minimise: wrong answers")
    clues = (out != 0).sum(axis=1)
    e = stats(ev)
    return {"n": n, "events": e, "wall": stats(wall), "timed_spans": launches,
            "grids_per_s": round(n / e["median_ms"] * 1e3), "grids_per_s_wall": round(n / statistics.median(wall) * 1e3),
            "clues_mean": round(float(clues.mean()), 2), "clues_min": int(clues.min()), "clues_max": int(clues.max())}


def profile_rounds(eng, grids):
    """The minimiser's rounds driven from the host (diagnostic: same results, far slower)."""
    n = len(grids)
    order = np.random.default_rng(1).permuted(np.tile(np.arange(81, dtype=np.uint8), (n, 1)), axis=1)
    rows = np.arange(n)
    cur = grids.copy()
    rounds = []
    for q in range(81):
        cell = order[:, q]
        live = cur[rows, cell] != 0
        cand = cur[live].copy()
        cand[np.arange(len(cand)), cell[live]] = 0
        st, _ = eng.classify_batch(cand)
        und = eng.get_option(L.SDK_OPT_PROP32_UNDECIDED)
        keep = np.zeros(n, dtype=bool)
        keep[live] = st == 1
        cur[rows[keep], cell[keep]] = 0
        rounds.append({"round": q, "candidates": int(live.sum()), "undecided_by_pass": int(und),
                       "decided_share": round(1.0 - und / max(1, int(live.sum())), 4), "removed": int(keep.sum())})
    return rounds


def grids_of(n):
    g0 = synth.minimal_grids(np.arange(min(n, 65536)), threads=16)
    if n <= len(g0):
        return g0
    gather, relabel = synth.random_symmetries(np.random.default_rng(2), n)
    return synth.apply_symmetries(g0[np.arange(n) % len(g0)], gather, relabel)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="hard,minimal,17clue")
    ap.add_argument("--n-minimal", type=int, default=1_000_000)
    ap.add_argument("--n-17clue", type=int, default=10_000_000)
    ap.add_argument("--minimize", default="65536,1000000", help="grid counts, comma separated ('' = none)")
    ap.add_argument("--cpu-minimal", type=int, default=65536, help="synth.make_minimal on 16 threads (0 = skip)")
    ap.add_argument("--profile-rounds", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    res = {"tool": "bench_classify", "warmup": a.warmup, "repeats": a.repeats, "sclk_before": sclk()}
    with SudokuEngine(0) as eng:
        res["classify"] = {}
        for name in filter(None, a.sets.split(",")):
            if name == "hard":
                p, s, _ = synth.load_hard(threads=16)
            elif name == "minimal":
                p, s = synth.make_minimal_sym(a.n_minimal, threads=16)
            elif name == "17clue":
                p, s = synth.make_17clue(a.n_17clue)
            else:
                raise SystemExit(f"unknown set {name}")
            res["classify"][name] = bench_classify(eng, name, p, s, a.warmup, a.repeats)
            print(name, json.dumps(res["classify"][name]), file=sys.stderr, flush=True)
        res["minimize"] = []
        for n in filter(None, a.minimize.split(",")):
            res["minimize"].append(bench_minimize(eng, grids_of(int(n)), a.warmup, a.repeats))
            print("minimize", json.dumps(res["minimize"][-1]), file=sys.stderr, flush=True)
        if a.cpu_minimal:
            t = time.perf_counter()
            synth.make_minimal(a.cpu_minimal, seed=77, threads=16)
            dt = time.perf_counter() - t
            res["cpu_make_minimal"] = {"n": a.cpu_minimal, "threads": 16, "seconds": round(dt, 3),
                                       "puzzles_per_s": round(a.cpu_minimal / dt),
                                       "note": "includes generating the grids"}
        if a.profile_rounds:
            res["round_profile"] = {"n": a.profile_rounds, "rounds": profile_rounds(eng, grids_of(a.profile_rounds))}
    res["sclk_after"] = sclk()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
