"""Chains rate beside the wings stage and grading on resident batches, and chains generation (measuring tool;
prints one JSON line and, with --out, writes it to a file).

chains: sdk_chains_batch_dev, sdk_wings_batch_dev and sdk_grade_batch_dev on the same boards in the same
  process, interleaved, `--repeats` rounds after `--warmup`: median, min and max of the HIP-event spans
  (SDK_OPT_TIMING) and of the host wall time around call + synchronise, the call ratio and the stage ratio
  against wings, the number of level-4 boards (the stage's work items), the `open7` histogram, the share with
  open7 == 0 and the share that needs a chain (open6 > 0, open7 == 0).  wings and grade are the yardsticks:
  the same call with the smaller stage and without one, on the same input in the same run.
generated: sdk_generate_puzzles_dev of `--n-generated` puzzles, then the three calls on the device-resident
  puzzles: the histogram of what the generator makes.
generate_chains: sdk_generate_chains_dev for `--n-chains` level-4 puzzles with open6 in 1..64 and open7 == 0
  from row 0 of the stream, beside what a caller does without the call over the same window:
  generate_batch, then chains_batch, then a numpy filter on the host (wall time, all three included); its
  keepers must be the call's.  0 skips it.

Every leg runs under a watchdog (`--leg-timeout` seconds): a leg that does not come back ends the process
with status 124, so nothing is started on the device after it.
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
from bench_generate_graded import leg, wall_leg  # noqa: E402
from bench_grade import Watchdog, stats  # noqa: E402


def counts_of(lv, op, o4, o5, o6, o7):
    four = lv == L.SDK_GRADE_SEARCH
    res = {"levels_0_to_4": np.bincount(lv, minlength=5)[:5].tolist(), "level4": int(four.sum())}
    if not all((col[~four] == 0xFF).all() for col in (o4, o5, o6, o7)):
        raise SystemExit("a board that is not of level 4 has a count")
    if four.any():
        t, u, v, w = o7[four], o6[four], o5[four], o4[four]
        if w.max() > 64 or (t > u).any() or (u > v).any() or (v > w).any() or (w > op[four]).any():
            raise SystemExit("inconsistent counts")
        hist = np.bincount(t, minlength=65)
        need = (u > 0) & (t == 0)
        res.update(open7_hist={int(k): int(hist[k]) for k in np.flatnonzero(hist)},
                   open6_zero=int((u == 0).sum()), open7_zero=int((t == 0).sum()),
                   open6_zero_share=round(float((u == 0).mean()), 4),
                   open7_zero_share=round(float((t == 0).mean()), 4), open7_below_open6=int((t < u).sum()),
                   need_chains=int(need.sum()), need_chains_share=round(float(need.mean()), 5),
                   open7_mean=round(float(t.mean()), 2))
    return res


def bench_chains(eng, name, d_in, n, sols, warmup, repeats):
    """d_in: the resident boards (left as they are); sols: their completions, or None."""
    d_out, d_st, d_lv, d_op, d_o4, d_o5, d_o6, d_o7 = [eng.alloc(n * 81)] + [eng.alloc(n) for _ in range(7)]

    def chains():
        eng.chains_batch_dev(d_in, d_out, d_st, d_lv, d_o7, n, d_open=d_op, d_open4=d_o4, d_open5=d_o5, d_open6=d_o6,
                             budget=0)

    def wings():
        eng.wings_batch_dev(d_in, d_out, d_st, d_lv, d_o6, n, d_open=d_op, d_open4=d_o4, d_open5=d_o5, budget=0)

    def grade():
        eng.grade_batch_dev(d_in, d_out, d_st, d_lv, n, d_open=d_op, budget=0)

    legs = (("chains", chains), ("wings", wings), ("grade", grade))
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
                if k == "chains":
                    own = u8(d_o4), u8(d_o5), u8(d_o6)
                    res.update(counts_of(first[k][1], first[k][2], *own, u8(d_o7)))
                if k == "wings" and not all((x == y).all() for x, y in zip(own, (u8(d_o4), u8(d_o5), u8(d_o6)))):
                    raise SystemExit(f"{name}: chains and wings disagree on open4, open5 or open6")
    for b in (d_out, d_st, d_lv, d_op, d_o4, d_o5, d_o6, d_o7):
        b.free()
    for k in ("wings", "grade"):
        if not all((x == y).all() for x, y in zip(first["chains"], first[k])):
            raise SystemExit(f"{name}: chains and {k} disagree on the shared outputs")
    for k, _ in legs:
        e = stats(ev[k])
        res[k] = {"events": e, "wall": stats(wall[k]), "boards_per_s": round(n / e["median_ms"] * 1e3),
                  "timed_spans": spans[k]}
    med = {k: res[k]["events"]["median_ms"] for k, _ in legs}
    c_stage, w_stage = med["chains"] - med["grade"], med["wings"] - med["grade"]
    res["chains_over_grade"] = round(med["chains"] / med["grade"], 3)
    res["chains_over_wings"] = round(med["chains"] / med["wings"], 3)
    res["chains_stage_ms"] = round(c_stage, 4)
    res["wings_stage_ms"] = round(w_stage, 4)
    res["chains_stage_over_wings_stage"] = round(c_stage / w_stage, 3) if w_stage > 0 else None
    res["level4_per_s_of_stage"] = round(res["level4"] / c_stage * 1e3) if c_stage > 0 and res["level4"] else None
    return res


def bench_generate(eng, n, seed, warmup, repeats):
    d_puz, d_grid = eng.alloc(n * 81), eng.alloc(n * 81)
    d_level, d_open, d_o6, d_o7 = (eng.alloc(n) for _ in range(4))
    d_index = eng.alloc(n * 8)
    got = []

    def call():
        got[:] = eng.generate_chains_dev(d_puz, d_grid, n, (4,), seed=seed, open6=(1, 64), open7=(0, 0), d_level=d_level,
                                         d_open=d_open, d_open6=d_o6, d_open7=d_o7, d_index=d_index)

    r = leg(eng, call, warmup, repeats)
    found, scanned = got
    index = d_index.download(np.empty(n, dtype=np.uint64))[:found]
    puz = d_puz.download(np.empty((n, 81), dtype=np.uint8))[:found]
    o6 = d_o6.download(np.empty(n, dtype=np.uint8))[:found]
    ms = r["events"]["median_ms"]
    r.update(n=n, found=found, scanned=scanned, delivered_per_s=round(found / ms * 1e3),
             scanned_per_s=round(scanned / ms * 1e3), delivered_per_s_wall=round(found / r["wall"]["median_ms"] * 1e3))

    def by_hand():
        p, s, st = eng.generate_batch(scanned, seed=seed)
        _, lv, op, v4, v5, v6, v7, _ = eng.chains_batch(p, budget=0)
        keep = np.flatnonzero((st == 1) & (lv == 4) & (v6 >= 1) & (v6 <= 64) & (v7 == 0))[:n]
        return p[keep], v6[keep], keep, int((lv == 4).sum())

    hand, out = wall_leg(by_hand, 1, max(3, repeats // 2))
    same = bool(len(out[2]) == found and (out[2] == index).all() and (out[0] == puz).all() and (out[1] == o6).all())
    r["by_hand"] = {"rows": scanned, "wall": hand, "same_keepers": same, "level4": out[3],
                    "wall_over_call_wall": round(hand["median_ms"] / r["wall"]["median_ms"], 3)}
    for b in (d_puz, d_grid, d_level, d_open, d_o6, d_o7, d_index):
        b.free()
    return r, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="hard,minimal")
    ap.add_argument("--n-minimal", type=int, default=1_000_000)
    ap.add_argument("--n-generated", type=int, default=1 << 16, help="0 = skip")
    ap.add_argument("--n-chains", type=int, default=64, help="quota of the generate_chains leg; 0 = skip")
    ap.add_argument("--seed", type=int, default=synth.DEFAULT_SEED + 3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--leg-timeout", type=float, default=120.0, help="seconds per GPU leg")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    res = {"tool": "bench_chains", "warmup": a.warmup, "repeats": a.repeats, "sclk_before": sclk(), "chains": {}}
    ok = True
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
                res["chains"][name] = bench_chains(eng, name, d_in, len(p), s, a.warmup, a.repeats)
            d_in.free()
            print(name, json.dumps(res["chains"][name]), file=sys.stderr, flush=True)
        if a.n_generated:
            n = a.n_generated
            d_p, d_g, d_st = eng.alloc(n * 81), eng.alloc(n * 81), eng.alloc(n)
            with Watchdog("generated", a.leg_timeout):
                eng.generate_batch_dev(d_p, d_g, d_st, n, seed=a.seed)
                eng.synchronize()
                kept = d_st.download(np.empty(n, dtype=np.int8)) == 1
                sols = d_g.download(np.empty((n, 81), dtype=np.uint8)) if kept.all() else None
                res["generated"] = bench_chains(eng, "generated", d_p, n, sols, a.warmup, a.repeats)
                res["generated"]["kept"] = int(kept.sum())
            for b in (d_p, d_g, d_st):
                b.free()
            print("generated", json.dumps(res["generated"]), file=sys.stderr, flush=True)
        if a.n_chains:
            with Watchdog("generate_chains", a.leg_timeout):
                res["generate_chains"], ok = bench_generate(eng, a.n_chains, a.seed, 1, max(3, a.repeats // 2))
            print("generate_chains", json.dumps(res["generate_chains"]), file=sys.stderr, flush=True)
    res["ok"] = ok
    res["sclk_after"] = sclk()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
