"""Canonical-form rate beside classify on resident batches (measuring tool; prints one JSON line and, with
--out, writes it to a file).

canonical: sdk_canonical_batch_dev and sdk_classify_batch_dev on the same boards in the same process,
  interleaved, `--repeats` rounds after `--warmup`: median, min and max of the HIP-event spans
  (SDK_OPT_TIMING) and of the host wall time around call + synchronise, the ratio, the canonical stage
  alone (canonical minus classify: the call is the classify path plus one launch), the `ties` histogram
  and the number of distinct classes.  classify is the yardstick: unchanged code on the same input in
  the same run.  For the symmetric copies of `--base` minimal puzzles the classes are also counted among
  the base puzzles alone: how many of them are inequivalent.
generated: sdk_generate_puzzles_dev of `--n-generated` puzzles, then the two calls on the
  device-resident puzzles.

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
from distributed_sudoku_solver_amd import SudokuEngine, synth  # noqa: E402
from bench_classify import sclk, timed  # noqa: E402
from bench_grade import Watchdog, stats  # noqa: E402


def classes_of(canon):
    """distinct rows of uint8[m, 81]"""
    return int(len(np.unique(np.ascontiguousarray(canon).view("V81"))))


def bench_canonical(eng, name, d_in, n, boards, sols, warmup, repeats):
    """d_in: the resident boards (left as they are); boards: the same rows on the host, or None; sols:
    their completions, or None."""
    d_canon, d_sol, d_out, d_g, d_rl, d_ties, d_st = (eng.alloc(n * 81), eng.alloc(n * 81), eng.alloc(n * 81),
                                                      eng.alloc(n * 81), eng.alloc(n * 10), eng.alloc(n * 2),
                                                      eng.alloc(n))

    def canonical():
        eng.canonical_batch_dev(d_in, d_canon, d_st, n, d_solution=d_sol, d_gather=d_g, d_relabel=d_rl,
                                d_ties=d_ties, budget=0)

    def classify():
        eng.classify_batch_dev(d_in, d_out, d_st, n, budget=0)

    legs = (("canonical", canonical), ("classify", classify))
    ev = {k: [] for k, _ in legs}
    wall = {k: [] for k, _ in legs}
    spans, status = {}, {}
    res = {"n": n}
    for r in range(warmup + repeats):
        for k, fn in legs:
            ms, w, spans[k] = timed(eng, fn)
            if r >= warmup:
                ev[k].append(ms)
                wall[k].append(w)
            if r == 0:      # every leg's answers, once
                status[k] = d_st.download(np.empty(n, dtype=np.int8))
                if k == "classify":
                    out = d_out.download(np.empty((n, 81), dtype=np.uint8))
                    if sols is not None and not ((status[k] == 1).all() and (out == sols).all()):
                        raise SystemExit(f"{name}/{k}: wrong answers")
                    continue
                canon = d_canon.download(np.empty((n, 81), dtype=np.uint8))
                m = d_sol.download(np.empty((n, 81), dtype=np.uint8))
                g = d_g.download(np.empty((n, 81), dtype=np.uint8))
                rl = d_rl.download(np.empty((n, 10), dtype=np.uint8))
                ties = d_ties.download(np.empty(n, dtype=np.uint16))
                ok = ties > 0
                if boards is not None:
                    if not (synth.apply_symmetries(boards, g.astype(np.int16), rl) == canon).all():
                        raise SystemExit(f"{name}: the returned symmetry does not give the canonical puzzle")
                    if sols is not None and not (synth.apply_symmetries(sols, g.astype(np.int16), rl)[ok] == m[ok]).all():
                        raise SystemExit(f"{name}: the returned symmetry does not give the canonical solution")
                if not (m[ok][:, :9] == np.arange(1, 10)).all():
                    raise SystemExit(f"{name}: a canonical solution whose first row is not 1..9")
                hist = np.bincount(ties)
                res.update(eligible=int(ok.sum()), ties_hist={int(k): int(hist[k]) for k in np.flatnonzero(hist)},
                           classes=classes_of(canon[ok]), solution_classes=classes_of(m[ok]))
                res["canon"] = canon
    for b in (d_canon, d_sol, d_out, d_g, d_rl, d_ties, d_st):
        b.free()
    if not (status["canonical"] == status["classify"]).all():
        raise SystemExit(f"{name}: canonical and classify disagree on the status")
    for k, _ in legs:
        e = stats(ev[k])
        res[k] = {"events": e, "wall": stats(wall[k]), "boards_per_s": round(n / e["median_ms"] * 1e3),
                  "timed_spans": spans[k]}
    med = {k: res[k]["events"]["median_ms"] for k, _ in legs}
    extra = med["canonical"] - med["classify"]
    res["canonical_over_classify"] = round(med["canonical"] / med["classify"], 3)
    res["canonical_stage_ms"] = round(extra, 4)
    res["boards_per_s_of_stage"] = round(n / extra * 1e3) if extra > 0 else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="hard,minimal")
    ap.add_argument("--n-minimal", type=int, default=1_000_000)
    ap.add_argument("--base", type=int, default=65536, help="base puzzles of the minimal set")
    ap.add_argument("--n-generated", type=int, default=1 << 16, help="0 = skip")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--leg-timeout", type=float, default=120.0, help="seconds per GPU leg")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    res = {"tool": "bench_canonical", "warmup": a.warmup, "repeats": a.repeats, "sclk_before": sclk(), "canonical": {}}
    with SudokuEngine(0) as eng:
        for name in filter(None, a.sets.split(",")):
            if name == "hard":
                p, s, _ = synth.load_hard(threads=16)
            elif name == "minimal":
                p, s = synth.make_minimal_sym(a.n_minimal, base=a.base, threads=16)
            else:
                raise SystemExit(f"unknown set {name}")
            d_in = eng.alloc(len(p) * 81)
            d_in.upload(p)
            with Watchdog(name, a.leg_timeout):
                r = bench_canonical(eng, name, d_in, len(p), p, s, a.warmup, a.repeats)
            d_in.free()
            canon = r.pop("canon")
            if name == "minimal":
                # row j is a copy of base puzzle j % base: the copies must agree, and the classes are the base's
                base = min(a.base, len(p))
                if not (canon == canon[np.arange(len(p)) % base]).all():
                    raise SystemExit("minimal: symmetric copies of one puzzle have different canonical forms")
                r.update(base=base, inequivalent_base_puzzles=classes_of(canon[:base]))
            res["canonical"][name] = r
            print(name, json.dumps(r), file=sys.stderr, flush=True)
        if a.n_generated:
            n = a.n_generated
            d_p, d_g, d_st = eng.alloc(n * 81), eng.alloc(n * 81), eng.alloc(n)
            with Watchdog("generated", a.leg_timeout):
                eng.generate_batch_dev(d_p, d_g, d_st, n)
                eng.synchronize()
                kept = d_st.download(np.empty(n, dtype=np.int8)) == 1
                puz = d_p.download(np.empty((n, 81), dtype=np.uint8))
                sols = d_g.download(np.empty((n, 81), dtype=np.uint8)) if kept.all() else None
                r = bench_canonical(eng, "generated", d_p, n, puz, sols, a.warmup, a.repeats)
                r.pop("canon")
                r["kept"] = int(kept.sum())
                res["generated"] = r
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
