"""Generation rates: the GPU generator beside the CPU one (measuring tool; prints one JSON line).

grids:   sdk_generate_grids_dev (grids, orders and placement counts; and grids alone) on `--grids`
         rows, device-resident -- beside gen_grid_batch (synth.minimal_grids) on 16 CPU threads.
puzzles: sdk_generate_puzzles_dev (generate + minimise) on `--puzzles` rows -- beside
         gen_minimal_batch (synth.make_minimal) on 16 CPU threads, `--cpu-puzzles` rows.
Each GPU leg: `--repeats` timed passes after `--warmup`, median and spread of the HIP-event span
(SDK_OPT_TIMING) and of the host wall time around call + synchronise.
parity:  the first `--parity` rows of both GPU calls equal synth.grid_orders / synth.make_minimal.

No oracle and no reference data are read.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_sudoku_solver_amd import SudokuEngine, synth  # noqa: E402

from bench_classify import sclk, stats, timed  # noqa: E402


def gpu_leg(eng, n, fn, warmup, repeats):
    ev, wall = [], []
    for r in range(warmup + repeats):
        ms, w, spans = timed(eng, fn)
        if r >= warmup:
            ev.append(ms)
            wall.append(w)
    e = stats(ev)
    return {"n": n, "events": e, "wall": stats(wall), "timed_spans": spans,
            "per_s": round(n / e["median_ms"] * 1e3), "per_s_wall": round(n / statistics.median(wall) * 1e3)}


def cpu_leg(n, fn):
    t = time.perf_counter()
    fn()
    dt = time.perf_counter() - t
    return {"n": n, "threads": 16, "seconds": round(dt, 3), "per_s": round(n / dt)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, default=1 << 20)
    ap.add_argument("--puzzles", type=int, default=1 << 16)
    ap.add_argument("--cpu-grids", type=int, default=1 << 20)
    ap.add_argument("--cpu-puzzles", type=int, default=1 << 16)
    ap.add_argument("--parity", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=synth.DEFAULT_SEED + 3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    res = {"tool": "bench_generate", "seed": a.seed, "warmup": a.warmup, "repeats": a.repeats, "sclk_before": sclk()}
    ng, npz, k = a.grids, a.puzzles, a.parity
    rows = max(ng, npz, k)
    with SudokuEngine(0) as eng:
        d_grids, d_order, d_puz = eng.alloc(rows * 81), eng.alloc(rows * 81), eng.alloc(rows * 81)
        d_plc, d_st = eng.alloc(rows * 4), eng.alloc(rows)
        # parity first: a wrong generator's rate means nothing
        rg, ro, rp = synth.grid_orders(np.arange(k), seed=a.seed, threads=16)
        rpuz, _ = synth.make_minimal(k, seed=a.seed, threads=16)
        eng.generate_grids_dev(d_grids, k, seed=a.seed, d_order=d_order, d_placements=d_plc)
        eng.synchronize()
        ok = bool((d_grids.download(np.empty((k, 81), dtype=np.uint8)) == rg).all()
                  and (d_order.download(np.empty((k, 81), dtype=np.uint8)) == ro).all()
                  and (d_plc.download(np.empty(k, dtype=np.uint32)) == rp).all())
        eng.generate_batch_dev(d_puz, d_grids, d_st, k, seed=a.seed)
        eng.synchronize()
        ok = ok and bool((d_puz.download(np.empty((k, 81), dtype=np.uint8)) == rpuz).all()
                         and (d_grids.download(np.empty((k, 81), dtype=np.uint8)) == rg).all()
                         and (d_st.download(np.empty(k, dtype=np.int8)) == 1).all())
        res["parity"] = {"rows": k, "ok": ok}
        res["gpu_grids_orders_counts"] = gpu_leg(
            eng, ng, lambda: eng.generate_grids_dev(d_grids, ng, seed=a.seed, d_order=d_order, d_placements=d_plc),
            a.warmup, a.repeats)
        res["gpu_grids"] = gpu_leg(eng, ng, lambda: eng.generate_grids_dev(d_grids, ng, seed=a.seed), a.warmup, a.repeats)
        plc = d_plc.download(np.empty(ng, dtype=np.uint32))
        res["placements"] = {"mean": round(float(plc.mean()), 1), "max": int(plc.max())}
        print("grids", json.dumps(res["gpu_grids_orders_counts"]), file=sys.stderr, flush=True)
        res["gpu_puzzles"] = gpu_leg(eng, npz, lambda: eng.generate_batch_dev(d_puz, d_grids, d_st, npz, seed=a.seed),
                                     a.warmup, a.repeats)
        print("puzzles", json.dumps(res["gpu_puzzles"]), file=sys.stderr, flush=True)
        for b in (d_grids, d_order, d_puz, d_plc, d_st):
            b.free()
    if a.cpu_grids:
        idx = np.arange(a.cpu_grids, dtype=np.uint64)
        res["cpu_grids"] = cpu_leg(a.cpu_grids, lambda: synth.minimal_grids(idx, seed=a.seed, threads=16))
    if a.cpu_puzzles:
        res["cpu_puzzles"] = cpu_leg(a.cpu_puzzles, lambda: synth.make_minimal(a.cpu_puzzles, seed=a.seed, threads=16))
    res["sclk_after"] = sclk()
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
