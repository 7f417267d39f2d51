"""Table of tools/ab_bench.sh runs: per build the figures of every run, their mean and range, and for
each later build against the first the two tests of a speed-up -- every run below every run of the
first, and the difference of means against the larger same-build range.
usage: python3 tools/ab_bench_summary.py <outdir> <name> [<name> ...]"""
import json
import os
import sys

FIGS = (
    ("c4_kernel_ms", lambda r: r["single_stream"]["avg_kernel_ms"]),
    ("ms_per_step", lambda r: r["ms_per_step"]),
    ("c2_kernel_ms", lambda r: r["c2_30clue"]["avg_kernel_ms"]),
    ("minimal_kernel_ms", lambda r: r["minimal_puzzles"]["avg_kernel_ms"]),
    ("hard_1m_ms", lambda r: r["hard_search"]["hard_1m"]["one_launch"]["ms"]),
)


def figure(rec, get):
    try:
        return float(get(rec))
    except (KeyError, TypeError):
        return None


out, names = sys.argv[1], sys.argv[2:]
runs = {}
for n in names:
    with open(os.path.join(out, n + ".jsonl")) as f:
        runs[n] = [json.loads(line) for line in f if line.startswith("{")]
table = {}
for n in names:
    print(n)
    for fig, get in FIGS:
        v = [figure(r, get) for r in runs[n]]
        if not v or any(x is None for x in v):
            continue
        table[(n, fig)] = v
        mean = sum(v) / len(v)
        print(f"   {fig:18s} " + " ".join(f"{x:.4f}" for x in v) +
              f"   mean {mean:.4f} min {min(v):.4f} max {max(v):.4f} range {max(v) - min(v):.4f}")
base = names[0]
for n in names[1:]:
    print(f"{n} against {base}")
    for fig, _ in FIGS:
        a, b = table.get((base, fig)), table.get((n, fig))
        if not a or not b:
            continue
        diff = sum(a) / len(a) - sum(b) / len(b)
        rng = max(max(a) - min(a), max(b) - min(b))
        print(f"   {fig:18s} mean difference {diff:+.4f} ms ({100 * diff / (sum(a) / len(a)):+.2f} %), "
              f"larger range {rng:.4f}, ratio {diff / rng if rng else float('inf'):.2f}, "
              f"every run below every run of {base}: {max(b) < min(a)}")
