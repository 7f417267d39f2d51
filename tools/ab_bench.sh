#!/bin/bash
# A/B of whole bench.py runs, alternating builds in one session on one box (dev tool).
#   usage: tools/ab_bench.sh <outdir> <rounds> <name> [<name> ...]
#   <name>: "tree" = the in-tree library, else build/variants/lib_<name>.so (tools/build_variant.sh,
#           tools/build_variant_commit.sh), selected through SDK_LIB_PATH
#   HARD=1: with the hard leg (hard_1m); the other side legs stay off
# Each run: bench.py --full --steps 20 --warmup 5 with the side legs off; its JSON line goes to
# <outdir>/<name>.jsonl.  Then: python3 tools/ab_bench_summary.py <outdir> <name> ...
set -o pipefail
out=$1; rounds=$2; shift 2
mkdir -p "$out"
ARGS="--full --steps 20 --warmup 5 --check-boards 0 --cpu-seconds 0 --http-requests 0 --hard-leg ${HARD:-0} --count-leg 0 --first-boards= --lane-puzzles 0 --frontier-probe 0"
for r in $(seq "$rounds"); do
  for v in "$@"; do
    if [ "$v" = tree ]; then unset SDK_LIB_PATH; else export SDK_LIB_PATH=$PWD/build/variants/lib_$v.so; fi
    timeout -k 10 ${RUN_TIMEOUT:-150} python3 bench.py $ARGS 2> "$out/$v.err" | tail -1 >> "$out/$v.jsonl" \
      || { echo "round $r: $v failed"; tail -5 "$out/$v.err"; exit 1; }
    echo "round $r $v done"
  done
done
python3 tools/ab_bench_summary.py "$out" "$@" | tee "$out/ab_summary.txt"
