#!/bin/bash
# The whole GPU suite, then the full benchmark (bench.py --full) on the GPU box: bash tools/run_full_check.sh OUTDIR
out=${1:?usage: tools/run_full_check.sh OUTDIR}
cd "$(dirname "$0")/.." && mkdir -p "$out" || exit 1
timeout -k 10 900 python -m pytest tests -x -q -m gpu > "$out/t_all.txt" 2>&1 || { tail -30 "$out/t_all.txt"; exit 1; }
timeout -k 10 600 python bench.py --full > "$out/bench_full.json" 2> "$out/bench_full.err" || { tail -20 "$out/bench_full.err"; exit 1; }
tail -c 3000 "$out/bench_full.json"
