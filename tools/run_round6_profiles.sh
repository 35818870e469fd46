#!/bin/bash
# Round 6: the whole profile set on ONE box, final tree (inside gpurun): GPU suite, forward PMC table + dominant conv + correlation + bench
# under rocprofv3 (prof_round.sh), wave states, launch list, dec23 issue counters, energy by stage, then bench.py --full.
#   bash tools/run_round6_profiles.sh OUTDIR
out=${1:?usage: tools/run_round6_profiles.sh OUTDIR}
cd "$(dirname "$0")/.."
mkdir -p "$out"
python -m pytest tests -m gpu -q > $out/gputests.txt 2>&1; tail -3 $out/gputests.txt
bash tools/prof_round.sh r06 > $out/prof_round.log 2>&1; tail -3 $out/prof_round.log
bash tools/prof_forward_sq.sh r06_sq > $out/sq.log 2>&1; echo "sq done"
bash tools/trace_forward_launches.sh r06_launches > $out/launches.log 2>&1; tail -1 $out/launches.log
bash tools/prof_dec23_sq.sh r06_d23sq > $out/d23sq.log 2>&1; echo "d23 counters done"
timeout -k 10 400 bash tools/energy_table.sh r06 4 > $out/energy.log 2>&1; tail -22 $out/energy.log
timeout -k 10 600 python tools/concurrency_check.py 6 > $out/concurrency.txt 2>&1; tail -1 $out/concurrency.txt
python bench.py --full > $out/bench.json 2> $out/bench.err; tail -c 300 $out/bench.err
python - "$out/bench.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print("bench:", d["value"], d["ms_per_step"], d["sustained"], d["config"]["single_stream_latency_ms"], d["roofline"]["launch_ms"], d["roofline"]["frac"], d["roofline"]["path"]["frac"])
PY
