#!/bin/bash
# round-3 evidence batch (GPU box): bench lines + rocprofv3 trace / PMC summaries of every kernel family that is quoted
cd ${GRAFT_REPO_ROOT:-/root/repo}
O=gpurun_out/r03; mkdir -p $O
run() { name=$1; shift; python bench.py --full "$@" 2>/dev/null | grep '^{' > $O/bench_$name.json; python - <<PY
import json
d=json.loads(open("$O/bench_$name.json").read())
print("$name", d["value"], d["roofline_encode"]["avg_launch_ms"], d["roofline_encode"]["frac"], d["roofline_decode"]["avg_launch_ms"], d["roofline_decode"]["frac"], d["dense_output"]["compact_ms"])
PY
}
run headline
run gather --gather --no-cpu-baseline
run uniform --table uniform --no-cpu-baseline
run config2_64Ki --chunks 65536 --no-cpu-baseline
run 192Ki --chunks 196608 --no-cpu-baseline
run tans_markov1 --coder tans --source markov1 --no-cpu-baseline
run range_markov1 --coder range --source markov1 --no-cpu-baseline
run aec_k256_64Ki --coder aec --aec-K 256 --chunks 65536 --steps 3 --warmup 1 --no-cpu-baseline
run aec_k256_256Ki --coder aec --aec-K 256 --chunks 262144 --steps 2 --warmup 1 --no-cpu-baseline
for spec in "rans_headline:" "rans_markov1:--source markov1" "tans:--coder tans" "range_uniform1:--coder range --table uniform1" \
            "range_t256:--coder range --table t256" "rans_b8:--num-bits-out 8 --range-factor 256" "aec_k16:--coder aec" \
            "aec_static:--coder aec --aec-model fixed" "aec_iid:--coder aec --aec-model iid --chunks 65536"; do
  BENCH_ARGS="${spec#*:}" bash tools/prof_bench.sh ${spec%%:*} > /dev/null 2>&1
  python - <<PY
import json
d=json.loads(open("gpurun_out/prof_${spec%%:*}/bench.json").read())
print("${spec%%:*}", d["value"], d["roofline_encode"]["avg_launch_ms"], d["roofline_encode"]["frac"], d["roofline_decode"]["avg_launch_ms"], d["roofline_decode"]["frac"])
PY
done
