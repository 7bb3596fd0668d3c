#!/bin/bash
# One GPU call: full bench line (+ its details file), the other configurations, then the GPU test suite.  Outputs under OUTDIR.
#     tools/gpu_round_check.sh TAG OUTDIR
tag=${1:-x}
out=${2:?usage: tools/gpu_round_check.sh TAG OUTDIR}
mkdir -p "$out"
python bench.py --full --steps 20 --warmup 5 --details $out/bench_${tag}_details.json > $out/bench_$tag.json 2> $out/bench_$tag.err
rm -f $out/bench_${tag}_other.jsonl
for c in cfg3 cfg4 cfg5; do python bench.py --full --config $c --no-cpu --details $out/bench_${tag}_${c}_details.json 2>/dev/null | tail -1 >> $out/bench_${tag}_other.jsonl; done
python bench.py --full --layout yz4 --no-cpu --no-modes --no-retries --details $out/bench_${tag}_yz4_details.json 2>/dev/null | tail -1 >> $out/bench_${tag}_other.jsonl
python - <<PY
import json
s = open("$out/bench_$tag.json").read().strip().splitlines()[-1]
d = json.loads(s)
print("line bytes", len(s), "value", d["value"], {k: (round(v["value"]), v.get("finals_within_1e_4")) for k, v in d.get("modes", {}).items()})
print("single", d.get("single_batch_traj_per_s"), "roofline", d["roofline"]["frac"], d["roofline"].get("frac_aggregate"), "cpu", d.get("cpu_baseline", {}).get("value"))
print("esdf", d["esdf_kernel"]["frac"], d["esdf_kernel"].get("whole_step_launch", {}).get("frac_8d2"), "build ms", d.get("esdf_build", {}).get("ms"), "cfg1", d.get("cfg1"))
for l in open("$out/bench_${tag}_other.jsonl"):
    d = json.loads(l); print(d["config"]["workload"][:70], d["config"].get("layout"), round(d["value"]), d["ms_per_step"], "esdf", (d.get("esdf_kernel") or {}).get("frac"))
PY
python -m pytest tests -m gpu -x -q 2>&1 | tail -3
