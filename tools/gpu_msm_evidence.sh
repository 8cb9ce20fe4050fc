#!/bin/bash
# the multiscalar profiles (kernel trace, traffic, counters per kernel: collect_msm_profiles.sh) and the bench line of the tree
bash tools/collect_msm_profiles.sh ${1:-r06v} 2>&1 | grep -v "^W2026\|amdgpu.ids" | tail -40
D=${BENCH_OUT:-bench_out}/${1:-r06v}_bench; mkdir -p $D
timeout 900 python bench.py --full > $D/bench.json 2> $D/bench.err
echo "bench rc=$? bytes=$(wc -c < $D/bench.json)"
