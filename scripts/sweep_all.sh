#!/bin/bash
# Per-task 4096-env step / fused rollout and the large-N HBM roofline sweep (4 M, 16 M envs), one line per task.
# bash scripts/sweep_all.sh [DIR]: the bench lines are kept as DIR/sweep_<task>.json (a temporary folder by default).
set -u
O=${1:-$(mktemp -d)}
mkdir -p "$O"
echo "bench lines and side files: $O"
for t in ${TASKS:-LeeLanded EKFLeeLanded QuadTracking QuadFault QuadMixed}; do
  timeout -k 10 300 python bench.py --full --task $t --steps 2000 --warmup 100 --no-cpu-baseline --detail "$O/detail_$t.json" > "$O/sweep_$t.json" 2>/dev/null || exit 1
  python -c "import json;d=json.load(open('$O/detail_$t.json'));f=d.get('per_step_launch',{});print('$t', 'value %.4g k_us %.3f per-step %.4g'%(d['value'],d['roofline']['kernel_us'],f.get('value',0)), ' '.join('N=%d k_us %.1f frac %.3f'%(s['num_envs'],s['kernel_us'],s['frac']) for s in d.get('roofline_sweep',[])))"
done
