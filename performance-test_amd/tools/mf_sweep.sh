#!/bin/bash
# Sweep of the matrix-free plan geometry (cells per block, workgroup size): tools/mf_bench.py per setting.
cd "$(dirname "$0")/../.."
out=gpurun_out/mf_sweep.log
mkdir -p gpurun_out
: > $out
for cfg in "p1 4096 512" "p1 2048 256" "p1 4096 256" "p1 1024 256" "p1 2048 128" "p1 3072 256" \
           "p3 512 256" "p3 1024 256" "p3 768 256" "p3 256 256" "p3 1024 512" "p3 512 128" "p2 1024 256" "p2 2048 256" "p2 1024 512"; do
  set -- $cfg
  ZZZ_MF_NC=$2 ZZZ_MF_T=$3 python performance-test_amd/tools/mf_bench.py $1 2>&1 | tail -1 | python -c "
import sys, json
d = json.loads(sys.stdin.read())
p = d.get('plan', {})
print('$cfg', 'nc', p.get('cells_per_block'), 'nloc_max', p.get('nloc_max'), 'shared', p.get('shared_dofs'), 'setup_ms %.1f' % d['setup_warm_ms'], 'action_ms %.4f' % d['action_ms'], 'GB/s %.0f' % d.get('action_GBs', 0), 'Gdof/s %.2f' % d['Gdofs'], 'cg_s %.4f' % d['cg_s'])
" >> $out
done
cat $out
