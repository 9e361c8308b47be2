#!/bin/bash
# Sweep of the matrix-free plan geometry at block size 3 (cells per block, workgroup size), as tools/mf_sweep.sh does for
# Poisson: one child of tools/ab_mf_elasticity.py per setting, one line per setting into LOG.  A child that fails ends the sweep.
cd "$(dirname "$0")/../.."
out=${1:-mf_el_sweep.log} # usage: tools/mf_el_sweep.sh [LOG]
: > $out
for cfg in "el_p1_c4 512 128" "el_p1_c4 512 256" "el_p1_c4 1024 128" "el_p1_c4 1024 256" "el_p1_c4 1024 512" "el_p1_c4 2048 256" \
           "el_p2_2m 256 128" "el_p2_2m 256 256" "el_p2_2m 512 128" "el_p2_2m 512 256" "el_p2_2m 512 512" "el_p2_2m 1024 256" \
           "el_p3_1m 128 128" "el_p3_1m 256 128" "el_p3_1m 256 256" "el_p3_1m 512 256"; do
  set -- $cfg
  line=$(ZZZ_MF_NC=$2 ZZZ_MF_T=$3 timeout -k 10 120 python performance-test_amd/tools/ab_mf_elasticity.py --child matfree --config $1 2>&1 | tail -1) || { echo "$cfg: FAILED: $line" >> $out; cat $out; exit 1; }
  echo "$line" | python -c "
import sys, json
d = json.loads(sys.stdin.read())
print('$cfg', 'nc', d['cells_per_block'], 'T', d['threads'], 'nloc_max', d['nloc_max'], 'shared', d['shared_nodes'], 'plan_ms %.1f' % d['plan_ms'], 'action_ms %.4f' % d['action_ms'], 'GB/s %.0f' % (d['bytes_per_action'] / d['action_ms'] / 1e6), 'Gdof/s %.3f' % d['Gdof_per_s'], 'jacobi_ms/it %.4f' % d['jacobi_ms_per_iteration'])
" >> $out || { echo "$cfg: no record: $line" >> $out; cat $out; exit 1; }
done
cat $out
