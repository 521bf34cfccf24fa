#!/bin/bash
# GPU box: does the PCF-shortcut build (profiles/patches/r06_pcf_uniform_shortcut.patch) stall at a lower occupancy target of the
# multisampled resolve as well?  Variants built by tools/variants.py; R3N_LIB picks the library.
for v in pcfocc4 occ4 pcf; do
  echo "=== variant $v"
  R3N_LIB=$PWD/variants/lib_$v.so bash tools/hunt_hang.sh r06p_$v 1 60 tests/test_gpu_parity.py -k "transparent_pass_multi_frame or msaa or multisample" 2>&1 | grep -v "wait hipStream\|wait done\|^  File\|^    " | tail -6 | cut -c1-200
done
echo "=== MSAA bench, occupancy target 4 against 5"
for v in base occ4; do
  R3N_LIB=$PWD/variants/lib_$v.so python bench.py --full --samples 4 --no-cpu-baseline --steps 30 --warmup 5 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$v', d['ms_per_step'], {k:round(v*1e3,1) for k,v in d['stage_ms_per_frame'].items() if v})"
done
