#!/bin/bash
# step-level numbers with the library variants under scratch/exp/ (phase-removal experiments: results WRONG by construction)
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
L=$ROOT/monocon-pytorch_amd/hipmonocon/libmonocon_hip.so
cp $L /tmp/lib_orig.so
for v in "$@"; do
  cp $ROOT/scratch/exp/lib_$v.so $L
  python $ROOT/bench.py --full --steps 6 --warmup 2 --forward-steps 0 --realistic-steps 0 --no-cpu-baseline --no-extra-modes 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read()); r=d['roofline']; print('$v', 'step', d['ms_per_step'], 'conv', r['conv_ms_per_step'], 'wgrad', r['wgrad']['ms_per_step'], 'other', r['other_ms_per_step'])"
done
cp /tmp/lib_orig.so $L
