#!/bin/bash
# Rasterizer-only bench of the in-tree libgsr.so once per value of an environment variable.
# usage: bash tools/sweep_env.sh VAR v1 v2 ...
set -u
var=$1; shift
log=$(mktemp)
for v in "$@"; do
  env $var=$v timeout -k 10 200 python -u bench.py --full --no-cpu-baseline --loss-steps 0 --densify-steps 0 --call-site-steps 0 --io-timesteps 0 > "$log" 2>&1 || { echo "run $v failed"; tail -3 "$log"; exit 1; }
  grep '^{' "$log" | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); p=d['phase_ms_per_launch']; print('$var=$v', d['value'], d['ms_per_step'], ' '.join(f'{k}={v*1e3:.1f}' for k,v in p.items()))"
done
rm -f "$log"
