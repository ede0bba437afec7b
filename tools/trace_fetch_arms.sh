#!/bin/bash
# The fetch arms of the tracer's hot loop against the shipped library, alternating on one GPU:
#   RT_TRACE_UNIFORM_MAX=0|1|2|4 (wave-shared pairs through the scalar path), RT_TRACE_UNIFORM_STICKY=0|1 (look at every step /
#   until the lanes first part), RT_TRACE_LEAF_WIDE=0|1 (leaf fetch as the compiler narrows it / four 16-byte requests),
#   RT_TRACE_TILE_2X2=1 (a workgroup's tiles as 2 x 2), RT_TRACE_PAIR_BARRIER=1 (scheduling barrier behind a pair's four loads).
# Build the arms first (where hipcc is):   bash tools/trace_fetch_arms.sh build
# Run (on the GPU, from the repo root):    bash tools/trace_fetch_arms.sh run <out dir> [bench.py arguments]
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
C=gpu-raytracing_amd/csrc
ARMS=("u0l0|-DRT_TRACE_UNIFORM_MAX=0 -DRT_TRACE_LEAF_WIDE=0" "u0l1|-DRT_TRACE_UNIFORM_MAX=0"
      "u1l0|-DRT_TRACE_UNIFORM_MAX=1 -DRT_TRACE_UNIFORM_STICKY=0 -DRT_TRACE_LEAF_WIDE=0" "u1l1|-DRT_TRACE_UNIFORM_MAX=1 -DRT_TRACE_UNIFORM_STICKY=0"
      "u2l1|-DRT_TRACE_UNIFORM_MAX=2 -DRT_TRACE_UNIFORM_STICKY=0" "u4l1|-DRT_TRACE_UNIFORM_MAX=4 -DRT_TRACE_UNIFORM_STICKY=0"
      "s1l1|-DRT_TRACE_UNIFORM_MAX=1" "s2l1|-DRT_TRACE_UNIFORM_MAX=2" "s4l1|-DRT_TRACE_UNIFORM_MAX=4"
      "tile2x2|-DRT_TRACE_TILE_2X2=1" "pairbarrier|-DRT_TRACE_PAIR_BARRIER=1")
if [ "$1" = build ]; then
  for a in "${ARMS[@]}"; do
    make -s -C $C librt_amd_exp.so EXPFLAGS="${a#*|}" EXPNAME=librt_amd_exp_${a%%|*}.so || exit 1
  done
elif [ "$1" = run ]; then
  O=$2; shift 2; mkdir -p $O
  for r in 1 2; do
    for a in base "${ARMS[@]}"; do
      a=${a%%|*}
      if [ $a = base ]; then unset RT_LIB; else export RT_LIB=$C/librt_amd_exp_$a.so; fi
      timeout -k 10 300 python3 tools/trace_exp.py --steps 50 --full --no-extras --no-cpu-baseline "$@" > $O/${a}_r$r.json 2> $O/${a}_r$r.err || { tail -5 $O/${a}_r$r.err; exit 1; }
      python3 -c "import json; d=json.loads(open('$O/${a}_r$r.json').read().strip().splitlines()[-1]); print('$a run $r: in flight', d['value'], 'serial', d.get('serial_mrays'))" | tee -a $O/summary.txt
    done
  done
else
  echo "usage: trace_fetch_arms.sh build | run <out dir> [bench.py arguments]"; exit 2
fi
