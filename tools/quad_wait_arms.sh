#!/bin/bash
# Hold at pop (rt_traverse.hpp quad_hold) against the same tree built without it, alternating on one GPU:
#   qw0  -DRT_TRACE_QUAD_WAIT=0   no instantiation holds: the parent's kernels
#   qw1  -DRT_TRACE_QUAD_WAIT=1   the 64-VGPR instantiations (render types 0 - 2) of cache-resident scenes hold
#   qw2  -DRT_TRACE_QUAD_WAIT=2   the shaded instantiations as well (measure with tools/shade_bench.py)
# ARMS="qw0 qw2" bash tools/quad_wait_arms.sh run ...   picks the arms of a run (default: qw0 qw1)
# Build the arms first (where hipcc is):   bash tools/quad_wait_arms.sh build
# Run (on the GPU, from the repo root):    bash tools/quad_wait_arms.sh run <out dir> <runs> [bench.py arguments]
#   every run is bench.py's own line: `value` with the frames in flight it was asked for, serial_mrays beside it
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
C=gpu-raytracing_amd/csrc
ARMS=(${ARMS:-qw0 qw1})
if [ "$1" = build ]; then
  for a in qw0 qw1 qw2; do
    make -s -j8 -C $C librt_amd_exp.so EXPFLAGS="-DRT_TRACE_QUAD_WAIT=${a#qw}" EXPNAME=librt_amd_exp_$a.so || exit 1
  done
elif [ "$1" = run ]; then
  O=$2; N=$3; shift 3; mkdir -p $O
  for r in $(seq 1 $N); do
    for a in "${ARMS[@]}"; do
      export RT_LIB=$C/librt_amd_exp_$a.so
      timeout -k 10 400 python3 tools/trace_exp.py --gpus 1 --no-extras --no-cpu-baseline "$@" > $O/${a}_r$r.json 2> $O/${a}_r$r.err || { tail -5 $O/${a}_r$r.err; exit 1; }
      python3 -c "import json; d=json.loads(open('$O/${a}_r$r.json').read().strip().splitlines()[-1]); print('$a run $r [$*]:', d['value'], d['unit'], 'serial', d.get('serial_mrays'))" | tee -a $O/summary.txt
    done
  done
else
  echo "usage: quad_wait_arms.sh build | run <out dir> <runs> [bench.py arguments]"; exit 2
fi
