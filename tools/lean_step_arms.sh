#!/bin/bash
# The lean vote of the hold-at-pop traversal (rt_traverse.hpp kLeanMargin) and its trims, alternating on one GPU:
#   lean0  -DRT_TRACE_LEAN_STEP=0                        every vote runs the full push / pop ladders: the parent's loop
#   lean   -DRT_TRACE_LEAN_STEP=1                        two loops: a vote with every lane outside the margin runs the LDS-only arm
#   site   -DRT_TRACE_LEAN_STEP=2                        one loop; every push / pop site branches on the vote's wave-uniform flag
#   sel    -DRT_TRACE_LEAN_SELECT=1                      lean + advance() as selects
#   hv     -DRT_TRACE_HOLD_VECTOR=1                      lean + quad_hold's combine in vector operations
#   leanr / siter  -DRT_TRACE_QUAD_WAIT_SECOND=1         lean / site + the hold rule before both steps of a vote
#   pad8 / pad16  -DRT_TRACE_LEAN_STEP=0 -DRT_EXP_BOX_PAD=8|16   the parent's loop with N more vector instructions per box step
#   pair0 / pair  -DRT_TRACE_PAIR_STEP=0|1                     every vote runs the general box step / narrow votes run the pair-local one (shipped)
# A library built elsewhere (the parent commit's) joins as arm NAME when copied to csrc/librt_amd_exp_NAME.so.
# Build the arms first (where hipcc is):   bash tools/lean_step_arms.sh build
# Run (on the GPU, from the repo root):    ARMS="lean0 lean sel" bash tools/lean_step_arms.sh run <out dir> <runs> [bench.py arguments]
#   every run is bench.py's own line; the last line of a run block is min - max per arm
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
C=gpu-raytracing_amd/csrc
ARMS=(${ARMS:-lean0 lean})
flags() {
  case $1 in
    lean0) echo "-DRT_TRACE_LEAN_STEP=0";; lean) echo "-DRT_TRACE_LEAN_STEP=1";; site) echo "-DRT_TRACE_LEAN_STEP=2";; sel) echo "-DRT_TRACE_LEAN_STEP=1 -DRT_TRACE_LEAN_SELECT=1";;
    hv) echo "-DRT_TRACE_LEAN_STEP=1 -DRT_TRACE_HOLD_VECTOR=1";; leanr) echo "-DRT_TRACE_LEAN_STEP=1 -DRT_TRACE_QUAD_WAIT_SECOND=1";;
    siter) echo "-DRT_TRACE_LEAN_STEP=2 -DRT_TRACE_QUAD_WAIT_SECOND=1";;
    pair0) echo "-DRT_TRACE_PAIR_STEP=0";; pair) echo "-DRT_TRACE_PAIR_STEP=1";;
    pad8) echo "-DRT_TRACE_LEAN_STEP=0 -DRT_EXP_BOX_PAD=8";; pad16) echo "-DRT_TRACE_LEAN_STEP=0 -DRT_EXP_BOX_PAD=16";;
    *) return 1;;
  esac
}
if [ "$1" = build ]; then
  shift
  for a in ${@:-lean0 lean site sel hv leanr siter pad8 pad16}; do
    f=$(flags $a) || { echo "unknown arm $a"; exit 2; }
    make -s -j8 -C $C librt_amd_exp.so EXPFLAGS="$f" EXPNAME=librt_amd_exp_$a.so || exit 1
  done
elif [ "$1" = run ]; then
  O=$2; N=$3; shift 3; mkdir -p $O
  for r in $(seq 1 $N); do
    for a in "${ARMS[@]}"; do
      export RT_LIB=$C/librt_amd_exp_$a.so
      timeout -k 10 400 python3 tools/trace_exp.py --gpus 1 --no-extras --no-cpu-baseline "$@" > $O/${a}_r$r.json 2> $O/${a}_r$r.err || { tail -5 $O/${a}_r$r.err; exit 1; }
      python3 -c "import json; d=json.loads(open('$O/${a}_r$r.json').read().strip().splitlines()[-1]); print('$a run $r [$*]:', d['value'], d['unit'])" | tee -a $O/summary.txt
    done
  done
  python3 - "$O" "$N" "$*" "${ARMS[@]}" <<'EOF' | tee -a $O/summary.txt
import json, sys
o, n, what, arms = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4:]
v = {a: [json.loads(open(f"{o}/{a}_r{r}.json").read().strip().splitlines()[-1])["value"] for r in range(1, n + 1)] for a in arms}
print(f"[{what}] " + "   ".join(f"{a} {min(v[a]):.1f} - {max(v[a]):.1f}" for a in arms))
EOF
else
  echo "usage: lean_step_arms.sh build [arms] | run <out dir> <runs> [bench.py arguments]"; exit 2
fi
