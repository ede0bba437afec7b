#!/bin/bash
# The lean vote (rt_traverse.hpp kLeanMargin) and the pair-local step of the hold-at-pop traversal, alternating on one GPU:
#   lean0  -DRT_TRACE_LEAN_STEP=0                        every vote runs the full push / pop ladders
#   site   -DRT_TRACE_LEAN_STEP=2                        every push / pop site branches on the vote's wave-uniform flag (shipped)
#   pair0 / pair  -DRT_TRACE_PAIR_STEP=0|1               every vote runs the general box step / narrow votes run the pair-local one
#   exact         -DRT_TRACE_PAIR_STEP=2                 exact votes run the pair-local step on a 32-bit pair offset (shipped)
# (The arms lean, sel, hv, leanr, siter, pad8 and pad16 of profiles/lean_step_bench.txt were retired with their knobs: DESIGN section 5.)
# A library built elsewhere (the parent commit's) joins as arm NAME when copied to csrc/librt_amd_exp_NAME.so.
# Build the arms first (where hipcc is):   bash tools/lean_step_arms.sh build
# Run (on the GPU, from the repo root):    ARMS="lean0 site pair0" bash tools/lean_step_arms.sh run <out dir> <runs> [bench.py arguments]
#   every run is bench.py's own line; the last line of a run block is min - max per arm
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
C=gpu-raytracing_amd/csrc
ARMS=(${ARMS:-lean0 site})
flags() {
  case $1 in
    lean0) echo "-DRT_TRACE_LEAN_STEP=0";; site) echo "-DRT_TRACE_LEAN_STEP=2";;
    pair0) echo "-DRT_TRACE_PAIR_STEP=0";; pair) echo "-DRT_TRACE_PAIR_STEP=1";; exact) echo "-DRT_TRACE_PAIR_STEP=2";;
    *) return 1;;
  esac
}
if [ "$1" = build ]; then
  shift
  for a in ${@:-lean0 site pair0 pair exact}; do
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
