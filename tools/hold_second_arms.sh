#!/bin/bash
# Hold by stack depth alone (rt_traverse.hpp quad_hold_sp) against the parent's loop, alternating on one GPU:
#   parent  -DRT_TRACE_HOLD_SECOND=0 -DRT_TRACE_HOLD_FIRST=0   the loop before the knobs, instruction for instruction
#   second  -DRT_TRACE_HOLD_SECOND=1                           the second step of a vote leaves out the lanes quad_hold_sp holds
#   first   -DRT_TRACE_HOLD_FIRST=1                            the first step's hold test is quad_hold_sp (no LDS read)
#   both    -DRT_TRACE_HOLD_SECOND=1 -DRT_TRACE_HOLD_FIRST=1
# Build the arms first (where hipcc is):   bash tools/hold_second_arms.sh build [arms]
# Run (on the GPU, from the repo root):    ARMS="parent second" bash tools/hold_second_arms.sh run <out dir> <runs> [bench.py arguments]
#   every run is bench.py's own line; the first alternation also dumps its outputs (--dump-outputs) and every arm's are compared
#   with the first arm's: the frame byte for byte, the counters one by one (0 / 1, the test counts, must be equal; 2 / 3, the
#   wave steps, are printed).  The last line of a run block is min - max per arm and the gain rule's verdict against the first arm.
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
C=gpu-raytracing_amd/csrc
ARMS=(${ARMS:-parent second first both})
flags() {
  case $1 in
    parent) echo "-DRT_TRACE_HOLD_SECOND=0 -DRT_TRACE_HOLD_FIRST=0";; second) echo "-DRT_TRACE_HOLD_SECOND=1 -DRT_TRACE_HOLD_FIRST=0";;
    first) echo "-DRT_TRACE_HOLD_SECOND=0 -DRT_TRACE_HOLD_FIRST=1";; both) echo "-DRT_TRACE_HOLD_SECOND=1 -DRT_TRACE_HOLD_FIRST=1";;
    *) return 1;;
  esac
}
if [ "$1" = build ]; then
  shift
  for a in ${@:-parent second first both}; do
    f=$(flags $a) || { echo "unknown arm $a"; exit 2; }
    make -s -j8 -C $C librt_amd_exp.so EXPFLAGS="$f" EXPNAME=librt_amd_exp_$a.so || exit 1
  done
elif [ "$1" = run ]; then
  O=$2; N=$3; shift 3; mkdir -p $O
  for r in $(seq 1 $N); do
    for a in "${ARMS[@]}"; do
      export RT_LIB=$C/librt_amd_exp_$a.so
      dump=(); [ $r = 1 ] && dump=(--dump-outputs $O/dump_$a)
      timeout -k 10 400 python3 tools/trace_exp.py --gpus 1 --no-extras --no-cpu-baseline "$@" "${dump[@]}" > $O/${a}_r$r.json 2> $O/${a}_r$r.err || { tail -5 $O/${a}_r$r.err; exit 1; }
      python3 -c "import json; d=json.loads(open('$O/${a}_r$r.json').read().strip().splitlines()[-1]); print('$a run $r [$*]:', d['value'], d['unit'])" | tee -a $O/summary.txt
    done
  done
  python3 - "$O" "$N" "$*" "${ARMS[@]}" <<'EOF' | tee -a $O/summary.txt
import glob, json, os, sys
import numpy as np
o, n, what, arms = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4:]
v = {a: [json.loads(open(f"{o}/{a}_r{r}.json").read().strip().splitlines()[-1])["value"] for r in range(1, n + 1)] for a in arms}
p = v[arms[0]]
spread = max(p) - min(p)
def verdict(x):
    if min(x) - max(p) > spread: return f"GAIN ({(sum(x) / len(x) / (sum(p) / len(p)) - 1) * 100:+.1f} %)"
    if min(p) - max(x) > max(x) - min(x): return f"LOSS ({(sum(x) / len(x) / (sum(p) / len(p)) - 1) * 100:+.1f} %)"
    return f"no gain, no loss ({(sum(x) / len(x) / (sum(p) / len(p)) - 1) * 100:+.1f} %)"
print(f"[{what}] " + "   ".join(f"{a} {min(v[a]):.1f} - {max(v[a]):.1f}" + ("" if a == arms[0] else " " + verdict(v[a])) for a in arms))
for a in arms:
    bad = []
    for f in sorted(glob.glob(f"{o}/dump_{arms[0]}/*.npy")):
        x, y = np.load(f), np.load(f"{o}/dump_{a}/{os.path.basename(f)}")
        if os.path.basename(f) == "counters.npy":
            if not np.array_equal(x.ravel()[:2], y.ravel()[:2]): bad.append("counters 0 / 1")
            print(f"[{what}] {a} counters {[int(c) for c in y.ravel()]}")
        elif x.tobytes() != y.tobytes(): bad.append(os.path.basename(f))
    print(f"[{what}] {a} outputs against {arms[0]}: " + ("identical" if not bad else "DIFFER in " + ", ".join(bad)))
EOF
  for a in "${ARMS[@]}"; do [ -d "$O/dump_$a" ] && rm -r "$O/dump_$a"; done   # (a 1080p frame is 33 MB: compared, not kept)
else
  echo "usage: hold_second_arms.sh build [arms] | run <out dir> <runs> [bench.py arguments]"; exit 2
fi
