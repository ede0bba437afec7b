#!/bin/bash
# device_asm_diff.sh <rev> -- is the device code of this tree the device code of <rev>, instruction for instruction and
# register for register?  The acceptance test of a refactor of the kernels: nothing runs, no GPU is needed.
#
# Every file of csrc/Makefile's SRCS is compiled on both sides with that side's own HIPFLAGS plus --offload-device-only -S;
# trace_kernel.hip and ray_query.hip once more per kept off-arm of the tracer's knobs and with -DRT_TRACE_TUNING.  Comment
# lines, .ident, .file and the __hip_cuid_* symbol (a hash of the source text) are dropped, the rest is compared with cmp.
# The other side is built in a `git worktree` under a temporary directory, removed on exit.  Prints one line per file and
# arm -- the line count and "identical" or "DIFFERS" -- and exits non-zero if anything differs or fails to compile.  A file
# of this tree's SRCS that <rev> does not have is reported as new and is no failure: there is nothing to compare it with.
#   JOBS=n tools/device_asm_diff.sh 30690cb > profiles/retired_arms_asm_diff.txt
set -uo pipefail
rev=${1:?usage: device_asm_diff.sh <rev>}
here=$(git -C "$(dirname "$0")" rev-parse --show-toplevel) || exit 2
csrc=gpu-raytracing_amd/csrc
tmp=$(mktemp -d)
trap 'git -C "$here" worktree remove --force "$tmp/other" 2>/dev/null; rm -rf "$tmp"' EXIT
git -C "$here" worktree add --quiet --detach "$tmp/other" "$rev" || exit 2

# (an arm of several defines is written with + between them; a define the other side does not know changes nothing there, so
# "both hold knobs off" is compared with <rev>'s own default where <rev> is older than the knobs)
ARMS="-DRT_TRACE_PAIR_STEP=0 -DRT_TRACE_PAIR_STEP=1 -DRT_TRACE_LEAN_STEP=0 -DRT_TRACE_QUAD_WAIT=0 -DRT_TRACE_QUAD_WAIT=2 -DRT_TRACE_TUNING -DRT_TRACE_HOLD_SECOND=0+-DRT_TRACE_HOLD_FIRST=0"
srcs=$(make -s --no-print-directory -C "$here/$csrc" --eval='_p: ; @echo $(SRCS)' _p)
cases=()
for f in $srcs; do cases+=("default||$f"); done
for f in trace_kernel.hip ray_query.hip; do
    for a in $ARMS; do cases+=("$a|${a//+/ }|$f"); done
done

# emit <tree> <outdir>: the filtered device assembly of every case, JOBS compilations at a time
emit() {
    local dir=$1/$csrc out=$2 hipcc flags
    hipcc=$(make -s --no-print-directory -C "$dir" --eval='_p: ; @echo $(HIPCC)' _p)
    flags=$(make -s --no-print-directory -C "$dir" --eval='_p: ; @echo $(HIPFLAGS)' _p)
    mkdir -p "$out"
    printf '%s\n' "${cases[@]}" | DIR=$dir OUT=$out HIPCC=$hipcc FLAGS=$flags xargs -P "${JOBS:-8}" -I{} bash -c '
        IFS="|" read -r name def f <<< "{}"
        cd "$DIR" && $HIPCC $FLAGS $def --offload-device-only -S "$f" -o - 2> "$OUT/$name.$f.err" |
            grep -v -e "^[[:space:]]*;" -e "\.ident" -e "\.file" -e "__hip_cuid_" > "$OUT/$name.$f.s"'
}
emit "$here" "$tmp/head"
emit "$tmp/other" "$tmp/rev"

echo "# tools/device_asm_diff.sh $rev: the device assembly of this tree against $rev's, per file and arm"
bad=0
for c in "${cases[@]}"; do
    IFS="|" read -r name def f <<< "$c"
    a=$tmp/head/$name.$f.s b=$tmp/rev/$name.$f.s
    if [ -s "$a" ] && [ ! -e "$tmp/other/$csrc/$f" ]; then echo "$f $name: $(wc -l < "$a") lines, new in this tree ($rev has no such file)"
    elif [ ! -s "$a" ] || [ ! -s "$b" ]; then echo "$f $name: FAILED TO COMPILE"; cat "$tmp/head/$name.$f.err" "$tmp/rev/$name.$f.err" >&2; bad=1
    elif cmp -s "$a" "$b"; then echo "$f $name: $(wc -l < "$a") lines, identical"
    else echo "$f $name: $(wc -l < "$a") / $(wc -l < "$b") lines, DIFFERS ($(diff "$a" "$b" | grep -c '^[<>]') lines of diff)"; bad=1
    fi
done
exit $bad
