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
#
# PER_KERNEL="a.hip ..." compares the named files kernel by kernel instead of as a whole, for a change that ADDS kernels to a
# file and must leave the old ones alone: every kernel of <rev>'s file is looked up in this tree's and its text -- from its
# label to its .Lfunc_end label, which takes in the .amdhsa_kernel block with its register counts -- is compared, one line per
# kernel.  The kernel's own symbol and the per-function number of the local labels (.LBB<n>_, .Lfunc_end<n>: a kernel's
# position in the file, also where trailing comments name a block as BB<n>_) are the only things made equal first.  RENAME='<sed expression>' turns a kernel symbol of <rev> into
# this tree's where a template parameter was added.  A kernel <rev> does not have is reported as new and is no failure.
#   PER_KERNEL=instance_mixed_query.hip RENAME='s/ELb\([01]\)EEEvNSt/ELb\1ELb0EEEvNSt/' tools/device_asm_diff.sh HEAD
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

# kernel_text <file.s> <symbol>: the kernel from its label to its end label, its own name and label numbers made neutral
kernel_text() {
    awk -v s="$2:" 'index($0, s) == 1 { on = 1 } on { print } on && /^\.Lfunc_end[0-9]+:/ { exit }' "$1" |
        sed -e "s/$2/KERNEL/g" -e 's/\([^A-Za-z0-9_]L\{0,1\}\)BB[0-9]*_/\1BB_/g' -e 's/\.Lfunc_end[0-9]*/.Lfunc_end/g'
}
# per_kernel <file> <head.s> <rev.s>: one line per kernel of either side
per_kernel() {
    local f=$1 a=$2 b=$3 k h n
    for k in $(sed -n 's/^[[:space:]]*\.amdhsa_kernel[[:space:]]*//p' "$b"); do
        h=$(printf '%s\n' "$k" | sed -e "${RENAME:-s/^//}")
        n=$(kernel_text "$b" "$k" | wc -l)
        if ! grep -q "^$h:" "$a"; then echo "$f kernel $k: MISSING in this tree (looked for $h)"; bad=1
        elif [ "$n" -gt 2 ] && cmp -s <(kernel_text "$a" "$h") <(kernel_text "$b" "$k"); then
            echo "$f kernel $k: $n lines, identical$([ "$h" != "$k" ] && echo " (here $h)")"
        else echo "$f kernel $k: DIFFERS ($(diff <(kernel_text "$a" "$h") <(kernel_text "$b" "$k") | grep -c '^[<>]') lines of diff)"; bad=1
        fi
    done
    for h in $(sed -n 's/^[[:space:]]*\.amdhsa_kernel[[:space:]]*//p' "$a"); do
        for k in $(sed -n 's/^[[:space:]]*\.amdhsa_kernel[[:space:]]*//p' "$b"); do
            [ "$(printf '%s\n' "$k" | sed -e "${RENAME:-s/^//}")" = "$h" ] && continue 2
        done
        echo "$f kernel $h: $(kernel_text "$a" "$h" | wc -l) lines, new in this tree"
    done
}

echo "# tools/device_asm_diff.sh $rev: the device assembly of this tree against $rev's, per file and arm"
bad=0
for c in "${cases[@]}"; do
    IFS="|" read -r name def f <<< "$c"
    a=$tmp/head/$name.$f.s b=$tmp/rev/$name.$f.s
    if [ -s "$a" ] && [ -s "$b" ] && [[ " ${PER_KERNEL:-} " == *" $f "* ]]; then per_kernel "$f $name" "$a" "$b"
    elif [ -s "$a" ] && [ ! -e "$tmp/other/$csrc/$f" ]; then echo "$f $name: $(wc -l < "$a") lines, new in this tree ($rev has no such file)"
    elif [ ! -s "$a" ] || [ ! -s "$b" ]; then echo "$f $name: FAILED TO COMPILE"; cat "$tmp/head/$name.$f.err" "$tmp/rev/$name.$f.err" >&2; bad=1
    elif cmp -s "$a" "$b"; then echo "$f $name: $(wc -l < "$a") lines, identical"
    else echo "$f $name: $(wc -l < "$a") / $(wc -l < "$b") lines, DIFFERS ($(diff "$a" "$b" | grep -c '^[<>]') lines of diff)"; bad=1
    fi
done
exit $bad
