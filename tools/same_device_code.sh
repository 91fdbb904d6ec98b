#!/usr/bin/env bash
# Is the gfx950 device code of this tree byte-identical to that of REF_TREE?  No GPU needed.
# Builds csrc/handarm_hip.hip of both trees with build.py's flags plus --save-temps (each in a temporary directory of
# its own, --save-temps writes into the working directory), extracts .text from each device code object and cmp's them.
# usage: tools/same_device_code.sh REF_TREE [extra hipcc flags...]
#   REF_TREE: a checkout of the commit to compare with (git worktree add DIR COMMIT, or git archive), never a copy of
#   this tree.  The extra flags go to both builds.  Exit status 0 = identical, 1 = different, 2 = a build failed.
set -u
HERE=$(cd "$(dirname "$0")/.." && pwd)
[ -d "${1:-}" ] || { echo "usage: $0 REF_TREE [extra hipcc flags...]" >&2; exit 2; }
REF=$(cd "$1" && pwd); shift
TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT
text_of() {   # text_of TREE NAME [flags...]: NAME.text = the .text section of TREE's device code object
    local tree=$1 name=$2; shift 2
    mkdir "$TMP/$name" && cd "$TMP/$name" &&
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -Wno-unused-result \
        --save-temps -I "$tree/include" "$@" -o lib.so "$tree/isaacgym-hand-arm_amd/csrc/handarm_hip.hip" > log 2>&1 &&
    /opt/rocm/llvm/bin/llvm-objcopy -O binary --only-section=.text ./*-gfx950.out "$TMP/$name.text"
}
text_of "$REF" ref "$@" & text_of "$HERE" new "$@"; new=$?; wait $!; ref=$?
if [ $ref -ne 0 ] || [ $new -ne 0 ]; then
    echo "BUILD FAILED (ref: $ref, this tree: $new)"
    grep -h -m 5 "error" "$TMP/ref/log" "$TMP/new/log"
    exit 2
fi
echo ".text bytes: ref $(stat -c %s "$TMP/ref.text"), this tree $(stat -c %s "$TMP/new.text")"
cmp "$TMP/ref.text" "$TMP/new.text" && echo IDENTICAL
