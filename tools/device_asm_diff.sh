#!/bin/bash
# tools/device_asm_diff.sh <git-rev> [file.hip ...]
# Is the gfx950 device code of the working tree the same as that of <git-rev>?  Both trees' copies of the named sources
# (default: every .hip under openess_amd/csrc, names relative to that directory) are compiled to device-only assembly with
# the COMMON and EXACT flags of their own Makefile, the lines that carry the per-build __hip_cuid_ symbol are dropped, and
# the two texts are compared.  Prints "<file>: identical" or the first kernel that differs; exit status 1 on any difference.
# The check for a refactor of a kernel file that must leave code generation alone.  Needs no GPU.
set -euo pipefail
[ $# -ge 1 ] || { echo "usage: $0 <git-rev> [file.hip ...]" >&2; exit 2; }
ROOT=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
REV=$1; shift
TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT
mkdir "$TMP/old" "$TMP/asm"
git -C "$ROOT" archive "$REV" -- include openess_amd/csrc | tar -x -C "$TMP/old"
if [ $# -gt 0 ]; then FILES=("$@"); else FILES=($(cd "$ROOT/openess_amd/csrc" && ls *.hip)); fi

# one compile: <side> <tree> <file>
asm_one() {
    local side=$1 tree=$2 f=$3 flags
    [ -f "$tree/openess_amd/csrc/$f" ] || { echo "absent" > "$TMP/asm/$side.$f.s"; return 0; }
    flags=$(make -s -C "$tree/openess_amd/csrc" --eval='print-asm-flags: ; @echo $(ARCH) $(COMMON) $(EXACT)' print-asm-flags)
    "$HIPCC" $flags -w --cuda-device-only -S "$tree/openess_amd/csrc/$f" -o - | grep -v __hip_cuid_ > "$TMP/asm/$side.$f.s"
}
export -f asm_one; export TMP HIPCC
for f in "${FILES[@]}"; do printf '%s\n' "old $TMP/old $f" "new $ROOT $f"; done | xargs -P 16 -L 1 bash -c 'asm_one "$@"' _

status=0
for f in "${FILES[@]}"; do
    a="$TMP/asm/old.$f.s"; b="$TMP/asm/new.$f.s"
    if cmp -s "$a" "$b"; then echo "$f: identical"; continue; fi
    status=1
    line=$(cmp "$a" "$b" | sed -E 's/.* line ([0-9]+)$/\1/') || true
    # the function label (not a .L local one) that the first differing line stands under
    sym=$(awk -v n="${line:-1}" 'NR > n { exit } /^[A-Za-z_$][A-Za-z0-9_$.]*:/ { s = $1 } END { sub(/:.*/, "", s); print s }' "$b")
    echo "$f: DIFFERENT at line ${line:-?}, first in ${sym:-the file header} ($(diff "$a" "$b" | grep -c '^[<>]') diff lines)"
done
exit $status
