#!/bin/bash
# Device-code identity against another checkout (no GPU needed):
#   bash tools/asm_identical.sh BASE_DIR        (JOBS=8; ASM_OUT=dir keeps the assembly texts there)
# Every csrc/*.hip of this tree and of BASE_DIR (a checkout of the commit to compare with) is compiled to
# gfx950 assembly with its Makefile's own compile line (HIPFLAGS and the per-file FLAGS_*), device side only.
# The two texts are compared wholesale, less the lines naming __hip_cuid_<hash> (a hash of the source text).
# One line per file, `identical` or `DIFFERS`; the exit status is non-zero on any difference.
set -u
BASE=$(cd "${1:?usage: asm_identical.sh BASE_DIR}" && pwd) || exit 2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
PKG=geometry-grounded-gaussian-splatting_amd
OUT=${ASM_OUT:-$(mktemp -d)}
mkdir -p "$OUT/new" "$OUT/base"

emit() {  # emit TREE NAME OUT.s: the Makefile's compile line for build/NAME.o, turned into -S of the device side
    local cmd
    cmd=$(make -s -n -B -C "$1/$PKG" "build/$2.o" 2>/dev/null | grep -- " -c csrc/$2.hip ") || return 1
    cmd=$(sed "s# -c csrc/$2.hip -o .*# --cuda-device-only -S csrc/$2.hip -o $3.raw#" <<<"$cmd")
    (cd "$1/$PKG" && eval "$cmd" 2>"$3.log") && grep -v __hip_cuid_ "$3.raw" >"$3"
}
export -f emit
export PKG

names=$(cd "$ROOT/$PKG/csrc" && ls *.hip | sed 's/\.hip$//')
for n in $names; do
    echo "$ROOT $n $OUT/new/$n.s"
    echo "$BASE $n $OUT/base/$n.s"
done | xargs -P "${JOBS:-8}" -L 1 bash -c 'emit "$0" "$1" "$2" || echo "compile failed: $0 $1" >&2'

status=0
for n in $names; do
    if [ -s "$OUT/new/$n.s" ] && cmp -s "$OUT/new/$n.s" "$OUT/base/$n.s"; then
        echo "$n.hip identical"
    else
        echo "$n.hip DIFFERS"
        status=1
    fi
done
exit $status
