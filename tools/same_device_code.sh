#!/bin/bash
# Is the GPU machine code of two builds of csrc/ the same, instruction for instruction?  For a kernel refactor that claims to touch
# only code the compiler already threw away.  Build both trees with the same hipcc and the Makefile's flags (`make all`), then
#   bash tools/same_device_code.sh PARENT_CSRC THIS_CSRC [PARENT_REV] > profiles/<change>/same_device_code.txt
# Every object of both builds (*.o and f16/*.o) is compared: equal md5 is enough; otherwise the gfx950 code object is taken out of
# the fat binary and its disassembly, its notes (kernel descriptors / metadata: registers, LDS, scratch, spills, launch bounds), its
# symbols (name, type, binding, size; without __hip_cuid_<hash>, a hash of the translation unit's text) and the host disassembly
# must all be identical.  One summary line per object; exit status 1 at the first difference.
set -o pipefail
A=${1:?usage: same_device_code.sh PARENT_CSRC THIS_CSRC [PARENT_REV]}
B=${2:?usage: same_device_code.sh PARENT_CSRC THIS_CSRC [PARENT_REV]}
LLVM=${LLVM:-/opt/rocm/llvm/bin}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
TMP=$(mktemp -d) || exit 2
trap 'rm -rf "$TMP"' EXIT

echo "parent: ${3:-$A}"
$HIPCC --version | sed 's/^/hipcc: /'
echo

# views of one object: $1 = object file, $2 = output prefix
views() {
  $LLVM/llvm-objcopy --dump-section .hip_fatbin=$2.fatbin $1 /dev/null || return 1
  $LLVM/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$2.fatbin --output=$2.co || return 1
  $LLVM/llvm-objdump -d $2.co | grep -v 'file format' > $2.dev || return 1
  $LLVM/llvm-readelf --notes $2.co > $2.notes || return 1
  $LLVM/llvm-readelf -sW $2.co | awk '$1 ~ /^[0-9]+:$/ && $8 !~ /^__hip_cuid_/ {print $8, $4, $5, $3}' | sort > $2.syms || return 1
  $LLVM/llvm-objdump -d $1 | grep -v 'file format' > $2.host || return 1
}

objs=$( (cd "$A" && ls *.o f16/*.o; cd "$B" && ls *.o f16/*.o) 2> /dev/null | sort -u)
[ -n "$objs" ] || { echo "no objects under $A and $B"; exit 2; }
for o in $objs; do
  [ -f "$A/$o" ] && [ -f "$B/$o" ] || { echo "$o: DIFFERENT (in one build only)"; exit 1; }
  if [ "$(md5sum < "$A/$o")" = "$(md5sum < "$B/$o")" ]; then
    echo "$o: identical file (md5 $(md5sum < "$B/$o" | cut -c1-32))"
    continue
  fi
  views "$A/$o" $TMP/a && views "$B/$o" $TMP/b || { echo "$o: cannot take the object apart"; exit 2; }
  for v in dev notes syms host; do
    cmp -s $TMP/a.$v $TMP/b.$v || { echo "$o: DIFFERENT ($v)"; diff $TMP/a.$v $TMP/b.$v | head -20; exit 1; }
  done
  echo "$o: same code ($(wc -l < $TMP/b.dev) lines of device disassembly, $(grep -c . $TMP/b.notes) of notes, $(wc -l < $TMP/b.syms) symbols," \
       "$(wc -l < $TMP/b.host) lines of host disassembly); the file differs through __hip_cuid_<hash> only"
done
echo
echo "all objects: same device and host code"
