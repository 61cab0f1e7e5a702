#!/bin/bash
# Is the generated device code of two checkouts the same?  The check of a refactor that must not change a kernel (CPU only).
#   tools/isa_cmp.sh <checkout A> <checkout B> [unit ...]          (default: every unit of build.sh's list)
# Compiles each unit of both trees to gfx950 assembly with build.sh's flags, for the default and the -DFDIPT_HALF_BF16 variant,
# drops what differs without a change of code (comments, .file / .ident / .loc lines, the per-file __hip_cuid_<hash> symbol) and
# prints one line per unit and variant.  Exit status 1 if any differs; the stripped files stay in $ISA_CMP_OUT (default
# /tmp/isa_cmp) as <unit>.<variant>.{a,b}.s for `diff`.
set -u
[ $# -ge 2 ] || { sed -n 2,7p "$0"; exit 2; }
A=$(cd "$1" && pwd); B=$(cd "$2" && pwd); shift 2
CSRC=framedipt_amd/csrc
if [ $# -gt 0 ]; then UNITS="$*"; else UNITS=$(sed -n 's/^UNITS="\(.*\)"$/\1/p' "$B/$CSRC/build.sh"); fi
FLAGS=$(sed -n 's/^FLAGS="\(.*\) \$EXTRA"$/\1/p' "$B/$CSRC/build.sh")
[ -n "$UNITS" ] && [ -n "$FLAGS" ] || { echo "cannot read the unit list / FLAGS from $B/$CSRC/build.sh" >&2; exit 2; }
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}; OUT=${ISA_CMP_OUT:-/tmp/isa_cmp}; JOBS=${ISA_CMP_JOBS:-8}
mkdir -p "$OUT"
one() {  # tree side unit variant extra-flag
  $HIPCC $FLAGS $5 --cuda-device-only -S "$1/$CSRC/$3.hip" -o "$OUT/$3.$4.$2.raw.s" 2> "$OUT/$3.$4.$2.log" || { rm -f "$OUT/$3.$4.$2.s"; return; }
  sed -e 's/[ \t]*;.*$//' -e '/^[ \t]*\.\(file\|ident\|loc\)[ \t]/d' -e '/__hip_cuid_/d' -e '/^[ \t]*$/d' "$OUT/$3.$4.$2.raw.s" > "$OUT/$3.$4.$2.s"
  rm -f "$OUT/$3.$4.$2.raw.s"
}
n=0
for u in $UNITS; do
  for v in "fp16:" "bf16:-DFDIPT_HALF_BF16"; do
    one "$A" a $u ${v%%:*} "${v#*:}" & one "$B" b $u ${v%%:*} "${v#*:}" &
    n=$((n + 2)); [ $((n % JOBS)) -eq 0 ] && wait
  done
done
wait
bad=0
for u in $UNITS; do
  for v in fp16 bf16; do
    a="$OUT/$u.$v.a.s"; b="$OUT/$u.$v.b.s"
    if [ ! -s "$a" ] || [ ! -s "$b" ]; then echo "$u $v: COMPILE FAILED (see $OUT/$u.$v.*.log)"; bad=1
    elif cmp -s "$a" "$b"; then echo "$u $v: identical ($(wc -l < "$a") lines)"
    else echo "$u $v: DIFFERENT ($(diff "$a" "$b" | grep -c '^[<>]') lines; diff $a $b)"; bad=1; fi
  done
done
exit $bad
