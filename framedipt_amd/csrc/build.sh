#!/bin/bash
# Build libfdipt_hip.so for gfx950 (MI355X).  Cross-compiles without a GPU.
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
OUT="$HERE/../lib"
BUILD="$HERE/build"; LIBNAME=libfdipt_hip.so; EXTRA=""
# FDIPT_VARIANT=name FDIPT_EXTRA="-D..." : a build with extra compile flags -> lib/libfdipt_hip_<name>.so (the bf16 library:
# FDIPT_VARIANT=bf16 FDIPT_EXTRA=-DFDIPT_HALF_BF16; loaded through FDIPT_LIB)
if [ -n "${FDIPT_VARIANT:-}" ]; then BUILD="$HERE/build_$FDIPT_VARIANT"; LIBNAME=libfdipt_hip_$FDIPT_VARIANT.so; EXTRA="${FDIPT_EXTRA:-}"; fi
mkdir -p "$OUT" "$BUILD"
# FDIPT_CLEAN=1 (what __graft_entry__.build() sets): drop every object first, so that the run proves the tree compiles
# (the default is mtime-incremental: objects and libraries travel with the tree to the GPU box)
if [ -n "${FDIPT_CLEAN:-}" ]; then rm -f "$BUILD"/*.o "$OUT/$LIBNAME"; fi
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
# -Wno-inline-asm: the LDS-DMA helpers name m0 (a reserved register hipcc re-materialises before each of its own uses) as clobbered
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value -Wno-unused-result -Wno-inline-asm $EXTRA"
UNITS="gemm ipa_proj2 pair_mlp edge_embed2 edge_transition3 edge_transition4 attention attention3 pair_bias attention_seq chain rowblock frames select evaluate violations dssp sasa tmscore tmalign structsearch mpnn lddt lddt_mapped gdt gdt_mapped seqalign seqalign_modes interface interface_mapped model"
pids=()
T0=$SECONDS
NCOMP=0
OBJS=()
for f in $UNITS; do
  OBJS+=("$BUILD/$f.o")
  # stale: no object, or the unit, any header of csrc/ or the C ABI is newer than it
  stale=
  for src in "$HERE/$f.hip" "$HERE"/*.hpp "$HERE/../../include/fdipt.h"; do
    if [ ! -f "$BUILD/$f.o" ] || [ "$src" -nt "$BUILD/$f.o" ]; then stale=1; break; fi
  done
  if [ -n "$stale" ]; then
    $HIPCC $FLAGS -c "$HERE/$f.hip" -o "$BUILD/$f.o" &
    pids+=($!)
    NCOMP=$((NCOMP + 1))
  fi
done
for p in "${pids[@]}"; do wait $p; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT/$LIBNAME" "${OBJS[@]}"
echo "compiled $NCOMP of ${#OBJS[@]} units for gfx950 in $((SECONDS - T0)) s: $(cd "$BUILD" && ls *.o | tr '\n' ' ')"
echo "built $OUT/$LIBNAME"
