#!/bin/bash
# Builds a variant of the library for A/B measurements on one box (one source file recompiled with extra flags):
#   bash tools/build_variant.sh <tag> [-DXH_...=...]            ->  xmipp3_amd/libxmipp_hip_<tag>.so   (XMIPP_HIP_LIB selects it)
#   SRC=xh_pm bash tools/build_variant.sh <tag> [-DXH_...=...]   the matcher instead of the reconstruction (SRC=xh_flexalign, ...): ONLY the named
#   file sees the flags
# The other objects are the product build's (xmipp3_amd/csrc/build.sh first).  Flags that leave the named file's object as it is (meant for
# another file, or a value the file already has) are refused: the variant would be the product library under another name.
set -e
tag=$1; shift
SRC=${SRC:-xh_rf}
cd "$(dirname "$0")/../xmipp3_amd/csrc"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
mkdir -p build/variants
# build.sh's flags (files that must round like the reference's scalar code: no FMA contraction)
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -Wno-unused-function -Wno-unused-result"
case $SRC in xh_rf|xh_fsc|xh_halves|xh_powell) FLAGS="$FLAGS -ffp-contract=off";; esac
# The file is compiled a second time without the extra flags to compare against.  hipcc gives every compilation a new unit id, which
# changes the object; with the same -cuid the two objects are equal byte for byte unless the flags changed the code.
obj=build/variants/${SRC}_$tag.o
$HIPCC $FLAGS -cuid=$tag "$@" -c $SRC.hip -o $obj & p1=$!
$HIPCC $FLAGS -cuid=$tag -c $SRC.hip -o build/variants/${SRC}_$tag.plain.o & p2=$!
wait $p1; wait $p2
if cmp -s $obj build/variants/${SRC}_$tag.plain.o; then
  echo "build_variant.sh: the flags '$*' do not change $SRC.hip's object (SRC= names the file they are meant for)" >&2
  exit 1
fi
objs=""
for f in *.hip; do          # build.sh links one object per source file
  o=${f%.hip}
  if [ "$o" == "$SRC" ]; then objs="$objs $obj"
  else
    [ -f build/$o.o ] || { echo "build_variant.sh: build/$o.o missing: run xmipp3_amd/csrc/build.sh first" >&2; exit 1; }
    objs="$objs build/$o.o"
  fi
done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o ../libxmipp_hip_$tag.so $objs
echo "built xmipp3_amd/libxmipp_hip_$tag.so"
