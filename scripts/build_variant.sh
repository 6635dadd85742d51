#!/bin/bash
# usage: scripts/build_variant.sh <tag> <source.hip> [-DNAME=VALUE ...]
# A/B builds of ONE translation unit: ptgnn_amd/csrc/libptgnn_amd_<tag>.so = that source compiled with the given
# macros + the other objects of the regular build (python -m ptgnn_amd.build first).  Select it at run time with
# PTGNN_AMD_LIB=ptgnn_amd/csrc/libptgnn_amd_<tag>.so.
# e.g. the whole-unit form of the streaming GEMMs:  scripts/build_variant.sh whole stream_gemm.hip -DPTGNN_TAIL_SPLIT=0
set -e
tag=$1; src=$2; shift 2
root="$(cd "$(dirname "$0")/.." && pwd)"
cd "$root/ptgnn_amd/csrc"
base=${src%.*}
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -fvisibility=hidden --offload-arch=gfx950 -Wno-unused-result -x hip "$@" -c $src -o ${base}_${tag}.o
objs=""
# the object list of the regular build (ptgnn_amd/build.py SOURCES)
for o in $(cd "$root" && python -c "from ptgnn_amd import build as b; print(' '.join(s.rsplit('.', 1)[0] for s in b.SOURCES))"); do
  if [ "$o" = "$base" ]; then objs="$objs ${base}_${tag}.o"; else objs="$objs $o.o"; fi
done
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -Wl,--version-script=exports.map -o libptgnn_amd_${tag}.so $objs
echo built libptgnn_amd_${tag}.so
