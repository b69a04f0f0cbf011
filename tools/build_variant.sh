#!/bin/bash
# A variant library that differs from the in-tree build in some source files:
# those recompiled with extra flags (on top of their per-source flags of
# csrc/SOURCES.txt), every other object reused from build/obj (run
# __graft_entry__.build() first).
#   bash tools/build_variant.sh <out.so> <a.hip[,b.hip...]> -DFLAG=... [more flags]
set -e
cd "$(dirname "$0")/.."
OUT=$1; SRCS=$2; shift 2
S=iwae_replication_project_amd/csrc
mkdir -p "$(dirname "$OUT")" build/var
TAG=$(basename "$OUT" .so)
OBJS=""
while read -r src flags; do
  f=${src%.hip}
  if [[ ",$SRCS," == *",$src,"* ]]; then
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-result $flags "$@" -c -o build/var/${f}_${TAG}.o $S/$src
    OBJS="$OBJS build/var/${f}_${TAG}.o"
  else
    OBJS="$OBJS build/obj/$f.o"
  fi
done < <(sed -e 's/#.*//' -e '/^[[:space:]]*$/d' $S/SOURCES.txt)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT" $OBJS -lrccl
