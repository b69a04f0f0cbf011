#!/bin/bash
# Debug build of the library into tools/_dbg/ (git-ignored .so; gpurun-ignored too:
# DBG_DIR=dbgx puts it where a gpurun call takes it along), e.g.
#   bash tools/build_debug.sh -DIWAE_GEMM_TRACE      -> tools/_dbg/libiwae_dbg.so
# then run a tool with IWAE_HIP_LIB=tools/_dbg/libiwae_dbg.so.
# Sources and their per-source flags: csrc/SOURCES.txt.
set -e
cd "$(dirname "$0")/.."
D=${DBG_DIR:-tools/_dbg}; mkdir -p $D/obj
S=iwae_replication_project_amd/csrc
OBJS=""
while read -r src flags; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-result $flags "$@" -c -o $D/obj/${src%.hip}.o $S/$src
  OBJS="$OBJS $D/obj/${src%.hip}.o"
done < <(sed -e 's/#.*//' -e '/^[[:space:]]*$/d' $S/SOURCES.txt)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $D/${OUT:-libiwae_dbg.so} $OBJS -lrccl
