#!/bin/bash
# Host check of the pose kernels' bodies (no GPU, no LD_PRELOAD): a stand-alone program under the address and
# undefined-behaviour sanitizers.  csrc/d3m_pose.h and csrc/d3m_set_sums.h are compiled as they are; of csrc/d3m_aux.h only
# mat3_mul and euler_factors are taken (cut out of the real file), the rest of the device side is ../morphable_host_check's
# shim and the d3m_aux.h / d3m_device.h here.
# usage: tools_dev/pose_host_check/run.sh [build directory, default dev_out/pose_host_check]
set -eo pipefail
cd "$(dirname "$0")"
OUT="${1:-../../dev_out/pose_host_check}"
mkdir -p "$OUT"
CSRC=../../deep3dmap_amd/csrc
sed -n '/^__device__ __forceinline__ void mat3_mul/,/^}/p;/^__device__ __forceinline__ void euler_factors/,/^}/p' \
    "$CSRC/d3m_aux.h" > "$OUT/aux_helpers.inc"
test "$(grep -c '^}' "$OUT/aux_helpers.inc")" = 2
cp "$CSRC/d3m_pose.h" "$CSRC/d3m_set_sums.h" "$OUT/"       # (beside no d3m_aux.h / d3m_device.h: the includes find the stand-ins)
g++ -std=c++20 -O1 -g -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread \
    -I"$OUT" -I. -I../morphable_host_check main.cpp -o "$OUT/pose_host_check"
"$OUT/pose_host_check"
