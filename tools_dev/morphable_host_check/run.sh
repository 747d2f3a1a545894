#!/bin/bash
# Host check of the morphable kernels' bodies (no GPU, no LD_PRELOAD): a stand-alone program, address + undefined-behaviour
# sanitizers.  The kernel header is compiled as it is, less the one clang loop pragma g++ does not know.
# usage: tools_dev/morphable_host_check/run.sh [build directory, default dev_out/morphable_host_check]
set -eo pipefail
cd "$(dirname "$0")"
OUT="${1:-../../dev_out/morphable_host_check}"
mkdir -p "$OUT"
grep -v '^#pragma clang loop' ../../deep3dmap_amd/csrc/d3m_morphable.h > "$OUT/d3m_morphable.h"
g++ -std=c++20 -O1 -g -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread \
    -I"$OUT" -I. main.cpp -o "$OUT/morphable_host_check"
"$OUT/morphable_host_check"
