#!/bin/bash
# The figures of docs/EXPERIMENTS.md "Linear morphable model": the two parts of tools_dev/morphable_cost.py, each a process
# of its own under its own time limit; a part that fails (or runs into its limit) stops the rest.
# usage: tools_dev/morphable_cost.sh [output directory, default dev_out]
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
OUT="${1:-dev_out}"
mkdir -p "$OUT"
timeout -k 10 300 python tools_dev/morphable_cost.py --part kernels --out "$OUT/morphable_cost_kernels.json" &&
timeout -k 10 300 python tools_dev/morphable_cost.py --part fit --out "$OUT/morphable_cost_fit.json"
