#!/bin/bash
# The figures of docs/EXPERIMENTS.md "Weak-perspective pose": tools_dev/pose_cost.py in a process of its own under a time limit.
# usage: tools_dev/pose_cost.sh [output directory, default dev_out]
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
OUT="${1:-dev_out}"
mkdir -p "$OUT"
timeout -k 10 300 python tools_dev/pose_cost.py --out "$OUT/pose_cost_basel.json"
