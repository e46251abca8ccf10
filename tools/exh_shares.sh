#!/bin/bash
# k_exh: per-cent shares of the rows for the four age groups of the grid (TSP_EXH_SHARES), two runs each; run on the GPU box.
# usage: exh_shares.sh [split ...]   (no argument: the pass around 48 / 29 / 15 / 8 that found 45 / 30 / 16 / 9)
# The default stands first and last: splits compare within one pass only.  The first run that fails ends the pass.
set -o pipefail
[ $# -gt 0 ] || set -- "48,29,15,8" "50,28,14,8" "47,29,15,9" "46,30,15,9" "46,29,16,9" "45,30,16,9" "44,30,16,10" "44,31,16,9" "42,30,17,11" "40,30,18,12" "48,29,15,8"
for sh in "$@"; do
  echo -n "shares $sh: "
  for r in 1 2; do
    TSP_EXH_SHARES=$sh timeout -k 10 120 python3 tools/exhaustive_time.py 4:4 2>&1 | tail -1 | sed 's/.* \([0-9.]* us per sweep\).*/\1/' | tr '\n' ' ' || { echo "failed"; exit 1; }
  done
  echo
done
