#!/bin/bash
# Runs on a GPU machine: measures the kernel choices of every benchmark configuration (bench.py --full) into the file named by the
# first argument (default /tmp/tune_db.txt).  Copy the result (below its three comment lines) into lighthand_amd/tune_db_gfx950.txt.
set -e
DB=$(realpath -m "${1:-/tmp/tune_db.txt}")
cd "$(dirname "$0")/.."
rm -f "$DB"
LH_TUNE_ITERS=20 LH_TUNE_DB=0 LH_TUNE_CACHE=$DB python bench.py --full --no-cpu-baseline --steps 5 > /dev/null
wc -l "$DB"
