#!/bin/bash
# rocprofv3 kernel-trace stats of a short bench run -> $PBRE_OUT/prof_$1/ (default out/)
TAG=$1; shift
ROOTDIR=$(pwd); export TMPDIR=/tmp
OUT=${PBRE_OUT:-out}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)      # results (PBRE_OUT, default out/)
(cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- python $ROOTDIR/bench.py --full --no-cpu-baseline --no-other-configs --no-host-path --preroll 200 "$@" > $OUT/rocprof_$TAG.log 2>&1)
f=$(find $OUT/prof_$TAG -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -8 "$f" | cut -c1-60,150-
find $OUT/prof_$TAG -name "*kernel_trace.csv" -size +8M -delete; find $OUT/prof_$TAG -name "*.db" -delete
