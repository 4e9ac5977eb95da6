#!/bin/bash
# Kernel trace of the Panda's stationary step (bench.py's protocol, 1000-step pre-roll): durations of k_fast / k_row_list over the last
# launches and their start offsets.   usage: tools/trace_panda_steady3.sh <envs> <tag> [env assignments...]
N=${1:-131072}; TAG=${2:-tp3}; shift 2
export TMPDIR=/tmp
ROOTDIR=$(pwd)
OUT=${PBRE_OUT:-out}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)      # results (PBRE_OUT, default out/)
rm -rf $OUT/prof_$TAG
(cd /tmp && env "$@" timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- python $ROOTDIR/bench.py --full --envs $N --no-cpu-baseline --no-other-configs --no-host-path --no-fresh --no-shards > $OUT/${TAG}_rocprof.log 2>&1)
t=$(find $OUT/prof_$TAG -name "*kernel_trace.csv" | head -1)
s=$(find $OUT/prof_$TAG -name "*kernel_stats.csv" | head -1)
[ -n "$s" ] && python tools/compact_stats.py $s $OUT/${TAG}_kernel_stats.csv && head -8 $OUT/${TAG}_kernel_stats.csv
[ -n "$t" ] && python tools/trace_steps.py $t 250 | tail -6
tail -1 $OUT/${TAG}_rocprof.log | cut -c1-200
find $OUT/prof_$TAG -name "*kernel_trace.csv" -delete; find $OUT/prof_$TAG -name "*.db" -delete
