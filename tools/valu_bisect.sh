#!/bin/bash
# VALU instructions per wave of the Panda step kernels for a list of build variants (tools/build_variant.sh), one short --pmc pass each.
#   usage: tools/valu_bisect.sh <suffix> [<suffix> ...]      ("main" = libpbre.so)
ROOTDIR=$(pwd); export TMPDIR=/tmp
OUT=${PBRE_OUT:-out}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)      # results (PBRE_OUT, default out/)
for S in "$@"; do
  L=$ROOTDIR/pybullet-robot-envs_amd/csrc/libpbre_$S.so; [ $S = main ] && L=$ROOTDIR/pybullet-robot-envs_amd/csrc/libpbre.so
  rm -rf $OUT/vb_$S
  (cd /tmp && PBRE_LIB=$L timeout 300 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_WAVE_CYCLES --output-format csv -d $OUT/vb_$S -o run -- python $ROOTDIR/bench.py --full --envs 131072 --no-cpu-baseline --no-other-configs --no-host-path --no-fresh --no-shards --steps 10 --warmup 2 --preroll 300 > $OUT/vb_$S.log 2>&1)
  python - $S "$OUT" <<'PY'
import csv, glob, re, sys, collections
s = sys.argv[1]
f = glob.glob("%s/vb_%s/**/*counter_collection.csv" % (sys.argv[2], s), recursive=True)
per = collections.defaultdict(lambda: collections.defaultdict(list))
for r in csv.DictReader(open(f[0])):
    m = re.match(r"(?:void )?(?:pbre::)?(k_fast\w*<[\d, ]+>|k_row_list<7>)", r["Kernel_Name"])
    if m:
        per[m.group(1)][r["Counter_Name"]].append(float(r["Counter_Value"]))
for k, d in sorted(per.items()):
    w, v, c = (sum(d[x]) for x in ("SQ_WAVES", "SQ_INSTS_VALU", "SQ_WAVE_CYCLES"))
    print("%-8s %-18s launches %4d  VALU/wave %8.0f  cycles/wave %8.0f" % (s, k, len(d["SQ_WAVES"]), v / max(w, 1), c / max(w, 1)))
PY
  find $OUT/vb_$S -name "*.csv" -size +2M -delete; find $OUT/vb_$S -name "*.db" -delete
done
