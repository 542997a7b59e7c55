# A/B of two builds of libroadrestore on ONE box: alternating bench runs
# (single-run noise ~0.7%; box-to-box spread is larger, so compare in-call).
# usage: bash tools/ab_libs.sh <other .so> [rounds]   -> $OUT/ab_libs.txt (OUT: default ab_out)
OTHER=$1; R=${2:-3}
OUT=${OUT:-ab_out}; mkdir -p $OUT
rm -f $OUT/ab_libs.txt
for i in $(seq $R); do
  for L in cur other; do
    if [ $L = other ]; then export RR_LIB_PATH=$OTHER; else unset RR_LIB_PATH; fi
    timeout -k 10 100 python bench.py --full --no-cpu-baseline --no-probe --steps 30 > $OUT/ab_$L.log 2>&1 || exit 1
    tail -1 $OUT/ab_$L.log | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('$L', d['value'], d['ms_per_step'])" >> $OUT/ab_libs.txt
  done
done
