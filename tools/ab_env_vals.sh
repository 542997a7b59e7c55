# A/B of two values of an env switch on ONE box (alternating bench runs).
# usage: bash tools/ab_env_vals.sh VAR VAL_A VAL_B [rounds] -> $OUT/ab_env_vals.txt (OUT: default ab_out)
VAR=$1; A=$2; B=$3; R=${4:-3}
OUT=${OUT:-ab_out}; mkdir -p $OUT
rm -f $OUT/ab_env_vals.txt
for i in $(seq $R); do
  for v in $A $B; do
    env $VAR=$v timeout -k 10 100 python bench.py --full --no-cpu-baseline --no-probe --steps 30 > $OUT/ab_ev_$v.log 2>&1 || exit 1
    tail -1 $OUT/ab_ev_$v.log | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('$VAR=$v', d['value'], d['ms_per_step'])" >> $OUT/ab_env_vals.txt
  done
done
