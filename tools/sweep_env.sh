#!/bin/bash
# bench.py under a list of values of one environment knob (GPU box):  tools/sweep_env.sh NAME v1 v2 ... [-- bench flags]
NAME=$1; shift
O=${OUT:-out}; mkdir -p "$O"                                   # logs (OUT: any directory)
VALS=(); while [ $# -gt 0 ] && [ "$1" != "--" ]; do VALS+=("$1"); shift; done; [ "$1" = "--" ] && shift
for v in "${VALS[@]}"; do
  env $NAME=$v timeout -k 10 200 python bench.py --full --cpu-sample 0 "$@" > $O/sw_${NAME}_$v.log 2>&1 || { echo "$NAME=$v failed"; tail -3 $O/sw_${NAME}_$v.log; exit 1; }
  echo "== $NAME=$v"; python tools/show_bench.py $O/sw_${NAME}_$v.log | grep -E "frame-pairs|eig |lk |gray|pyr"
done
