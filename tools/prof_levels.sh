#!/bin/bash
# per-launch durations of the pyramid kernel (one line per level) from a rocprofv3 kernel trace of bench.py
R=$(cd "$(dirname "$0")/.." && pwd); O=${OUT:-$R/out}; mkdir -p "$O"   # OUT: an absolute directory for the trace
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_pyr -o pyr -- python3 $R/bench.py --full --no-overlap --steps 10 --warmup 2 --cpu-sample 0 > $O/prof_pyr.log 2>&1
cd "$R" && python - "$O" <<'PY'
import csv,glob,collections,sys
f=glob.glob(sys.argv[1]+'/prof_pyr/**/*kernel_trace.csv',recursive=True)[0]
d=collections.defaultdict(list)
for r in csv.DictReader(open(f)):
    n=r['Kernel_Name'].split('(')[0]
    d[(n,r['Grid_Size_X'],r['Grid_Size_Y'],r['Grid_Size_Z'])].append(int(r['End_Timestamp'])-int(r['Start_Timestamp']))
for k,v in sorted(d.items()): print(k, len(v), round(sum(v)/len(v)/1e3,1),'us')
PY
