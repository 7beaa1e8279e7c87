#!/bin/bash
# SQ_INSTS_VALU / SQ_WAVES / SQ_BUSY_CU_CYCLES of one kernel for every library variant in build_variants/ (GPU box):
#   tools/pmc_variants.sh <kernel-substring>
K=${1:-k_lk15}
R=/root/repo
O=${OUT:-$R/out}; mkdir -p "$O"                              # logs and traces (OUT: an absolute directory)
PKG=$R/drone-stabilisation-using-optical-flow-gps-and-inertial-sensors_amd
cd /tmp && export TMPDIR=/tmp
for lib in $R/build_variants/libofk_*.so; do
  name=$(basename $lib .so); name=${name#libofk_}
  cp $lib $PKG/libofk.so
  rm -rf $O/pv_$name
  rocprofv3 --pmc SQ_WAVES SQ_BUSY_CU_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAIT_INST_ANY SQ_WAVE_CYCLES SQ_ACTIVE_INST_ANY --kernel-trace --output-format csv -d $O/pv_$name -o p -- python3 $R/bench.py --full --batch 128 --no-overlap --steps 2 --warmup 1 --cpu-sample 0 > $O/pv_$name.log 2>&1 || { tail -3 $O/pv_$name.log; exit 1; }
  python3 - $O/pv_$name $K $name <<'PY'
import csv, glob, sys, collections
d, k, name = sys.argv[1:4]
tot = collections.defaultdict(float); n = collections.defaultdict(int)
for f in glob.glob(d + '/**/*counter_collection.csv', recursive=True):
    for r in csv.DictReader(open(f)):
        if k in r['Kernel_Name']:
            tot[r['Counter_Name']] += float(r['Counter_Value']); n[r['Counter_Name']] += 1
print(name, ' '.join(f"{c}={tot[c]/n[c]:.0f}" for c in sorted(tot)))
PY
done
