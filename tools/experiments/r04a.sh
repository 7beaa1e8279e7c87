set -x
cd $GRAFT_REPO_ROOT
O=${OUT:-out}; mkdir -p "$O"                                   # logs (OUT: any directory)
TESTS="tests/test_gpu_image_parity.py tests/test_gpu_pipeline.py" OUT=$(cd "$O" && pwd) bash tools/experiments/run_variants.sh > $O/r04a_variants.log 2>&1
# baseline schedule with the product lib (rd2 default build), alternating
for i in 1 2; do
python bench.py --full --cpu-sample 0 --no-ingest --steps 40 --tune no_bgr_eig=1 > $O/r04a_base_$i.json 2>> $O/r04a.err
python bench.py --full --cpu-sample 0 --no-ingest --steps 40 > $O/r04a_new_$i.json 2>> $O/r04a.err
done
python - "$O" <<'PY'
import json,glob,sys
for f in sorted(glob.glob(sys.argv[1] + '/r04a_*_?.json')):
    d=json.load(open(f)); print(f, d['value'], d['ms_per_step'], {k:(v['ms_per_step']) for k,v in d['stages'].items()}, {k:(v['ms_per_step']) for k,v in d['stages_isolated'].items()})
PY
