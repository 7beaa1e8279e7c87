O=${OUT:-out}; mkdir -p "$O"                                   # logs (OUT: any directory)
for b in 256 264 270 272 288 360; do timeout -k 10 200 python bench.py --full --batch $b --cpu-sample 0 --steps 15 --warmup 3 > $O/sb_$b.log 2>&1 || exit 1; python tools/show_bench.py $O/sb_$b.log | grep -E "frame-pairs|eig "; done
