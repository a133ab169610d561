set -x
export OUT=${OUT:?set OUT to the absolute directory the results go to}
mkdir -p $OUT
timeout -k 10 300 python scripts/bench_matrix.py > $OUT/bench_matrix.log 2>&1; cat $OUT/bench_matrix.log
timeout -k 10 600 python bench.py --full --grid 32768 --steps 5 --warmup 1 --no-cpu-baseline > $OUT/bench_32768_wj.json 2> $OUT/bench_32768_wj.err; cat $OUT/bench_32768_wj.json; tail -3 $OUT/bench_32768_wj.err
timeout -k 10 600 python bench.py --full --grid 32768 --steps 5 --warmup 1 --no-cpu-baseline --smoother rb > $OUT/bench_32768_rb.json 2> $OUT/bench_32768_rb.err; cat $OUT/bench_32768_rb.json
timeout -k 10 300 python bench.py --full --grid 4096 --steps 50 --warmup 5 --no-cpu-baseline --smoother rb > $OUT/bench_4096_rb.json 2> $OUT/bench_4096_rb.err; cat $OUT/bench_4096_rb.json
timeout -k 10 400 python scripts/bench_config5.py 8192 > $OUT/config5_misc.log 2>&1; cat $OUT/config5_misc.log
