set -x
export OUT=${OUT:?set OUT to the absolute directory the results go to}
mkdir -p $OUT
TAG=${1:-r01f}
timeout -k 10 1000 python -m pytest tests -m gpu -x -q > $OUT/pytest_gpu_$TAG.log 2>&1 ; echo "pytest rc=$?" >> $OUT/pytest_gpu_$TAG.log
tail -4 $OUT/pytest_gpu_$TAG.log
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1; tail -2 $OUT/smoke_$TAG.log
timeout -k 10 400 python bench.py --full > $OUT/bench_${TAG}_default.json 2> $OUT/bench_${TAG}_default.err; cat $OUT/bench_${TAG}_default.json; tail -2 $OUT/bench_${TAG}_default.err
timeout -k 10 400 python bench.py --full --smoother rb --no-cpu-baseline > $OUT/bench_${TAG}_rb.json 2> $OUT/bench_${TAG}_rb.err; cat $OUT/bench_${TAG}_rb.json
bash scripts/gpu_pmc.sh wjacobi $TAG > $OUT/pmc_run_wj.log 2>&1
bash scripts/gpu_pmc.sh rb $TAG > $OUT/pmc_run_rb.log 2>&1
export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
cd /tmp
for sm in wjacobi rb; do
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_$sm -- python3 $R/bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --smoother $sm > $OUT/prof_${TAG}_$sm.log 2>&1
done
