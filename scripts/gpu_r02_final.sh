# round 2 verification: the whole GPU suite, smoke, the default bench line, then the profile passes
set -x
export OUT=${OUT:?set OUT to the absolute directory the results go to}
TAG=${1:-r02f}
R=$GRAFT_REPO_ROOT
mkdir -p $OUT
cd $R
timeout -k 10 1100 python -m pytest tests -x -q -m gpu > $OUT/${TAG}_tests.log 2>&1
echo "tests rc=$?" | tee -a $OUT/${TAG}_tests.log
tail -4 $OUT/${TAG}_tests.log
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1; tail -2 $OUT/${TAG}_smoke.log
timeout -k 10 600 python bench.py --full --steps 20 --warmup 5 > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
echo "bench rc=$?"; tail -c 600 $OUT/${TAG}_bench.json
timeout -k 10 300 python bench.py --full --smoother rb --steps 20 --warmup 5 --no-cpu-baseline > $OUT/${TAG}_bench_rb.json 2> $OUT/${TAG}_bench_rb.err
timeout -k 10 300 python bench.py --full --config 1 --steps 40 --warmup 5 --no-cpu-baseline --no-extras > $OUT/${TAG}_bench_cfg2.json 2>/dev/null
timeout -k 10 300 python scripts/bench_config5.py > $OUT/${TAG}_bench_cfg5.json 2>/dev/null
timeout -k 10 300 python scripts/bench_python_call.py > $OUT/${TAG}_pycall.log 2>&1
timeout -k 10 400 python scripts/bench_lex.py > $OUT/${TAG}_bench_lex.log 2>&1
bash scripts/gpu_r02_profiles.sh $TAG > $OUT/${TAG}_profiles.log 2>&1
tail -12 $OUT/${TAG}_profiles.log
