# session 2, last verification: whole GPU suite, smoke, the default bench line, the drop-in call with host arrays, the examples
set -x
export OUT=${OUT:?set OUT to the absolute directory the results go to}
mkdir -p $OUT
TAG=${1:-s2h}
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $OUT/pytest_gpu_$TAG.log 2>&1; echo "pytest rc=$?" >> $OUT/pytest_gpu_$TAG.log
tail -3 $OUT/pytest_gpu_$TAG.log
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1; tail -2 $OUT/${TAG}_smoke.log
timeout -k 10 600 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err; echo "bench rc=$?"
timeout -k 10 300 python scripts/bench_python_call.py > $OUT/${TAG}_pycall.log 2>&1; head -3 $OUT/${TAG}_pycall.log
bash scripts/gpu_examples.sh > $OUT/${TAG}_examples.log 2>&1; grep "rc=" $OUT/${TAG}_examples.log
