# round 2 profiles: rocprofv3 kernel stats of the bench command (wjacobi = the default line, rb), PMC passes for HBM
# traffic (FETCH_SIZE, WRITE_SIZE: separate passes) and for the SQ view of every kernel of the cycle (VALU activity,
# wave cycles, waits), kernel stats of BASELINE configs 2 and 5.  Summaries: scripts/collect_profiles_r02.py.
set -x
export OUT=${OUT:?set OUT to the absolute directory the results go to}
TAG=${1:-r02}
export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
mkdir -p $OUT
cd /tmp
SQ="SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY"
for sm in wjacobi rb; do
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_$sm -- python3 $R/bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-extras --smoother $sm > $OUT/prof_${TAG}_$sm.log 2>&1
  echo "stats $sm rc=$?"
  for C in FETCH_SIZE WRITE_SIZE; do
    timeout -k 10 300 rocprofv3 --kernel-trace --pmc $C --output-format csv -d $OUT/pmc_${TAG}_${sm}_$C -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extras --smoother $sm > $OUT/pmc_${TAG}_${sm}_$C.log 2>&1
    echo "pmc $sm $C rc=$?"
  done
  timeout -k 10 300 rocprofv3 --kernel-trace --pmc $SQ --output-format csv -d $OUT/pmc_${TAG}_${sm}_SQ -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extras --smoother $sm > $OUT/pmc_${TAG}_${sm}_SQ.log 2>&1
  echo "pmc $sm SQ rc=$?"
done
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_cfg2 -- python3 $R/bench.py --full --config 1 --steps 20 --warmup 5 --no-cpu-baseline --no-extras > $OUT/prof_${TAG}_cfg2.log 2>&1
echo "cfg2 rc=$?"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_cfg5 -- python3 $R/scripts/bench_config5.py > $OUT/prof_${TAG}_cfg5.log 2>&1
echo "cfg5 rc=$?"
cd $R
git rev-parse HEAD > $OUT/prof_${TAG}_commit.txt 2>/dev/null || true
