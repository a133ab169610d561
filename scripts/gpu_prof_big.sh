set -x
export OUT=${OUT:?set OUT to the absolute directory the results go to}
export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
mkdir -p $OUT
cd /tmp
for sm in wjacobi rb; do
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_big_$sm -- python3 $R/bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --smoother $sm > $OUT/prof_big_$sm.log 2>&1
done
