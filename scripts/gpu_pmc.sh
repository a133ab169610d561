# HBM traffic of the bench's kernels from PMC counters: separate passes for FETCH_SIZE and WRITE_SIZE
# (MI355X_MICROARCH.md "HBM": they do not fit one pass; FETCH_SIZE under-reports 16-byte streams by 2x on gfx950)
set -x
export OUT=${OUT:?set OUT to the absolute directory the results go to}
SM=${1:-wjacobi}
TAG=${2:-r01}
export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
mkdir -p $OUT
cd /tmp
for C in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 300 rocprofv3 --kernel-trace --pmc $C --output-format csv -d $OUT/pmc_${TAG}_${SM}_$C -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --smoother $SM > $OUT/pmc_${TAG}_${SM}_$C.log 2>&1
done
ls -R $OUT/pmc_${TAG}_${SM}_FETCH_SIZE | head
