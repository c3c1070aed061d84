# rocprofv3 passes for profiles/ (run on an MI355X); outputs under $WS_PROFILE_OUT (default profile_out/)
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
export WS_PROFILE_OUT=${WS_PROFILE_OUT:-profile_out}; OUT=$WS_PROFILE_OUT  # where the passes write (git-ignored)
mkdir -p "$OUT"
TAG=${1:-r01}
python bench.py --steps 20 --warmup 3 --full > $OUT/bench_${TAG}.json 2> $OUT/bench_${TAG}.err
rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG}_sparse -o trace -- python bench.py --steps 10 --warmup 2 --no-cpu-baseline --full > $OUT/prof_${TAG}_sparse.log 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG}_dense -o trace -- python bench.py --steps 10 --warmup 2 --no-cpu-baseline --integrate dense --full > $OUT/prof_${TAG}_dense.log 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG}_tiles -o trace -- python bench.py --steps 5 --warmup 1 --no-cpu-baseline --scatter tiles --full > $OUT/prof_${TAG}_tiles.log 2>&1
# PMC passes in their own runs (kernel-trace only), one counter per run
for mode in sparse dense; do
  rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/prof_${TAG}_pmc_fetch_${mode} -o pmc -- python bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-registration --integrate ${mode} > $OUT/prof_${TAG}_pmc_fetch_${mode}.log 2>&1
  rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/prof_${TAG}_pmc_write_${mode} -o pmc -- python bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-registration --integrate ${mode} > $OUT/prof_${TAG}_pmc_write_${mode}.log 2>&1
done
cat $OUT/bench_${TAG}.json | cut -c1-400
