# rocprofv3 passes for profiles/ (run on an MI355X); outputs under $WS_PROFILE_OUT (default profile_out/)
#   bash tools/profile_r02.sh TAG [quick]
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
export WS_PROFILE_OUT=${WS_PROFILE_OUT:-profile_out}; OUT=$WS_PROFILE_OUT  # where the passes write (git-ignored)
mkdir -p "$OUT"
TAG=${1:-r02}
QUICK=${2:-}
for mode in sparse dense; do
  rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG}_${mode} -o trace -- python bench.py --steps 10 --warmup 2 --no-cpu-baseline --integrate ${mode} --full > $OUT/prof_${TAG}_${mode}.log 2>&1
  python tools/rocpd_stats.py $OUT/prof_${TAG}_${mode}/*/trace_results.db > $OUT/${TAG}_kernel_stats_${mode}.txt 2>/dev/null || python tools/rocpd_stats.py $(ls $OUT/prof_${TAG}_${mode}/*.db $OUT/prof_${TAG}_${mode}/*/*.db 2>/dev/null | head -1) > $OUT/${TAG}_kernel_stats_${mode}.txt
done
if [ -z "$QUICK" ]; then
  python bench.py --steps 20 --warmup 3 --full > $OUT/bench_${TAG}.json 2> $OUT/bench_${TAG}.err
  # PMC passes in their own runs (kernel-trace only), one counter per run
  for mode in sparse dense; do
    for ctr in FETCH_SIZE WRITE_SIZE; do
      rocprofv3 --kernel-trace --pmc ${ctr} -d $OUT/prof_${TAG}_pmc_${ctr}_${mode} -o pmc -- python bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-registration --integrate ${mode} > $OUT/prof_${TAG}_pmc_${ctr}_${mode}.log 2>&1
      python tools/pmc_summary.py $(ls $OUT/prof_${TAG}_pmc_${ctr}_${mode}/*.db $OUT/prof_${TAG}_pmc_${ctr}_${mode}/*/*.db 2>/dev/null | head -1) > $OUT/${TAG}_pmc_${ctr}_${mode}.txt
    done
  done
fi
head -20 $OUT/${TAG}_kernel_stats_sparse.txt
