# rocprofv3 passes behind profiles/r03_* (run on an MI355X); outputs under $WS_PROFILE_OUT (default profile_out/), summaries are copied
# into profiles/ afterwards (tools/make_traffic.py writes profiles/pmc_traffic.json).
#   bash tools/profile_r03.sh [TAG] [quick]
# Counter passes are separate runs with --kernel-trace only (no --stats, no other trace domain), one TCC counter per run
# (FETCH_SIZE and WRITE_SIZE do not fit one pass), the SQ counters in two groups of eight.
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
export WS_PROFILE_OUT=${WS_PROFILE_OUT:-profile_out}; OUT=$WS_PROFILE_OUT  # where the passes write (git-ignored)
# the traced runs leave out the multi-rank sections of bench.py (RCCL start-up, HIP-graph capture and a child process under the
# tracer aborted rocprofv3 once); the untraced bench run below has them
export WS_BENCH_SKIP_SHARDED=1
TAG=${1:-r03}
QUICK=${2:-}
mkdir -p "$OUT"
for mode in sparse dense; do
  rm -rf $OUT/prof_${TAG}_${mode}
  rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG}_${mode} -o trace -- python bench.py --steps 10 --warmup 2 --no-cpu-baseline --integrate ${mode} --full > $OUT/prof_${TAG}_${mode}.log 2>&1
  python tools/rocpd_stats.py $(ls $OUT/prof_${TAG}_${mode}/*.db $OUT/prof_${TAG}_${mode}/*/*.db 2>/dev/null | head -1) > $OUT/${TAG}_kernel_stats_${mode}.txt
done
if [ -z "$QUICK" ]; then
  WS_BENCH_SKIP_SHARDED=0 python bench.py --steps 20 --warmup 3 --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
  for mode in sparse dense; do
    for ctr in FETCH_SIZE WRITE_SIZE; do
      rocprofv3 --kernel-trace --pmc ${ctr} -d $OUT/prof_${TAG}_pmc_${ctr}_${mode} -o pmc -- python bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-registration --integrate ${mode} > $OUT/prof_${TAG}_pmc_${ctr}_${mode}.log 2>&1
      python tools/pmc_summary.py $(ls $OUT/prof_${TAG}_pmc_${ctr}_${mode}/*.db $OUT/prof_${TAG}_pmc_${ctr}_${mode}/*/*.db 2>/dev/null | head -1) > $OUT/${TAG}_pmc_${ctr}_${mode}.txt
    done
  done
  # where the cycles of the march / resolve kernels go (the issue-bound claim needs tracked evidence)
  i=0
  for grp in "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_WAVES" \
             "SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM"; do
    i=$((i+1))
    rocprofv3 --kernel-trace --pmc ${grp} -d $OUT/prof_${TAG}_pmc_sq${i} -o pmc -- python bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-registration > $OUT/prof_${TAG}_pmc_sq${i}.log 2>&1
    python tools/pmc_summary.py $(ls $OUT/prof_${TAG}_pmc_sq${i}/*.db $OUT/prof_${TAG}_pmc_sq${i}/*/*.db 2>/dev/null | head -1) | grep -E "^kernel|march|resolve|tile_scan|ray_s" > $OUT/${TAG}_pmc_valu_sq${i}.txt
  done
  [ -x tools/valu_rate.out ] && ./tools/valu_rate.out > $OUT/${TAG}_valu_rate.txt 2>&1
  python tools/make_traffic.py $OUT/prof_${TAG} > $OUT/${TAG}_traffic.log 2>&1
  cp profiles/pmc_traffic.json $OUT/${TAG}_pmc_traffic.json
fi
head -20 $OUT/${TAG}_kernel_stats_sparse.txt
