# Round-3 evidence for profiles/ (GPU box: bash tools/profile_r03.sh; then python3 tools/collect_profiles_r03.py here).
# Kernel stats of the bench lines, HBM-side traffic (separate PMC passes, gfx950 correction applied by the
# collector), SQ counters of the headline / config-4 / config-5 kernels, the un-profiled default line, and
# the headline at 8 M training points (table beyond the Infinity Cache).
set -x
O=gpurun_out/r03/prof
mkdir -p $O
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
B="python3 bench.py --cpu-sample 0 --no-secondary"
rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_c2 -- $B > $O/stats_c2.json 2> $O/stats_c2.err
for c in 3 4 5; do
  rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_c$c -- $B --config $c --steps 5 > $O/stats_c$c.json 2> $O/stats_c$c.err
done
rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_dropin -- $B --route dropin --steps 10 > $O/stats_dropin.json 2> $O/stats_dropin.err
for c in 2 4 5; do
  rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/fetch_c$c -- $B --config $c --steps 3 --warmup 1 > $O/fetch_c$c.json 2> $O/fetch_c$c.err
  rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/write_c$c -- $B --config $c --steps 3 --warmup 1 > $O/write_c$c.json 2> $O/write_c$c.err
  rocprofv3 --pmc SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_ANY SQ_WAVES --output-format csv -d $O/sq1_c$c -- $B --config $c --steps 3 --warmup 1 > $O/sq1_c$c.json 2> $O/sq1_c$c.err
  rocprofv3 --pmc SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_SALU SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_INSTS_VMEM SQ_LDS_ADDR_CONFLICT --output-format csv -d $O/sq2_c$c -- $B --config $c --steps 3 --warmup 1 > $O/sq2_c$c.json 2> $O/sq2_c$c.err
done
rocprofv3 --pmc TCC_EA0_RDREQ_sum TCC_HIT_sum TCC_MISS_sum --output-format csv -d $O/tcc_c2 -- $B --steps 3 --warmup 1 > $O/tcc_c2.json 2> $O/tcc_c2.err
rocprofv3 --pmc GRBM_GUI_ACTIVE --output-format csv -d $O/grbm_c2 -- $B --steps 3 --warmup 1 > $O/grbm_c2.json 2> $O/grbm_c2.err
$B --points 8000000 > $O/bench_8M.json 2> $O/bench_8M.err
$B --points 4000000 > $O/bench_4M.json 2> $O/bench_4M.err
python3 bench.py --full > $O/bench_default.json 2> $O/bench_default.err
find $O -name "*kernel_trace.csv" -size +2000k -delete
find $O -name "*.csv" -size +3000k -delete
ls $O | head -50
