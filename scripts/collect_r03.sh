#!/bin/bash
# Round-3 evidence for profiles/: the bench line, kernel-trace stats of the bench command, separate PMC passes
# (FETCH_SIZE, WRITE_SIZE, SQ busy counters, the K build's VALU instruction count) over one step, and the
# multi-rank driver forced on one rank with its self-diagnosis.  Run on the GPU box from the repository root:
#   bash scripts/collect_r03.sh <tag>        (writes gpurun_out/<tag>_*)
set -o pipefail
TAG=${1:-r03}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=gpurun_out
rm -rf $OUT/prof_tmp && mkdir -p $OUT/prof_tmp
python3 bench.py --full --steps 10 --warmup 3 > $OUT/${TAG}_bench_N65536.json 2> $OUT/${TAG}_bench.err || exit 1
echo "bench done"
rocprofv3 --kernel-trace --stats -d $OUT/prof_tmp/kt -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/${TAG}_bench_under_trace.json 2> $OUT/${TAG}_kt.err || exit 1
python3 scripts/rocpd_extract.py stats $(find $OUT/prof_tmp/kt -name "*.db" | head -1) $OUT/${TAG}_bench_N65536_kernel_stats.csv > $OUT/${TAG}_kernel_stats_top.txt || exit 1
echo "kernel trace done"
rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/prof_tmp/f -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > $OUT/${TAG}_pmc_fetch.json 2> $OUT/${TAG}_f.err || exit 1
echo "fetch pass done"
rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/prof_tmp/w -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > $OUT/${TAG}_pmc_write.json 2> $OUT/${TAG}_w.err || exit 1
echo "write pass done"
python3 scripts/rocpd_extract.py traffic $(find $OUT/prof_tmp/f -name "*.db" | head -1) $(find $OUT/prof_tmp/w -name "*.db" | head -1) $OUT/${TAG}_roofline_traffic.json > /dev/null || exit 1
python3 scripts/rocpd_extract.py pmc $(find $OUT/prof_tmp/f -name "*.db" | head -1) $OUT/${TAG}_pmc_fetch_summary.txt > /dev/null
python3 scripts/rocpd_extract.py pmc $(find $OUT/prof_tmp/w -name "*.db" | head -1) $OUT/${TAG}_pmc_write_summary.txt > /dev/null
rocprofv3 --kernel-trace --pmc SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F64 GRBM_GUI_ACTIVE -d $OUT/prof_tmp/s -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > $OUT/${TAG}_pmc_sq.json 2> $OUT/${TAG}_s.err || exit 1
python3 scripts/rocpd_extract.py pmc $(find $OUT/prof_tmp/s -name "*.db" | head -1) $OUT/${TAG}_pmc_sq_summary.txt > /dev/null
echo "sq pass done"
rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_WAVES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE -d $OUT/prof_tmp/v -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > $OUT/${TAG}_pmc_valu.json 2> $OUT/${TAG}_v.err || exit 1
python3 scripts/rocpd_extract.py pmc $(find $OUT/prof_tmp/v -name "*.db" | head -1) $OUT/${TAG}_pmc_valu_summary.txt > /dev/null
echo "valu pass done"
GPMI_BENCH_FORCE_DIST=1 python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $OUT/${TAG}_bench_forced_dist.json 2> $OUT/${TAG}_fd.err || exit 1
echo "forced dist done"
rm -rf $OUT/prof_tmp
cat $OUT/${TAG}_kernel_stats_top.txt; cat $OUT/${TAG}_roofline_traffic.json; grep -A8 "rbf_regs" $OUT/${TAG}_pmc_valu_summary.txt | head -20
