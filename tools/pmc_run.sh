#!/bin/bash
# tools/pmc_run.sh TAG [bench args...] -- rocprofv3 kernel-trace stats + PMC passes of `bench.py --full`.
# Each --pmc set is collected in a run of its own with --kernel-trace only (counters are never combined with
# other trace domains).  Every pass runs under `timeout`: some TA/TCP counter sets have stalled.
# PTK_PMC_SETS=N collects only the first N counter sets (2: FETCH_SIZE and WRITE_SIZE, what TAG_traffic.json needs).
# Output in $PTK_PROF_OUT (default: prof_out/ of the repository): TAG_{stats,pmc,timeline}.txt, TAG_traffic.json,
# prof_TAG_bench.json; summarise further with tools/rocprof_summary.py.
TAG=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
O=${PTK_PROF_OUT:-$R/prof_out}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
timeout 240 rocprofv3 --kernel-trace --stats -d $O/prof_$TAG -o trace -- python $R/bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --no-pipelined "$@" > $O/prof_${TAG}_bench.json 2> $O/prof_$TAG.log
rc=$?; echo "trace rc=$rc"
[ $rc -ne 0 ] && exit $rc  # (nothing more is started on a device after a run that failed or stalled)
i=0
for c in "FETCH_SIZE" "WRITE_SIZE" "TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum" \
         "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT" \
         "SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_LDS SQ_INSTS_SALU SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_INST_CYCLES_VMEM_RD GRBM_GUI_ACTIVE" \
         "SQ_THREAD_CYCLES_VALU SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_WAVE_CYCLES"; do
  [ $i -ge ${PTK_PMC_SETS:-6} ] && break
  i=$((i+1))
  timeout 180 rocprofv3 --kernel-trace --pmc $c -d $O/pmc_${TAG}_$i -o pmc -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-pipelined "$@" > /dev/null 2>> $O/pmc_$TAG.log
  rc=$?; echo "pmc pass $i ($c) rc=$rc"
  [ $rc -ne 0 ] && break
done
# Summarise where the run was and drop the (large) databases.
python $R/tools/rocprof_summary.py stats $O/prof_$TAG/trace_results.db > $O/${TAG}_stats.txt 2>&1
python $R/tools/rocprof_summary.py pmc $O/pmc_${TAG}_*/pmc_results.db > $O/${TAG}_pmc.txt 2>&1
python $R/tools/rocprof_summary.py traffic $O/pmc_${TAG}_1/pmc_results.db $O/pmc_${TAG}_2/pmc_results.db > $O/${TAG}_traffic.json 2>&1
python $R/tools/rocprof_summary.py timeline $O/prof_$TAG/trace_results.db > $O/${TAG}_timeline.txt 2>&1
rm -rf $O/prof_$TAG $O/pmc_${TAG}_*
