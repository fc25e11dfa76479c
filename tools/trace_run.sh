#!/bin/bash
# tools/trace_run.sh TAG [bench args...] -- rocprofv3 --kernel-trace --stats of a short `bench.py --full` run (no counters).
# Environment knobs of libptk (PTK_*) pass through.  Output in $PTK_PROF_OUT (default: prof_out/ of the repository):
# TAG_stats.txt, TAG_timeline.txt, TAG_bench.json
TAG=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
O=${PTK_PROF_OUT:-$R/prof_out}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
timeout 240 rocprofv3 --kernel-trace --stats -d $O/prof_$TAG -o trace -- python $R/bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --no-pipelined "$@" > $O/${TAG}_bench.json 2> $O/prof_$TAG.log
echo "trace rc=$?"
python $R/tools/rocprof_summary.py stats $O/prof_$TAG/trace_results.db > $O/${TAG}_stats.txt 2>&1
python $R/tools/rocprof_summary.py timeline $O/prof_$TAG/trace_results.db > $O/${TAG}_timeline.txt 2>&1
rm -rf $O/prof_$TAG
