#!/bin/bash
# rocprofv3 kernel-trace + stats of a short bench run (no PMC counters in this pass).
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export TMPDIR=/tmp
TAG=${PROF_TAG:-r1}
mkdir -p ${OUT:-bench_out}/prof_$TAG
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d ${OUT:-bench_out}/prof_$TAG -o bench -- \
  python3 bench.py --full --steps ${BENCH_STEPS:-5} --warmup 2 --no-cpu-baseline --no-accuracy --no-parity --no-host-input ${BENCH_ARGS:-} > ${OUT:-bench_out}/prof_$TAG/bench_under_rocprof.log 2>&1 \
  || { echo "rocprof run failed"; tail -30 ${OUT:-bench_out}/prof_$TAG/bench_under_rocprof.log; exit 5; }
python3 scripts/kernel_stats_model.py ${OUT:-bench_out}/prof_$TAG --out ${OUT:-bench_out}/prof_$TAG/bench_kernel_stats_model.csv || exit 5
# keep the summaries only: the per-dispatch trace (weights fit included) is large
find ${OUT:-bench_out}/prof_$TAG -name "*kernel_trace*" -delete
find ${OUT:-bench_out}/prof_$TAG -name "*stats*" | head
grep "^{\"metric\"" ${OUT:-bench_out}/prof_$TAG/bench_under_rocprof.log | cut -c1-400
