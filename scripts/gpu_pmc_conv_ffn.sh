#!/bin/bash
# PMC sets over the 3x3 conv family (pconv) and the encoder FFN, summaries as JSON for profiles/.
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p ${OUT:-bench_out}
KB="gemm --only 3x3" PROF_TAG=pconv bash scripts/gpu_pmc_sets.sh > ${OUT:-bench_out}/pmc_pconv.txt 2>&1 || { tail -20 ${OUT:-bench_out}/pmc_pconv.txt; exit 1; }
cat ${OUT:-bench_out}/pmc_pconv.txt
python3 scripts/pmc_summary.py ${OUT:-bench_out}/pmc_pconv --min-us 20 --json ${OUT:-bench_out}/pmc_pconv.json > /dev/null
KB="ffn" PROF_TAG=ffn bash scripts/gpu_pmc_sets.sh > ${OUT:-bench_out}/pmc_ffn.txt 2>&1 || { tail -20 ${OUT:-bench_out}/pmc_ffn.txt; exit 2; }
cat ${OUT:-bench_out}/pmc_ffn.txt
python3 scripts/pmc_summary.py ${OUT:-bench_out}/pmc_ffn --min-us 20 --json ${OUT:-bench_out}/pmc_ffn.json > /dev/null
