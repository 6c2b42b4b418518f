#!/bin/bash
# Instruction / scalar cache counters of the ResNet kernels (one PMC pass).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
cd "$R" && mkdir -p bench_out/ic && export TMPDIR=/tmp
B="python bench.py --full --net resnet --no-cpu --steps 2 --warmup 1 --pipeline-moves 0 --train-moves 0 --learner-steps 20"
timeout -s KILL 120 rocprofv3 --pmc SQC_ICACHE_HITS SQC_ICACHE_MISSES SQC_ICACHE_MISSES_DUPLICATE SQC_DCACHE_HITS SQC_DCACHE_MISSES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM --output-format csv -d bench_out/ic/p1 -o run -- $B > bench_out/ic/p1.log 2>&1 || { tail -20 bench_out/ic/p1.log; exit 1; }
python tools/pmc_kernels.py bench_out/ic/ic.json "$B" bench_out/ic/p1 -- mz_runroll_chain1 mz_runroll_chain_r mz_runroll_pred mz_rsearch_nets mz_rsearch_tree_lds > /dev/null && cat bench_out/ic/ic.json
