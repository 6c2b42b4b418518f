#!/bin/bash
# rocprofv3 kernel-trace summary of the default bench line (configs[1]).
set -o pipefail
cd $(cd "$(dirname "$0")/.." && pwd) && mkdir -p bench_out && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d bench_out/prof_default -o run -- python bench.py --full ${BENCH_ARGS} > bench_out/prof_default.log 2>&1 || { tail -20 bench_out/prof_default.log; exit 1; }
grep '^{' bench_out/prof_default.log | tail -1 | cut -c1-300
head -14 bench_out/prof_default/run_kernel_stats.csv
