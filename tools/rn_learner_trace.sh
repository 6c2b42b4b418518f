#!/bin/bash
# ResNet learner (configs[2] learner leg): kernel trace of the one-launch unroll; per-kernel
# durations and launch gaps.  (The legs that forced the chain + prediction launches and the
# unroll without the fused ADAM blocks went with their switches.)
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
cd "$R" && mkdir -p bench_out/rl && export TMPDIR=/tmp
B="python bench.py --full --net resnet --no-cpu --steps 2 --warmup 1 --pipeline-moves 0 --train-moves 0 --learner-steps 200"
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d bench_out/rl/fuse -o run -- $B > bench_out/rl/fuse.log 2>&1 || { tail -20 bench_out/rl/fuse.log; exit 1; }
python tools/trace_gaps.py bench_out/rl/fuse/run_kernel_trace.csv runroll rp_sample learner_grad
