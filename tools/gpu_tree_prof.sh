set -o pipefail
cd "$(dirname "$0")/.." && mkdir -p bench_out && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d bench_out/prof_lds -o run -- python bench.py --full --game atari --no-cpu --steps 3 --warmup 1 --pipeline-moves 0 > bench_out/p1.log 2>&1 || { tail -20 bench_out/p1.log; exit 1; }
MZ_RTREE_HBM=1 timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d bench_out/prof_hbm -o run -- python bench.py --full --game atari --no-cpu --steps 3 --warmup 1 --pipeline-moves 0 > bench_out/p2.log 2>&1 || { tail -20 bench_out/p2.log; exit 1; }
find bench_out/prof_lds bench_out/prof_hbm -name "*kernel_stats.csv" | xargs -I{} sh -c 'echo {}; head -8 {}'
