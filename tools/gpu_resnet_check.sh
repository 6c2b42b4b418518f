set -o pipefail
cd "$(dirname "$0")/.." && mkdir -p bench_out
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > bench_out/gpu_tests.log 2>&1 || { tail -40 bench_out/gpu_tests.log; exit 1; }
tail -2 bench_out/gpu_tests.log
timeout -k 10 300 python bench.py --full --game atari --no-cpu > bench_out/bench_atari.log 2>&1 || { tail -20 bench_out/bench_atari.log; exit 1; }
tail -1 bench_out/bench_atari.log
timeout -k 10 300 python bench.py --full --net resnet --no-cpu > bench_out/bench_resnet.log 2>&1 || { tail -20 bench_out/bench_resnet.log; exit 1; }
tail -1 bench_out/bench_resnet.log
