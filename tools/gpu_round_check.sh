#!/bin/bash
# One visit to the GPU: parity suite, smoke, the full bench line (GAN step + config 2), the GAN line alone, rocprof
# kernel stats.   usage: bash tools/gpu_round_check.sh [out_dir]      (default prof_out)
set -e
O=${1:-prof_out}
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $O/pytest_gpu.log 2>&1
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1
timeout -k 10 600 python -u bench.py --full > $O/bench_pretrain.json 2> $O/bench_pretrain.err
timeout -k 10 400 python -u bench.py --full --mode gan --no-cpu-baseline > $O/bench_gan.json 2> $O/bench_gan.err
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $O/prof -o run -- python3 -u bench.py --full --no-cpu-baseline --steps 10 > $O/bench_prof.json 2> $O/bench_prof.err
echo done
