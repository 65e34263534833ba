#!/bin/bash
# The multi-GPU exchange path over a one-rank RCCL communicator (library loaded before torch)
# usage: [ALLL_OUT=<dir>] bash tools/gpu_rccl_self.sh      (output under build/bench by default)
cd "$(dirname "$0")/.."
O=${ALLL_OUT:-build/bench}
mkdir -p $O
timeout -k 10 300 python bench.py --full --rccl-self --no-cpu-baseline --steps 20 --warmup 3 > $O/bench_rccl_self.json 2> $O/bench_rccl_self.err
rc=$?; echo "rccl-self rc=$rc"; tail -3 $O/bench_rccl_self.err
python -c "import json; d=json.load(open('$O/bench_rccl_self.json')); print(d['resample_iters_per_s'], d['config']['exchange'], d['graphs'], d['phase_ms'])"
exit $rc
