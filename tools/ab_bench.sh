#!/bin/bash
# A/B timing of two builds of liballl.so on one box: build/ab/liballl_A.so vs liballl_B.so,
# alternating bench.py runs of config M (no CPU baseline; VARIANTS="A B C" for more builds).
# usage: [ALLL_OUT=<dir>] bash tools/ab_bench.sh [rounds] [bench args]    (output under build/bench by default)
cd "$(dirname "$0")/.."
R=${1:-3}; shift
O=${ALLL_OUT:-build/bench}
mkdir -p $O
for i in $(seq $R); do
  for v in ${VARIANTS:-A B}; do
    ALLL_LIB_AB=build/ab/liballl_$v.so timeout -k 10 200 python bench.py --full --no-cpu-baseline "$@" > $O/ab_$v$i.json 2> $O/ab_$v$i.err || exit $?
    python3 -c "
import json; d=json.load(open('$O/ab_$v$i.json'))
print('$v$i iters/s %.0f  phases %s  eval %.1f us b2b %s'%(d['resample_iters_per_s'],
 {k:round(v*1e3,1) for k,v in d['phase_ms'].items()}, d['roofline']['eval_ms_in_loop']*1e3, d['roofline'].get('eval_ms_back_to_back')))"
  done
done
