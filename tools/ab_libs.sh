#!/bin/bash
# A/B of library builds on the GPU box: bash tools/ab_libs.sh "<bench args>" base build/ab/libX.so ...   (each variant twice, interleaved)
args=$1; shift
out=${BENCH_OUT:-bench_out}/ab
mkdir -p $out
for rep in 1 2; do
for v in "$@"; do
  if [ "$v" = base ]; then unset CP_LIB_PATH; else export CP_LIB_PATH=$PWD/$v; fi
  timeout -k 10 150 python bench.py --full --no-extras --no-cpu-baseline $args > $out/s.json 2> $out/s.err || { echo "FAIL $v"; tail -n 3 $out/s.err; exit 1; }
  python -c "
import json; d=json.load(open('$out/s.json')); k=d['kernels_ms_per_step']
print('%-40s %7.1f  ' % ('$v', d['ms_per_step']) + ' '.join('%s %.1f' % (a[3:], b) for a, b in sorted(k.items(), key=lambda x: -x[1])[:9]))" | tee -a $out/ab.txt
done
done
