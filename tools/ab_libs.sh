#!/bin/bash
# A/B of library builds on the GPU box: bash tools/ab_libs.sh "<bench args>" base build/ab/libX.so base:own_pack=0 ...   (each variant
# three times, interleaved; `lib:name=value` runs that library with the tunable set, cp_set_option; every run dumps its outputs and
# keeps its result line as run_<variant>_<rep>.json, and the last line says whether all variants returned the same arrays, bit for bit)
args=$1; shift
out=${BENCH_OUT:-bench_out}/ab
mkdir -p $out
for rep in 1 2 3; do
for v in "$@"; do
  lib=${v%%:*}; opt=; tag=$(basename $lib .so)
  if [ "$lib" != "$v" ]; then opt="--opt ${v#*:}"; tag=${tag}_$(echo ${v#*:} | tr '=' '_'); fi
  if [ "$lib" = base ]; then unset CP_LIB_PATH; else export CP_LIB_PATH=$PWD/$lib; fi
  timeout -k 10 150 python bench.py --full --no-extras --no-cpu-baseline --dump-outputs $out/dump_$tag $opt $args > $out/s.json 2> $out/s.err || { echo "FAIL $v"; tail -n 3 $out/s.err; exit 1; }
  cp $out/s.json $out/run_${tag}_$rep.json
  python -c "
import json; d=json.load(open('$out/s.json')); k=d['kernels_ms_per_step']
print('%-40s %7.1f  ' % ('$v', d['ms_per_step']) + ' '.join('%s %.1f' % (a[3:], b) for a, b in sorted(k.items(), key=lambda x: -x[1])[:9]))" | tee -a $out/ab.txt
done
done
python -c "
import glob, os
import numpy as np
dirs = sorted(glob.glob('$out/dump_*'))
same = all(np.array_equal(np.load(f), np.load(os.path.join(d, os.path.basename(f)))) for d in dirs[1:] for f in glob.glob(dirs[0] + '/*.npy'))
print('outputs of %s: %s' % (' '.join(os.path.basename(d) for d in dirs), 'identical' if same else 'DIFFERENT'))" | tee -a $out/ab.txt
