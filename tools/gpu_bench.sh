#!/bin/bash
# GPU-box: full default bench line (--full), then the same command under rocprofv3 kernel trace.
# usage: tools/gpu_bench.sh <tag>      (results under $YRT_OUT_DIR, default bench_out/ in the tree)
R=$(cd "$(dirname "$0")/.." && pwd)
O=${YRT_OUT_DIR:-$R/bench_out}
mkdir -p $O
export TMPDIR=/tmp
TAG=${1:-r01}
cd $R && timeout -k 10 600 python bench.py --full > $O/bench_$TAG.json 2> $O/bench_$TAG.err
rc=$?; echo "bench rc=$rc"; cat $O/bench_$TAG.json; tail -5 $O/bench_$TAG.err
[ $rc -ne 0 ] && exit $rc
cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv rocpd -d $O/prof_$TAG -o run -- \
  python3 $R/bench.py --full --no-cpu-baseline > $O/bench_prof_$TAG.json 2> $O/bench_prof_$TAG.err
rc=$?; echo "rocprof rc=$rc"; cat $O/bench_prof_$TAG.json
find $O/prof_$TAG -name "*stats*" | head
exit $rc
