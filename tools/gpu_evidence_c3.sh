#!/bin/bash
# GPU-box: PMC passes of the C3 bench workload (-> pmc.json), then the default bench line with
# every leg (--full) reading it, and the same command under rocprofv3 kernel stats (tree already
# through the GPU suite).
# usage: tools/gpu_evidence_c3.sh <tag>      (results under $YRT_OUT_DIR, default bench_out/ in the tree)
export TMPDIR=/tmp
TAG=${1:-r3p}
R=$(cd "$(dirname "$0")/.." && pwd)
O=${YRT_OUT_DIR:-$R/bench_out}
cd $R && mkdir -p $O
bash tools/gpu_pmc.sh $TAG || exit $?
cp $O/pmc_$TAG/pmc.json profiles/pmc_c3.json
cd $R && timeout -k 10 600 python bench.py --full > $O/bench_$TAG.json 2> $O/bench_$TAG.err
rc=$?; echo "bench rc=$rc"; cut -c1-200 $O/bench_$TAG.json
[ $rc -ne 0 ] && exit $rc
cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$TAG -o run -- \
  python3 $R/bench.py --full --no-cpu-baseline > $O/bench_prof_$TAG.json 2> $O/bench_prof_$TAG.err
rc=$?; echo "rocprof rc=$rc"; cut -c1-200 $O/bench_prof_$TAG.json
[ $rc -ne 0 ] && exit $rc
python3 $R/tools/kstats_csv.py $O/prof_$TAG 6
exit 0
