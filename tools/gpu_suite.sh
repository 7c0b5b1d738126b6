#!/bin/bash
# GPU-box: GPU suite and smoke() on the working tree, the default bench line with every leg
# (--full), and the N=2 gloo rehearsal of bench.py --full (two ranks on this one GPU).
# usage: tools/gpu_suite.sh <tag>      (results under $YRT_OUT_DIR, default bench_out/ in the tree)
export TMPDIR=/tmp
TAG=${1:-suite}
R=$(cd "$(dirname "$0")/.." && pwd)
O=${YRT_OUT_DIR:-$R/bench_out}
cd $R && mkdir -p $O
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 200 --timeout-method thread > $O/pytest_gpu_$TAG.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -n 2 $O/pytest_gpu_$TAG.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke_$TAG.log 2>&1
rc=$?; echo "smoke rc=$rc"; tail -n 1 $O/smoke_$TAG.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 400 python bench.py --full > $O/bench_$TAG.json 2> $O/bench_$TAG.err
rc=$?; echo "bench rc=$rc"; cut -c1-200 $O/bench_$TAG.json
[ $rc -ne 0 ] && exit $rc
YRT_DIST_BACKEND=gloo timeout -k 10 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
  --master-port 29541 bench.py --gpus 2 --full --steps 2 --warmup 1 > $O/bench_n2_$TAG.json 2> $O/bench_n2_$TAG.err
rc=$?; echo "n2 rc=$rc"; grep "^{" $O/bench_n2_$TAG.json | cut -c1-200
exit $rc
