#!/bin/bash
# Round check on the GPU box: GPU tests, smoke, the default bench with --full (compact line + detail file), then
# rocprofv3 passes of the cfg2 headline (all counter groups), all into $OUT_DIR (default bench_out).
# Usage: bash scripts/round_check.sh [tag]
cd "$GRAFT_REPO_ROOT"
TAG=${1:-r06}
OUT_DIR=${OUT_DIR:-bench_out}
mkdir -p $OUT_DIR
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread -p no:cacheprovider > $OUT_DIR/gpu_tests.log 2>&1; rc=$?
tail -2 $OUT_DIR/gpu_tests.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT_DIR/smoke.log 2>&1 && tail -1 $OUT_DIR/smoke.log && \
timeout -k 10 900 python bench.py --full --detail $OUT_DIR/bench_detail.json > $OUT_DIR/bench_default.log 2>&1 && tail -c 600 $OUT_DIR/bench_default.log && \
rm -rf $OUT_DIR/prof_cfg2 && OUT=$OUT_DIR/prof_cfg2 bash scripts/profile.sh 2> $OUT_DIR/profile_cfg2.err && echo PROFILES_OK
