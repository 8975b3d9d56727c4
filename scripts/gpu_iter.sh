#!/bin/bash
# One build -> measure iteration on the GPU box: the k_scan_ax parity tests, then the default bench line (--full
# without CPU baseline / PCIe / extra lines) into $OUT_DIR/<tag>.json (OUT_DIR default bench_out).
# Usage: bash scripts/gpu_iter.sh <tag> [bench args...]
cd "$GRAFT_REPO_ROOT"
OUT_DIR=${OUT_DIR:-bench_out}
mkdir -p $OUT_DIR
TAG=$1; shift
timeout -k 10 600 python -u -m pytest tests/test_gpu_ax.py tests/test_gpu_golden.py tests/test_gpu_parity.py -m gpu -x -q \
    --timeout 120 --timeout-method thread -p no:cacheprovider > $OUT_DIR/$TAG.tests.log 2>&1; rc=$?
tail -3 $OUT_DIR/$TAG.tests.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-pcie --no-lf-compare --no-extra "$@" > $OUT_DIR/$TAG.json \
    2> $OUT_DIR/$TAG.err
rc=$?; echo "bench rc=$rc"; exit $rc
