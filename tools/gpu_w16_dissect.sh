#!/bin/bash
# conv5 + max alone on the queue (B = 250, N = 1024) under each build of the library given, in the order given:
#   tools/gpu_w16_dissect.sh geoa3_amd/lib_parent geoa3_amd/lib_w16cut1 ...     (directories relative to the repository;
# the phase-cut variants come from tools/build_w16_variants.sh).  Stops at the first build that does not run clean.
# TAPS=1 times the T-Nets' conv3 (wide_split_kernel) instead.
cd "$(dirname "$0")/.."
for d in "$@"; do
  echo -n "$d: "
  GEOA3_LIB_PATH=$PWD/$d/libgeoa3_hip.so timeout -k 10 180 python3 tools/bench_wide16.py 250 1024 ${TAPS:-3} 2>&1 | tail -1
  rc=${PIPESTATUS[0]}
  if [ $rc -ne 0 ]; then echo "exit $rc: stopping"; exit $rc; fi
done
