#!/bin/bash
# Timing-only variants of wide16_kernel (conv5) with phases compiled out: geoa3_amd/lib_w16cutN/ for N in the bit mask of
# pointnet_wide16.hip's GEOA3_W16_CUT (1 no staging, 2 no epilogue, 4 no weight-fragment loads).  Only that one file differs
# from the product build, so the other objects are copied from it.   tools/build_w16_variants.sh [N ...]   (default 1 2 4 7)
# The T-Nets' wide_split_kernel takes the same bit mask (pointnet_wide_split.hip's GEOA3_WSP_CUT): geoa3_amd/lib_wspcutN/ are
# built for the same N.
set -e
cd "$(dirname "$0")/.."
python3 -m geoa3_amd.build
for n in ${@:-1 2 4 7}; do
  d=geoa3_amd/lib_w16cut$n
  mkdir -p $d/obj
  cp -u geoa3_amd/lib/obj/*.o geoa3_amd/lib/obj/*.sha1 $d/obj/
  GEOA3_EXTRA_FILE_FLAGS="pointnet_wide16.hip:-DGEOA3_W16_CUT=$n" python3 -m geoa3_amd.build --variant $d
  d=geoa3_amd/lib_wspcut$n
  mkdir -p $d/obj
  cp -u geoa3_amd/lib/obj/*.o geoa3_amd/lib/obj/*.sha1 $d/obj/
  GEOA3_EXTRA_FILE_FLAGS="pointnet_wide_split.hip:-DGEOA3_WSP_CUT=$n" python3 -m geoa3_amd.build --variant $d
done
