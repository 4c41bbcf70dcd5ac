#!/bin/bash
# Variant build of the library for A/B timing: tools/build_variant.sh NAME -DFOO=1 ...
# -> khoice_amd/lib/variants/libkhoice_hip_NAME.so ; run with KHOICE_HIP_LIB=<that path>.  Never shipped.
# k_skm_union's switches (kh_skm.hip): -DKH_TUNE_SKM_UNION_PRIO=0..7 (bit mask; shipped 1) -DKH_TUNE_SKM_UNION_PRIO_LEVEL=1..3
#   -DKH_TUNE_SKM_UNION_COMPACT=0|1|2 (shipped 0) -DKH_TUNE_SKM_UNION_LEAN=0 -DKH_TUNE_SKM_UNION_KT=0
#   -DKH_TUNE_SKM_UNION_OVERLAP=0|1|2 -DKH_TUNE_SKM_UNION_CHUNK_REV=0|1 (shipped: see the defaults in kh_skm.hip)
set -e
cd "$(dirname "$0")/.."
python -c 'import sys; from khoice_amd import build as b; print("built", b.build_library(True, f"{b.LIBDIR}/variants/libkhoice_hip_{sys.argv[1]}.so", sys.argv[2:]))' "$@"
