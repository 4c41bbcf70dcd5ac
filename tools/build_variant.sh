#!/bin/bash
# Variant build of the library for A/B timing: tools/build_variant.sh NAME -DFOO=1 ...
# -> khoice_amd/lib/variants/libkhoice_hip_NAME.so ; run with KHOICE_HIP_LIB=<that path>.  Never shipped.
set -e
cd "$(dirname "$0")/.."
python -c 'import sys; from khoice_amd import build as b; print("built", b.build_library(True, f"{b.LIBDIR}/variants/libkhoice_hip_{sys.argv[1]}.so", sys.argv[2:]))' "$@"
