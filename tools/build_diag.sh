#!/bin/bash
# Diagnostic build with in-kernel phase stamps (-DKH_STAMPS): never shipped, never benchmarked.
# Usage: tools/build_diag.sh ; KHOICE_HIP_LIB=khoice_amd/lib/diag/libkhoice_hip_diag.so python bench.py ...
set -e
cd "$(dirname "$0")/.."
python -c 'from khoice_amd import build as b; print("built", b.build_library(True, f"{b.LIBDIR}/diag/libkhoice_hip_diag.so", ["-DKH_STAMPS"]))'
