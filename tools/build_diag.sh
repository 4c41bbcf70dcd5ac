#!/bin/bash
# Diagnostic build with in-kernel phase stamps (-DKH_STAMPS): never shipped, never benchmarked.
# Usage: tools/build_diag.sh ; KHOICE_HIP_LIB=khoice_amd/lib/diag/libkhoice_hip_diag.so python bench.py ...
#        tools/build_diag.sh wg [-DKH_TUNE_SKM_CLAIM=0 ...]: two stamps per workgroup of the persistent unions instead
#        (-DKH_STAMPS_WG) -> khoice_amd/lib/diag/libkhoice_hip_diag_wg.so; KHOICE_WG_DUMP=file appends one line per
#        workgroup and call, tools/wg_ends.py reads the file.
#        KHOICE_WG_DUMP_SCATTER=file: the same for the workgroups of k_skm_scatter (tools/wg_ends.py file --resident 768).
set -e
cd "$(dirname "$0")/.."
if [ "${1:-}" = wg ]; then
  shift
  python -c 'import sys; from khoice_amd import build as b; print("built", b.build_library(True, f"{b.LIBDIR}/diag/libkhoice_hip_diag_wg.so", ["-DKH_STAMPS", "-DKH_STAMPS_WG"] + sys.argv[1:]))' "$@"
else
  # (extra flags, e.g. -DKH_TUNE_SKM_FULL_ROUNDS=3; KHOICE_STAMP_DUMP=file appends every part's stamps of a call,
  # tools/union_stamps.py reads the union's per-slot intervals from it)
  python -c 'import sys; from khoice_amd import build as b; print("built", b.build_library(True, f"{b.LIBDIR}/diag/libkhoice_hip_diag.so", ["-DKH_STAMPS"] + sys.argv[1:]))' "$@"
fi
