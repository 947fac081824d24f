#!/bin/bash
# A/B library variant (float32 state, two ships: the bench workloads only):
#   tools/build_var.sh NAME [SRC] [extra hipcc flags...]
#   -> astro_amd/libastro_hip_NAME.so, for tools/ab.py --libs libastro_hip_NAME
# The compiler and its flags are build()'s own (__graft_entry__.HIPCC, HIPCC_FLAGS).
set -eu
cd "$(dirname "$0")/.."
NAME=$1; shift
SRC=${1:-astro_amd/csrc/astro_kernels.hip}; [ $# -gt 0 ] && shift
HIPCC=$(python -c 'import __graft_entry__ as g; print(g.HIPCC)')
FLAGS=$(python -c 'import __graft_entry__ as g; print(" ".join(g.HIPCC_FLAGS))')
$HIPCC $FLAGS -DASTRO_ONLY_F32_S2 "$@" "$SRC" -o astro_amd/libastro_hip_$NAME.so
