#!/bin/bash
# Builds a variant of the engine library for A/B measurements: scripts/build_variant.sh <name> [extra hipcc flags ...]
# -> build/variants/<name>.so (git-ignored; travels to the GPU box with gpurun; use with EMAT_LIB_PATH).  The shipped library
# stays delphy_amd/libemat_hip.so.  Sources, flags and build id are csrc/Makefile's.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
mkdir -p $ROOT/build/variants
make -B -C $ROOT/delphy_amd/csrc OUT=$ROOT/build/variants/$NAME.so EXTRA_FLAGS="$*"
echo built build/variants/$NAME.so
