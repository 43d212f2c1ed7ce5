#!/usr/bin/env bash
# Build librt_amd.so with extra compile definitions into ray-tracer-from-scratch_amd/lib/ab/
# for in-process A/B (tools/ab.py).   Usage: tools/build_variant.sh NAME [-DX=1 ...]
# The units, compilers and flags are the Makefile's: the definitions reach every unit
# through DEFS, the objects go to build/ab_NAME.
set -eu
cd "$(dirname "$0")/../ray-tracer-from-scratch_amd"
name=$1; shift
B=build/ab_$name
make -s -B -j16 OBJ="$B" LIB="$B" DEFS="$*" "$B/librt_amd.so"
mkdir -p lib/ab
cp "$B/librt_amd.so" "lib/ab/$name.so"
echo "lib/ab/$name.so"
