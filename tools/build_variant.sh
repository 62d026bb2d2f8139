#!/bin/bash
# Developer tool: builds parallel-reverb-raytracer_amd/_variants/lib_<name>.so = the shipped library with
# the three trace units (trace_kernels.hip, image_kernels.hip, shadow_kernels.hip) recompiled under extra flags (A/B experiments over the same C-ABI, see tools/ab_bench.sh).
#   tools/build_variant.sh <name> [-Dflags...]
set -e
name=$1; shift
cd "$(dirname "$0")/../parallel-reverb-raytracer_amd"
make -j4 librvb_hip.so > /dev/null
make variant NAME="$name" EXTRA="$*" > /dev/null
echo built _variants/lib_$name.so
