#!/bin/bash
# Developer tool: gfx950 ISA of the three trace units (trace_kernels.hip: path, image_kernels.hip, shadow_kernels.hip; extra flags pass
# through) -> /tmp/isa/<name>.s, plus per-kernel files.
#   tools/isa.sh <name> [-Dflags...]
set -e
name=$1; shift
mkdir -p /tmp/isa
cd "$(dirname "$0")/../parallel-reverb-raytracer_amd"
: > /tmp/isa/$name.s
for unit in trace_kernels image_kernels shadow_kernels; do
    make -s asm SRC=csrc/$unit.hip OUT=/tmp/isa/$name.$unit.s EXTRA="$*" 2>&1 | grep -E "error" -A3 || true
    cat /tmp/isa/$name.$unit.s >> /tmp/isa/$name.s
done
for k in path image shadow; do
    awk "/^_ZN12_GLOBAL__N_1[0-9]+${k}_[a-z_]*kernel[A-Za-z0-9_]*:/,/s_endpgm/" /tmp/isa/$name.s > /tmp/isa/${name}_$k.s
done
grep -E "vgpr_count|Spill|Reload" /tmp/isa/$name.s | sort | uniq -c
