#!/bin/bash
# Developer tool: is the gfx950 code of every kernel the same as at <git-revision>?  Compiles every csrc/*.hip of that revision (git
# archive into a temporary directory) and of the working tree to assembly with the Makefile's flags, drops what differs without the
# code differing (comment lines, .file / .ident / .loc, the lines naming the per-file __hip_cuid_* symbol) and prints `same` or
# `differs` per kernel (its code and its descriptor) and for the rest of each file (header, metadata).  Exit status 1 if any differs.
#   tools/isa_compare.sh <git-revision>
# ISA_COMPARE_VECTOR=1 compares per kernel only what a change of the kernel-argument layout must leave alone: the register, scratch
# and LDS sizes of the descriptor and the sequence of vector / LDS / memory mnemonics (operands ignored); scalar code may differ.
set -e
rev=${1:?usage: tools/isa_compare.sh <git-revision>}
root=$(cd "$(dirname "$0")/.." && pwd)
pkg=parallel-reverb-raytracer_amd
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
mkdir "$tmp/old" "$tmp/asm_old" "$tmp/asm_new"
git -C "$root" archive "$rev" $pkg/csrc include | tar -x -C "$tmp/old"

# every line goes to the section of the symbol it belongs to: a function (from its .type line) and its kernel descriptor
# (.amdhsa_kernel) share one, the lines before the first function and the metadata notes are sections of their own
sections='
/^[ \t]*(;|\/\/)/ || /^[ \t]*\.(file|ident|loc)[ \t]/ || /__hip_cuid_/ { next }
/^[ \t]*\.type[ \t]+[^,]+,@function/ { name = $2; sub(/,.*/, "", name) }
/^[ \t]*\.amdhsa_kernel[ \t]/ { name = $2 }
/^[ \t]*\.amdgpu_metadata/ { name = "(metadata)" }
{ sub(/[ \t]*(;|\/\/).*/, "") }'
if [ -n "$ISA_COMPARE_VECTOR" ]; then
    sections="$sections"'
$1 ~ /^(v_|ds_|global_|buffer_|flat_|scratch_)/ { print name "\t" $1 }
$1 ~ /^\.amdhsa_(next_free_vgpr|accum_offset|private_segment_fixed_size|group_segment_fixed_size|uses_dynamic_stack)$/ { print name "\t" $0 }'
else
    sections="$sections"' { print name "\t" $0 }'
fi

status=0
for src in "$root"/$pkg/csrc/*.hip; do
    f=$(basename "$src" .hip)
    [ -f "$tmp/old/$pkg/csrc/$f.hip" ] || { echo "$f.hip: not in $rev"; continue; }
    make -s -C "$root/$pkg" asm SRC="$tmp/old/$pkg/csrc/$f.hip" OUT="$tmp/asm_old/$f.s" &
    make -s -C "$root/$pkg" asm SRC="$src" OUT="$tmp/asm_new/$f.s"
    wait
    awk -v name="(header)" "$sections" "$tmp/asm_old/$f.s" > "$tmp/old.tsv"
    awk -v name="(header)" "$sections" "$tmp/asm_new/$f.s" > "$tmp/new.tsv"
    while read -r name; do
        if cmp -s <(awk -F'\t' -v n="$name" '$1 == n' "$tmp/old.tsv") <(awk -F'\t' -v n="$name" '$1 == n' "$tmp/new.tsv"); then verdict=same
        else verdict=differs; status=1; fi
        printf '%-20s %-8s %s\n' "$f.hip" "$verdict" "$(echo "$name" | c++filt | cut -c1-140)"
    done < <(cut -f1 "$tmp/old.tsv" "$tmp/new.tsv" | awk '!seen[$0]++')
done
exit $status
