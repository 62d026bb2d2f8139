#!/bin/bash
# Developer tool: is the gfx950 code of every kernel the same as at <git-revision>?  Compiles every csrc/*.hip of that revision (git
# archive into a temporary directory) and of the working tree to assembly with the Makefile's flags, drops what differs without the
# code differing (comment lines, .file / .ident / .loc, the lines naming the per-file __hip_cuid_* symbol), pools the kernels of all
# files of each side and pairs them by symbol, so a kernel is followed from one file to another.  Prints per kernel (its code and its
# descriptor) `same` or `differs` with the file it was found in (old -> new where it moved), and `only in <rev>` / `only in tree` for
# a symbol without a partner.  The rest of a file (header, metadata) is compared for files that exist on both sides.
# Exit status 1 if anything differs or is unpaired.
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

for side in old new; do
    dir=$root/$pkg/csrc
    [ $side = old ] && dir=$tmp/old/$pkg/csrc
    for src in "$dir"/*.hip; do
        echo "SRC=$src OUT=$tmp/asm_$side/$(basename "$src" .hip).s"
    done
done | xargs -P 8 -L 1 make -s -C "$root/$pkg" asm

# Every line goes to the section of the symbol it belongs to: a function (from its .type line, with the .section / .globl / .p2align
# lines that lead up to it) and its kernel descriptor (.amdhsa_kernel) share one; the lines before the first function, the metadata
# notes and what follows the last function are sections of their file.  Labels lose the function's number within its file.
sections='
function out(l,   f) {
    if (!vec) { print side "\t" file "\t" name "\t" l; return }
    split(l, f, " ")
    if (f[1] ~ /^(v_|ds_|global_|buffer_|flat_|scratch_)/) print side "\t" file "\t" name "\t" f[1]
    else if (f[1] ~ /^\.amdhsa_(next_free_vgpr|accum_offset|private_segment_fixed_size|group_segment_fixed_size|uses_dynamic_stack)$/) print side "\t" file "\t" name "\t" l
}
FNR == 1 { file = FILENAME; sub(/.*\//, "", file); sub(/\.s$/, ".hip", file); name = file " (header)"; held = 0 }
/^[ \t]*(;|\/\/)/ || /^[ \t]*\.(file|ident|loc)[ \t]/ || /__hip_cuid_/ { next }
{ sub(/[ \t]*(;|\/\/).*/, ""); gsub(/\.LBB[0-9]+_/, ".LBB_"); gsub(/\.LJTI[0-9]+_/, ".LJTI_"); gsub(/\.Lfunc_begin[0-9]+/, ".Lfunc_begin"); gsub(/\.Lfunc_end[0-9]+/, ".Lfunc_end") }
/^[ \t]*\.(text|globl|protected|weak|hidden|p2align)([ \t]|$)/ || /^[ \t]*\.section[ \t]+\.text/ { hold[++held] = $0; next }
/^[ \t]*\.type[ \t]+[^,]+,@function/ { name = $2; sub(/,.*/, "", name) }
/^[ \t]*\.amdhsa_kernel[ \t]/ { name = $2 }
/^[ \t]*\.section[ \t]+\.AMDGPU\.gpr_maximums/ { name = file " (trailer)" }
/^[ \t]*\.amdgpu_metadata/ { name = file " (metadata)" }
{ for (i = 1; i <= held; ++i) out(hold[i]); held = 0; out($0) }'
vec=0; [ -n "$ISA_COMPARE_VECTOR" ] && vec=1

{ awk -v vec=$vec -v side=old "$sections" "$tmp"/asm_old/*.s; awk -v vec=$vec -v side=new "$sections" "$tmp"/asm_new/*.s; } | awk -F'\t' -v rev="$rev" '
{
    if (!(($1, $3) in body)) {
        where[$1, $3] = $2
        if (!($3 in seen)) { seen[$3]; order[++n] = $3 }
    } else if (index(where[$1, $3], $2) == 0) where[$1, $3] = where[$1, $3] "," $2
    body[$1, $3] = body[$1, $3] $4 "\n"
    files[$1, $2]
}
END {
    for (i = 1; i <= n; ++i) {
        k = order[i]; o = ("old", k) in body; w = ("new", k) in body
        if (o && w) {
            verdict = body["old", k] == body["new", k] ? "same" : "differs"
            at = where["old", k] == where["new", k] ? where["new", k] : where["old", k] " -> " where["new", k]
        } else if (k ~ / \((header|metadata|trailer)\)$/) {
            continue                                 # the rest of a file that one side does not have
        } else {
            verdict = o ? "only in " rev : "only in tree"
            at = o ? where["old", k] : where["new", k]
        }
        if (verdict != "same") status = 1
        printf "%-16s %-44s %s\n", verdict, at, k
    }
    exit status
}' | c++filt | cut -c1-200
exit "${PIPESTATUS[1]}"
