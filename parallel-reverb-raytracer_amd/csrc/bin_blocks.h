// bin_blocks.h — `parts` ranges of whole 64-byte segments (16 floats) over the `bins` bins of a histogram row: the export slices of
// csrc/ir.hip and the chain blocks of csrc/multi.hip.  Integers only, no HIP, no rvb_*.  The caller chooses `parts` (>= 1; multi.hip
// clamps it to the segments there are, ir.hip does not); fewer ranges than asked come out where the rounding fills the row early.
#pragma once

#include <algorithm>
#include <cstdint>

struct BinRange { uint64_t b0, b1; };

struct BinBlocks {
    uint64_t bins, per;                           // per: bins of every range but the last
    BinBlocks(uint64_t bins_, uint64_t parts) : bins(bins_), per(((bins_ + parts - 1) / parts + 15) & ~15ull) {}
    uint64_t count() const { return per ? (bins + per - 1) / per : 0; }
    BinRange range(uint64_t k) const { return BinRange{k * per, std::min(bins, k * per + per)}; }
};
