// window_select.h — the arithmetic of the exact top-K select behind include/rvb_capi_window.h: the composite key, the digit schedule,
// the walk over a digit histogram to the threshold bucket, the places left behind it, and whether the record number has to decide.
// Integers only: no HIP include, no kernel, no rvb_*, so that a host program can include it alone (tests/cpp/window_select.cpp replays the
// whole select through it).  csrc/window_kernels.hip and csrc/window.hip share it.
//
// THE ORDER.  A record in the window has a key, the bit pattern of its score: a positive float, so keys order as unsigned integers, and
// a key is never 0 (0 is the key of a record outside the window, and no pass counts it).  The list is ordered by the 64-bit composite
//     (key << 32) | ~record          descending: higher score first, equal scores by ascending record number.
// Composites are distinct, so "the `want` highest" is one set, whatever order the hardware counted in.
//
// THE SELECT.  want = min(max_entries, records in the window).  Three passes over the key, most significant digit first, 11 + 11 + 10
// bits: a pass counts, per value of its digit, the keys that agree with the threshold in every digit decided so far; the walk goes
// down from the highest bucket until the places left are used up inside a bucket — that bucket is the threshold's next digit, and the
// keys of the buckets above it are in the list for certain.  After the third pass the threshold key T is known, `above` keys lie above
// it and `ties` are equal to it.  Only where ties > want - above does the record number decide: three more passes of the same kind over
// ~record of the keys equal to T.  Either way the end is one composite: the list is every composite >= it, exactly `want` of them.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RVB_WINDOW_FN __host__ __device__ inline
#else
#define RVB_WINDOW_FN inline
#endif

namespace window_select {

constexpr uint32_t kPasses = 3;                         // per 32-bit word: the key, and ~record where ties decide
constexpr uint32_t kMaxBuckets = 2048;

// digit `pass` (0 = most significant) of a 32-bit word
RVB_WINDOW_FN uint32_t digit_bits(uint32_t pass) { return pass == 2 ? 10u : 11u; }
RVB_WINDOW_FN uint32_t digit_shift(uint32_t pass) { return pass == 0 ? 21u : pass == 1 ? 10u : 0u; }
RVB_WINDOW_FN uint32_t digit_buckets(uint32_t pass) { return 1u << digit_bits(pass); }
RVB_WINDOW_FN uint32_t digit_of(uint32_t word, uint32_t pass) { return (word >> digit_shift(pass)) & (digit_buckets(pass) - 1u); }
// `word` agrees with `prefix` in the digits decided before `pass`
RVB_WINDOW_FN bool agrees(uint32_t word, uint32_t prefix, uint32_t pass)
{
    return pass == 0 || ((word ^ prefix) >> (digit_shift(pass) + digit_bits(pass))) == 0;
}

RVB_WINDOW_FN uint64_t composite(uint32_t key, uint32_t record) { return ((uint64_t) key << 32) | (uint32_t) ~record; }
RVB_WINDOW_FN uint32_t key_of(uint64_t c) { return (uint32_t) (c >> 32); }
RVB_WINDOW_FN uint32_t record_of(uint64_t c) { return ~(uint32_t) c; }

// The state of one select, 32 bytes, in device memory between the passes (the walk runs there) and fetched once at the end.
struct State {
    uint32_t in_window;     // records in the window (the score pass)
    uint32_t want;          // entries of the list: min(max_entries, in_window)
    uint32_t key;           // the threshold key's digits decided so far, the rest 0
    uint32_t above;         // keys above every key that agrees with `key`: listed for certain
    uint32_t ties;          // after the third pass: keys equal to `key`
    uint32_t by_record;     // 1: ties > want - above, the record passes run
    uint32_t word;          // ~record of the threshold's digits decided so far (0 without record passes: every tie is listed)
    uint32_t taken;         // during the record passes: ties above every tie that agrees with `word`
};

// The walk: from the highest bucket down to the one where `left` (>= 1, at most the sum of the histogram) runs out.
struct Walk { uint32_t bucket, before, inside; };      // before: the counts of the buckets above; inside: the bucket's own
RVB_WINDOW_FN Walk walk(const uint32_t * histogram, uint32_t buckets, uint32_t left)
{
    uint32_t before = 0;
    for (uint32_t b = buckets; b-- > 1;) {
        if (before + histogram[b] >= left) return Walk{b, before, histogram[b]};
        before += histogram[b];
    }
    return Walk{0u, before, histogram[0]};
}

// the score pass has counted: how long the list is
RVB_WINDOW_FN void begin(State & s, uint32_t in_window, uint64_t max_entries)
{
    s.in_window = in_window;
    s.want = (uint64_t) in_window < max_entries ? in_window : (uint32_t) max_entries;
    s.key = s.above = s.ties = s.by_record = s.word = s.taken = 0;
}

// is this key counted by key pass `pass`?  (0 is no key)
RVB_WINDOW_FN bool counts_in_key_pass(const State & s, uint32_t key, uint32_t pass) { return key != 0 && agrees(key, s.key, pass); }
// Key pass `pass` has filled its histogram: key_left places are still open among the counted keys (0: nothing to select), and the
// walk for them has ended at `w`.  Behind the last pass the decision whether the record number has to decide.
RVB_WINDOW_FN uint32_t key_left(const State & s) { return s.want - s.above; }
RVB_WINDOW_FN void key_walked(State & s, const Walk & w, uint32_t pass)
{
    s.key |= w.bucket << digit_shift(pass);
    s.above += w.before;
    if (pass + 1 == kPasses) {
        s.ties = w.inside;
        s.by_record = s.ties > s.want - s.above ? 1u : 0u;
    }
}
RVB_WINDOW_FN void key_step(State & s, const uint32_t * histogram, uint32_t pass)
{
    if (s.want != 0) key_walked(s, walk(histogram, digit_buckets(pass), key_left(s)), pass);
}
RVB_WINDOW_FN bool record_passes_needed(const State & s) { return s.by_record != 0; }

// is this record counted by record pass `pass`?  (only ties at the threshold key; the word is ~record)
RVB_WINDOW_FN bool counts_in_record_pass(const State & s, uint32_t key, uint32_t record, uint32_t pass)
{
    return s.by_record && key == s.key && agrees(~record, s.word, pass);
}
RVB_WINDOW_FN uint32_t record_left(const State & s) { return s.want - s.above - s.taken; }
RVB_WINDOW_FN void record_walked(State & s, const Walk & w, uint32_t pass)
{
    s.word |= w.bucket << digit_shift(pass);
    s.taken += w.before;
}
RVB_WINDOW_FN void record_step(State & s, const uint32_t * histogram, uint32_t pass)
{
    if (s.by_record) record_walked(s, walk(histogram, digit_buckets(pass), record_left(s)), pass);
}

// The end of the select: the lowest composite of the list.  Listed: a key that is not 0 whose composite is >= it.
RVB_WINDOW_FN uint64_t threshold(const State & s) { return ((uint64_t) s.key << 32) | s.word; }
RVB_WINDOW_FN bool listed(const State & s, uint32_t key, uint32_t record) { return s.want != 0 && key != 0 && composite(key, record) >= threshold(s); }

} // namespace window_select
