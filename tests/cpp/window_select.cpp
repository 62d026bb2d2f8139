// The select of csrc/window_select.h replayed on the host, through the header's own functions in the order the kernels of
// csrc/window_kernels.hip call them (count a digit, walk, move the state on; the record passes only where the header says so; list what the
// header says is listed), against std::sort of the composite keys.  Includes nothing else of the library; tests/test_window_select_host.py
// compiles it with AddressSanitizer and UndefinedBehaviorSanitizer, runs it once and reads one line per (key set, K):
//   select <set> k=<K> n=<keys> in_window=<keys that are not 0> count=<listed> by_record=<0|1> equal=<1: the list is std::sort's>
#include "window_select.h"

#include <algorithm>
#include <cstdio>
#include <functional>
#include <random>
#include <vector>

namespace ws = window_select;

static std::vector<uint64_t> by_sort(const std::vector<uint32_t> & keys, uint64_t k)
{
    std::vector<uint64_t> all;
    for (size_t i = 0; i < keys.size(); ++i)
        if (keys[i]) all.push_back(ws::composite(keys[i], (uint32_t) i));
    std::sort(all.begin(), all.end(), std::greater<uint64_t>());
    if (all.size() > k) all.resize(k);
    return all;
}

static std::vector<uint64_t> by_select(const std::vector<uint32_t> & keys, uint64_t k, ws::State & s)
{
    uint32_t in_window = 0;
    for (uint32_t key : keys) in_window += key != 0;
    ws::begin(s, in_window, k);
    std::vector<uint32_t> histogram(ws::kMaxBuckets);
    for (uint32_t pass = 0; pass < ws::kPasses; ++pass) {
        std::fill(histogram.begin(), histogram.end(), 0u);
        for (uint32_t key : keys)
            if (ws::counts_in_key_pass(s, key, pass)) ++histogram[ws::digit_of(key, pass)];
        ws::key_step(s, histogram.data(), pass);
    }
    if (ws::record_passes_needed(s))
        for (uint32_t pass = 0; pass < ws::kPasses; ++pass) {
            std::fill(histogram.begin(), histogram.end(), 0u);
            for (size_t i = 0; i < keys.size(); ++i)
                if (ws::counts_in_record_pass(s, keys[i], (uint32_t) i, pass)) ++histogram[ws::digit_of(~(uint32_t) i, pass)];
            ws::record_step(s, histogram.data(), pass);
        }
    std::vector<uint64_t> list;
    for (size_t i = 0; i < keys.size(); ++i)
        if (ws::listed(s, keys[i], (uint32_t) i)) list.push_back(ws::composite(keys[i], (uint32_t) i));
    std::sort(list.begin(), list.end(), std::greater<uint64_t>());
    return list;
}

static void run(const char * name, const std::vector<uint32_t> & keys)
{
    for (uint64_t k : {1ull, 2ull, 1023ull, 1024ull}) {
        ws::State s;
        const std::vector<uint64_t> got = by_select(keys, k, s), want = by_sort(keys, k);
        bool equal = got == want && s.want == want.size();
        for (uint64_t c : got) equal = equal && keys[ws::record_of(c)] == ws::key_of(c);
        std::printf("select %s k=%llu n=%zu in_window=%u count=%zu by_record=%u equal=%d\n", name, (unsigned long long) k, keys.size(), s.in_window,
                    got.size(), s.by_record, equal ? 1 : 0);
    }
}

int main()
{
    std::mt19937 rng(20240607u);
    const uint32_t one = 0x3F800000u;                                   // the key of a score of 1

    run("empty", {});
    run("all_zero", std::vector<uint32_t>(5000, 0u));
    run("all_equal", std::vector<uint32_t>(5000, one));
    run("fewer_than_k", {one, 0u, one + 7u, 0x7F800000u, 1u, 0u, one});          // +inf and the smallest denormal among them
    {   // keys that differ only in the lowest bit of each digit: bit 0, bit 10, bit 21 — 700 of each of the eight
        std::vector<uint32_t> keys;
        for (uint32_t i = 0; i < 5600; ++i) keys.push_back(one ^ ((i & 1u) << 0) ^ (((i >> 1) & 1u) << 10) ^ (((i >> 2) & 1u) << 21));
        std::shuffle(keys.begin(), keys.end(), rng);
        run("digit_low_bits", keys);
    }
    {   // every tie at the threshold: 5 keys above, then 3000 equal ones spread among zeros
        std::vector<uint32_t> keys(9000, 0u);
        for (uint32_t i = 0; i < 3000; ++i) keys[3 * i + 1] = one;
        for (uint32_t i = 0; i < 5; ++i) keys[1700 * i + 2] = one + 1u + i;
        run("ties_at_threshold", keys);
    }
    {   // exactly as many ties as places: 1000 above, 24 equal — the record passes stay off at K = 1024
        std::vector<uint32_t> keys(4000, 0u);
        for (uint32_t i = 0; i < 1000; ++i) keys[4 * i] = one + 1u + i;
        for (uint32_t i = 0; i < 24; ++i) keys[4 * i + 1] = one;
        run("ties_fill_exactly", keys);
    }
    {   // seeded: all 31 bits at random (no ties to speak of)
        std::vector<uint32_t> keys(20000);
        for (uint32_t & key : keys) key = rng() & 0x7FFFFFFFu;
        run("seeded_wide", keys);
    }
    {   // seeded: 37 distinct values and zeros (ties everywhere)
        std::vector<uint32_t> values(37);
        for (uint32_t & v : values) v = (rng() & 0x7FFFFFFFu) | 1u;
        std::vector<uint32_t> keys(20000);
        for (uint32_t & key : keys) key = rng() % 3 == 0 ? 0u : values[rng() % values.size()];
        run("seeded_ties", keys);
    }
    {   // seeded: neighbours in the lowest digit around its edges
        std::vector<uint32_t> keys(20000);
        for (uint32_t & key : keys) key = one + rng() % 2050u;
        run("seeded_neighbours", keys);
    }
    return 0;
}
