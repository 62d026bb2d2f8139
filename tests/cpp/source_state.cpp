// source_state — the host half of the source directivity and the staging block of a launch of several pairs, without a GPU:
// SourceState (csrc/source_state.h, linked from csrc/source_state.hip) through its refusals, transitions and count check, PairBlock
// and PairLaunch (csrc/ctx.h) through the block's bytes.  Prints one line per fact; tests/test_source_state_host.py builds it with
// AddressSanitizer and UndefinedBehaviorSanitizer, runs it and holds the lines against values written out there.  No argument.
#include "ctx.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

namespace {

const size_t kTableFloats = (size_t) 360 * 180 * 8;        // what a caller passes: RVB_HRTF_ROWS - 1 rows, and not a float more
const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

rvb_source_pattern pattern(float x, float y, float z, float shape)
{
    rvb_source_pattern p = {{x, y, z, kNaN}, {}};          // direction[3] is not inspected
    for (int b = 0; b < 8; ++b) p.shape[b] = shape;
    return p;
}

rvb_source_orientation orientation(float fx, float fy, float fz, float ux, float uy, float uz)
{
    const rvb_source_orientation o = {{fx, fy, fz, kNaN}, {ux, uy, uz, kNaN}};
    return o;
}

bool same(const SourceState & a, const SourceState & b)
{
    return a.patterns.size() == b.patterns.size() && (a.patterns.empty() || !std::memcmp(a.patterns.data(), b.patterns.data(), a.patterns.size() * sizeof(SourcePatternDev)))
           && a.table.size() == b.table.size() && (a.table.empty() || !std::memcmp(a.table.data(), b.table.data(), a.table.size() * sizeof(float)))
           && a.bases.size() == b.bases.size() && (a.bases.empty() || !std::memcmp(a.bases.data(), b.bases.data(), a.bases.size() * sizeof(float)))
           && a.patterns_dirty == b.patterns_dirty && a.table_dirty == b.table_dirty;
}

// what SourceDirectivity::upload does to the host half
void uploaded(SourceState & s)
{
    if (s.patterns_need_upload()) s.patterns_dirty = false;
    if (s.table_needs_upload()) s.table_dirty = false;
}

void show(const char * step, int rc, const SourceState & s)
{
    const SourceShading sh = s.shading();
    std::printf("step %s rc=%d patterns=%zu orientations=%u table_floats=%zu patterns_upload=%d table_upload=%d off=%d\n", step, rc, sh.patterns.size(),
                sh.table_orientations, s.table.size(), (int) s.patterns_need_upload(), (int) s.table_needs_upload(), (int) sh.off());
}

// every refusal on a copy of `base`: the code, whether the copy still equals `base`, the text
void refusals(const char * base_name, const SourceState & base, const std::vector<float> & table)
{
    std::string error;
    const rvb_source_orientation good[2] = {orientation(0, 0, 1, 0, 1, 0), orientation(1, 0, 0, 0, 1, 0)};
    struct { const char * name; rvb_source_pattern second; } bad_patterns[] = {
        {"pattern_nan_shape", pattern(1, 0, 0, kNaN)}, {"pattern_zero", pattern(0, 0, 0, 0.5f)},
        {"pattern_tiny", pattern(1e-30f, 0, 0, 0.5f)}, {"pattern_huge", pattern(3e38f, 0, 0, 0.5f)}};
    for (const auto & bad : bad_patterns) {
        SourceState s = base;
        const rvb_source_pattern two[2] = {pattern(0, 2, 0, 0.25f), bad.second};
        const int rc = s.set_patterns(two, 2, error);
        std::printf("refusal %s %s code=%d unchanged=%d text=%s\n", base_name, bad.name, rc, (int) same(s, base), error.c_str());
    }
    {
        SourceState s = base;
        std::vector<float> bad(table);
        bad[64800 * 8 - 1] = kInf;
        const int rc = s.set_table(bad.data(), good, 1, error);
        std::printf("refusal %s table_inf code=%d unchanged=%d text=%s\n", base_name, rc, (int) same(s, base), error.c_str());
    }
    {
        SourceState s = base;
        const int rc = s.set_table(table.data(), good, 0, error);
        std::printf("refusal %s no_orientations code=%d unchanged=%d text=%s\n", base_name, rc, (int) same(s, base), error.c_str());
    }
    {
        SourceState s = base;
        const rvb_source_orientation two[2] = {good[0], orientation(0, 1, 0, 0, 2, 0)};
        const int rc = s.set_table(table.data(), two, 2, error);
        std::printf("refusal %s up_parallel code=%d unchanged=%d text=%s\n", base_name, rc, (int) same(s, base), error.c_str());
    }
}

void show_block(const char * name, const std::vector<unsigned char> & block)
{
    std::printf("block %s ", name);
    for (unsigned char b : block) std::printf("%02x", b);
    std::printf("\n");
}

}  // namespace

int main()
{
    std::vector<float> table(kTableFloats);
    for (size_t i = 0; i < table.size(); ++i) table[i] = 0.25f + (float) (i % 97) * 0.5f;
    const rvb_source_pattern one[1] = {pattern(0, 2, 0, 0.25f)}, other[1] = {pattern(0, 0, -3, 0.75f)};
    const rvb_source_pattern three[3] = {pattern(1, 0, 0, 0.5f), pattern(0, 1, 0, 0.5f), pattern(0, 0, 1, 0.5f)};
    const rvb_source_orientation orient[3] = {orientation(0, 0, 1, 0, 1, 0), orientation(1, 0, 0, 0, 1, 0), orientation(0, 1, 0, 0, 0, 1)};
    std::string error;

    // refusals, from each of the three states a context can be in
    SourceState off, with_patterns, with_table;
    with_patterns.set_patterns(one, 1, error);
    uploaded(with_patterns);
    with_table.set_table(table.data(), orient, 2, error);
    uploaded(with_table);
    refusals("off", off, table);
    refusals("patterns", with_patterns, table);
    refusals("table", with_table, table);

    // transitions
    SourceState s;
    show("initial", RVB_OK, s);
    int rc = s.set_patterns(one, 1, error);
    show("off_to_patterns", rc, s);
    std::printf("form direction=%g,%g,%g,%g shape0=%g\n", s.patterns[0].direction[0], s.patterns[0].direction[1], s.patterns[0].direction[2],
                s.patterns[0].direction[3], s.patterns[0].shape[0]);
    uploaded(s);
    show("uploaded", RVB_OK, s);
    rc = s.set_patterns(one, 1, error);
    show("same_patterns_again", rc, s);
    rc = s.set_patterns(other, 1, error);
    show("other_patterns", rc, s);
    uploaded(s);
    rc = s.set_table(table.data(), orient, 2, error);
    show("patterns_to_table", rc, s);
    std::printf("table first=%g last=%g basis0=%g,%g,%g\n", s.table.front(), s.table.back(), s.bases[0], s.bases[1], s.bases[2]);
    uploaded(s);
    show("table_uploaded", RVB_OK, s);
    rc = s.set_table(table.data(), orient, 2, error);
    show("same_table_again", rc, s);
    uploaded(s);
    rc = s.set_patterns(one, 1, error);
    show("table_to_patterns", rc, s);
    uploaded(s);
    rc = s.set_table(nullptr, nullptr, 0, error);
    show("null_table_while_patterns_on", rc, s);
    rc = s.set_patterns(nullptr, 1, error);
    show("null_patterns", rc, s);
    rc = s.set_table(table.data(), orient, 1, error);
    uploaded(s);
    rc = s.set_table(nullptr, orient, 1, error);
    show("null_table_while_table_on", rc, s);

    // "n for npairs pairs"
    struct { const char * name; const rvb_source_pattern * patterns; uint64_t n; } sets[] = {{"1", one, 1}, {"3", three, 3}, {"2", three, 2}};
    for (const auto & set : sets) {
        SourceState c;
        error.clear();
        c.set_patterns(set.patterns, set.n, error);
        rc = c.check_counts("rvb_trace", 3, error);
        std::printf("counts patterns %s_for_3 code=%d text=%s\n", set.name, rc, error.c_str());
        error.clear();
        c.set_table(table.data(), orient, set.n, error);
        rc = c.check_counts("rvb_reshade", 3, error);
        std::printf("counts orientations %s_for_3 code=%d text=%s\n", set.name, rc, error.c_str());
    }

    // the staging block of three pairs, then new microphones
    const float mics[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9}, sources[9] = {-1, -2, -3, -4, -5, -6, -7, -8, -9}, new_mics[9] = {10, 11, 12, 13, 14, 15, 16, 17, 18};
    std::printf("block_bytes %zu %zu\n", PairBlock::bytes(3), PairBlock::bytes(1));
    std::vector<unsigned char> block(PairBlock::bytes(3), 0xAB);
    PairBlock::fill(block.data(), mics, sources, 3);
    show_block("staged", block);
    PairBlock::fill_mics(block.data(), new_mics, 3);
    show_block("restaged", block);
    std::printf("block_ranges_offset %zu\n", (size_t) (static_cast<const unsigned char *>(PairBlock::ranges(block.data(), 3)) - block.data()));

    // one pair: the owner stages nothing and leaves the launch's pointers alone
    PairLaunch launch;
    TraceArgs a = {};
    const hipError_t e = launch.stage(mics, sources, 1, nullptr, a);
    std::printf("one_pair error=%d block=%d geom=%d direct=%d range=%d event=%d pointers=%d\n", (int) e, launch.block.block.p != nullptr, launch.geom.p != nullptr,
                launch.direct.p != nullptr, launch.range.p != nullptr, launch.block.free.h != nullptr,
                a.pair_mics != nullptr || a.pair_sources != nullptr || a.direct != nullptr || a.time_range != nullptr);
    return 0;
}
