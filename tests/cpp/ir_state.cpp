// ir_state — the host half of the impulse-response stage without a GPU: IrState (csrc/ir_state.h) through every transition, one line
// per step with every reader's value.  tests/test_ir_state_host.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer, runs
// it and holds the lines against values written out there.  No argument.
#include "ir_state.h"

#include <cstdio>

namespace {

typedef unsigned long long ull;

const float kArrayA[4] = {}, kArrayB[4] = {};
const ExactList kSpeakers = {false, 4096, 700, 660, 40}, kEars = {true, 512, 1400, 1320, 80};

void show(const char * step, const IrState & s)
{
    std::printf("step %s configured=%d which=%d nimages=%llu merged=%d stale=%d range_pending=%d table_ears=%d tenant=%d prepared=%d", step,
                (int) s.configured(), s.which(), (ull) s.nimages(), (int) s.from_merged_list(), (int) s.host_images_stale(), (int) s.range_pending(),
                s.table_ears(), (int) s.tenant(), (int) s.prepared());
    if (s.tenant() == IrState::FLATTEN_QUERY)
        std::printf(" query_a=%d query_n=%llu query_rate=%g query_bins=%llu", (int) (s.query().host == kArrayA), (ull) s.query().n, s.query().sample_rate, (ull) s.query().bins);
    if (s.prepared())
        std::printf(" hrtf_combined=%d nbins=%llu n=%llu ndiffuse=%llu exact_nimages=%llu", (int) s.exact().hrtf_combined, (ull) s.exact().nbins, (ull) s.exact().n,
                    (ull) s.exact().ndiffuse, (ull) s.exact().nimages);
    std::printf("\n");
}

// the query (kArrayA, 300, 44100): the same, each of the three differing alone, and a null pointer without impulses
void show_resident(const char * step, const IrState & s)
{
    std::printf("resident %s same=%d other_pointer=%d other_n=%d other_rate=%d null=%d\n", step, (int) s.resident(kArrayA, 300, 44100.0f),
                (int) s.resident(kArrayB, 300, 44100.0f), (int) s.resident(kArrayA, 299, 44100.0f), (int) s.resident(kArrayA, 300, 8192.0f), (int) s.resident(nullptr, 0, 44100.0f));
}

void show_prepared_for(const char * step, const IrState & s, uint64_t nbins)
{
    std::printf("prepared_for %s nbins=%d nbins_plus_1=%d\n", step, (int) s.prepared_for(nbins), (int) s.prepared_for(nbins + 1));
}

}  // namespace

int main()
{
    IrState s;
    show("initial", s);
    show_resident("initial", s);
    show_prepared_for("initial", s, 0);

    // the configuration
    s.configure(1, 40, false);
    show("configure", s);
    s.configure(3, 7, true);
    show("configure_gathered", s);
    s.images_fetched();
    show("images_fetched", s);
    s.drop_configuration();
    show("drop", s);

    // the table's ears: two, then one ear's table under a configuration with a prepared list
    s.two_ear_table();
    s.configure(3, 40, false);
    s.exact_prepared(kEars);
    show("two_ear_table_prepared", s);
    s.one_ear_table();
    show("one_ear_table", s);

    // the time range
    s.configure(2, 3, false);
    s.range_enqueued();
    show("range_enqueued", s);
    s.range_taken();
    show("range_taken", s);
    s.range_enqueued();
    s.configure(2, 3, false);
    show("range_voided_by_configure", s);

    // a flatten query, then its fill
    s.flatten_queried(kArrayA, 300, 44100.0f, 12345);
    show("flatten_query", s);
    show_resident("flatten_query", s);
    s.flatten_filled();
    show("flatten_fill", s);
    show_resident("flatten_fill", s);
    s.flatten_queried(nullptr, 0, 44100.0f, 1);
    show_resident("flatten_query_null", s);
    // ... then the sort buffers claimed
    s.flatten_queried(kArrayA, 300, 44100.0f, 12345);
    s.sort_buffers_claimed();
    show("query_then_claimed", s);
    show_resident("query_then_claimed", s);

    // a prepared list
    s.exact_prepared(kSpeakers);
    show("prepare", s);
    show_prepared_for("prepare", s, 4096);
    s.sort_buffers_claimed();
    show("prepare_then_claimed", s);
    show_prepared_for("prepare_then_claimed", s, 4096);
    s.exact_prepared(kSpeakers);
    s.void_exact_list();                        // (a successful rvb_ir_accumulate)
    show("prepare_then_accumulate", s);
    show_prepared_for("prepare_then_accumulate", s, 4096);
    s.flatten_queried(kArrayA, 300, 44100.0f, 12345);
    s.void_exact_list();
    show("query_then_accumulate", s);
    show_resident("query_then_accumulate", s);
    s.exact_prepared(kSpeakers);
    show_resident("query_then_prepare", s);
    s.drop_configuration();
    show("prepare_then_drop", s);
    show_prepared_for("prepare_then_drop", s, 4096);
    s.flatten_queried(kArrayA, 300, 44100.0f, 12345);
    s.configure(1, 0, false);
    show("query_then_configure", s);
    show_resident("query_then_configure", s);
    return 0;
}
