// trace_state — the host half of the trace stage without a GPU: TraceState (csrc/trace_state.h) through every transition, one line per
// step with every reader's value.  tests/test_trace_state_host.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer, runs
// it and holds the lines against values written out there.  No argument.
#include "trace_state.h"

#include <cstdio>

namespace {

typedef unsigned long long ull;

void show(const char * step, const TraceState & s)
{
    std::printf("step %s traced=%d npairs=%llu rays=%llu nreflections=%llu ray_offset=%llu pair=%llu fetched=%d count_holds=%d\n", step, (int) s.traced(),
                (ull) s.npairs(), (ull) s.rays(), (ull) s.nreflections(), (ull) s.ray_offset(), (ull) s.pair(), (int) s.fetched(), (int) s.live_count_holds());
}

// a finished trace of two pairs whose count holds, its small block fetched
TraceState fetched_trace()
{
    TraceState s;
    s.begin();
    s.finished(2, 128, 5, 1000, true);
    s.small_fetched();
    return s;
}

}  // namespace

int main()
{
    TraceState s;
    show("initial", s);

    // a trace whose shadow stage wrote the final records, then one with a directivity pass behind it
    s.begin();
    show("begin", s);
    s.finished(2, 128, 5, 1000, true);
    show("finished", s);
    s.small_fetched();
    show("fetched", s);
    s.begin();
    s.finished(1, 64, 5, 0, false);
    show("finished_count_does_not_hold", s);

    // what follows a fetched block
    s = fetched_trace();
    s.records_rewritten();
    show("fetched_then_rewritten", s);
    s = fetched_trace();
    s.select_pair(1);
    show("fetched_then_select_1", s);
    s.records_rewritten();
    show("select_1_then_rewritten", s);
    s = fetched_trace();
    s.select_pair(1);
    s.begin();
    show("fetched_then_begin", s);
    s.finished(2, 128, 5, 1000, false);
    show("select_1_then_next_trace", s);

    // the scene or the directions change behind a finished trace; the next trace has other sizes
    s = fetched_trace();
    s.select_pair(1);
    s.inputs_changed();
    show("inputs_changed", s);
    s.begin();
    s.finished(3, 21, 9, 77, true);
    show("inputs_changed_then_finished", s);
    return 0;
}
