// kept_state — the host halves of a kept trace and of the merged image list without a GPU: KeptState (csrc/kept_state.h) and
// MergedState (csrc/merged_state.h) through every transition, one line per step with every reader's value.
// tests/test_kept_state_host.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer, runs it and holds the lines against
// values written out there.  No argument.
#include "kept_state.h"
#include "merged_state.h"

#include <cstdio>

namespace {

void show(const char * step, const KeptState & s, int released = -1)
{
    std::printf("kept %s keeping=%d keeping_listener=%d valid=%d listener_valid=%d", step, (int) s.keeping(), (int) s.keeping_listener(), (int) s.valid(),
                (int) s.listener_valid());
    if (released >= 0) std::printf(" release=%d", released);
    std::printf("\n");
}

// every (pair, remove_direct) the steps ask for
void show(const char * step, const MergedState & m)
{
    std::printf("merged %s valid=%d count=%llu serves_0_0=%d serves_0_1=%d serves_1_0=%d serves_1_1=%d\n", step, (int) m.valid(), (unsigned long long) m.count(),
                (int) m.serves(0, false), (int) m.serves(0, true), (int) m.serves(1, false), (int) m.serves(1, true));
}

// a finished trace made under rvb_keep_paths(keep)
KeptState kept_trace(int keep)
{
    KeptState s;
    s.ask(keep);
    s.trace_begins();
    s.trace_taken();
    return s;
}

}  // namespace

int main()
{
    KeptState s;
    show("initial", s);
    s.trace_begins();
    s.trace_taken();
    show("initial_then_trace", s);

    // asked, then traced
    const char * asked[] = {nullptr, "ask_1", "ask_2", "ask_3"}, * taken[] = {nullptr, "ask_1_then_trace", "ask_2_then_trace", "ask_3_then_trace"};
    const char * off[] = {nullptr, "trace_1_then_ask_0", "trace_2_then_ask_0", "trace_3_then_ask_0"};
    for (int keep = 1; keep <= 3; ++keep) {
        s = KeptState();
        show(asked[keep], s, s.ask(keep));
        s.trace_begins();
        s.trace_taken();
        show(taken[keep], s);
        show(off[keep], s, s.ask(0));
    }

    // the listener bit dropped behind a trace that kept it: valid until the next trace
    s = kept_trace(3);
    show("trace_3_then_ask_1", s, s.ask(1));
    s.trace_begins();
    show("trace_3_ask_1_then_begins", s);
    s.trace_taken();
    show("trace_3_ask_1_then_trace", s);
    // ... and dropped, then switched off
    s = kept_trace(3);
    s.ask(1);
    show("trace_3_ask_1_then_ask_0", s, s.ask(0));

    // asking again for what is kept, and for more than was kept
    s = kept_trace(1);
    show("trace_1_then_ask_1", s, s.ask(1));
    show("trace_1_then_ask_3", s, s.ask(3));

    // a trace that fails: it begins and is never taken
    s = kept_trace(3);
    s.trace_begins();
    show("trace_3_then_failed_trace", s);

    // switched off and on again between two traces: nothing is valid until the next trace
    s = kept_trace(3);
    s.ask(0);
    show("trace_3_ask_0_then_ask_3", s, s.ask(3));

    MergedState m;
    show("initial", m);
    m.made(1, true, 7);
    show("made_1_1_7", m);
    m.void_list();
    show("void", m);
    m.made(0, false, 3);
    show("void_then_made_0_0_3", m);
    m.void_list();
    m.void_list();
    show("void_twice", m);
    return 0;
}
