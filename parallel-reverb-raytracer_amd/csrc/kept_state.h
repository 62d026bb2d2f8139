// kept_state.h — the host half of a kept trace (the rvb_keep_paths, rvb_reshade and rvb_relisten rules of include/rvb_capi.h): what
// the traces of the context are asked to keep, and what the last one did keep.  Plain C++: no HIP call, no kernel, so a host program
// can include it alone (tests/cpp/kept_state.cpp does).  The fields are private: the named transitions below are the only code that
// writes them.  The device half, KeptTrace of ctx.h, is built on it; the entry points are in kept.hip, trace.hip and images.hip.
// listener_valid() implies valid(): every transition that sets the first sets the second, and none clears the second alone.
#pragma once

#pragma GCC visibility push(hidden)

class KeptState {
public:
    static constexpr int kListenerBit = 2;          // RVB_KEEP_LISTENER (ctx.h holds the two against each other)

    // asked for: the buffers come with the next trace, sized for it
    bool keeping() const { return keep_paths_; }
    bool keeping_listener() const { return keep_listener_; }
    // the last trace was made with keeping on, and nothing has voided it since ...
    bool valid() const { return valid_; }
    // ... and with RVB_KEEP_LISTENER
    bool listener_valid() const { return listener_valid_; }

    // rvb_keep_paths.  "`keep` is a set of bits": any bit keeps what rvb_reshade needs, RVB_KEEP_LISTENER "in addition what rvb_relisten
    // needs".  "from now on the traces of this context keep": what the last trace kept stays valid, its listener records too, until
    // the next trace.  0: "the side buffers of an earlier keep are freed ... and rvb_reshade fails until the next kept trace" — returns
    // true: the caller releases the buffers.
    bool ask(int keep)
    {
        keep_paths_ = keep != 0;
        keep_listener_ = (keep & kListenerBit) != 0;
        if (keep) return false;
        valid_ = listener_valid_ = false;
        return true;
    }
    // A trace begins: "the next trace voids the kept state" before it regroups the records; a trace that fails leaves nothing kept.
    void trace_begins() { valid_ = listener_valid_ = false; }
    // A trace has finished: "from now on the traces of this context ... keep what rvb_reshade needs", and with RVB_KEEP_LISTENER set
    // "everything that 1 keeps and in addition what rvb_relisten needs".
    void trace_taken()
    {
        valid_ = keep_paths_;
        listener_valid_ = keep_paths_ && keep_listener_;
    }

private:
    bool keep_paths_ = false, keep_listener_ = false, valid_ = false, listener_valid_ = false;
};

#pragma GCC visibility pop
