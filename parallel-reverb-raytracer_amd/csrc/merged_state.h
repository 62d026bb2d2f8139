// merged_state.h — the host half of the merged image list made on the device (include/rvb_capi_images.h, MECHANISM): whether the
// winner list in the context describes the candidates on the device, and for which (pair, remove_direct) it was made.  Plain C++: no
// HIP call, no kernel, so a host program can include it alone (tests/cpp/kept_state.cpp does).  The fields are private: the two
// transitions below are the only code that writes them.  The device half, MergedImages of ctx.h, is built on it.
#pragma once

#include <cstdint>

#pragma GCC visibility push(hidden)

class MergedState {
public:
    bool valid() const { return valid_; }
    // entries of the list; read behind serves() or made() only
    uint64_t count() const { return count_; }
    // the cache-hit rule: made "once per (trace or relisten, pair, remove_direct)"
    bool serves(uint64_t pair, bool remove_direct) const { return valid_ && pair_ == pair && remove_direct_ == remove_direct; }

    // "Everything that voids a trace voids the cache: a trace, rvb_relisten, rvb_set_scene, rvb_share_scene, rvb_set_directions*" —
    // and the list on the device is about to be replaced ("the list of another pair replaces it when that pair is configured").
    void void_list() { valid_ = false; }
    // the list of `count` entries for (pair, remove_direct) is on the device: "cached in the context and uploaded once"
    void made(uint64_t pair, bool remove_direct, uint64_t count)
    {
        pair_ = pair;
        remove_direct_ = remove_direct;
        count_ = count;
        valid_ = true;
    }

private:
    bool valid_ = false, remove_direct_ = false;
    uint64_t pair_ = 0, count_ = 0;
};

#pragma GCC visibility pop
