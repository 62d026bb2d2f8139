// ir_state.h — the host half of a context's impulse-response stage (the rvb_ir_* and rvb_flatten* rules of include/rvb_capi.h): the
// configuration, the pending time range, the ears of the HRTF table, and what the sort buffers hold.  Plain C++: no HIP call, no
// kernel, so a host program can include it alone (tests/cpp/ir_state.cpp does).  The fields are private: the named transitions below
// are the only code that writes them.  The device half, IrStage of ctx.h, is built on it; the entry points are in ir.hip, flatten.hip
// and images.hip.
#pragma once

#include <cstdint>

#pragma GCC visibility push(hidden)

// The keys of an rvb_flatten size query (keys_a / vals_a; the array itself sits in IrStage::flat_in): the fill that follows for the
// same array finds them and neither uploads nor keys again.
struct FlattenQuery {
    const void * host = nullptr;                 // the caller's array
    uint64_t n = 0, bins = 0;
    float sample_rate = 0.0f;
};

// Exact mode in two steps (rvb_ir_exact_prepare / rvb_ir_exact_fold): what the sorted list in keys_b / vals_b / bin_starts was prepared for.
// `listed` entries per ear: the impulses that carry volume and a tail that matches no bin (live_list, ir.hip), listed <= n; the full
// list of RVB_SORT=own has listed == n and !compacted.  count_valid: the trace's live count sized the list.
// coarse_shift: 0 for a list ordered by bin with boundaries per bin; s > 0 for one ordered by bin >> s only, with boundaries per run of
// 2^s bins (sort_and_bin) — the fold takes the form from here, so it never reads boundaries of the other kind.
struct ExactList {
    bool hrtf_combined = false;
    uint64_t nbins = 0, n = 0, ndiffuse = 0, nimages = 0;
    uint64_t listed = 0;
    bool count_valid = false, compacted = false;
    int coarse_shift = 0;
};

class IrState {
public:
    // The sort buffers have one tenant at a time.  Whoever writes them next claims them first (ensure_sort_buffers), which turns out
    // the tenant; a tenant is recorded behind the work that made it.
    enum Tenant { NOTHING, FLATTEN_QUERY, EXACT_LIST };

    bool configured() const { return configured_; }
    int which() const { return which_; }
    uint64_t nimages() const { return nimages_; }
    // the configuration was made from the merged list on the device (rvb_ir_configure_*_merged): IrStage::images is its gather ...
    bool from_merged_list() const { return from_merged_list_; }
    // ... and IrStage::images_host has not been fetched yet (ir_images_on_host)
    bool host_images_stale() const { return host_images_stale_; }
    // rvb_ir_time_range_begin has enqueued the HRTF time-range pass of the current configuration
    bool range_pending() const { return range_pending_; }
    // ears of the HRTF table on the device: 2 after rvb_ir_configure_hrtf, 1 after the one-ear attenuate calls
    int table_ears() const { return table_ears_; }
    Tenant tenant() const { return tenant_; }
    const FlattenQuery & query() const { return query_; }
    const ExactList & exact() const { return exact_; }
    // the fill that follows a size query of the same array finds it (and its keys) on the device
    bool resident(const void * in, uint64_t n, float sample_rate) const
    {
        return tenant_ == FLATTEN_QUERY && in != nullptr && query_.host == in && query_.n == n && query_.sample_rate == sample_rate;
    }
    bool prepared() const { return tenant_ == EXACT_LIST; }
    // exact() describes a list that was made, prepared still or not (rvb_ir_exact_list_info)
    bool ever_listed() const { return ever_listed_; }
    bool prepared_for(uint64_t nbins) const { return prepared() && exact_.nbins == nbins; }

    // A successful rvb_ir_configure_*: replaces the previous configuration as a whole.  gathered: the list comes from the merged list
    // on the device, no host copy exists yet.
    void configure(int which, uint64_t nimages, bool gathered)
    {
        which_ = which;
        nimages_ = nimages;
        from_merged_list_ = host_images_stale_ = gathered;
        configured_ = true;
        void_exact_list();
        range_pending_ = false;
    }
    // The records, the selected pair, the table image or the merged list that the configuration was made for are no longer: it goes,
    // and with it a prepared list (which names those records and folds with that table).
    void drop_configuration()
    {
        configured_ = false;
        from_merged_list_ = false;
        void_exact_list();
    }
    void images_fetched() { host_images_stale_ = false; }
    // One ear's table in its slot of the device image: not what rvb_ir_configure_hrtf(table == NULL) may reuse.
    void one_ear_table() { table_ears_ = 1; drop_configuration(); }
    void two_ear_table() { table_ears_ = 2; }
    void range_enqueued() { range_pending_ = true; }
    void range_taken() { range_pending_ = false; }

    // ensure_sort_buffers, on every call: the caller is about to rewrite the buffers (or they are about to be freed)
    void sort_buffers_claimed() { tenant_ = NOTHING; }
    void flatten_queried(const void * in, uint64_t n, float sample_rate, uint64_t bins)
    {
        tenant_ = FLATTEN_QUERY;
        query_.host = in;
        query_.n = n;
        query_.sample_rate = sample_rate;
        query_.bins = bins;
    }
    // the fill's sort consumes the keys
    void flatten_filled() { tenant_ = NOTHING; }
    void exact_prepared(const ExactList & list) { tenant_ = EXACT_LIST; exact_ = list; ever_listed_ = true; }
    // include/rvb_capi.h: rvb_ir_accumulate voids a prepared list, whatever its mode and its nbins.  The keys of a size query stay:
    // RVB_IR_FAST with up to 8 speakers does not touch the sort buffers.
    void void_exact_list() { if (tenant_ == EXACT_LIST) tenant_ = NOTHING; }

private:
    bool configured_ = false, from_merged_list_ = false, host_images_stale_ = false, range_pending_ = false, ever_listed_ = false;
    int which_ = 3;                              // RVB_IR_ALL
    int table_ears_ = 0;
    uint64_t nimages_ = 0;
    Tenant tenant_ = NOTHING;
    FlattenQuery query_;
    ExactList exact_;
};

#pragma GCC visibility pop
