// sort.hip — the sorts of the host layer: the library's own radix sort behind RVB_SORT=own, the buffers of the (key, value) lists and
// the one sequence every binning path shares, "sorted list and bin boundaries".
#include "ctx.h"

#include <cstdlib>
#include <cstring>

// rocPRIM's radix sort unless RVB_SORT=own asks for the library's own (csrc/radix_sort.hip: same results, kernels that fit beside
// resident path waves; measured 3-4 % slower per IR in the bench pipeline, see the file's header).
bool own_sort_enabled()
{
    static const bool own = getenv("RVB_SORT") && std::strcmp(getenv("RVB_SORT"), "own") == 0;
    return own;
}

// (keys[i], value_base + i) sorted on key bits [begin_bit, end_bit) into (keys_out, values_out); keys_out is always a buffer of n
// words (intermediate passes use it) but holds the sorted keys only if want_keys.
int own_sort(rvb_ctx * ctx, const uint32_t * keys, uint32_t value_base, uint64_t n, int begin_bit, int end_bit,
             uint32_t * keys_out, uint32_t * values_out, bool want_keys)
{
    if (n == 0 || end_bit <= begin_bit) return RVB_OK;
    const int passes = (end_bit - begin_bit + 7) / 8;
    RVB_HIP(fail, ctx, ctx->sort.own_temp.ensure(rvb_radix_sort_temp_bytes(n)));
    uint32_t * tmp_k = nullptr, * tmp_v = nullptr;
    if (passes > 1) {
        RVB_HIP(fail, ctx, ctx->sort.own_keys.ensure(n * 4));
        RVB_HIP(fail, ctx, ctx->sort.own_values.ensure(n * 4));
        tmp_k = ctx->sort.own_keys.as<uint32_t>();
        tmp_v = ctx->sort.own_values.as<uint32_t>();
    }
    // passes alternate A, B, A, ...: the last one must land in the caller's buffers
    const bool last_in_b = ((passes - 1) & 1) != 0;
    uint32_t * ka = last_in_b ? tmp_k : keys_out, * va = last_in_b ? tmp_v : values_out;
    uint32_t * kb = last_in_b ? keys_out : tmp_k, * vb = last_in_b ? values_out : tmp_v;
    const uint32_t * ks = nullptr, * vs = nullptr;
    RVB_HIP(fail, ctx, rvb_radix_sort_pairs(ctx->sort.own_temp.p, ctx->sort.own_temp.cap, keys, nullptr, value_base, ka, va, kb, vb, n,
                                            begin_bit, end_bit, want_keys, &ks, &vs, ctx->stream));
    if (vs != values_out || (want_keys && ks != keys_out)) return fail(ctx, RVB_ERR_HIP, "internal error: radix sort result in the wrong buffer");
    return RVB_OK;
}

int ensure_sort_buffers(rvb_ctx * ctx, uint64_t n)
{
    SortBuffers & b = ctx->sort;
    ctx->ir.sort_buffers_claimed();           // (every caller rewrites the sort buffers: the keys of a size query or a prepared list go)
    RVB_HIP(fail, ctx, b.keys_a.ensure(n * 4));
    RVB_HIP(fail, ctx, b.keys_b.ensure(n * 4));
    RVB_HIP(fail, ctx, b.vals_a.ensure(n * 4));
    RVB_HIP(fail, ctx, b.vals_b.ensure(n * 4));
    RVB_HIP(fail, ctx, b.temp.ensure(rvb_sort_temp_bytes(n)));
    return RVB_OK;
}

// The (key, value) list of n entries in keys_a / vals_a, keys below nkeys in key_bits bits -> the sorted list in keys_b / vals_b and
// bin_starts[2 * nkeys]: where each key's run starts, then where it ends.  RVB_SORT=own takes identity values only: it may serve the
// sort (may_sort_own) where the key pass wrote the entry numbers 0 .. n-1 as values; every other list is rocPRIM's.
// coarse_shift > 0 (rocPRIM's sort only): the list is ordered on key bits [coarse_shift, key_bits) alone — stable, so every run of
// 2^coarse_shift neighbouring keys is contiguous and each key's entries keep their order within it; keys_b holds the whole keys and
// the boundaries are those of key >> coarse_shift, coarse_keys(nkeys, coarse_shift) of them.  Keys that fit into coarse_shift bits
// are one run: the list is copied.
int sort_and_bin(rvb_ctx * ctx, uint64_t n, uint64_t nkeys, int key_bits, bool may_sort_own, int coarse_shift)
{
    SortBuffers & b = ctx->sort;
    const uint64_t nruns = coarse_keys(nkeys, coarse_shift);
    RVB_HIP(fail, ctx, b.bin_starts.ensure(nruns * 8));
    uint32_t * starts = b.bin_starts.as<uint32_t>();
    if (coarse_shift > 0 && key_bits <= coarse_shift) {
        RVB_HIP(fail, ctx, hipMemcpyAsync(b.keys_b.p, b.keys_a.p, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        RVB_HIP(fail, ctx, hipMemcpyAsync(b.vals_b.p, b.vals_a.p, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    } else if (coarse_shift == 0 && may_sort_own && own_sort_enabled()) {
        const int rc = own_sort(ctx, b.keys_a.as<uint32_t>(), 0u, n, 0, key_bits, b.keys_b.as<uint32_t>(), b.vals_b.as<uint32_t>(), true);
        if (rc != RVB_OK) return rc;
    } else {
        rvb_sort_pairs(b.temp.p, b.temp.cap, b.keys_a.as<uint32_t>(), b.keys_b.as<uint32_t>(),
                       b.vals_a.as<uint32_t>(), b.vals_b.as<uint32_t>(), n, coarse_shift, key_bits, ctx->stream);
    }
    RVB_HIP(fail, ctx, hipMemsetAsync(starts, 0xFF, nruns * 4, ctx->stream));
    if (coarse_shift > 0) RVB_HIP(fail, ctx, hipMemsetAsync(starts + nruns, 0, nruns * 4, ctx->stream));
    rvb_launch_bin_starts(b.keys_b.as<uint32_t>(), n, nkeys, starts, starts + nruns, ctx->stream, coarse_shift);
    return RVB_OK;
}
