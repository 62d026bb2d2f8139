// resident_cache — the rules of the mirror's opt-in device-resident handover without a GPU: ResidentCache
// (parallel-reverb-raytracer_amd/host/resident_cache.h) through every rule, one line per step with what find() answered and how
// often a deleter has run so far.  "Device copies" are malloc'ed blocks whose deleter counts and frees, so AddressSanitizer sees a
// second free or a read after the last holder let go.  tests/test_resident_cache_host.py builds it with AddressSanitizer and
// UndefinedBehaviorSanitizer, runs it and holds the lines against values written out there.  No argument.
#include "resident_cache.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

struct Elem { unsigned char b[16]; };
const size_t N = 600, BYTES = N * sizeof(Elem);      // sampled at stride 251: elements 0, 251, 502 and the last, 599
const size_t CAP = 20000;                            // two owned copies of a vector (19200 bytes) fit, three do not

std::vector<int> g_runs;                             // deleter runs per block made
int g_freed = 0;

// a "device copy" of a vector: a block of its own under a counting deleter
std::shared_ptr<void> block()
{
    const size_t id = g_runs.size();
    g_runs.push_back(0);
    void * p = std::malloc(BYTES);
    std::memset(p, 0x5a, BYTES);
    return std::shared_ptr<void>(p, [id](void * q) { ++g_runs[id]; ++g_freed; std::free(q); });
}

std::vector<Elem> vector_of(unsigned char seed)
{
    std::vector<Elem> v(N);
    for (size_t i = 0; i < N; ++i) std::memset(v[i].b, (int) (unsigned char) (seed + i), sizeof(Elem));
    return v;
}

// what find() answered (`device` is what it should have handed out, null if nothing) and the deleter runs so far
void show(const char * step, const ResidentCache::Found & f, const void * device)
{
    std::printf("%s found=%d device_count=%zu owned=%d lease=%d device_ok=%d freed=%d\n", step, (int) (bool) f, f.device_count, (int) f.owned, (int) (bool) f.lease,
                (int) (f.device == device), g_freed);
}

void note(const char * step, const char * what, int value) { std::printf("%s %s=%d freed=%d\n", step, what, value, g_freed); }

bool readable(const void * device)
{
    const unsigned char * p = static_cast<const unsigned char *>(device);
    size_t same = 0;
    for (size_t i = 0; i < BYTES; ++i) same += p[i] == 0x5a;
    return same == BYTES;
}

ResidentCache::Found find(ResidentCache & c, const std::vector<Elem> & v) { return c.find(v.data(), v.size(), sizeof(Elem)); }

}  // namespace

int main()
{
    std::vector<Elem> a = vector_of(1), b = vector_of(2), c = vector_of(3), x = vector_of(4), y = vector_of(5);
    static unsigned char trace_buffer_1[BYTES], trace_buffer_2[BYTES];      // two owners' trace buffers: borrowed, never freed
    const int owner_1 = 0, owner_2 = 0;

    // ---- finding and keys
    ResidentCache keys(true, CAP, 251);
    show("fresh", find(keys, a), nullptr);
    show("null_host", keys.find(nullptr, N, sizeof(Elem)), nullptr);
    std::shared_ptr<void> p = block();
    const void * d = p.get();
    keys.remember_owned(a.data(), N, sizeof(Elem), std::move(p));
    show("remembered", find(keys, a), d);
    show("other_address", find(keys, b), nullptr);
    show("other_address_then_right_key", find(keys, a), d);
    show("other_count", keys.find(a.data(), N - 1, sizeof(Elem)), nullptr);
    show("other_count_then_right_key", find(keys, a), nullptr);
    keys.remember_owned(a.data(), N, sizeof(Elem), block());
    show("other_elem", keys.find(a.data(), N, sizeof(Elem) / 2), nullptr);
    show("other_elem_then_right_key", find(keys, a), nullptr);

    // ---- edits and samples
    ResidentCache edits(true, CAP, 251);
    const size_t sampled[] = {0, 251, 599};
    const char * edited[] = {"edit_0", "edit_251", "edit_599"}, * after[] = {"edit_0_then_again", "edit_251_then_again", "edit_599_then_again"};
    for (int i = 0; i < 3; ++i) {
        edits.remember_owned(a.data(), N, sizeof(Elem), block());
        a[sampled[i]].b[7] ^= 1;
        show(edited[i], find(edits, a), nullptr);
        show(after[i], find(edits, a), nullptr);
    }
    p = block();
    d = p.get();
    edits.remember_owned(a.data(), N, sizeof(Elem), std::move(p));
    a[1].b[7] ^= 1;
    show("edit_1_unseen", find(edits, a), d);               // the documented promise: an edit that misses the sample is NOT seen
    a[251].b[7] ^= 1;
    edits.resample(a.data(), N, sizeof(Elem));
    show("edit_251_then_resample", find(edits, a), d);

    // ---- replacement and eviction
    ResidentCache cap(true, CAP, 251);
    cap.remember_owned(a.data(), N, sizeof(Elem), block());
    p = block();
    d = p.get();
    cap.remember_owned(a.data(), N, sizeof(Elem), std::move(p));
    show("replaced", find(cap, a), d);
    cap.remember_borrowed(x.data(), N, sizeof(Elem), trace_buffer_1, N, &owner_1, cap.trace_count(&owner_1));
    cap.remember_owned(b.data(), N, sizeof(Elem), block());
    show("two_owned_one_borrowed_a", find(cap, a), d);       // 19200 owned bytes: the borrowed 9600 do not count
    cap.remember_owned(c.data(), N, sizeof(Elem), block());
    show("third_owned_a", find(cap, a), nullptr);           // the oldest owned copy went
    note("third_owned_b", "found", (int) (bool) find(cap, b));
    note("third_owned_c", "found", (int) (bool) find(cap, c));
    show("third_owned_borrowed", find(cap, x), trace_buffer_1);
    note("evict_0", "answer", (int) cap.evict(0));
    note("evict_0_b", "found", (int) (bool) find(cap, b));
    note("evict_0_c", "found", (int) (bool) find(cap, c));
    show("evict_0_borrowed", find(cap, x), trace_buffer_1);
    note("evict_0_again", "answer", (int) cap.evict(0));

    // ---- leases
    ResidentCache leases(true, CAP, 251);
    leases.remember_owned(a.data(), N, sizeof(Elem), block());
    ResidentCache::Found held = find(leases, a);
    note("lease_evicted", "answer", (int) leases.evict(0));
    note("lease_evicted_block", "readable", (int) readable(held.device));
    show("lease_evicted_then_find", find(leases, a), nullptr);
    held = ResidentCache::Found();
    note("lease_evicted_then_dropped", "answer", 1);
    leases.remember_owned(a.data(), N, sizeof(Elem), block());
    held = find(leases, a);
    p = block();
    d = p.get();
    leases.remember_owned(a.data(), N, sizeof(Elem), std::move(p));
    note("lease_replaced_block", "readable", (int) readable(held.device));
    show("lease_replaced_then_find", find(leases, a), d);
    held = ResidentCache::Found();
    note("lease_replaced_then_dropped", "answer", 1);

    // ---- owners and stamps
    ResidentCache owners(true, CAP, 251);
    owners.remember_borrowed(x.data(), N, sizeof(Elem), trace_buffer_1, N - 100, &owner_1, owners.trace_count(&owner_1));
    owners.remember_borrowed(y.data(), N, sizeof(Elem), trace_buffer_2, N - 100, &owner_2, owners.trace_count(&owner_2));
    p = block();
    d = p.get();
    owners.remember_owned(a.data(), N, sizeof(Elem), std::move(p));
    show("borrowed", find(owners, x), trace_buffer_1);
    owners.owner_traces(&owner_1);
    show("owner_1_traced_its_borrowed", find(owners, x), nullptr);
    show("owner_1_traced_other_borrowed", find(owners, y), trace_buffer_2);
    show("owner_1_traced_owned", find(owners, a), d);
    const uint64_t stamp = owners.trace_count(&owner_1);      // read, then the owner traces again, then the entry is made
    owners.owner_traces(&owner_1);
    owners.remember_borrowed(x.data(), N, sizeof(Elem), trace_buffer_1, N - 100, &owner_1, stamp);
    show("stale_stamp", find(owners, x), nullptr);
    owners.remember_borrowed(x.data(), N, sizeof(Elem), trace_buffer_1, N - 100, &owner_1, owners.trace_count(&owner_1));
    show("fresh_stamp", find(owners, x), trace_buffer_1);

    // ---- cache off
    ResidentCache off(false, CAP, 251);
    off.remember_owned(a.data(), N, sizeof(Elem), block());
    show("off_owned", find(off, a), nullptr);
    off.remember_borrowed(x.data(), N, sizeof(Elem), trace_buffer_1, N, &owner_1, off.trace_count(&owner_1));
    show("off_borrowed", find(off, x), nullptr);

    // ---- end: every block let go had its deleter run once; the rest are still held by the caches above
    int once = 0, more = 0, still = 0;
    for (int runs : g_runs) { once += runs == 1; more += runs > 1; still += runs == 0; }
    std::printf("end made=%zu once=%d more=%d held=%d freed=%d\n", g_runs.size(), once, more, still, g_freed);
    return 0;
}
