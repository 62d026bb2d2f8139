// resident_cache.h — device copies of vectors the mirror handed out (OPT-IN: RVB_API_RESIDENT=1), behind one owner.
// The reference's API moves every stage's result through std::vector and its implementation uploads whatever vector it is handed,
// stage by stage (rayverb.cpp:863-875).  That is what the mirror does by default: every stage uploads the vector it receives.
//
// With RVB_API_RESIDENT=1 in the environment the CALLER PROMISES not to edit a vector the mirror returned between the
// stages of the sequence Raytracer::getAllRaw -> Attenuator::attenuate -> fixPredelay -> flattenImpulses (cmd/main.cpp:241-298
// does not).  The producer of a vector then remembers where its device copy lives, keyed by the vector's buffer (address,
// element count, element size), and the next stage uses that copy instead of uploading.  A changed length or address is caught by
// the key and a sample of the contents (every `stride`-th element and the last; production: 251) is compared as a courtesy, but an
// in-place edit that misses the sample is NOT seen — checking all of a 0.8 GB vector costs as much host-memory traffic as
// uploading it, which is why the mechanism is a promise the caller opts into and not the default.
//
// A copy is OWNED (allocated for its entry: a shared_ptr whose deleter the caller supplies) or BORROWED (an owner's trace buffer:
// current only while that owner's trace count is the stamp the entry was made with).  The cache holds one reference to an owned copy
// and find() hands the reader another (the lease): dropping, replacing or evicting an entry lets go of the cache's reference only,
// so the deleter runs once, when the last holder is done — never under a reader.  A deleter may run under the cache's one mutex
// and must not call back into the cache.
#pragma once

#include <cstddef>
#include <cstdint>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

class ResidentCache {
public:
    // what find() answers; false when nothing was found
    struct Found {
        void * device = nullptr;          // device copy of the `device_count` leading elements
        size_t device_count = 0;
        bool owned = false;
        std::shared_ptr<void> lease;      // owned: keeps `device` alive for as long as the reader holds it
        explicit operator bool() const { return device != nullptr; }
    };

    // off: nothing is remembered or found.  byte_cap: owned device copies kept at a time (bytes), oldest dropped first
    ResidentCache(bool on, size_t byte_cap, size_t stride) : on_(on), byte_cap_(byte_cap), stride_(stride) {}

    // `copy` holds all `count` elements of the vector at `host`; with the cache off it is simply let go
    void remember_owned(const void * host, size_t count, size_t elem, std::shared_ptr<void> copy)
    {
        void * const device = copy.get();
        if (on_) insert(Entry{host, count, elem, device, count, std::move(copy), nullptr, 0, {}});
    }

    // `device` holds the `device_count` leading elements and belongs to `owner`, whose trace_count() the caller read as `stamp`
    // before it read the buffer
    void remember_borrowed(const void * host, size_t count, size_t elem, void * device, size_t device_count, const void * owner, uint64_t stamp)
    {
        if (on_) insert(Entry{host, count, elem, device, device_count, nullptr, owner, stamp, {}});
    }

    // the entry of `host` if it is current and the vector still reads as it did; an entry of that address that fails is dropped
    Found find(const void * host, size_t count, size_t elem)
    {
        Found f;
        if (!on_ || !host) return f;
        std::lock_guard<std::mutex> lock(mutex_);
        for (auto it = entries_.begin(); it != entries_.end(); ++it) {
            if (it->host != host) continue;
            const bool current = it->copy || traces_[it->owner] == it->stamp;
            if (current && it->count == count && it->elem == elem && it->sample == sample(host, count, elem)) {
                f.device = it->device; f.device_count = it->device_count; f.owned = (bool) it->copy; f.lease = it->copy;
            } else
                entries_.erase(it);
            break;
        }
        return f;
    }

    // the caller edited the vector and its device copy alike
    void resample(const void * host, size_t count, size_t elem)
    {
        std::lock_guard<std::mutex> lock(mutex_);
        for (Entry & e : entries_)
            if (e.host == host && e.count == count && e.elem == elem) e.sample = sample(host, count, elem);
    }

    // traces `owner` has started
    uint64_t trace_count(const void * owner)
    {
        std::lock_guard<std::mutex> lock(mutex_);
        return traces_[owner];
    }

    // `owner` is about to trace (or goes away): its trace buffer no longer holds what its borrowed entries describe
    void owner_traces(const void * owner)
    {
        std::lock_guard<std::mutex> lock(mutex_);
        ++traces_[owner];
        for (auto it = entries_.begin(); it != entries_.end();)
            if (!it->copy && it->owner == owner) it = entries_.erase(it); else ++it;
    }

    // lets go of owned copies, oldest first, until at most `keep_bytes` of them remain; whether anything was let go
    bool evict(size_t keep_bytes)
    {
        std::lock_guard<std::mutex> lock(mutex_);
        size_t held = 0;
        for (const Entry & e : entries_) if (e.copy) held += e.device_count * e.elem;
        bool freed = false;
        for (auto it = entries_.end(); held > keep_bytes && it != entries_.begin();) {      // from the back: the oldest
            if (!(--it)->copy) continue;
            held -= it->device_count * it->elem;
            it = entries_.erase(it);
            freed = true;
        }
        return freed;
    }

private:
    struct Entry {
        const void * host;                // the vector's buffer
        size_t count, elem;               // elements, bytes per element
        void * device;
        size_t device_count;
        std::shared_ptr<void> copy;       // owned: the cache's reference to `device`; borrowed: empty
        const void * owner;               // borrowed: whose trace buffer this is ...
        uint64_t stamp;                   // ... and that owner's trace count when the buffer was read: a later trace voids the entry
        std::vector<unsigned char> sample;
    };

    std::vector<unsigned char> sample(const void * host, size_t count, size_t elem) const
    {
        std::vector<unsigned char> s;
        s.reserve((count / stride_ + 2) * elem);
        const unsigned char * p = static_cast<const unsigned char *>(host);
        for (size_t i = 0; i < count; i += stride_) s.insert(s.end(), p + i * elem, p + (i + 1) * elem);
        if (count) s.insert(s.end(), p + (count - 1) * elem, p + count * elem);
        return s;
    }

    void insert(Entry e)
    {
        e.sample = sample(e.host, e.count, e.elem);
        {
            std::lock_guard<std::mutex> lock(mutex_);
            for (auto it = entries_.begin(); it != entries_.end();)      // a buffer address names one vector at a time
                if (it->host == e.host) it = entries_.erase(it); else ++it;
            entries_.push_front(std::move(e));
        }
        (void) evict(byte_cap_);
    }

    const bool on_;
    const size_t byte_cap_, stride_;
    std::mutex mutex_;
    std::list<Entry> entries_;            // newest first
    std::map<const void *, uint64_t> traces_;
};
