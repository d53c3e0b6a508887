// residency.h -- host-only helper of the engine: the per-allocation cache of where a caller's "device" frame pointers live.
// (Header-only and HIP-free so tests/csrc/test_residency.cpp exercises exactly the code the engine runs; the runtime lookup and
// the clock are the caller's.)
#pragma once
#include <cstddef>
#include <cstdint>
#include <iterator>
#include <map>

namespace rf {

// One allocation.  where: -1 = readable in place by the engine's kernels, >= 0 = the ordinal of ANOTHER device; owner: the device
// the runtime reports; checked_us: when the runtime last confirmed it.
struct Residency { uintptr_t base; size_t bytes; int where; int owner; double checked_us; };

// The answer is cached per ALLOCATION (hipMemGetAddressRange: base + size of the allocation the pointer lies in), so a camera
// ring or a frame tensor costs one runtime lookup, not one per frame per call (hipPointerGetAttributes takes the runtime's
// allocation-map lock: ~1 us x 256 frames per super-batch).  Round 4 cached per 2 MiB page and never looked again: a buffer
// freed and re-allocated under the same address on another device kept its old answer.  Now (1) an entry covers
// exactly one allocation, so two small allocations sharing a page cannot alias; (2) an entry is re-validated against the
// runtime once it is older than kResidencyTtlUs -- base, size and owner must still match or the entry is dropped and the
// pointer looked up afresh -- which bounds the lifetime of a stale answer to 2 ms of wall clock and costs one runtime call
// per 2 ms per allocation; (3) rf_invalidate_residency() drops the cache at once for callers that free or re-home frame
// buffers while the handle lives (documented in include/retinaface_amd.h).  Host / managed memory and pointers the runtime
// rejects are never cached.
constexpr double kResidencyTtlUs = 2000.0;

class ResidencyCache {
public:
    // `where` of the allocation address `a` lies in.  lookup(a, &fresh) is one runtime lookup: it fills every field of `fresh`
    // (checked_us included) and returns whether the answer is cacheable (base / bytes valid); now_us() is the clock of checked_us.
    template <typename Lookup, typename Clock> int where(uintptr_t a, Lookup &&lookup, Clock &&now_us) {
        auto it = map_.upper_bound(a);
        if (it != map_.begin()) {
            --it;
            Residency &r = it->second;
            if (a >= r.base && a < r.base + r.bytes) {
                if (now_us() - r.checked_us <= kResidencyTtlUs) return r.where;
                Residency fresh;                                  // stale: the allocation must still be the one that was cached
                const bool cacheable = lookup(a, &fresh);
                if (cacheable && fresh.base == r.base && fresh.bytes == r.bytes && fresh.owner == r.owner) { r.checked_us = fresh.checked_us; return r.where; }
                map_.erase(it);
                revalidation_misses_++;
                if (cacheable) insert(fresh);
                return fresh.where;
            }
        }
        Residency fresh;
        if (lookup(a, &fresh)) insert(fresh);
        return fresh.where;
    }
    void clear() { map_.clear(); }
    size_t size() const { return map_.size(); }
    long revalidation_misses() const { return revalidation_misses_; }      // cached entries whose allocation had changed when they were re-validated

private:
    // a new allocation may overlap stale entries of freed ones: drop every entry that intersects it (both the miss path and the
    // stale-revalidation path come through here)
    void insert(const Residency &fresh) {
        if (map_.size() > 4096) map_.clear();
        auto lo = map_.lower_bound(fresh.base);
        if (lo != map_.begin()) { auto pv = std::prev(lo); if (pv->second.base + pv->second.bytes > fresh.base) lo = pv; }
        while (lo != map_.end() && lo->second.base < fresh.base + fresh.bytes) lo = map_.erase(lo);
        map_[fresh.base] = fresh;
    }
    std::map<uintptr_t, Residency> map_;          // allocation base -> where it lives
    long revalidation_misses_ = 0;
};

}  // namespace rf
