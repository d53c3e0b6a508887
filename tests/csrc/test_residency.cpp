// Host unit test of retinaface_amd/csrc/residency.h (the engine's per-allocation residency cache) with a fake runtime lookup that
// counts its calls and a fake clock.
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -o test_residency tests/csrc/test_residency.cpp && ./test_residency
#include <cstdio>
#include <random>
#include <vector>

#include "../../retinaface_amd/csrc/residency.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

// the "runtime": a list of live allocations; host ranges answer -1 and are not cacheable
struct Alloc { uintptr_t base; size_t bytes; int device; bool host; };
struct FakeRuntime {
    std::vector<Alloc> allocs;
    double now = 0.0;
    long lookups = 0;
    rf::ResidencyCache cache;
    bool lookup(uintptr_t a, rf::Residency *out) {
        lookups++;
        for (const Alloc &al : allocs)
            if (a >= al.base && a < al.base + al.bytes) {
                *out = rf::Residency{al.host ? 0 : al.base, al.host ? 0 : al.bytes, al.host ? -1 : al.device, al.device, now};
                return !al.host;
            }
        *out = rf::Residency{0, 0, -7, -7, now};           // unknown to the runtime: an answer, never stored
        return false;
    }
    int where(uintptr_t a) {
        return cache.where(a, [this](uintptr_t p, rf::Residency *out) { return lookup(p, out); }, [this] { return now; });
    }
};

int main() {
    const double ttl = rf::kResidencyTtlUs;
    CHECK(ttl == 2000.0);
    {   // fresh hit, stale hit that still holds, one byte past the end
        FakeRuntime rt;
        rt.allocs = {{0x10000, 0x1000, 3, false}};
        CHECK(rt.where(0x10010) == 3 && rt.lookups == 1 && rt.cache.size() == 1);
        rt.now = ttl;                                           // exactly the TTL old: still young
        CHECK(rt.where(0x10fff) == 3 && rt.lookups == 1);
        CHECK(rt.where(0x11000) == -7 && rt.lookups == 2 && rt.cache.size() == 1);      // one byte past the allocation: a miss
        rt.now = ttl + 1.0;                                     // stale, allocation unchanged: one lookup, same answer, fresh again
        CHECK(rt.where(0x10800) == 3 && rt.lookups == 3 && rt.cache.revalidation_misses() == 0 && rt.cache.size() == 1);
        rt.now = 2 * ttl + 1.0;
        CHECK(rt.where(0x10800) == 3 && rt.lookups == 3);       // re-stamped at ttl + 1: young until 2 ttl + 1
        rt.now = 2 * ttl + 2.0;
        CHECK(rt.where(0x10800) == 3 && rt.lookups == 4);
    }
    {   // stale hit whose owner / extent changed: dropped, counted, replaced by the fresh answer
        FakeRuntime rt;
        rt.allocs = {{0x20000, 0x2000, 1, false}};
        CHECK(rt.where(0x20100) == 1);
        rt.allocs = {{0x20000, 0x2000, 5, false}};              // freed and re-allocated on another device
        rt.now = 10.0;
        CHECK(rt.where(0x20100) == 1 && rt.lookups == 1);       // young: the old answer, by design for at most the TTL
        rt.now = ttl + 1.0;
        CHECK(rt.where(0x20100) == 5 && rt.lookups == 2 && rt.cache.revalidation_misses() == 1 && rt.cache.size() == 1);
        CHECK(rt.where(0x21fff) == 5 && rt.lookups == 2);       // the replacement is cached and fresh
        rt.allocs = {{0x20000, 0x800, 5, false}};               // same owner, smaller extent
        rt.now = 2 * ttl + 2.0;
        CHECK(rt.where(0x20100) == 5 && rt.lookups == 3 && rt.cache.revalidation_misses() == 2);
        CHECK(rt.where(0x20800) == -7 && rt.lookups == 4);      // beyond the new extent
        rt.allocs = {{0x20000, 0x800, 0, true}};                // now host memory: stale entry dropped, the answer not stored
        rt.now = 3 * ttl + 3.0;
        CHECK(rt.where(0x20100) == -1 && rt.lookups == 5 && rt.cache.revalidation_misses() == 3 && rt.cache.size() == 0);
    }
    {   // non-cacheable answers are returned and never stored
        FakeRuntime rt;
        rt.allocs = {{0x30000, 0x1000, 2, true}};
        for (int k = 0; k < 3; k++) CHECK(rt.where(0x30000 + k) == -1);
        CHECK(rt.where(0x99999) == -7);
        CHECK(rt.lookups == 4 && rt.cache.size() == 0);
    }
    {   // a new allocation evicts every cached entry it overlaps, on either side, and no other
        std::mt19937 rng(11);
        for (int round = 0; round < 200; round++) {
            FakeRuntime rt;
            // 12 disjoint cached allocations [base, base + len) on a 0x1000 grid
            std::vector<Alloc> old;
            for (int k = 0; k < 12; k++) old.push_back(Alloc{(uintptr_t)(0x100000 + k * 0x1000), (size_t)(0x400 + rng() % 0xc00), k % 4, false});
            rt.allocs = old;
            for (const Alloc &a : old) CHECK(rt.where(a.base) == a.device);
            CHECK(rt.cache.size() == 12);
            // they are all freed; one new allocation covers a random span.  Even rounds meet it while the old entries are young (the
            // miss path inserts), odd rounds after the TTL (a stale entry under the probed address is re-validated, dropped and replaced)
            const bool stale = round & 1;
            const uintptr_t nb = 0x100000 + rng() % 0xb000;
            const size_t nlen = 1 + rng() % 0x3000;
            const uintptr_t probe = nb + rng() % nlen;
            const Alloc *hit = nullptr;
            for (const Alloc &a : old) if (probe >= a.base && probe < a.base + a.bytes) hit = &a;
            rt.allocs = {{nb, nlen, 6, false}};
            rt.now = stale ? ttl + 1.0 : 0.0;
            const long before = rt.lookups;
            const int got = rt.where(probe);
            if (hit && !stale) {                                // a young entry of the freed allocation answers for at most the TTL, by design
                CHECK(got == hit->device && rt.lookups == before && rt.cache.size() == 12);
                continue;
            }
            CHECK(got == 6 && rt.lookups == before + 1 && rt.cache.revalidation_misses() == (hit ? 1 : 0));
            size_t survivors = 0;
            for (const Alloc &a : old) survivors += !(a.base < nb + nlen && nb < a.base + a.bytes);
            CHECK(rt.cache.size() == survivors + 1);
            rt.now = stale ? ttl : 0.0;                         // every entry young again: answers below come from the cache or from a miss
            for (const Alloc &a : old) {
                const bool overlapped = a.base < nb + nlen && nb < a.base + a.bytes;
                const long l0 = rt.lookups;
                const int w = rt.where(a.base);
                if (!overlapped) CHECK(w == a.device && rt.lookups == l0);             // untouched
                else if (a.base >= nb) CHECK(w == 6 && rt.lookups == l0);              // evicted; the address lies in the new allocation
                else CHECK(w == -7 && rt.lookups == l0 + 1);                           // evicted; the address is nobody's now
            }
        }
    }
    {   // entry 4098 empties the map first; clear forgets everything
        FakeRuntime rt;
        for (int k = 0; k < 4097; k++) rt.allocs.push_back(Alloc{(uintptr_t)(0x1000000 + (uintptr_t)k * 0x100), 0x100, 1, false});
        for (int k = 0; k < 4097; k++) CHECK(rt.where(rt.allocs[k].base) == 1);
        CHECK(rt.cache.size() == 4097 && rt.lookups == 4097);
        rt.allocs.push_back(Alloc{0x9000000, 0x100, 2, false});
        CHECK(rt.where(0x9000000) == 2 && rt.cache.size() == 1);
        CHECK(rt.where(rt.allocs[0].base) == 1 && rt.lookups == 4099 && rt.cache.size() == 2);
        rt.cache.clear();
        CHECK(rt.cache.size() == 0);
        CHECK(rt.where(0x9000000) == 2 && rt.lookups == 4100);
    }
    std::printf(fails ? "FAILED (%d)\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
