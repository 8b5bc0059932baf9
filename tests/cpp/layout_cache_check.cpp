// layout_cache_check.cpp -- the host cache of what a scratch buffer was carved with (csrc/stp_layout_cache.h), run on the host alone:
// hit / miss by num_rendered, the "whatever forward carved it last" lookup, and the batch eviction of the least recently used entries.
//     g++ -O1 -std=c++17 -fsanitize=address,undefined -I stopthepop-rasterization_amd/csrc tests/cpp/layout_cache_check.cpp -o layout_cache_check && ./layout_cache_check
#include "stp_layout_cache.h"

#include <cstdio>

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

static const void* key(size_t i) { return reinterpret_cast<const void*>((i + 1) * 256); } // (addresses are only compared, never read)

int main()
{
    using stp::LayoutCache;
    const size_t CAP = LayoutCache::CAP;
    uint32_t v = 0;
    {
        LayoutCache c;
        c.put(key(0), 1234u, 1000);
        v = 0; CHECK(c.get(key(0), 1000, &v) && v == 1234u);  // the same R: a hit
        v = 77; CHECK(!c.get(key(0), 999, &v) && v == 77u);   // another forward's R: a miss, *v untouched
        v = 0; CHECK(c.get(key(0), -1, &v) && v == 1234u);    // R < 0: whatever R was stored
        CHECK(!c.get(key(1), -1, &v));                        // an address nobody carved
        c.put(key(0), 5678u, 2000);                           // the address is carved again: the entry is overwritten
        CHECK(c.map.size() == 1 && !c.get(key(0), 1000, &v) && c.get(key(0), 2000, &v) && v == 5678u);
    }
    {
        LayoutCache c;
        for (size_t i = 0; i < CAP; i++) c.put(key(i), (uint32_t)i, (int64_t)i);
        CHECK(c.map.size() == CAP);
        c.put(key(5), 55555u, 5); // overwriting an existing key at capacity evicts nothing
        CHECK(c.map.size() == CAP);
        v = 0; CHECK(c.get(key(5), 5, &v) && v == 55555u);
        CHECK(c.get(key(0), 0, &v) && v == 0u);
        for (size_t i = 1; i < CAP; i++) CHECK(c.map.count(key(i)) == 1);
    }
    {
        LayoutCache c;
        for (size_t i = 0; i < CAP; i++) c.put(key(i), (uint32_t)i, (int64_t)i);
        CHECK(c.get(key(1), 1, &v) && v == 1u);   // touched last before the overflow: the most recently used entry
        c.put(key(CAP), (uint32_t)CAP, (int64_t)CAP); // the (CAP + 1)-th distinct key
        CHECK(c.map.size() <= CAP);
        CHECK(c.map.size() >= CAP / 2);           // (a batch went, not everything)
        v = 0; CHECK(c.get(key(1), 1, &v) && v == 1u);            // the key touched last is still there
        CHECK(!c.get(key(0), -1, &v));                            // the first-inserted, never-touched key is gone
        v = 0; CHECK(c.get(key(CAP), (int64_t)CAP, &v) && v == (uint32_t)CAP); // the new key is there
        v = 0; CHECK(c.get(key(CAP - 1), -1, &v) && v == (uint32_t)(CAP - 1)); // and so is the youngest of the old ones
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
