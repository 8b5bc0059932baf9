// stp_layout_cache.h -- the host's memory of what a scratch buffer was carved with (stp_buffers.hip: buffer headers): buffer address ->
// (value, num_rendered of the forward that carved it), least-recently-used entries dropped in batches.  Standard headers only, no HIP:
// tests/cpp/layout_cache_check.cpp includes this one file.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <iterator>
#include <unordered_map>
#include <vector>

namespace stp {

struct LayoutCache {
    struct Entry { uint32_t value; int64_t R; uint64_t tick; };
    std::unordered_map<const void*, Entry> map;
    uint64_t tick = 0;
    static constexpr size_t CAP = 8192;
    void put(const void* p, uint32_t v, int64_t R)
    {
        if (map.size() >= CAP && map.find(p) == map.end()) { // drop the least recently used quarter (forwards whose buffers nobody came back for)
            std::vector<uint64_t> t; t.reserve(map.size());
            for (const auto& kv : map) t.push_back(kv.second.tick);
            std::nth_element(t.begin(), t.begin() + t.size() / 4, t.end());
            const uint64_t cut = t[t.size() / 4];
            for (auto it = map.begin(); it != map.end();) it = it->second.tick <= cut ? map.erase(it) : std::next(it);
        }
        map[p] = Entry{v, R, ++tick};
    }
    bool get(const void* p, int64_t R, uint32_t* v) // R < 0: whatever forward carved the address last (introspection right behind a forward)
    {
        const auto it = map.find(p);
        if (it == map.end() || (R >= 0 && it->second.R != R)) return false;
        it->second.tick = ++tick;
        *v = it->second.value;
        return true;
    }
};

} // namespace stp
