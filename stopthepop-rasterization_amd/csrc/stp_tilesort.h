// stp_tilesort.h -- the per-tile (depth, id) sort in LDS and the entry gather behind it, as device code shared by
// tile_sort_gather_kernel (stp_tilesort.hip) and the prologue of the hierarchical forwards (stp_render_hier.inc, RenderArgs::fused_gather).
// Both run it for one tile per 256-thread workgroup; keys, list and entry records come out the same bit for bit.
#pragma once

#include "stp_device.h"

namespace stp {

// Entries a workgroup sorts in LDS with the bitonic network (8 KB of keys): the tiles with up to TS_SMALL entries.  Longer lists are
// tile_sort_gather_kernel<TS_CAP, TS_SMALL>'s (stp_tilesort.hip).
constexpr int TS_SMALL = 1024;

// What the per-tile sort writes, and what the entry records are gathered from.
struct EntryGather {
    uint64_t* keys;           // in: grouped by tile, out: sorted
    uint32_t* point_list;     // likewise
    const float4* gpack;      // nullptr: no entry records (GLOBAL mode)
    const float* features;
    int gx;                   // tiles per row
    int cull_mask;            // leave every entry's 16-bit sub-tile mask in entF.w (see write_entry): 1 = hierarchical mode's 4x4 culling, 2 = the k-buffer kernel's sub-tile pre-test
    float4* entA; float4* entB; float4* entC; float4* entD; float4* entF;
};

// What the gather costs (round 4, C2-full, sort stage 0.330 ms, timing ablations, two alternating rounds): the sub-tile masks 15 us, the
// colour read 22, the entry stores 48 (240 MB: the HBM floor of that part), the bitonic network 37; the rest is key / list / gpack IO.
__device__ __forceinline__ void write_entry(const EntryGather& a, size_t i, int id, int tile)
{
    const float4* __restrict__ gp = a.gpack + 4 * (size_t)id; // one 64-byte line written by preprocess_kernel
    const float4 pa = gp[0], pb = gp[1], pc = gp[2], pd = gp[3];
    const float3 col = make_float3(a.features[3 * (size_t)id], a.features[3 * (size_t)id + 1], a.features[3 * (size_t)id + 2]);
    a.entA[i] = pa;
    a.entB[i] = pb;
    a.entC[i] = make_float4(pc.x, pc.y, pc.z, __int_as_float(id));
    a.entD[i] = pd;
    float spare = 0.0f;
    if (a.cull_mask) spare = __uint_as_float(subtile_mask(a.cull_mask, pd, make_float2(pc.y, pc.z), tile % a.gx, tile / a.gx)); // (stp_device.h)
    a.entF[i] = make_float4(col.x, col.y, col.z, spare);
}

// Sorts tile `tile`'s segment [range.x, range.x + n), n >= 1, by (depth bits, Gaussian id) in s_key (room for n keys rounded up to a power
// of two: 8 KB for TS_SMALL), writes the sorted keys and list back and, with a.gpack, the list-ordered entry records.  Called by all 256
// threads of the workgroup (it holds workgroup barriers).  Behind it, __threadfence_block() + __syncthreads() before the workgroup reuses
// s_key or reads what it wrote.
__device__ __forceinline__ void tile_sort_gather_lds(const EntryGather& a, uint64_t* s_key, int tile, uint2 range, int n, int tid)
{
    uint64_t* const keys = a.keys + range.x;
    uint32_t* const list = a.point_list + range.x;
    int m = 2;
    while (m < n) m <<= 1;
    const uint64_t tile_bits = keys[0] & 0xFFFFFFFF00000000ull;
    for (int i = tid; i < m; i += 256) {
        s_key[i] = i < n ? ((keys[i] << 32) | list[i]) : ~0ull;
    }
    __syncthreads();
    // A stage with partner distance j <= 64 keeps every wave inside its own 128 keys (the 64 consecutive comparators c of a wave cover keys
    // [128 (c / 64), 128 (c / 64) + 128)): between two such stages the wave's own LDS order is all the synchronisation there is to need --
    // a workgroup barrier only around the stages that cross waves (3 of the 45 stages of a 512-key network, 6 of 55 at 1024 keys).
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int c = tid; c < (m >> 1); c += 256) {
                const int lo = ((c & ~(j - 1)) << 1) | (c & (j - 1));
                const int hi = lo | j;
                const bool up = (lo & k) == 0;
                const uint64_t x = s_key[lo], y = s_key[hi];
                if ((x > y) == up) { s_key[lo] = y; s_key[hi] = x; }
            }
            const int j_next = j > 1 ? (j >> 1) : k; // (the first distance of the next merge; behind the last stage: the read-out, which crosses waves)
            const bool last = j == 1 && k == m;
            if (j > 64 || j_next > 64 || last) __syncthreads();
            else wave_sync();
        }
    for (int i = tid; i < n; i += 256) {
        const uint64_t k = s_key[i];
        const int id = (int)(uint32_t)k;
        keys[i] = tile_bits | (k >> 32);
        list[i] = (uint32_t)id;
        if (a.gpack) write_entry(a, (size_t)range.x + i, id, tile);
    }
}

} // namespace stp
