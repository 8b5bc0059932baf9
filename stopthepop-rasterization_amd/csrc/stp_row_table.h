// stp_row_table.h -- what the training-side kernels beside the rasterizer share (stp_adam.hip, stp_densify.hip, stp_mcmc_relocate.hip, stp_reorder.hip;
// stp_mcmc.hip takes f32x4 and aligned16 only): a launch that serves up to ROW_TABLE_ENTRIES tensors through a table of descriptors passed by value, and the
// workgroup scan of the two tile-sum prefixes.
//
// Row table.  A tensor owns consecutive work units of a launch, a workgroup is one unit and finds its tensor by a wave-uniform search for the
// last descriptor whose first unit is not behind its own (row_table_entry; blockIdx.x is in SGPRs: the search is scalar code).  The Adam step
// has a descriptor of its own (AdamDesc: four streams, a learning rate, units counted in elements); the applies of the densification and of the
// 3DGS-MCMC relocation share RowDesc: rows of `row` floats, flattened over (row, element) into items of 16 bytes where the row stream is 16-byte
// aligned (row % 4 == 0 and every pointer of the tensor aligned) and of one float otherwise.  launch_row_tables packs the caller's entries, eight
// per table, and hands every table to the caller's launch.
//
// Tile-sum prefix.  A scan over more items than a workgroup holds runs in three steps: (1) every workgroup sums its tile, (2) one workgroup turns
// the tile sums into their exclusive prefix in place (tile_prefix_kernel), (3) every workgroup scans its tile again from that prefix.  Steps 1 and
// 3 belong to the file that knows what an item is; block_exclusive is the workgroup scan all three use.  The sums are integers: exact whatever
// the order.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "stp_adam_div.h"

namespace stp {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <class... T> inline bool aligned16(const T*... p) { return ((reinterpret_cast<uintptr_t>(p) | ...) & 15u) == 0; }

constexpr int ROW_BLOCK = 256;        // threads of a workgroup of every kernel here and of the kernels that use block_exclusive
constexpr int ROW_TABLE_ENTRIES = 8;  // descriptors of a launch

// the entry of workgroup `unit`: the last of the table's first n whose first unit is <= unit (wave-uniform)
template <class Table> __device__ __forceinline__ auto row_table_entry(const Table& table, const int n, const uint32_t unit) -> decltype((table.t[0]))
{
    int ti = 0;
#pragma unroll
    for (int i = 1; i < ROW_TABLE_ENTRIES; i++)
        if (i < n && unit >= table.t[i].first_unit) ti = i;
    return table.t[ti];
}

constexpr int ROW_PIECES = 4;                            // items a thread owns in its unit
constexpr uint32_t ROW_UNIT = ROW_BLOCK * ROW_PIECES;    // items of a work unit

struct RowDesc {
    const float *p, *m, *v; // the rows that are read (in place: the same arrays as po, mo, vo, hence no __restrict__ in the kernels); m, v: both or neither
    float *po, *mo, *vo;    // the rows that are written
    uint32_t row, items;    // floats per row; items of the rows the work is flattened over (floats, or 16-byte pieces where wide)
    uint32_t first_unit, wide;
    int32_t role;           // the caller's (0: a plain tensor)
    AdamDivisor div;        // e / row
};
struct RowTable {
    RowDesc t[ROW_TABLE_ENTRIES];
};

// the launches of an apply over all entries (StpDensifyTensor or StpMcmcTensor), eight per launch.  rows: the rows the work is flattened over
// (rows * row < 2^31: checked by the caller); in_place: the *_out pointers are not looked at.  launch(table, n, units) launches one table;
// returns the launches made, *err = the launch error that ended them early (or hipSuccess).
template <class Entry, class Launch>
int launch_row_tables(const int n_tensors, const Entry* tensors, const uint32_t rows, const bool in_place, hipError_t* err, Launch launch)
{
    *err = hipSuccess;
    int launches = 0;
    for (int next = 0; next < n_tensors;) {
        RowTable table{};
        int n = 0;
        uint32_t units = 0;
        for (; next < n_tensors && n < ROW_TABLE_ENTRIES; next++) {
            const Entry& t = tensors[next];
            RowDesc& d = table.t[n++];
            d.p = t.param; d.m = t.exp_avg; d.v = t.exp_avg_sq;
            d.po = in_place ? const_cast<float*>(d.p) : t.param_out;
            d.mo = in_place ? const_cast<float*>(d.m) : t.exp_avg_out;
            d.vo = in_place ? const_cast<float*>(d.v) : t.exp_avg_sq_out;
            d.row = (uint32_t)t.row;
            d.role = t.role;
            d.wide = t.row % 4 == 0 && aligned16(d.p, d.m, d.v, d.po, d.mo, d.vo);
            const uint32_t numel = rows * d.row;
            d.items = d.wide ? numel >> 2 : numel;
            d.first_unit = units;
            d.div = adam_divisor(d.row);
            units += (d.items + ROW_UNIT - 1) / ROW_UNIT;
        }
        launch(table, n, units);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) { *err = e; return launches; }
        launches++;
    }
    return launches;
}

__device__ __forceinline__ uint32_t wave_shfl_up(const uint32_t v, const int d) { return __shfl_up(v, d, 64); }
__device__ __forceinline__ uint64_t wave_shfl_up(const uint64_t v, const int d)
{
    const uint32_t lo = __shfl_up((uint32_t)v, d, 64), hi = __shfl_up((uint32_t)(v >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}

// the exclusive prefix of v over the workgroup's ROW_BLOCK threads and (total) the workgroup's sum; T: uint32_t or uint64_t; lds: ROW_BLOCK / 64 words
template <class T> __device__ __forceinline__ T block_exclusive(const T v, T* lds, T& total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = wave_shfl_up(inc, d);
        if (lane >= (uint32_t)d) inc += up;
    }
    __syncthreads(); // (lds may still be read from an earlier call)
    if (lane == 63u) lds[wave] = inc;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < ROW_BLOCK / 64; w++) {
        const T t = lds[w];
        if (w < wave) before += t;
        total += t;
    }
    return before + inc - v;
}

// one workgroup: tile_sums[0 .. tiles) -> their exclusive prefix, in place, and, where asked, total_out[0] = their sum; a thread owns `chunk`
// consecutive entries (chunk = ceil(tiles / ROW_BLOCK))
template <class T>
__global__ void __launch_bounds__(ROW_BLOCK) tile_prefix_kernel(const uint32_t tiles, const uint32_t chunk, T* __restrict__ tile_sums, T* __restrict__ total_out)
{
    __shared__ T lds[ROW_BLOCK / 64];
    const uint32_t first = threadIdx.x * chunk;
    T sum = 0;
    for (uint32_t k = first; k < first + chunk && k < tiles; k++) sum += tile_sums[k];
    T total;
    T run = block_exclusive(sum, lds, total);
    for (uint32_t k = first; k < first + chunk && k < tiles; k++) {
        const T t = tile_sums[k];
        tile_sums[k] = run;
        run += t;
    }
    if (total_out && threadIdx.x == 0) total_out[0] = total;
}

} // namespace stp
