// stp_reorder.hip -- stp_gather_rows: output row s of every tensor and of both its Adam moments is input row index[s], bit for bit -- the move
// behind reorder_gaussians_ (a model sorted along stp_spatial_order's Morton curve) and gather_tensors (any index: a permutation, a subset, a
// list with repeats).  Out of place; no atomics, no host synchronisation, equal inputs give equal bits.
//
// Up to eight tensors go in one launch through the row table of stp_row_table.h, as in the applies of the densification and of the 3DGS-MCMC
// relocation.  The work is flattened over (OUTPUT row, element) into items of 16 bytes where the row stream is 16-byte aligned and of one
// float otherwise: consecutive lanes store consecutive items, and the loads of an output row are one contiguous run of the input.  The row of
// an item comes from the multiply-shift of stp_adam_div.h, not from a division.  An index outside [0, P) is read as the nearest valid row, so
// nothing is ever read out of bounds.  The items are moved as integers: a row may hold int32 or NaN payloads, and nothing computes on them.
#include "stp_internal.h"
#include "stp_row_table.h"

namespace stp {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(ROW_BLOCK) gather_rows_kernel(const RowTable table, const int n_tensors, const uint32_t P, const int32_t* __restrict__ index)
{
    const uint32_t unit = blockIdx.x;
    const RowDesc& d = row_table_entry(table, n_tensors, unit);
    const uint32_t row = d.row, items = d.items;
    const AdamDivisor div = d.div;
    const bool moments = d.m != nullptr;
    const uint32_t base = (unit - d.first_unit) * ROW_UNIT;

#pragma unroll
    for (int k = 0; k < ROW_PIECES; k++) {
        const uint32_t item = base + threadIdx.x + (uint32_t)k * ROW_BLOCK;
        if (item >= items) break;
        const uint32_t e = d.wide ? item << 2 : item;   // the item's first float in the OUTPUT (< M * row < 2^31)
        const uint32_t s = adam_div(e, div), col = e - s * row;
        const int32_t want = index[s];
        const uint32_t i = want < 0 ? 0u : min((uint32_t)want, P - 1u); // (P >= 1)
        const size_t src = (size_t)i * row + col;       // (< P * row < 2^31)
        if (d.wide) { // (16 bytes inside one row: row % 4 == 0, so col % 4 == 0 too)
            reinterpret_cast<u32x4*>(d.po)[item] = reinterpret_cast<const u32x4*>(d.p)[src >> 2];
            if (moments) {
                reinterpret_cast<u32x4*>(d.mo)[item] = reinterpret_cast<const u32x4*>(d.m)[src >> 2];
                reinterpret_cast<u32x4*>(d.vo)[item] = reinterpret_cast<const u32x4*>(d.v)[src >> 2];
            }
        } else {
            reinterpret_cast<uint32_t*>(d.po)[e] = reinterpret_cast<const uint32_t*>(d.p)[src];
            if (moments) {
                reinterpret_cast<uint32_t*>(d.mo)[e] = reinterpret_cast<const uint32_t*>(d.m)[src];
                reinterpret_cast<uint32_t*>(d.vo)[e] = reinterpret_cast<const uint32_t*>(d.v)[src];
            }
        }
    }
}

} // namespace

int launch_gather_rows(int P, int M, const int32_t* index, int n_tensors, const StpGatherTensor* tensors, hipStream_t st, hipError_t* err)
{
    // (the work is flattened over the M OUTPUT rows)
    return launch_row_tables(n_tensors, tensors, (uint32_t)M, false, err, [&](const RowTable& table, int n, uint32_t units) {
        hipLaunchKernelGGL(gather_rows_kernel, dim3(units), dim3(ROW_BLOCK), 0, st, table, n, (uint32_t)P, index);
    });
}

} // namespace stp
