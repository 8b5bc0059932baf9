// stp_knn.hip -- stp_knn_mean_dist2: the mean of the three smallest squared distances from every point of a cloud to the other points, what 3DGS
// code bases import as simple_knn's distCUDA2 to initialise the scales (no counterpart in the reference, which is the rasterizer only).
//
// THE RESULT IS FIXED TO THE BIT.  In float32, every operation rounded to nearest and none contracted:
//     dx = xj - xi, dy = yj - yi, dz = zj - zi        d2 = (dx * dx + dy * dy) + dz * dz
//     b0 <= b1 <= b2 the three smallest d2 over j != i (by index: a duplicate of i is a neighbour at distance 0)
//     out[i] = ((b0 + b1) + b2) / 3.0f
// The three smallest VALUES of a multiset depend neither on how ties are broken nor on the order of the search, so every exact search gives
// the bits of a brute-force evaluation.  The search here skips work box by box, and each skip is conservative IN FLOAT32: the lower bound of a
// box [lo, hi] against a point q (or against a box of points [qlo, qhi]) is, per axis, g = max(lo - q, q - hi, 0) (max(lo - qhi, qlo - hi, 0)),
// and (gx * gx + gy * gy) + gz * gz in the order of d2.  Rounded subtraction, squaring of non-negative numbers and rounded addition are
// monotone, so the bound is <= the COMPUTED d2 of every pair it stands for, and a box is skipped only where bound > b2: nothing that could
// enter the best three is lost.  A NaN bound compares false and skips nothing.
//
// Pipeline, all on the caller's stream, no host synchronisation (nothing about the cloud ever comes to the host), no atomics:
//   1. Per axis: knn_axis_keys (the coordinates as order-preserving integers), rocprim::radix_sort_keys, knn_splitters (the 1023 values that
//      cut the sorted coordinates into 1024 runs of equal length).
//   2. knn_morton: 30-bit Morton codes, 10 bits per axis, of the CELLS the splitters define -- a grid of equal counts per axis, not of equal
//      widths: a few far outliers take no cells from the rest, and a dense cluster gets as many cells as it has points for.  Equal
//      coordinates share a cell, so an axis without extent (a planar or a collinear cloud) contributes one cell and nothing is divided by it.
//      The original index is the value.  (Measured with cells of equal width between the cloud's bounds first: five points at 1e4 put a
//      clustered cloud of 6M points into a handful of cells, the boxes became random subsets of whole clusters, and the search took 4.4 s.)
//   3. rocprim::radix_sort_pairs over the 30 bits, between two buffers of the scratch.
//   4. knn_boxes: gathers the sorted points into 16-byte records (x, y, z, original index) and writes the AABB of every box of KNN_BOX = 256
//      consecutive records.  Morton order makes the boxes compact; the search is exact whatever the order is.
//   5. knn_search: a workgroup owns one box of queries, one query per lane.  It seeds every lane's best three from its own box (all pairs,
//      through LDS), then walks the other boxes outwards -- own - 1, own + 1, own - 2, ... : the near boxes in Morton order first, so that b2
//      shrinks early -- 256 boxes per step, one box-to-box test per lane against the workgroup's largest b2.  The boxes that pass are taken
//      in order: tested once more against the largest b2 of now (the same value in every lane: no divergence), staged in LDS, and scanned by
//      every lane whose own point-to-box bound does not exceed its b2.  The result goes to out[original index].
//
// stp_spatial_order is steps 1-3 by themselves (launch_morton_order, the one function both calls run) and one kernel that hands the sorted
// indices -- and, where asked, the sorted codes -- to the caller: the order a trainer re-sorts its model into (stp_reorder.hip moves the rows).
// There the code IS the result, so include/stp_raster.h fixes it to the bit; it takes clouds from one point on.
#include "stp_internal.h"

#include <rocprim/rocprim.hpp>

namespace stp {

namespace {

constexpr int KNN_BOX = STP_KNN_BOX;         // points per box == lanes per workgroup of knn_boxes and knn_search
constexpr int KNN_BLOCK = 256;               // the streaming kernels
constexpr int KNN_WAVES = KNN_BOX / 64;
constexpr uint32_t KNN_CELLS = 1024;         // cells per axis of the Morton code (10 bits)
constexpr uint32_t KNN_SORT_BITS = 30;
static_assert(KNN_BOX % 64 == 0 && KNN_BOX == KNN_BLOCK, "a box is a whole number of waves, and block_bounds reduces KNN_WAVES of them");

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// min and max per axis over the workgroup; the result is valid in thread 0.  red: 6 * KNN_WAVES floats of LDS.
__device__ __forceinline__ void block_bounds(float lo[3], float hi[3], float* red)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = wave_min(lo[a]);
        hi[a] = wave_max(hi[a]);
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            red[wave * 6 + a] = lo[a];
            red[wave * 6 + 3 + a] = hi[a];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < KNN_WAVES; w++) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                lo[a] = fminf(lo[a], red[w * 6 + a]);
                hi[a] = fmaxf(hi[a], red[w * 6 + 3 + a]);
            }
        }
    }
}

// a float as an unsigned integer of the same order (-0 below +0; NaNs at the two ends)
__device__ __forceinline__ uint32_t ordered_bits(const float v)
{
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(KNN_BLOCK) knn_axis_keys_kernel(const uint32_t P, const float* __restrict__ points, const uint32_t axis, uint32_t* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * (uint32_t)KNN_BLOCK + threadIdx.x; // (< 2^31 + 256)
    if (i < P) keys[i] = ordered_bits(points[3 * (size_t)i + axis]);
}

// the KNN_CELLS - 1 values that cut the sorted coordinates of one axis into KNN_CELLS runs of equal length: splitters[k - 1] = sorted[k P / KNN_CELLS]
__global__ void __launch_bounds__(KNN_BLOCK) knn_splitters_kernel(const uint32_t P, const uint32_t* __restrict__ sorted, uint32_t* __restrict__ splitters)
{
    const uint32_t k = blockIdx.x * (uint32_t)KNN_BLOCK + threadIdx.x;
    if (k >= 1u && k < KNN_CELLS) splitters[k - 1u] = sorted[(uint32_t)(((unsigned long long)k * P) / KNN_CELLS)]; // (k P / KNN_CELLS < P)
}

// 10 bits -> every third bit of 30
__device__ __forceinline__ uint32_t spread10(uint32_t v)
{
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// The cell of a point on an axis is the number of that axis's splitters <= its coordinate, 0 .. KNN_CELLS - 1: equal coordinates share a cell
// (an axis without extent has one), and every cell holds about P / KNN_CELLS points however far the outliers lie.  The code only places the
// point in the sort: any value gives the same results.
__global__ void __launch_bounds__(KNN_BLOCK) knn_morton_kernel(const uint32_t P, const float* __restrict__ points, const uint32_t* __restrict__ splitters,
                                                               uint32_t* __restrict__ keys, uint32_t* __restrict__ values)
{
    __shared__ uint32_t cut[3][KNN_CELLS];
    for (uint32_t e = threadIdx.x; e < 3u * KNN_CELLS; e += KNN_BLOCK) {
        const uint32_t a = e / KNN_CELLS, k = e % KNN_CELLS;
        cut[a][k] = k < KNN_CELLS - 1u ? splitters[a * KNN_CELLS + k] : 0xFFFFFFFFu;
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * (uint32_t)KNN_BLOCK + threadIdx.x; // (< 2^31 + 256)
    if (i >= P) return;
    uint32_t code = 0;
#pragma unroll
    for (uint32_t a = 0; a < 3; a++) {
        const uint32_t key = ordered_bits(points[3 * (size_t)i + a]);
        uint32_t cell = 0;
#pragma unroll
        for (uint32_t step = KNN_CELLS / 2; step > 0; step >>= 1)
            if (cut[a][cell + step - 1u] <= key) cell += step;      // (cell + step - 1 <= KNN_CELLS - 2)
        code |= spread10(cell) << a;
    }
    keys[i] = code;
    values[i] = i;
}

// the result of stp_spatial_order leaves the scratch: order[s] = the row that moves to position s, codes[s] = its code (where asked)
__global__ void __launch_bounds__(KNN_BLOCK) spatial_order_emit_kernel(const uint32_t P, const uint32_t* __restrict__ sorted_values, const uint32_t* __restrict__ sorted_keys,
                                                                       int32_t* __restrict__ order, uint32_t* __restrict__ codes)
{
    const uint32_t s = blockIdx.x * (uint32_t)KNN_BLOCK + threadIdx.x; // (< 2^31 + 256)
    if (s >= P) return;
    order[s] = (int32_t)sorted_values[s];                             // (< P < 2^31)
    if (codes) codes[s] = sorted_keys[s];
}

// workgroup b: the records of sorted positions [b * KNN_BOX, ...) and their AABB
__global__ void __launch_bounds__(KNN_BOX) knn_boxes_kernel(const uint32_t P, const float* __restrict__ points, const uint32_t* __restrict__ order,
                                                            f32x4* __restrict__ records, f32x4* __restrict__ box_lo, f32x4* __restrict__ box_hi)
{
    __shared__ float red[6 * KNN_WAVES];
    const uint32_t s = blockIdx.x * (uint32_t)KNN_BOX + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (s < P) {
        const uint32_t i = order[s];
        f32x4 r;
#pragma unroll
        for (int a = 0; a < 3; a++) r[a] = lo[a] = hi[a] = points[3 * (size_t)i + a];
        r[3] = __uint_as_float(i);
        records[s] = r;
    }
    block_bounds(lo, hi, red);
    if (threadIdx.x == 0) {
        box_lo[blockIdx.x] = f32x4{lo[0], lo[1], lo[2], 0.0f};
        box_hi[blockIdx.x] = f32x4{hi[0], hi[1], hi[2], 0.0f};
    }
}

// THE squared distance: (dx * dx + dy * dy) + dz * dz, every operation rounded once.  Plain products and sums under the pragma, not
// __fmul_rn / __fadd_rn: those are inline functions of a header compiled with contraction allowed, and a product in one of them is fused
// with the sum in the next (v_fmac_f32 in the listing); operations written inside the pragma's scope are not.
__device__ __forceinline__ float dist2(const float dx, const float dy, const float dz)
{
#pragma clang fp contract(off)
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz;
}

// lower bound, in the arithmetic of dist2, of the distance between anything in [qlo, qhi] and anything in [lo, hi] (a point: qlo == qhi)
__device__ __forceinline__ float box_bound(const float qlo[3], const float qhi[3], const f32x4 lo, const f32x4 hi)
{
    float g[3];
#pragma unroll
    for (int a = 0; a < 3; a++) g[a] = fmaxf(fmaxf(lo[a] - qhi[a], qlo[a] - hi[a]), 0.0f);
    return dist2(g[0], g[1], g[2]);
}

// d joins the sorted best three (min and max return their operands: the multiset of values is kept exactly)
__device__ __forceinline__ void insert3(float& b0, float& b1, float& b2, const float d)
{
    const float t1 = fmaxf(b0, d);
    b0 = fminf(b0, d);
    const float t2 = fmaxf(b1, t1);
    b1 = fminf(b1, t1);
    b2 = fminf(b2, t2);
}

__global__ void __launch_bounds__(KNN_BOX) knn_search_kernel(const uint32_t P, const uint32_t boxes, const f32x4* __restrict__ records,
                                                             const f32x4* __restrict__ box_lo, const f32x4* __restrict__ box_hi, float* __restrict__ out)
{
    __shared__ f32x4 pts[KNN_BOX];
    __shared__ float wave_b2[2][KNN_WAVES];            // the waves' largest b2, written after a scan into the half the next barrier publishes
    __shared__ unsigned long long hits[KNN_WAVES];     // the boxes of a step that passed the box-to-box test, one bit per lane
    const uint32_t own = blockIdx.x, t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t base = own * (uint32_t)KNN_BOX;      // (< 2^31)
    const uint32_t count = min((uint32_t)KNN_BOX, P - base);
    const bool active = t < count;
    const f32x4 me = records[base + (active ? t : 0u)]; // (a lane past the end of the cloud looks on as the box's first point and writes nothing)
    if (active) pts[t] = me;
    // a lane without a query holds -inf: nothing enters, and it never raises the workgroup's largest b2
    float b0 = active ? INFINITY : -INFINITY, b1 = b0, b2 = b0;
    __syncthreads();
    for (uint32_t j = 0; j < count; j++) {
        const f32x4 p = pts[j];
        const float d = dist2(p[0] - me[0], p[1] - me[1], p[2] - me[2]);
        insert3(b0, b1, b2, j == t ? INFINITY : d);     // (j != i is by index)
    }
    uint32_t half = 0;
    {
        const float w = wave_max(b2);
        if (lane == 0) wave_b2[half][wave] = w;
    }
    const f32x4 own_lo = box_lo[own], own_hi = box_hi[own];
    const float qlo[3] = {own_lo[0], own_lo[1], own_lo[2]}, qhi[3] = {own_hi[0], own_hi[1], own_hi[2]}, q[3] = {me[0], me[1], me[2]};
    __syncthreads();
    float largest = wave_b2[half][0];
#pragma unroll
    for (int w = 1; w < KNN_WAVES; w++) largest = fmaxf(largest, wave_b2[half][w]);

    // position n of the walk is box own - (n / 2 + 1) (n even) or own + (n / 2 + 1) (n odd); positions outside the cloud are passed over
    const uint32_t below = own, above = boxes - 1u - own, reach = below > above ? below : above;
    const auto box_at = [&](const uint32_t n, uint32_t& box) -> bool {
        const uint32_t k = (n >> 1) + 1u;
        if (n & 1u) { box = own + k; return k <= above; }
        box = own - k;
        return k <= below;
    };
    for (uint32_t step = 0; step < 2u * reach; step += (uint32_t)KNN_BOX) { // (2 * reach < 2^25)
        uint32_t box;
        bool hit = false;
        if (box_at(step + t, box)) hit = !(box_bound(qlo, qhi, box_lo[box], box_hi[box]) > largest);
        const unsigned long long mine = __ballot(hit);
        if (lane == 0) hits[wave] = mine;
        __syncthreads();
        for (uint32_t w = 0; w < (uint32_t)KNN_WAVES; w++) {
            unsigned long long todo = hits[w];
            // (the same word in every lane; readfirstlane returns an int: through uint32_t, or the low half's bit 31 would sign-extend over the high half)
            const uint32_t todo_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)todo);
            const uint32_t todo_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(todo >> 32));
            todo = ((unsigned long long)todo_hi << 32) | (unsigned long long)todo_lo;
            while (todo) {
                const uint32_t bit = (uint32_t)__builtin_ctzll(todo);
                todo &= todo - 1ull;
                uint32_t target;
                if (!box_at(step + w * 64u + bit, target)) continue; // (never: it was in the cloud when it was tested; the index is checked before it is used all the same)
                const f32x4 lo = box_lo[target], hi = box_hi[target];
                __syncthreads();                        // the last scan has read pts, and its b2 are in wave_b2[half]
                largest = wave_b2[half][0];
#pragma unroll
                for (int v = 1; v < KNN_WAVES; v++) largest = fmaxf(largest, wave_b2[half][v]);
                // the same numbers in every lane: the workgroup goes one way
                if (__builtin_amdgcn_readfirstlane((int)(box_bound(qlo, qhi, lo, hi) > largest))) continue;
                const uint32_t first = target * (uint32_t)KNN_BOX, n = min((uint32_t)KNN_BOX, P - first);
                if (t < n) pts[t] = records[first + t];
                __syncthreads();
                if (!(box_bound(q, q, lo, hi) > b2)) {
                    for (uint32_t j = 0; j < n; j++) {
                        const f32x4 p = pts[j];
                        insert3(b0, b1, b2, dist2(p[0] - me[0], p[1] - me[1], p[2] - me[2]));
                    }
                }
                half ^= 1u;                             // (the other half: lanes may still be reading the one the barrier above published)
                const float wmax = wave_max(b2);
                if (lane == 0) wave_b2[half][wave] = wmax;
            }
        }
        __syncthreads();                                // hits is free again, and the last b2 are visible
        largest = wave_b2[half][0];
#pragma unroll
        for (int v = 1; v < KNN_WAVES; v++) largest = fmaxf(largest, wave_b2[half][v]);
    }
    if (active) out[__float_as_uint(me[3])] = ((b0 + b1) + b2) / 3.0f; // (sums and an IEEE division: nothing to fuse)
}

uint32_t knn_boxes(int P) { return ((uint32_t)P + KNN_BOX - 1) / KNN_BOX; }

// rocPRIM's temporary storage for a sort of n keys or pairs between two buffers of ours (histograms and look-back states: small)
size_t knn_sort_temp(size_t n)
{
    size_t bytes = 0;
    rocprim::double_buffer<uint32_t> keys(nullptr, nullptr), values(nullptr, nullptr);
    (void)rocprim::radix_sort_pairs(nullptr, bytes, keys, values, n, 0u, KNN_SORT_BITS);
    size_t axis_bytes = 0; // (the three sorts of one axis's coordinates: keys alone, all 32 bits)
    (void)rocprim::radix_sort_keys(nullptr, axis_bytes, keys, n, 0u, 32u);
    return bytes > axis_bytes ? bytes : axis_bytes;
}

// What the scratch reserves for rocPRIM: its demand at the powers of two up to the first one >= P, the largest of them.  Non-decreasing in P
// by construction, whatever rocPRIM's own sizes do between its algorithms.
size_t knn_sort_reserve(int P)
{
    size_t most = 0;
    for (size_t n = 1;; n <<= 1) {
        const size_t bytes = knn_sort_temp(n);
        if (bytes > most) most = bytes;
        if (n >= (size_t)P) break;
    }
    return most;
}

// what steps 1-3 work in: the head of the knn call's scratch, and the whole of stp_spatial_order's
struct MortonScratch {
    uint32_t* splitters; // 3 x KNN_CELLS
    uint32_t *keys[2], *values[2];
    char* sort_temp;
    size_t sort_temp_bytes;
};
struct KnnScratch {
    MortonScratch m;
    f32x4 *records, *box_lo, *box_hi;
    size_t total;
};

// with_boxes: the records and boxes of the search lie between the sort's buffers and rocPRIM's temporary storage
KnnScratch knn_carve(char* base, int P, bool with_boxes) // P >= 1
{
    KnnScratch s{};
    size_t off = 0;
    const auto take = [&](size_t bytes) {
        char* const p = base ? base + off : nullptr;
        off += (bytes + ALIGN - 1) & ~(ALIGN - 1);
        return p;
    };
    const size_t n = (size_t)P, boxes = knn_boxes(P);
    s.m.splitters = reinterpret_cast<uint32_t*>(take(3 * KNN_CELLS * sizeof(uint32_t)));
    for (int k = 0; k < 2; k++) s.m.keys[k] = reinterpret_cast<uint32_t*>(take(n * sizeof(uint32_t)));
    for (int k = 0; k < 2; k++) s.m.values[k] = reinterpret_cast<uint32_t*>(take(n * sizeof(uint32_t)));
    if (with_boxes) {
        s.records = reinterpret_cast<f32x4*>(take(n * sizeof(f32x4)));
        s.box_lo = reinterpret_cast<f32x4*>(take(boxes * sizeof(f32x4)));
        s.box_hi = reinterpret_cast<f32x4*>(take(boxes * sizeof(f32x4)));
    }
    s.m.sort_temp_bytes = knn_sort_reserve(P);
    s.m.sort_temp = take(s.m.sort_temp_bytes);
    s.total = off;
    return s;
}

// Steps 1-3 of the pipeline above, THE Morton order of a cloud of n >= 1 points (include/stp_raster.h: stp_spatial_order states it): *codes and
// *order are the buffers of s that hold the sorted codes and, beside them, the original indices -- rocPRIM's radix sort is stable and the
// values start as 0 .. n - 1, so equal codes stay in index order.  Returns the launches made (a sort of the library counting as one), *err =
// the error that ended them early (or hipSuccess).
int launch_morton_order(const uint32_t n, const float* points, const MortonScratch& s, hipStream_t st, hipError_t* err, const uint32_t** codes,
                        const uint32_t** order)
{
    const uint32_t blocks = (n + KNN_BLOCK - 1) / KNN_BLOCK;
    *err = hipSuccess;
    *codes = *order = nullptr;
    if (knn_sort_temp((size_t)n) > s.sort_temp_bytes) { // (rocPRIM wants more at P than at the powers of two around it: refuse in front of the first launch)
        *err = hipErrorInvalidValue;
        return 0;
    }
    int launches = 0;
    for (uint32_t axis = 0; axis < 3; axis++) {
        hipLaunchKernelGGL(knn_axis_keys_kernel, dim3(blocks), dim3(KNN_BLOCK), 0, st, n, points, axis, s.keys[0]);
        if ((*err = hipGetLastError()) != hipSuccess) return launches;
        launches++;
        rocprim::double_buffer<uint32_t> axis_keys(s.keys[0], s.keys[1]);
        size_t axis_bytes = s.sort_temp_bytes;
        if ((*err = rocprim::radix_sort_keys(s.sort_temp, axis_bytes, axis_keys, (size_t)n, 0u, 32u, st)) != hipSuccess) return launches;
        launches++; // (a sort of the library counts as one)
        hipLaunchKernelGGL(knn_splitters_kernel, dim3(KNN_CELLS / KNN_BLOCK), dim3(KNN_BLOCK), 0, st, n, axis_keys.current(), s.splitters + axis * KNN_CELLS);
        if ((*err = hipGetLastError()) != hipSuccess) return launches;
        launches++;
    }
    hipLaunchKernelGGL(knn_morton_kernel, dim3(blocks), dim3(KNN_BLOCK), 0, st, n, points, s.splitters, s.keys[0], s.values[0]);
    if ((*err = hipGetLastError()) != hipSuccess) return launches;
    launches++;
    rocprim::double_buffer<uint32_t> keys(s.keys[0], s.keys[1]), values(s.values[0], s.values[1]);
    size_t bytes = s.sort_temp_bytes;
    if ((*err = rocprim::radix_sort_pairs(s.sort_temp, bytes, keys, values, (size_t)n, 0u, KNN_SORT_BITS, st)) != hipSuccess) return launches;
    launches++;
    *codes = keys.current();
    *order = values.current();
    return launches;
}

} // namespace

size_t knn_scratch_bytes(int P) { return P <= 0 ? 0 : knn_carve(nullptr, P, true).total; }

int launch_knn_mean_dist2(int P, const float* points, void* scratch, float* mean_dist2, hipStream_t st, hipError_t* err)
{
    const KnnScratch s = knn_carve(static_cast<char*>(scratch), P, true);
    const uint32_t n = (uint32_t)P, boxes = knn_boxes(P);
    const uint32_t *codes, *order;
    int launches = launch_morton_order(n, points, s.m, st, err, &codes, &order);
    if (*err != hipSuccess) return launches;
    hipLaunchKernelGGL(knn_boxes_kernel, dim3(boxes), dim3(KNN_BOX), 0, st, n, points, order, s.records, s.box_lo, s.box_hi);
    if ((*err = hipGetLastError()) != hipSuccess) return launches;
    launches++;
    hipLaunchKernelGGL(knn_search_kernel, dim3(boxes), dim3(KNN_BOX), 0, st, n, boxes, s.records, s.box_lo, s.box_hi, mean_dist2);
    if ((*err = hipGetLastError()) != hipSuccess) return launches;
    launches++;
    return launches;
}

size_t spatial_order_scratch_bytes(int P) { return P <= 0 ? 0 : knn_carve(nullptr, P, false).total; }

int launch_spatial_order(int P, const float* xyz, void* scratch, int32_t* order_out, uint32_t* codes_out, hipStream_t st, hipError_t* err)
{
    const KnnScratch s = knn_carve(static_cast<char*>(scratch), P, false);
    const uint32_t n = (uint32_t)P;
    const uint32_t *codes, *order;
    int launches = launch_morton_order(n, xyz, s.m, st, err, &codes, &order);
    if (*err != hipSuccess) return launches;
    hipLaunchKernelGGL(spatial_order_emit_kernel, dim3((n + KNN_BLOCK - 1) / KNN_BLOCK), dim3(KNN_BLOCK), 0, st, n, order, codes, order_out, codes_out);
    if ((*err = hipGetLastError()) != hipSuccess) return launches;
    launches++;
    return launches;
}

} // namespace stp
