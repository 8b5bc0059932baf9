// stp_mcmc_relocate.hip -- the rest of a 3DGS-MCMC trainer's relocate_gs and add_new_gs beside compute_relocation (no counterpart in the
// reference; the semantics are that trainer's, restated in include/stp_raster.h): the multinomial draw of the sources, and the apply that
// rewrites every parameter and both Adam moments -- in place for the relocation, out of place for the growth.  No host synchronisation, no
// float atomics: equal inputs (the uniforms included) give equal bits whatever the launch shape.
//
// Sampling.  An inverse CDF over INTEGER weights: w_i = rint(clamp(o_i, 0, 1) * 2^24) (round to nearest even; exact, the scaling is a power of
// two) for a candidate row and 0 for any other, o the opacity (raw: 1 / (1 + expf(-logit)), as mcmc_noise_kernel evaluates it).  The inclusive
// prefix S_i = w_0 + ... + w_i is a 64-bit integer sum -- exact whatever the scan order -- by the tile-sum pattern of stp_row_table.h: a thread
// owns SAMPLE_ITEMS consecutive rows, a workgroup SAMPLE_TILE; (1) every workgroup sums its tile (and clears its rows of `count`), (2) one
// workgroup turns the tile sums into their exclusive prefix and leaves the total, (3) every workgroup scans its tile again from that prefix
// and writes S.  (4) A lane per draw: u is clamped into [0, 1) (NaN and negatives: 0), t = min(total - 1, (uint64)(double(u) * double(total)))
// (one float64 product; total <= 2^28 * 2^24 = 2^52 is exact there), and the source is the smallest k with S_k > t by binary search -- never a
// row of weight 0.  count[k] += 1 is an integer atomic: the sum does not depend on the order.  Relocation (rule 0): the candidates are the rows
// with o > min_opacity, draw i belongs to row i and is made only where o_i <= min_opacity (a dead row; a NaN opacity is neither); growth
// (rule 1): every row with a non-NaN opacity is a candidate and all n_draws draws are made.  total == 0: every src is -1, every count 0.
//
// Apply.  THE WRITE HAZARD: a dead row takes its source's opacity and scaling while the source's own row is rewritten, and several dead rows
// share a source.  Chosen here: the new values are computed PER SOURCE INTO SCRATCH in a pass of its own before any write (fresh_kernel: row k
// with count[k] > 0 gets its stored (o', s'_0, s'_1, s'_2) as 16 bytes), and the apply reads opacity and scaling of a source from that scratch
// only.  The other tensors need nothing: a row that is read (a source: count > 0) is never a row that is written (count == 0 and src >= 0).
// o' and s' are mcmc_relocation_row's (stp_mcmc_relocation.h: the bits of stp_mcmc_relocation) with N = min(count + 1, 50); then
// o' = min(max(o', min_opacity), 1 - 2^-23); raw: the stored values are logf(o' / (1 - o')) and logf(s'), the inputs expf(scaling) and the sigmoid above.
// The work is flattened over (row, element) by the row table of stp_row_table.h: 16 bytes per lane where a tensor's rows are multiples of 16 bytes and its
// pointers aligned, one float otherwise, with equal bits.  src values outside [0, P) are treated as -1: no plan can make a lane leave its arrays.
#include "stp_internal.h"
#include "stp_mcmc_relocation.h"
#include "stp_row_table.h"

// Nothing in this file is contracted (the reason is stp_densify.hip's).
#pragma clang fp contract(off)

namespace stp {

namespace {

constexpr int RELOCATE_BLOCK = ROW_BLOCK;

constexpr uint32_t SAMPLE_ITEMS = 8;                            // consecutive rows of a thread
constexpr uint32_t SAMPLE_TILE = RELOCATE_BLOCK * SAMPLE_ITEMS; // rows of a workgroup
constexpr size_t SAMPLE_HEAD = 4;                               // 64-bit words in front of the tile sums: [0] the total weight (three spare)

__device__ __forceinline__ float stored_opacity(const float x, const int raw) { return raw ? __fdiv_rn(1.0f, 1.0f + expf(-x)) : x; }

// rule 0: o > min_opacity; rule 1: any opacity that is a number
__device__ __forceinline__ uint32_t sample_weight(const float o, const int rule, const float min_opacity)
{
    const bool candidate = rule == 0 ? o > min_opacity : o == o;
    return candidate ? (uint32_t)rintf(fminf(fmaxf(o, 0.0f), 1.0f) * 16777216.0f) : 0u;
}

__global__ void __launch_bounds__(RELOCATE_BLOCK) sample_tile_sums_kernel(const uint32_t P, const float* __restrict__ opacity, const int rule,
                                                                           const float min_opacity, const int raw, uint64_t* __restrict__ tile_sums,
                                                                           int32_t* __restrict__ count)
{
    __shared__ uint64_t lds[RELOCATE_BLOCK / 64];
    const uint32_t i0 = blockIdx.x * SAMPLE_TILE + threadIdx.x * SAMPLE_ITEMS; // (< 2^28 + SAMPLE_TILE)
    uint64_t sum = 0;
    for (uint32_t k = 0; k < SAMPLE_ITEMS; k++) {
        const uint32_t i = i0 + k;
        if (i >= P) break;
        sum += sample_weight(stored_opacity(opacity[i], raw), rule, min_opacity);
        count[i] = 0;
    }
    uint64_t total;
    (void)block_exclusive(sum, lds, total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(RELOCATE_BLOCK) sample_prefix_kernel(const uint32_t P, const float* __restrict__ opacity, const int rule,
                                                                        const float min_opacity, const int raw, const uint64_t* __restrict__ tile_sums,
                                                                        uint64_t* __restrict__ prefix, uint32_t* __restrict__ weights)
{
    __shared__ uint64_t lds[RELOCATE_BLOCK / 64];
    const uint32_t i0 = blockIdx.x * SAMPLE_TILE + threadIdx.x * SAMPLE_ITEMS;
    uint32_t w[SAMPLE_ITEMS];
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < SAMPLE_ITEMS; k++) {
        const uint32_t i = i0 + k;
        w[k] = i < P ? sample_weight(stored_opacity(opacity[i], raw), rule, min_opacity) : 0u;
        sum += w[k];
    }
    uint64_t total;
    uint64_t run = tile_sums[blockIdx.x] + block_exclusive(sum, lds, total);
#pragma unroll
    for (uint32_t k = 0; k < SAMPLE_ITEMS; k++) {
        const uint32_t i = i0 + k;
        if (i < P) {
            run += w[k];
            prefix[i] = run;
            if (weights) weights[i] = w[k];
        }
    }
}

__global__ void __launch_bounds__(RELOCATE_BLOCK) sample_draw_kernel(const uint32_t P, const float* __restrict__ opacity, const int rule, const float min_opacity,
                                                                      const int raw, const uint32_t n_draws, const float* __restrict__ uniforms,
                                                                      const uint64_t* __restrict__ head, const uint64_t* __restrict__ prefix,
                                                                      int32_t* __restrict__ src, int32_t* __restrict__ count)
{
    const uint32_t j = blockIdx.x * (uint32_t)RELOCATE_BLOCK + threadIdx.x;
    if (j >= n_draws) return;
    const uint64_t total = head[0];
    bool draws = total > 0;
    if (rule == 0) draws = draws && stored_opacity(opacity[j], raw) <= min_opacity; // (n_draws == P: draw j is row j's)
    if (!draws) {
        src[j] = -1;
        return;
    }
    float u = uniforms[j];
    u = u >= 0.0f ? u : 0.0f;            // (NaN too)
    u = u < 1.0f ? u : 0x1.fffffep-1f;   // the largest float32 below 1
    uint64_t t = (uint64_t)__dmul_rn((double)u, (double)total);
    if (t > total - 1) t = total - 1;
    uint32_t lo = 0, hi = P; // the smallest k with prefix[k] > t: prefix[P - 1] = total > t, so lo < P at the end
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (prefix[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    if (lo >= P) lo = P - 1; // (unreachable: keeps a lane inside the arrays whatever the scratch holds)
    src[j] = (int32_t)lo;
    atomicAdd(&count[lo], 1);
}

// ---- the applies ---------------------------------------------------------------------------------------------------------------------------

constexpr int MAX_COPIES = 50;                                  // compute_relocation's clamp of N
constexpr float ONE_MINUS_EPS = 0x1.fffffcp-1f;                 // 1 - float32 eps (2^-23)

// (RowDesc of stp_row_table.h: the items are those of the tensor's WRITTEN rows; role 0 plain, 1 opacity, 2 scaling)

// the stored (o', s') of every row that was drawn, 16 bytes per row; rows with count <= 0 are not written (and never read)
__global__ void __launch_bounds__(RELOCATE_BLOCK) fresh_kernel(const uint32_t P, const int32_t* __restrict__ count, const float* __restrict__ opacity,
                                                                const float* __restrict__ scaling, const float min_opacity, const int raw,
                                                                f32x4* __restrict__ fresh)
{
    const uint32_t i = blockIdx.x * (uint32_t)RELOCATE_BLOCK + threadIdx.x;
    if (i >= P) return;
    const int32_t c = count[i];
    if (c <= 0) return;
    const int copies = c >= MAX_COPIES ? MAX_COPIES : c + 1;
    double x, coef;
    mcmc_relocation_row(stored_opacity(opacity[i], raw), copies, x, coef);
    float o = fminf(fmaxf((float)x, min_opacity), ONE_MINUS_EPS);
    if (raw) o = logf(__fdiv_rn(o, 1.0f - o));
    f32x4 out;
    out[0] = o;
    const size_t e = 3 * (size_t)i;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const float s_old = raw ? expf(scaling[e + j]) : scaling[e + j];
        const float s = (float)__dmul_rn(coef, (double)s_old);
        out[1 + j] = raw ? logf(s) : s;
    }
    fresh[i] = out;
}

// element `col` of a row of role 1 (opacity: the row is one float) or 2 (scaling: three)
__device__ __forceinline__ float fresh_value(const f32x4* __restrict__ fresh, const uint32_t k, const int32_t role, const uint32_t col)
{
    const float* const f = reinterpret_cast<const float*>(fresh + k);
    return role == 1 ? f[0] : f[1 + col];
}

// in place: rows with count > 0 take (o', s') and zero moments; rows with count <= 0 and a src in [0, P) take row src (with its (o', s')), and
// zero moments where reset_dead
__global__ void __launch_bounds__(RELOCATE_BLOCK) relocate_apply_kernel(const RowTable table, const int n_tensors, const uint32_t P, const int32_t* __restrict__ src,
                                                                         const int32_t* __restrict__ count, const f32x4* __restrict__ fresh, const int reset_dead)
{
    const RowDesc& d = row_table_entry(table, n_tensors, blockIdx.x);
    const uint32_t row = d.row, items = d.items;
    const AdamDivisor div = d.div;
    const bool moments = d.mo != nullptr;
    const uint32_t base = (blockIdx.x - d.first_unit) * ROW_UNIT;
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};

#pragma unroll
    for (int k = 0; k < ROW_PIECES; k++) {
        const uint32_t item = base + threadIdx.x + (uint32_t)k * RELOCATE_BLOCK;
        if (item >= items) break;
        const uint32_t e = d.wide ? item << 2 : item;   // the item's first float (< P * row < 2^31)
        const uint32_t i = adam_div(e, div), col = e - i * row;
        if (count[i] > 0) { // a source: its plain parameters stay
            if (d.wide) {
                if (moments) {
                    reinterpret_cast<f32x4*>(d.mo)[item] = zero4;
                    reinterpret_cast<f32x4*>(d.vo)[item] = zero4;
                }
            } else {
                if (d.role != 0) d.po[e] = fresh_value(fresh, i, d.role, col);
                if (moments) {
                    d.mo[e] = 0.0f;
                    d.vo[e] = 0.0f;
                }
            }
            continue;
        }
        const uint32_t s = (uint32_t)src[i];
        if (s >= P) continue; // -1 (or anything outside the model): the row keeps its bits
        if (d.wide) { // (16 bytes inside one row: row % 4 == 0, so col % 4 == 0 too; a wide tensor has role 0)
            reinterpret_cast<f32x4*>(d.po)[item] = reinterpret_cast<const f32x4*>(d.p)[((size_t)s * row + col) >> 2];
            if (moments && reset_dead) {
                reinterpret_cast<f32x4*>(d.mo)[item] = zero4;
                reinterpret_cast<f32x4*>(d.vo)[item] = zero4;
            }
        } else {
            d.po[e] = d.role != 0 ? fresh_value(fresh, s, d.role, col) : d.p[(size_t)s * row + col];
            if (moments && reset_dead) {
                d.mo[e] = 0.0f;
                d.vo[e] = 0.0f;
            }
        }
    }
}

// out of place, over the P + n_new OUTPUT rows: row r < P is row r (with (o', s') and zero moments where count[r] > 0), row P + j is row src[j]
// with its (o', s') and zero moments -- or, where src[j] is outside [0, P) (a model without any weight), +0.0 everywhere
__global__ void __launch_bounds__(RELOCATE_BLOCK) add_apply_kernel(const RowTable table, const int n_tensors, const uint32_t P, const int32_t* __restrict__ src,
                                                                    const int32_t* __restrict__ count, const f32x4* __restrict__ fresh)
{
    const RowDesc& d = row_table_entry(table, n_tensors, blockIdx.x);
    const uint32_t row = d.row, items = d.items;
    const AdamDivisor div = d.div;
    const bool moments = d.mo != nullptr;
    const uint32_t base = (blockIdx.x - d.first_unit) * ROW_UNIT;
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};

#pragma unroll
    for (int k = 0; k < ROW_PIECES; k++) {
        const uint32_t item = base + threadIdx.x + (uint32_t)k * RELOCATE_BLOCK;
        if (item >= items) break;
        const uint32_t e = d.wide ? item << 2 : item;   // the item's first float in the OUTPUT (< (P + n_new) * row < 2^31)
        const uint32_t r = adam_div(e, div), col = e - r * row;
        uint32_t s = r;       // the row that is read
        bool drawn = true;    // (o', s') and zero moments
        if (r < P) drawn = count[r] > 0;
        else s = (uint32_t)src[r - P];
        const bool there = s < P;
        const size_t in = (size_t)s * row + col;
        if (d.wide) {
            reinterpret_cast<f32x4*>(d.po)[item] = there ? reinterpret_cast<const f32x4*>(d.p)[in >> 2] : zero4;
            if (moments) {
                reinterpret_cast<f32x4*>(d.mo)[item] = drawn ? zero4 : reinterpret_cast<const f32x4*>(d.m)[in >> 2];
                reinterpret_cast<f32x4*>(d.vo)[item] = drawn ? zero4 : reinterpret_cast<const f32x4*>(d.v)[in >> 2];
            }
        } else {
            d.po[e] = !there ? 0.0f : (drawn && d.role != 0) ? fresh_value(fresh, s, d.role, col) : d.p[in];
            if (moments) {
                d.mo[e] = drawn ? 0.0f : d.m[in];
                d.vo[e] = drawn ? 0.0f : d.v[in];
            }
        }
    }
}

uint32_t sample_tiles(int P) { return ((uint32_t)P + SAMPLE_TILE - 1) / SAMPLE_TILE; }

const float* role_param(int n_tensors, const StpMcmcTensor* tensors, int role)
{
    for (int k = 0; k < n_tensors; k++)
        if (tensors[k].role == role) return tensors[k].param;
    return nullptr;
}

} // namespace

size_t mcmc_relocate_scratch_bytes(int P) // P in [0, 2^28]
{
    const size_t sample = (SAMPLE_HEAD + sample_tiles(P) + (size_t)P) * sizeof(uint64_t); // head | tile sums | prefix
    const size_t apply = (size_t)P * sizeof(f32x4);                                       // fresh
    const size_t bytes = sample > apply ? sample : apply;
    return (bytes + 255) & ~(size_t)255;
}

int launch_mcmc_sample(int P, const float* opacity, int rule, float min_opacity, int raw, int n_draws, const float* uniforms, void* scratch, uint32_t* weights,
                       int32_t* src, int32_t* count, hipStream_t st, hipError_t* err)
{
    uint64_t* const head = static_cast<uint64_t*>(scratch);
    uint64_t* const tile_sums = head + SAMPLE_HEAD;
    const uint32_t tiles = sample_tiles(P);
    uint64_t* const prefix = tile_sums + tiles;
    const dim3 block(RELOCATE_BLOCK);
    int launches = 0;
    hipLaunchKernelGGL(sample_tile_sums_kernel, dim3(tiles), block, 0, st, (uint32_t)P, opacity, rule, min_opacity, raw, tile_sums, count);
    if ((*err = hipGetLastError()) != hipSuccess) return launches;
    launches++;
    hipLaunchKernelGGL(tile_prefix_kernel<uint64_t>, dim3(1), block, 0, st, tiles, (tiles + RELOCATE_BLOCK - 1) / RELOCATE_BLOCK, tile_sums, head);
    if ((*err = hipGetLastError()) != hipSuccess) return launches;
    launches++;
    hipLaunchKernelGGL(sample_prefix_kernel, dim3(tiles), block, 0, st, (uint32_t)P, opacity, rule, min_opacity, raw, tile_sums, prefix, weights);
    if ((*err = hipGetLastError()) != hipSuccess) return launches;
    launches++;
    if (n_draws > 0) {
        hipLaunchKernelGGL(sample_draw_kernel, dim3(((uint32_t)n_draws + RELOCATE_BLOCK - 1) / RELOCATE_BLOCK), block, 0, st, (uint32_t)P, opacity, rule, min_opacity, raw,
                           (uint32_t)n_draws, uniforms, head, prefix, src, count);
        if ((*err = hipGetLastError()) != hipSuccess) return launches;
        launches++;
    }
    return launches;
}

static int launch_fresh(int P, const int32_t* count, int n_tensors, const StpMcmcTensor* tensors, float min_opacity, int raw, void* scratch, hipStream_t st, hipError_t* err)
{
    hipLaunchKernelGGL(fresh_kernel, dim3(((uint32_t)P + RELOCATE_BLOCK - 1) / RELOCATE_BLOCK), dim3(RELOCATE_BLOCK), 0, st, (uint32_t)P, count,
                       role_param(n_tensors, tensors, 1), role_param(n_tensors, tensors, 2), min_opacity, raw, static_cast<f32x4*>(scratch));
    *err = hipGetLastError();
    return *err == hipSuccess ? 1 : 0;
}

int launch_mcmc_relocate_apply(int P, const int32_t* src, const int32_t* count, int n_tensors, const StpMcmcTensor* tensors, float min_opacity, int raw,
                               int reset_dead_moments, void* scratch, hipStream_t st, hipError_t* err)
{
    int launches = launch_fresh(P, count, n_tensors, tensors, min_opacity, raw, scratch, st, err);
    if (*err != hipSuccess) return launches;
    const f32x4* const fresh = static_cast<const f32x4*>(scratch);
    launches += launch_row_tables(n_tensors, tensors, (uint32_t)P, true, err, [&](const RowTable& table, int n, uint32_t units) {
        hipLaunchKernelGGL(relocate_apply_kernel, dim3(units), dim3(RELOCATE_BLOCK), 0, st, table, n, (uint32_t)P, src, count, fresh, reset_dead_moments);
    });
    return launches;
}

int launch_mcmc_add_apply(int P, int n_new, const int32_t* src, const int32_t* count, int n_tensors, const StpMcmcTensor* tensors, float min_opacity, int raw,
                          void* scratch, hipStream_t st, hipError_t* err)
{
    int launches = launch_fresh(P, count, n_tensors, tensors, min_opacity, raw, scratch, st, err);
    if (*err != hipSuccess) return launches;
    const f32x4* const fresh = static_cast<const f32x4*>(scratch);
    launches += launch_row_tables(n_tensors, tensors, (uint32_t)P + (uint32_t)n_new, false, err, [&](const RowTable& table, int n, uint32_t units) {
        hipLaunchKernelGGL(add_apply_kernel, dim3(units), dim3(RELOCATE_BLOCK), 0, st, table, n, (uint32_t)P, src, count, fresh);
    });
    return launches;
}

} // namespace stp
