// stp_densify.hip -- adaptive density control of a 3DGS / StopThePop trainer in four steps (no counterpart in the reference rasterizer; the
// semantics are those of the trainer's add_densification_stats and densify_and_prune): the per-step statistics, the plan (one byte per
// Gaussian), the scan that turns the plan into destination rows, and the apply that writes every parameter and both Adam moments of the
// new model in one pass.  No atomics anywhere: equal inputs give equal bits whatever the launch shape.
//
// Statistics.  One lane per Gaussian, in place: for a visible i, grad_accum[i] += sqrt(gx * gx + gy * gy) (two products, one sum, one
// correctly rounded root -- sqrtf: __fsqrt_rn is the hardware's approximate one in this toolchain -- with contraction off for the whole
// file), denom[i] += 1 and, where asked, max_radii2D[i] = max(max_radii2D[i], (float)radii[i]).  An invisible lane loads nothing but its
// visibility.
//
// Plan.  One lane per Gaussian; bit 0 = the original stays (K), bit 1 = one copy is appended (C), bit 2 = two children are appended (S); the
// rule is in include/stp_raster.h.  The division is the correctly rounded one; exp and the sigmoid's exp are expf.
//
// Scan.  The 3P flags [K bits | C bits | S bits] are never materialised: flag j is bit j / P of plan[j % P].  A thread owns SCAN_ITEMS
// consecutive flags, a workgroup SCAN_TILE; (1) every workgroup sums its tile, (2) one workgroup turns the tile sums into their exclusive
// prefix in place (tile_prefix_kernel of stp_row_table.h), (3) every workgroup scans its tile again from that prefix and writes the offsets.  The thread that passes flag P, flag 2P
// and the last flag leaves the running sum there in three words, from which the host forms (nK, nC, nS).  The scratch is the tile sums and
// those words: its size depends on P alone.
//
// Apply.  The work is flattened over (source row, element) by the row table of stp_row_table.h: a tensor of P rows of `row` floats owns ceil(items /
// ROW_UNIT) consecutive work units, an item being 16 bytes of a row where the row stream is 16-byte aligned (row % 4 == 0 and all the
// tensor's pointers aligned) and one float otherwise; the arithmetic does not depend on the path.  A lane reads its Gaussian's plan byte;
// a row that goes nowhere is skipped before its loads.  K: parameter and moments are copied to row offsets[i]; C: the parameter is copied to
// row offsets[P + i] with zero moments; S: rows offsets[2P + i] and offsets[2P + i] + nS get the parameter -- or, in the xyz and scaling
// tensors, the child's value -- with zero moments.  The row index e / row uses the host-computed multiplier of stp_adam_div.h.
// EVALUATION ORDER of a child (float32, every operation written out): s = raw ? expf(scaling) : scaling; n = |q| from
// sqrtf(fma(q3, q3, fma(q2, q2, fma(q1, q1, q0 * q0)))), q / n by division; R as in stp_mcmc.hip; t = s * noise; xyz'_c = xyz_c + fma(R_c2, t_2,
// fma(R_c1, t_1, R_c0 * t_0)); scaling' = raw ? logf(s / split_shrink) : s / split_shrink.
#include "stp_internal.h"
#include "stp_row_table.h"

// Nothing in this file is contracted: __fmul_rn / __fadd_rn are plain operators to the compiler, which would otherwise fuse gx * gx + gy * gy
// into a multiply-add.  The fused multiply-adds that are wanted are written as __fmaf_rn.
#pragma clang fp contract(off)

namespace stp {

namespace {

constexpr int DENSIFY_BLOCK = ROW_BLOCK;

template <int KIND> __device__ __forceinline__ bool densify_visible(const void* __restrict__ visible, uint32_t i)
{
    if constexpr (KIND == 0) return static_cast<const uint8_t*>(visible)[i] != 0;
    else return static_cast<const int32_t*>(visible)[i] > 0;
}

template <int KIND>
__global__ void __launch_bounds__(DENSIFY_BLOCK) densify_stats_kernel(const uint32_t P, float* __restrict__ grad_accum, float* __restrict__ denom,
                                                                       float* __restrict__ max_radii2D, const float* __restrict__ grad2d,
                                                                       const uint32_t grad_stride, const void* __restrict__ visible)
{
    const uint32_t i = blockIdx.x * (uint32_t)DENSIFY_BLOCK + threadIdx.x;
    if (i >= P) return;
    if (!densify_visible<KIND>(visible, i)) return;
    const size_t g = (size_t)grad_stride * i;
    const float gx = grad2d[g], gy = grad2d[g + 1];
    grad_accum[i] = __fadd_rn(grad_accum[i], sqrtf(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy))));
    denom[i] = __fadd_rn(denom[i], 1.0f);
    if constexpr (KIND == 1) {
        if (max_radii2D) max_radii2D[i] = fmaxf(max_radii2D[i], (float)static_cast<const int32_t*>(visible)[i]);
    }
}

__global__ void __launch_bounds__(DENSIFY_BLOCK) densify_plan_kernel(const uint32_t P, const float* __restrict__ grad_accum, const float* __restrict__ denom,
                                                                      const float* __restrict__ scaling, const float* __restrict__ opacity,
                                                                      const float* __restrict__ max_radii2D, const StpDensifyRule rule,
                                                                      uint8_t* __restrict__ plan)
{
    const uint32_t i = blockIdx.x * (uint32_t)DENSIFY_BLOCK + threadIdx.x;
    if (i >= P) return;
    const float den = denom[i];
    const float g = den > 0.0f ? __fdiv_rn(grad_accum[i], den) : 0.0f;
    const size_t e = 3 * (size_t)i;
    float s0 = scaling[e], s1 = scaling[e + 1], s2 = scaling[e + 2], o = opacity[i];
    if (rule.raw) {
        s0 = expf(s0); s1 = expf(s1); s2 = expf(s2);
        o = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-o)));
    }
    const float smax = fmaxf(fmaxf(s0, s1), s2);
    const bool hot = g >= rule.grad_threshold;
    const bool clone = hot && smax <= rule.split_size, split = hot && smax > rule.split_size;
    const bool low = o < rule.min_opacity;
    const bool big = rule.prune_big != 0;
    const bool ws = big && smax > rule.max_world_size;
    const bool ws_child = big && __fdiv_rn(smax, rule.split_shrink) > rule.max_world_size;
    const bool vs = big && max_radii2D && max_radii2D[i] > rule.max_screen_size;
    const bool K = !split && !(low || ws || vs);
    const bool C = clone && !(low || ws);
    const bool S = split && !(low || ws_child);
    plan[i] = (uint8_t)((K ? 1 : 0) | (C ? 2 : 0) | (S ? 4 : 0));
}

// ---- the scan ------------------------------------------------------------------------------------------------------------------------------

constexpr uint32_t SCAN_ITEMS = 16;                          // consecutive flags of a thread
constexpr uint32_t SCAN_TILE = DENSIFY_BLOCK * SCAN_ITEMS;   // flags of a workgroup
constexpr size_t SCAN_MARKS = 4;                             // the words in front of the tile sums: running sums at flag P, at flag 2P, at the end (one spare)

__device__ __forceinline__ uint32_t plan_flag(const uint8_t* __restrict__ plan, const uint32_t P, const uint32_t j) // j < 3P < 2^31
{
    const uint32_t seg = (j >= P ? 1u : 0u) + (j >= 2u * P ? 1u : 0u);
    return ((uint32_t)plan[j - seg * P] >> seg) & 1u;
}

__device__ __forceinline__ uint32_t thread_flags(const uint8_t* __restrict__ plan, const uint32_t P, const uint32_t n, const uint32_t j0)
{
    uint32_t sum = 0;
    for (uint32_t k = 0; k < SCAN_ITEMS; k++) {
        const uint32_t j = j0 + k;
        if (j < n) sum += plan_flag(plan, P, j);
    }
    return sum;
}

__global__ void __launch_bounds__(DENSIFY_BLOCK) densify_tile_sums_kernel(const uint32_t P, const uint8_t* __restrict__ plan, uint32_t* __restrict__ tile_sums)
{
    __shared__ uint32_t lds[DENSIFY_BLOCK / 64];
    const uint32_t n = 3u * P;
    const uint32_t j0 = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS; // (< 2^31 + SCAN_TILE)
    uint32_t total;
    (void)block_exclusive(thread_flags(plan, P, n, j0), lds, total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(DENSIFY_BLOCK) densify_offsets_kernel(const uint32_t P, const uint8_t* __restrict__ plan, const uint32_t* __restrict__ tile_sums,
                                                                         uint32_t* __restrict__ marks, uint32_t* __restrict__ offsets)
{
    __shared__ uint32_t lds[DENSIFY_BLOCK / 64];
    const uint32_t n = 3u * P;
    const uint32_t j0 = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    uint32_t total;
    uint32_t run = tile_sums[blockIdx.x] + block_exclusive(thread_flags(plan, P, n, j0), lds, total);
    for (uint32_t k = 0; k < SCAN_ITEMS; k++) {
        const uint32_t j = j0 + k;
        if (j >= n) break;
        const uint32_t f = plan_flag(plan, P, j);
        offsets[j] = run;
        if (j == P) marks[0] = run;
        if (j == 2u * P) marks[1] = run;
        run += f;
        if (j == n - 1u) marks[2] = run;
    }
}

// ---- the apply -----------------------------------------------------------------------------------------------------------------------------

// what the children of a split need beside their own tensor
struct ApplySplit {
    const float *scaling, *rotation, *noise; // the INPUT scaling (P, 3) and rotation (P, 4), noise (2 nS, 3)
    uint32_t first_row, nS;                  // nK + nC: the row of the first split Gaussian's first child
    float shrink;
    int32_t raw;
};

__device__ __forceinline__ float child_scale(const float raw_or_s, const ApplySplit& sp)
{
    const float s = sp.raw ? expf(raw_or_s) : raw_or_s;
    const float c = __fdiv_rn(s, sp.shrink);
    return sp.raw ? logf(c) : c;
}

// component `col` of xyz[i] + R(q / |q|) (s * noise[n])
__device__ __forceinline__ float child_xyz(const float x, const uint32_t i, const uint32_t col, const uint32_t n, const ApplySplit& sp)
{
    const float* __restrict__ const q = sp.rotation + 4 * (size_t)i;
    const float* __restrict__ const sc = sp.scaling + 3 * (size_t)i;
    const float* __restrict__ const nz = sp.noise + 3 * (size_t)n;
    float t[3];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = __fmul_rn(sp.raw ? expf(sc[k]) : sc[k], nz[k]);
    const float q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    const float norm = sqrtf(__fmaf_rn(q3, q3, __fmaf_rn(q2, q2, __fmaf_rn(q1, q1, __fmul_rn(q0, q0)))));
    const float r = __fdiv_rn(q0, norm), a = __fdiv_rn(q1, norm), b = __fdiv_rn(q2, norm), c = __fdiv_rn(q3, norm);
    float R0, R1, R2; // row `col` of the rotation
    if (col == 0) {
        R0 = 1.0f - 2.0f * __fmaf_rn(b, b, __fmul_rn(c, c)); R1 = 2.0f * __fmaf_rn(a, b, -__fmul_rn(r, c)); R2 = 2.0f * __fmaf_rn(a, c, __fmul_rn(r, b));
    } else if (col == 1) {
        R0 = 2.0f * __fmaf_rn(a, b, __fmul_rn(r, c)); R1 = 1.0f - 2.0f * __fmaf_rn(a, a, __fmul_rn(c, c)); R2 = 2.0f * __fmaf_rn(b, c, -__fmul_rn(r, a));
    } else {
        R0 = 2.0f * __fmaf_rn(a, c, -__fmul_rn(r, b)); R1 = 2.0f * __fmaf_rn(b, c, __fmul_rn(r, a)); R2 = 1.0f - 2.0f * __fmaf_rn(a, a, __fmul_rn(b, b));
    }
    return __fadd_rn(x, __fmaf_rn(R2, t[2], __fmaf_rn(R1, t[1], __fmul_rn(R0, t[0]))));
}

__global__ void __launch_bounds__(DENSIFY_BLOCK) densify_apply_kernel(const RowTable table, const int n_tensors, const uint32_t P,
                                                                       const uint8_t* __restrict__ plan, const uint32_t* __restrict__ offsets,
                                                                       const ApplySplit sp)
{
    const uint32_t unit = blockIdx.x;
    const RowDesc& d = row_table_entry(table, n_tensors, unit);
    const uint32_t row = d.row, items = d.items;
    const AdamDivisor div = d.div;
    const bool moments = d.m != nullptr;
    const uint32_t base = (unit - d.first_unit) * ROW_UNIT;
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};

#pragma unroll
    for (int k = 0; k < ROW_PIECES; k++) {
        const uint32_t item = base + threadIdx.x + (uint32_t)k * DENSIFY_BLOCK;
        if (item >= items) break;
        const uint32_t e = d.wide ? item << 2 : item;   // the item's first float (< P * row < 2^31)
        const uint32_t i = adam_div(e, div), col = e - i * row;
        const uint32_t pl = plan[i];
        if (!(pl & 7u)) continue; // the row goes nowhere: nothing is loaded
        if (d.wide) { // (16 bytes inside one row: row % 4 == 0, so col % 4 == 0 too)
            const f32x4 x = reinterpret_cast<const f32x4*>(d.p)[item];
            if (pl & 1u) {
                const size_t o = ((size_t)offsets[i] * row + col) >> 2;
                reinterpret_cast<f32x4*>(d.po)[o] = x;
                if (moments) {
                    reinterpret_cast<f32x4*>(d.mo)[o] = reinterpret_cast<const f32x4*>(d.m)[item];
                    reinterpret_cast<f32x4*>(d.vo)[o] = reinterpret_cast<const f32x4*>(d.v)[item];
                }
            }
            if (pl & 2u) {
                const size_t o = ((size_t)offsets[P + i] * row + col) >> 2;
                reinterpret_cast<f32x4*>(d.po)[o] = x;
                if (moments) {
                    reinterpret_cast<f32x4*>(d.mo)[o] = zero4;
                    reinterpret_cast<f32x4*>(d.vo)[o] = zero4;
                }
            }
            if (pl & 4u) {
                const uint32_t first = offsets[2u * P + i];
#pragma unroll
                for (uint32_t j = 0; j < 2; j++) {
                    const size_t o = ((size_t)(first + j * sp.nS) * row + col) >> 2;
                    reinterpret_cast<f32x4*>(d.po)[o] = x;
                    if (moments) {
                        reinterpret_cast<f32x4*>(d.mo)[o] = zero4;
                        reinterpret_cast<f32x4*>(d.vo)[o] = zero4;
                    }
                }
            }
        } else {
            const float x = d.p[e];
            if (pl & 1u) {
                const size_t o = (size_t)offsets[i] * row + col;
                d.po[o] = x;
                if (moments) {
                    d.mo[o] = d.m[e];
                    d.vo[o] = d.v[e];
                }
            }
            if (pl & 2u) {
                const size_t o = (size_t)offsets[P + i] * row + col;
                d.po[o] = x;
                if (moments) {
                    d.mo[o] = 0.0f;
                    d.vo[o] = 0.0f;
                }
            }
            if (pl & 4u) {
                const uint32_t first = offsets[2u * P + i];
                const uint32_t r = first - sp.first_row; // this Gaussian's rank among the split ones
                const float scaled = d.role == 2 ? child_scale(x, sp) : x;
#pragma unroll
                for (uint32_t j = 0; j < 2; j++) {
                    const size_t o = (size_t)(first + j * sp.nS) * row + col;
                    d.po[o] = d.role == 1 ? child_xyz(x, i, col, j * sp.nS + r, sp) : scaled;
                    if (moments) {
                        d.mo[o] = 0.0f;
                        d.vo[o] = 0.0f;
                    }
                }
            }
        }
    }
}

uint32_t scan_tiles(int P) { return (uint32_t)((3ull * (uint32_t)P + SCAN_TILE - 1) / SCAN_TILE); }

} // namespace

int launch_densify_stats(int P, float* grad_accum, float* denom, float* max_radii2D, const float* grad2d, int grad_stride, const void* visible,
                         int visible_kind, hipStream_t st, hipError_t* err)
{
    const dim3 grid(((uint32_t)P + DENSIFY_BLOCK - 1) / DENSIFY_BLOCK), block(DENSIFY_BLOCK);
    if (visible_kind == 0)
        hipLaunchKernelGGL(densify_stats_kernel<0>, grid, block, 0, st, (uint32_t)P, grad_accum, denom, max_radii2D, grad2d, (uint32_t)grad_stride, visible);
    else
        hipLaunchKernelGGL(densify_stats_kernel<1>, grid, block, 0, st, (uint32_t)P, grad_accum, denom, max_radii2D, grad2d, (uint32_t)grad_stride, visible);
    *err = hipGetLastError();
    return *err == hipSuccess ? 1 : 0;
}

int launch_densify_plan(int P, const float* grad_accum, const float* denom, const float* scaling, const float* opacity, const float* max_radii2D,
                        const StpDensifyRule& rule, uint8_t* plan, hipStream_t st, hipError_t* err)
{
    const dim3 grid(((uint32_t)P + DENSIFY_BLOCK - 1) / DENSIFY_BLOCK), block(DENSIFY_BLOCK);
    hipLaunchKernelGGL(densify_plan_kernel, grid, block, 0, st, (uint32_t)P, grad_accum, denom, scaling, opacity, max_radii2D, rule, plan);
    *err = hipGetLastError();
    return *err == hipSuccess ? 1 : 0;
}

size_t densify_scratch_bytes(int P) // P >= 0, 3P < 2^31
{
    const size_t bytes = (SCAN_MARKS + scan_tiles(P)) * sizeof(uint32_t);
    return (bytes + 255) & ~(size_t)255;
}

int launch_densify_scan(int P, const uint8_t* plan, void* scratch, uint32_t* offsets, int64_t counts[3], hipStream_t st, hipError_t* err)
{
    uint32_t* const marks = static_cast<uint32_t*>(scratch);
    uint32_t* const tile_sums = marks + SCAN_MARKS;
    const uint32_t tiles = scan_tiles(P);
    const dim3 block(DENSIFY_BLOCK);
    int launches = 0;
    hipLaunchKernelGGL(densify_tile_sums_kernel, dim3(tiles), block, 0, st, (uint32_t)P, plan, tile_sums);
    if ((*err = hipGetLastError()) != hipSuccess) return launches;
    launches++;
    hipLaunchKernelGGL(tile_prefix_kernel<uint32_t>, dim3(1), block, 0, st, tiles, (tiles + DENSIFY_BLOCK - 1) / DENSIFY_BLOCK, tile_sums, (uint32_t*)nullptr);
    if ((*err = hipGetLastError()) != hipSuccess) return launches;
    launches++;
    hipLaunchKernelGGL(densify_offsets_kernel, dim3(tiles), block, 0, st, (uint32_t)P, plan, tile_sums, marks, offsets);
    if ((*err = hipGetLastError()) != hipSuccess) return launches;
    launches++;
    uint32_t host_marks[3] = {0, 0, 0};
    if ((*err = hipMemcpyAsync(host_marks, marks, sizeof(host_marks), hipMemcpyDeviceToHost, st)) != hipSuccess) return launches;
    if ((*err = hipStreamSynchronize(st)) != hipSuccess) return launches; // the feature's ONE host synchronisation: the new row count
    counts[0] = host_marks[0];
    counts[1] = (int64_t)host_marks[1] - host_marks[0];
    counts[2] = (int64_t)host_marks[2] - host_marks[1];
    return launches;
}

int launch_densify_apply(int P, const uint8_t* plan, const uint32_t* offsets, const int64_t counts[3], int n_tensors, const StpDensifyTensor* tensors,
                         const float* noise, float split_shrink, int raw, hipStream_t st, hipError_t* err)
{
    ApplySplit sp{};
    sp.noise = noise;
    sp.first_row = (uint32_t)(counts[0] + counts[1]);
    sp.nS = (uint32_t)counts[2];
    sp.shrink = split_shrink;
    sp.raw = raw;
    for (int k = 0; k < n_tensors; k++) {
        if (tensors[k].role == 2) sp.scaling = tensors[k].param;
        if (tensors[k].role == 3) sp.rotation = tensors[k].param;
    }
    // (the work is flattened over the P SOURCE rows)
    return launch_row_tables(n_tensors, tensors, (uint32_t)P, false, err, [&](const RowTable& table, int n, uint32_t units) {
        hipLaunchKernelGGL(densify_apply_kernel, dim3(units), dim3(DENSIFY_BLOCK), 0, st, table, n, (uint32_t)P, plan, offsets, sp);
    });
}

} // namespace stp
