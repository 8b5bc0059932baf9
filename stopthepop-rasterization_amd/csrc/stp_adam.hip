// stp_adam.hip -- the fused sparse Adam step of stp_sparse_adam (no counterpart in the reference; the semantics are those of the
// SparseGaussianAdam of the accelerated 3DGS rasterizer): for every element of every Gaussian (row) that is visible in the frame
//     m <- b1 * m + (1 - b1) * g      v <- b2 * v + (1 - b2) * g * g      p <- p - lr * m / (sqrt(v) + eps)
// in float32, without bias correction; the elements of invisible rows are neither read nor written.
//
// One launch serves up to ROW_TABLE_ENTRIES tensors.  The kernel arguments carry a table of descriptors by value; a tensor of numel
// elements owns ceil(numel / ADAM_UNIT) consecutive work units, a workgroup is one unit and finds its tensor by the wave-uniform search
// of stp_row_table.h (row_table_entry).  The descriptor and the packing loop are this file's own: four streams, a learning rate, units
// counted in elements with a tail, tensors without elements skipped.
//
// Streaming shape.  p, g, m and v of a unit are read and p, m, v written with 16 bytes per lane where all four pointers are 16-byte
// aligned (every tensor torch allocates); a thread owns the 16-byte pieces t, t + 256, t + 512 and t + 768 of its unit, so that a wave's
// access is 1 KiB contiguous per stream, and the last numel % 4 elements of a tensor belong to the first threads of its last unit.
// Tensors with an unaligned pointer take the same units one float per lane and access.  Every piece has exactly one owner; a piece that
// is only partly visible is written back whole, the lanes of its invisible rows carrying the bits that were loaded.  A piece without a
// visible element is skipped before its loads are issued (exec-masked: a wave whose pieces are all invisible branches over loads, maths
// and stores, and has read nothing but visibility).  No atomics, no LDS, no scratch; equal inputs give equal bits.
//
// Row index.  The row of element e is e / M (M = numel / N floats per Gaussian).  It is formed with a HOST-COMPUTED MULTIPLIER
// (stp_adam_div.h: mulhi(e, ceil(2^(32+s) / M)) >> s with 2^s < M <= 2^(s+1), exact for every e < 2^31 -- the proof is in that header,
// and tests/cpp/adam_div_check.cpp holds it against e / M), once per 16-byte piece; the three following elements advance (row, e % M)
// by increment and compare.  No integer division sequence on the device.  Chosen over instantiations per M because one kernel then
// serves every row width -- a trainer's feature tensors are (P, 15, 3) today and anything tomorrow -- at the cost of one v_mul_hi_u32
// per 16 bytes of each of seven streams.
//
// Visibility is read where the trainer has it: N bytes (bool / uint8, non-zero = visible) or the N int32 radii of the forward (> 0 =
// visible).  A lane reads the entry of its piece's first row and again only where the row changes inside the piece.
//
// The division is the correctly rounded one (v_div_scale / v_rcp / refinement / v_div_fmas / v_div_fixup).  The root is NOT: __fsqrt_rn
// compiles in this toolchain to the hardware's approximate v_sqrt_f32 between two v_ldexp_f32 (a denormal v is scaled up first) without a
// refinement step, as stp_densify.hip's comment says of it.  The step's bits are pinned as they are (the kernel has about 180 VALU slots per element at
// the HBM rate and uses a fraction); a denormal v or denominator is handled like any other value.
//
// The DENSE step of stp_dense_adam (dense_adam_kernel, below the sparse one; the step of GaussianAdam, a drop-in for the bias-corrected
// torch.optim.Adam a 3DGS or 3DGS-MCMC trainer constructs) has the same unit geometry -- ROW_BLOCK threads, four 16-byte pieces per thread
// and stream, 4096 elements per unit, the tail numel % 4 with the first threads of the last unit, one float per access where a pointer is
// not 16-byte aligned -- and needs no visibility, no row index and no adam_div.  Per element
//     g' = g + r      m <- b1 m + omb1 g'      v <- b2 v + omb2 g' g'      p <- p - (step_size m) / (sqrt(v) / bias2_sqrt + eps)
// with r = 0, c s (1 - s) (s = the sigmoid of stp_activations.h: the gradient of c * sum sigmoid(p)) or c exp(p) (of c * sum exp(p)): the two
// 3DGS-MCMC regularisers, folded in.  Every coefficient comes from the host, formed in float64 and rounded once (omb = 1 - beta from the
// unrounded beta: torch's convention, which the sparse kernel's in-kernel 1.0f - b is not), per tensor.  The g stream is only read.  Both
// divisions are the correctly rounded one; the root is the same __fsqrt_rn as above, the approximate v_sqrt_f32 between two v_ldexp_f32,
// and the step's bits are pinned as they are.  No atomics, no LDS, no scratch; equal inputs give equal bits, on either path.
#include "stp_activations.h"
#include "stp_internal.h"
#include "stp_row_table.h"

namespace stp {

namespace {

constexpr int ADAM_BLOCK = ROW_BLOCK;
constexpr int ADAM_PIECES = 4;                              // 16-byte pieces a thread owns in its unit
constexpr uint32_t ADAM_UNIT = ADAM_BLOCK * ADAM_PIECES * 4; // elements of a work unit (4096: 16 KiB of each stream)

struct AdamDesc {
    float* p;
    const float* g;
    float* m;
    float* v;
    uint32_t M, numel;
    float lr, eps;
    uint32_t first_unit; // of this tensor among the launch's units
    uint32_t wide;       // 16-byte accesses (all four pointers aligned)
    AdamDivisor div;     // e / M
};
struct AdamTable {
    AdamDesc t[ROW_TABLE_ENTRIES];
};

template <int KIND> __device__ __forceinline__ bool row_visible(const void* __restrict__ visible, uint32_t row)
{
    if constexpr (KIND == 0) return static_cast<const uint8_t*>(visible)[row] != 0;
    else return static_cast<const int32_t*>(visible)[row] > 0;
}

struct AdamCoef { float b1, omb1, b2, omb2, lr, eps; };

// one element's step (fused multiply-adds written out, so that the result does not hang on the compiler's contraction choices)
__device__ __forceinline__ void adam_element(float& p, const float g, float& m, float& v, const AdamCoef& c)
{
    m = __fmaf_rn(c.b1, m, c.omb1 * g);
    v = __fmaf_rn(c.omb2 * g, g, c.b2 * v);
    p = p - (c.lr * m) / (__fsqrt_rn(v) + c.eps);
}

template <int KIND>
__global__ void __launch_bounds__(ADAM_BLOCK) sparse_adam_kernel(const AdamTable table, const int n_tensors, const void* __restrict__ visible,
                                                                 const float b1, const float b2)
{
    const uint32_t unit = blockIdx.x;
    const AdamDesc& d = row_table_entry(table, n_tensors, unit);
    const uint32_t M = d.M, numel = d.numel;
    const AdamDivisor div = d.div;
    const AdamCoef c = {b1, 1.0f - b1, b2, 1.0f - b2, d.lr, d.eps};
    float* __restrict__ const P = d.p;
    const float* __restrict__ const G = d.g;
    float* __restrict__ const Mo = d.m;
    float* __restrict__ const V = d.v;
    const uint32_t base = (unit - d.first_unit) * ADAM_UNIT; // < numel < 2^31
    const uint32_t tid = threadIdx.x;

    if (d.wide) {
        const uint32_t numel4 = numel & ~3u;
#pragma unroll
        for (int k = 0; k < ADAM_PIECES; k++) {
            const uint32_t e0 = base + 4u * (tid + (uint32_t)k * ADAM_BLOCK);
            if (e0 >= numel4) break; // (e0 + 3 < numel4 <= numel: whole pieces only)
            uint32_t row = adam_div(e0, div), rem = e0 - row * M;
            bool vis[4];
            vis[0] = row_visible<KIND>(visible, row);
#pragma unroll
            for (int j = 1; j < 4; j++) {
                vis[j] = vis[j - 1];
                if (++rem == M) { // the next row begins inside the piece
                    rem = 0;
                    row++;
                    vis[j] = row_visible<KIND>(visible, row);
                }
            }
            if (!(vis[0] | vis[1] | vis[2] | vis[3])) continue; // nothing visible: no load, no store
            const uint32_t q = e0 >> 2;
            f32x4 p = reinterpret_cast<f32x4*>(P)[q], m = reinterpret_cast<f32x4*>(Mo)[q], v = reinterpret_cast<f32x4*>(V)[q];
            const f32x4 g = reinterpret_cast<const f32x4*>(G)[q];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float pj = p[j], mj = m[j], vj = v[j];
                adam_element(pj, g[j], mj, vj, c);
                p[j] = vis[j] ? pj : p[j]; // (an invisible lane keeps the bits that were loaded, whatever its g holds)
                m[j] = vis[j] ? mj : m[j];
                v[j] = vis[j] ? vj : v[j];
            }
            reinterpret_cast<f32x4*>(P)[q] = p;
            reinterpret_cast<f32x4*>(Mo)[q] = m;
            reinterpret_cast<f32x4*>(V)[q] = v;
        }
        // the tensor's last numel % 4 elements: threads 0 .. 2 of its last unit
        const uint32_t e = numel4 + tid;
        if (e < numel && numel - base <= ADAM_UNIT) {
            if (row_visible<KIND>(visible, adam_div(e, div))) {
                float pj = P[e], mj = Mo[e], vj = V[e];
                adam_element(pj, G[e], mj, vj, c);
                P[e] = pj;
                Mo[e] = mj;
                V[e] = vj;
            }
        }
    } else {
#pragma unroll 4
        for (int k = 0; k < ADAM_PIECES * 4; k++) {
            const uint32_t e = base + tid + (uint32_t)k * ADAM_BLOCK;
            if (e >= numel) break;
            if (!row_visible<KIND>(visible, adam_div(e, div))) continue;
            float pj = P[e], mj = Mo[e], vj = V[e];
            adam_element(pj, G[e], mj, vj, c);
            P[e] = pj;
            Mo[e] = mj;
            V[e] = vj;
        }
    }
}

// ---- the dense, bias-corrected step (stp_dense_adam) ----
struct DenseAdamCoef { float b1, omb1, b2, omb2, step_size, bias2_sqrt, eps, reg_coef; };
struct DenseAdamDesc {
    float* p;
    const float* g;
    float* m;
    float* v;
    uint32_t numel;
    uint32_t first_unit; // of this tensor among the launch's units
    uint32_t wide;       // 16-byte accesses (all four pointers aligned)
    int32_t reg_kind;    // 0: none, 1: sigmoid, 2: exp
    DenseAdamCoef c;
};
struct DenseAdamTable {
    DenseAdamDesc t[ROW_TABLE_ENTRIES];
};

// one element's step, the one both paths call (every operation a correctly rounded one that no contraction setting can merge, expf and
// the root excepted); reg_kind is uniform over the workgroup
__device__ __forceinline__ void dense_adam_element(float& p, const float g, float& m, float& v, const DenseAdamCoef& c, const int reg_kind)
{
    float r = 0.0f;
    if (reg_kind == 1) {
        const float s = activate_opacity(p);
        r = __fmul_rn(c.reg_coef, __fmul_rn(s, __fsub_rn(1.0f, s)));
    } else if (reg_kind == 2) {
        r = __fmul_rn(c.reg_coef, activate_scale(p));
    }
    const float gr = __fadd_rn(g, r);
    m = __fmaf_rn(c.b1, m, __fmul_rn(c.omb1, gr));
    v = __fmaf_rn(__fmul_rn(c.omb2, gr), gr, __fmul_rn(c.b2, v));
    const float den = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), c.bias2_sqrt), c.eps);
    p = __fsub_rn(p, __fdiv_rn(__fmul_rn(c.step_size, m), den));
}

__global__ void __launch_bounds__(ADAM_BLOCK) dense_adam_kernel(const DenseAdamTable table, const int n_tensors)
{
    const uint32_t unit = blockIdx.x;
    const DenseAdamDesc& d = row_table_entry(table, n_tensors, unit);
    const uint32_t numel = d.numel;
    const DenseAdamCoef c = d.c;
    const int kind = d.reg_kind;
    float* __restrict__ const P = d.p;
    const float* __restrict__ const G = d.g;
    float* __restrict__ const Mo = d.m;
    float* __restrict__ const V = d.v;
    const uint32_t base = (unit - d.first_unit) * ADAM_UNIT; // < numel < 2^31
    const uint32_t tid = threadIdx.x;

    if (d.wide) {
        const uint32_t numel4 = numel & ~3u;
#pragma unroll
        for (int k = 0; k < ADAM_PIECES; k++) {
            const uint32_t e0 = base + 4u * (tid + (uint32_t)k * ADAM_BLOCK);
            if (e0 >= numel4) break; // (e0 + 3 < numel4 <= numel: whole pieces only)
            const uint32_t q = e0 >> 2;
            f32x4 p = reinterpret_cast<f32x4*>(P)[q], m = reinterpret_cast<f32x4*>(Mo)[q], v = reinterpret_cast<f32x4*>(V)[q];
            const f32x4 g = reinterpret_cast<const f32x4*>(G)[q];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float pj = p[j], mj = m[j], vj = v[j];
                dense_adam_element(pj, g[j], mj, vj, c, kind);
                p[j] = pj;
                m[j] = mj;
                v[j] = vj;
            }
            reinterpret_cast<f32x4*>(P)[q] = p;
            reinterpret_cast<f32x4*>(Mo)[q] = m;
            reinterpret_cast<f32x4*>(V)[q] = v;
        }
        // the tensor's last numel % 4 elements: threads 0 .. 2 of its last unit
        const uint32_t e = numel4 + tid;
        if (e < numel && numel - base <= ADAM_UNIT) {
            float pj = P[e], mj = Mo[e], vj = V[e];
            dense_adam_element(pj, G[e], mj, vj, c, kind);
            P[e] = pj;
            Mo[e] = mj;
            V[e] = vj;
        }
    } else {
#pragma unroll 4
        for (int k = 0; k < ADAM_PIECES * 4; k++) {
            const uint32_t e = base + tid + (uint32_t)k * ADAM_BLOCK;
            if (e >= numel) break;
            float pj = P[e], mj = Mo[e], vj = V[e];
            dense_adam_element(pj, G[e], mj, vj, c, kind);
            P[e] = pj;
            Mo[e] = mj;
            V[e] = vj;
        }
    }
}

} // namespace

int launch_dense_adam(int n_tensors, const StpDenseAdamTensor* tensors, hipStream_t st, hipError_t* err)
{
    *err = hipSuccess;
    int launches = 0;
    for (int next = 0; next < n_tensors;) {
        DenseAdamTable table{};
        int n = 0;
        uint32_t units = 0;
        for (; next < n_tensors && n < ROW_TABLE_ENTRIES; next++) {
            const StpDenseAdamTensor& t = tensors[next];
            if (t.numel == 0) continue;
            DenseAdamDesc& d = table.t[n++];
            d.p = t.param; d.g = t.grad; d.m = t.exp_avg; d.v = t.exp_avg_sq;
            d.numel = (uint32_t)t.numel;
            d.first_unit = units;
            d.wide = aligned16(t.param, t.grad, t.exp_avg, t.exp_avg_sq);
            d.reg_kind = t.reg_kind;
            d.c = {t.beta1, t.one_minus_beta1, t.beta2, t.one_minus_beta2, t.step_size, t.bias2_sqrt, t.eps, t.reg_coef};
            units += (d.numel + ADAM_UNIT - 1) / ADAM_UNIT; // <= 2^19 per tensor
        }
        if (n == 0) break;
        hipLaunchKernelGGL(dense_adam_kernel, dim3(units), dim3(ADAM_BLOCK), 0, st, table, n);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) { *err = e; return launches; }
        launches++;
    }
    return launches;
}

int launch_sparse_adam(int n_tensors, const StpAdamTensor* tensors, int N, const void* visible, int visible_kind, float beta1, float beta2,
                       hipStream_t st, hipError_t* err)
{
    *err = hipSuccess;
    int launches = 0;
    for (int next = 0; next < n_tensors;) {
        AdamTable table{};
        int n = 0;
        uint32_t units = 0;
        for (; next < n_tensors && n < ROW_TABLE_ENTRIES; next++) {
            const StpAdamTensor& t = tensors[next];
            if (t.numel == 0) continue;
            AdamDesc& d = table.t[n++];
            d.p = t.param; d.g = t.grad; d.m = t.exp_avg; d.v = t.exp_avg_sq;
            d.numel = (uint32_t)t.numel;
            d.M = (uint32_t)(t.numel / N);
            d.lr = t.lr; d.eps = t.eps;
            d.first_unit = units;
            d.wide = aligned16(t.param, t.grad, t.exp_avg, t.exp_avg_sq);
            d.div = adam_divisor(d.M);
            units += (d.numel + ADAM_UNIT - 1) / ADAM_UNIT; // <= 2^19 per tensor
        }
        if (n == 0) break;
        if (visible_kind == 0) hipLaunchKernelGGL(sparse_adam_kernel<0>, dim3(units), dim3(ADAM_BLOCK), 0, st, table, n, visible, beta1, beta2);
        else hipLaunchKernelGGL(sparse_adam_kernel<1>, dim3(units), dim3(ADAM_BLOCK), 0, st, table, n, visible, beta1, beta2);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) { *err = e; return launches; }
        launches++;
    }
    return launches;
}

} // namespace stp
