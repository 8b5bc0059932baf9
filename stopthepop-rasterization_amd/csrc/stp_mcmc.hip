// stp_mcmc.hip -- the two kernels a 3DGS-MCMC trainer needs beside the rasterizer ("3D Gaussian Splatting as Markov Chain Monte Carlo";
// no counterpart in the reference): stp_mcmc_relocation (that project's compute_relocation) and stp_mcmc_add_noise (its per-iteration
// position noise, fused into one pass).  Both are streaming kernels without atomics, LDS or scratch: equal inputs give equal bits
// whatever the launch shape.
//
// Relocation.  One Gaussian per lane.  A Gaussian of opacity o and scales s that is replaced by N copies of itself gets
//     o_new = 1 - (1 - o)^(1/N)
//     denom = sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k o_new^(k+1) / sqrt(k+1),      s_new = (o / denom) s
// EVALUATION ORDER.  The double sum is collapsed with sum_{i=k+1..N} C(i-1, k) = C(N, k+1) to the N terms
//     denom = sum_{k=0..N-1} C(N, k+1) (-1)^k o_new^(k+1) / sqrt(k+1)
// and summed in ascending k IN FLOAT64: term k is (c_k * p_k) / sqrt(k + 1) with the binomial c_k = C(N, k+1) from the recurrence
// c_{k+1} = c_k (N - k - 1) / (k + 2) (every product is an integer below 2^53 for N <= 50 and every quotient an integer: exact) and the
// signed power p_k = (-1)^k o_new^(k+1) from p_{k+1} = p_k * (-o_new).  The terms alternate and reach 7e3 times the sum (o near 1, N = 50):
// a float32 accumulator loses 5e-4 there, the float64 one 1e-12.  o_new = -expm1(log1p(-o) / N) in float64 keeps its digits at small o,
// where 1 - pow(1 - o, 1 / N) cancels.  Every float64 operation is written out (__dmul_rn ...), so that the result does not hang on the
// compiler's contraction choices; the only roundings to float32 are those of the two results.  At most 50 float64 divisions and square roots
// per Gaussian: a relocation of 50 000 Gaussians is a few microseconds of VALU work beside its launch.
//
// Noise.  xyz[i] += R diag(s^2) R^T (noise[i] * g * noise_scale), g = 1 / (1 + exp(-k ((1 - o) - x0))), R the rotation of the normalised
// quaternion (w, x, y, z), in float32 with every multiply-add written out: v = (noise * g) * noise_scale, u = R^T v, u *= s * s, d = R u,
// xyz += d -- Sigma itself is never formed.  raw: o = 1 / (1 + exp(-opacity)) and s = exp(scale) first.  The quaternion's norm is __fsqrt_rn,
// which in this toolchain is the hardware's approximate v_sqrt_f32 between two v_ldexp_f32 (denormal pre-scaling), without a refinement step -- not
// the correctly rounded root; the divisions by it are correctly rounded.  The kernel's bits stay as they are.
// Streaming shape.  Where all five pointers are 16-byte aligned a lane owns FOUR consecutive Gaussians: their 48 bytes of xyz, of scales
// and of noise are three 16-byte pieces each, their quaternions four and their opacities one -- 14 loads and 3 stores of 16 bytes, every
// one aligned, and a wave covers 3 KiB contiguous of each (P, 3) stream.  The last P % 4 Gaussians belong to the lane after the last
// whole group, one float per access.  With an unaligned pointer a lane owns one Gaussian, one float per access.  The arithmetic of a
// Gaussian is the same function on every path.
#include "stp_internal.h"
#include "stp_mcmc_relocation.h"
#include "stp_row_table.h"

namespace stp {

namespace {

constexpr int MCMC_BLOCK = 256;

template <typename NT>
__global__ void __launch_bounds__(MCMC_BLOCK) mcmc_relocation_kernel(const uint32_t n, const float* __restrict__ opacity_old, const float* __restrict__ scale_old,
                                                                      const NT* __restrict__ N, const int n_cap, float* __restrict__ opacity_new,
                                                                      float* __restrict__ scale_new)
{
    const uint32_t i = blockIdx.x * (uint32_t)MCMC_BLOCK + threadIdx.x; // (< 2^31 + 256)
    if (i >= n) return;
    const long long asked = (long long)N[i];
    const int copies = asked < 1 ? 1 : asked > n_cap ? n_cap : (int)asked;
    double x, coef;
    mcmc_relocation_row(opacity_old[i], copies, x, coef);
    opacity_new[i] = (float)x;
    const size_t e = 3 * (size_t)i;
#pragma unroll
    for (int j = 0; j < 3; j++) scale_new[e + j] = (float)__dmul_rn(coef, (double)scale_old[e + j]);
}

struct NoiseCoef { float noise_scale, k, x0; };

// one Gaussian's step: pos (3 floats) += R diag(s^2) R^T v
template <bool RAW>
__device__ __forceinline__ void noise_row(float* pos, const float* scl, const float* q, const float opacity, const float* nz, const NoiseCoef& c)
{
    const float o = RAW ? __fdiv_rn(1.0f, 1.0f + expf(-opacity)) : opacity;
    const float g = __fdiv_rn(1.0f, 1.0f + expf(-__fmul_rn(c.k, (1.0f - o) - c.x0)));
    float v[3], s2[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const float s = RAW ? expf(scl[j]) : scl[j];
        s2[j] = __fmul_rn(s, s);
        v[j] = __fmul_rn(__fmul_rn(nz[j], g), c.noise_scale);
    }
    const float norm = __fsqrt_rn(__fmaf_rn(q[3], q[3], __fmaf_rn(q[2], q[2], __fmaf_rn(q[1], q[1], __fmul_rn(q[0], q[0])))));
    const float r = __fdiv_rn(q[0], norm), x = __fdiv_rn(q[1], norm), y = __fdiv_rn(q[2], norm), z = __fdiv_rn(q[3], norm);
    const float R00 = 1.0f - 2.0f * __fmaf_rn(y, y, __fmul_rn(z, z)), R01 = 2.0f * __fmaf_rn(x, y, -__fmul_rn(r, z)), R02 = 2.0f * __fmaf_rn(x, z, __fmul_rn(r, y));
    const float R10 = 2.0f * __fmaf_rn(x, y, __fmul_rn(r, z)), R11 = 1.0f - 2.0f * __fmaf_rn(x, x, __fmul_rn(z, z)), R12 = 2.0f * __fmaf_rn(y, z, -__fmul_rn(r, x));
    const float R20 = 2.0f * __fmaf_rn(x, z, -__fmul_rn(r, y)), R21 = 2.0f * __fmaf_rn(y, z, __fmul_rn(r, x)), R22 = 1.0f - 2.0f * __fmaf_rn(x, x, __fmul_rn(y, y));
    const float u0 = __fmul_rn(s2[0], __fmaf_rn(R20, v[2], __fmaf_rn(R10, v[1], __fmul_rn(R00, v[0]))));
    const float u1 = __fmul_rn(s2[1], __fmaf_rn(R21, v[2], __fmaf_rn(R11, v[1], __fmul_rn(R01, v[0]))));
    const float u2 = __fmul_rn(s2[2], __fmaf_rn(R22, v[2], __fmaf_rn(R12, v[1], __fmul_rn(R02, v[0]))));
    pos[0] = __fadd_rn(pos[0], __fmaf_rn(R02, u2, __fmaf_rn(R01, u1, __fmul_rn(R00, u0))));
    pos[1] = __fadd_rn(pos[1], __fmaf_rn(R12, u2, __fmaf_rn(R11, u1, __fmul_rn(R10, u0))));
    pos[2] = __fadd_rn(pos[2], __fmaf_rn(R22, u2, __fmaf_rn(R21, u1, __fmul_rn(R20, u0))));
}

// Gaussian i, one float per access
template <bool RAW>
__device__ __forceinline__ void noise_row_narrow(const size_t i, float* __restrict__ xyz, const float* __restrict__ scales, const float* __restrict__ rotations,
                                                 const float* __restrict__ opacities, const float* __restrict__ noise, const NoiseCoef& c)
{
    float pos[3], scl[3], nz[3], q[4];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        pos[j] = xyz[3 * i + j];
        scl[j] = scales[3 * i + j];
        nz[j] = noise[3 * i + j];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = rotations[4 * i + j];
    noise_row<RAW>(pos, scl, q, opacities[i], nz, c);
#pragma unroll
    for (int j = 0; j < 3; j++) xyz[3 * i + j] = pos[j];
}

// WIDE: thread t owns Gaussians 4t .. 4t + 3 (all pointers 16-byte aligned), thread P / 4 the last P % 4; otherwise thread t owns Gaussian t
template <bool RAW, bool WIDE>
__global__ void __launch_bounds__(MCMC_BLOCK) mcmc_noise_kernel(const uint32_t P, float* __restrict__ xyz, const float* __restrict__ scales,
                                                                 const float* __restrict__ rotations, const float* __restrict__ opacities,
                                                                 const float* __restrict__ noise, const NoiseCoef c)
{
    const uint32_t t = blockIdx.x * (uint32_t)MCMC_BLOCK + threadIdx.x;
    if constexpr (WIDE) {
        const uint32_t groups = P >> 2;
        if (t < groups) {
            const size_t t3 = 3 * (size_t)t, t4 = 4 * (size_t)t;
            f32x4 a[3], s[3], w[3], q[4];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                a[j] = reinterpret_cast<const f32x4*>(xyz)[t3 + j];
                s[j] = reinterpret_cast<const f32x4*>(scales)[t3 + j];
                w[j] = reinterpret_cast<const f32x4*>(noise)[t3 + j];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) q[j] = reinterpret_cast<const f32x4*>(rotations)[t4 + j];
            const f32x4 op = reinterpret_cast<const f32x4*>(opacities)[t];
            float pos[12], scl[12], nz[12];
#pragma unroll
            for (int j = 0; j < 12; j++) {
                pos[j] = a[j >> 2][j & 3];
                scl[j] = s[j >> 2][j & 3];
                nz[j] = w[j >> 2][j & 3];
            }
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const float quat[4] = {q[g][0], q[g][1], q[g][2], q[g][3]};
                noise_row<RAW>(pos + 3 * g, scl + 3 * g, quat, op[g], nz + 3 * g, c);
            }
#pragma unroll
            for (int j = 0; j < 3; j++) {
                f32x4 out;
#pragma unroll
                for (int e = 0; e < 4; e++) out[e] = pos[4 * j + e];
                reinterpret_cast<f32x4*>(xyz)[t3 + j] = out;
            }
        } else if (t == groups) {
            for (uint32_t i = groups << 2; i < P; i++) noise_row_narrow<RAW>(i, xyz, scales, rotations, opacities, noise, c);
        }
    } else {
        if (t < P) noise_row_narrow<RAW>(t, xyz, scales, rotations, opacities, noise, c);
    }
}

} // namespace

int launch_mcmc_relocation(int n, const float* opacity_old, const float* scale_old, const void* N, int n_kind, int n_max, float* opacity_new,
                           float* scale_new, hipStream_t st, hipError_t* err)
{
    const dim3 grid(((uint32_t)n + MCMC_BLOCK - 1) / MCMC_BLOCK), block(MCMC_BLOCK);
    if (n_kind == 0)
        hipLaunchKernelGGL(mcmc_relocation_kernel<int32_t>, grid, block, 0, st, (uint32_t)n, opacity_old, scale_old, static_cast<const int32_t*>(N), n_max - 1,
                           opacity_new, scale_new);
    else
        hipLaunchKernelGGL(mcmc_relocation_kernel<int64_t>, grid, block, 0, st, (uint32_t)n, opacity_old, scale_old, static_cast<const int64_t*>(N), n_max - 1,
                           opacity_new, scale_new);
    *err = hipGetLastError();
    return *err == hipSuccess ? 1 : 0;
}

int launch_mcmc_add_noise(int P, float* xyz, const float* scales, const float* rotations, const float* opacities, const float* noise, float noise_scale,
                          float k, float x0, int raw, hipStream_t st, hipError_t* err)
{
    const NoiseCoef c = {noise_scale, k, x0};
    const bool wide = aligned16(xyz, scales, rotations, opacities, noise);
    const uint32_t threads = wide ? ((uint32_t)P + 3) / 4 : (uint32_t)P; // (wide: P / 4 groups and, where P % 4, the thread of the tail)
    const dim3 grid((threads + MCMC_BLOCK - 1) / MCMC_BLOCK), block(MCMC_BLOCK);
    if (wide) {
        if (raw) hipLaunchKernelGGL((mcmc_noise_kernel<true, true>), grid, block, 0, st, (uint32_t)P, xyz, scales, rotations, opacities, noise, c);
        else hipLaunchKernelGGL((mcmc_noise_kernel<false, true>), grid, block, 0, st, (uint32_t)P, xyz, scales, rotations, opacities, noise, c);
    } else {
        if (raw) hipLaunchKernelGGL((mcmc_noise_kernel<true, false>), grid, block, 0, st, (uint32_t)P, xyz, scales, rotations, opacities, noise, c);
        else hipLaunchKernelGGL((mcmc_noise_kernel<false, false>), grid, block, 0, st, (uint32_t)P, xyz, scales, rotations, opacities, noise, c);
    }
    *err = hipGetLastError();
    return *err == hipSuccess ? 1 : 0;
}

} // namespace stp
