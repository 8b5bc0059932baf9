// stp_mip_filter.hip -- Mip-Splatting's 3D smoothing filter ("Mip-Splatting: Alias-free 3D Gaussian Splatting"; no counterpart in the reference):
// stp_mip_filter_3d (that project's compute_3D_filter over all training cameras in one pass) and stp_mip_activations_forward / _backward (its
// get_scaling_with_3D_filter and get_opacity_with_3D_filter with their chain rule).  Streaming kernels without float atomics and without scratch:
// equal inputs give equal bits whatever the launch shape.
//
// Filter.  One Gaussian per lane, the camera loop inside the kernel, xyz read once.  The camera's numbers -- M[:3, :3] and M[3, :3] of its
// world-view matrix (row-vector layout, p_cam = [p, 1] @ M) and (focal_x, focal_y, width, height) -- are read at a wave-uniform index from
// read-only memory: they arrive as scalar loads, no lane loads them.
// EVALUATION ORDER, float32, per camera, k = 0, 1, 2 for x, y, z:
//     p_cam[k] = fma(p2, M[2][k], fma(p1, M[1][k], fma(p0, M[0][k], M[3][k])))
//     valid    = z > 0.2  and  |x * focal_x| <= (0.65 * width) * z  and  |y * focal_y| <= (0.65 * height) * z
//     distance = min(distance, z) where valid                                                            (initial value 100000)
// The screen test is the division-free form of  -0.15 W <= x / max(z, 0.001) * focal_x + W / 2 <= 1.15 W:  behind z > 0.2 the clamp of z is
// idle, z is positive, and the two bounds are -0.65 W and 0.65 W around W / 2.  Every comparison with a NaN is false: a NaN coordinate is never
// valid.  On inputs 1e-4 (relative to 0.2, the width and the height) away from every threshold each decision is the float64 one
// (tests/test_mip_filter_cpu.py).  A row that no camera sees is stored as -1 by the first kernel; the largest distance of the other rows is
// reduced per wave and per workgroup and joins the 4-byte workspace by an unsigned integer maximum on the float's bits (the distances are
// positive, so the two orders agree; a maximum does not depend on the order of its operands).  The second kernel gives the rows without a
// camera that maximum -- 100000 where no row at all has a camera -- and scales:  filter_3d = (distance / max_c(focal_x)) * sqrtf(0.2), the
// division correctly rounded, max_c(focal_x) over ALL cameras by fmaxf in every workgroup.
//
// Activations.  With e = expf(scaling_j), f = filter_3d, per row in float32:
//     e2 = e * e     f2 = f * f     d = fma(e, e, f2)     scales_j = sqrt(d)     r_j = e2 / d     q_j = f2 / d  (= 1 - r_j without the cancellation)
//     sig = 1 / (1 + expf(-opacity))      c = sqrt((r_0 * r_1) * r_2)      opacities = sig * c
//     grad_scaling_j = g_s_j * (e2 / scales_j) + (g_o * opacities) * q_j         grad_opacity = ((g_o * c) * sig) * (1 / (1 + expf(opacity)))
// the last factor being 1 - sig without the cancellation at large logits (3e-4 relative at a logit of 9 otherwise), the sum of grad_scaling_j
// one fma (written out, like d: a product next to a sum that the compiler may or may not contract would give the two paths different bits);
// sqrt is __fsqrt_rn (the hardware's root between two scalings, within an ulp), every division is correctly rounded.  The ratio form equals
// upstream's sqrt(prod e2 / prod d) without pushing the two determinants into the denormal range.
// An absent upstream gradient (NULL) counts as zero.  IEEE arithmetic as written: f = 0 with an e2 that underflows to 0 is 0 / 0.
// Streaming shape (that of mcmc_noise_kernel): where every pointer is 16-byte aligned a lane owns FOUR consecutive rows -- three 16-byte pieces
// of each (P, 3) stream and one of each (P,) stream -- and the last P % 4 rows belong to the lane after the last whole group, one float per
// access.  With an unaligned pointer a lane owns one row, one float per access.  The arithmetic of a row is the same function on every path.
#include "stp_internal.h"
#include "stp_activations.h"
#include "stp_row_table.h"

namespace stp {

namespace {

constexpr int MIP_BLOCK = 256;
constexpr float MIP_FAR = 100000.0f;      // the distance of a row before any camera has seen it
constexpr float MIP_NEAR = 0.2f;          // valid_depth = z > MIP_NEAR
constexpr float MIP_HALF_SCREEN = 0.65f;  // 0.5 + 0.15: half the screen and its 15 % border, in widths
constexpr float MIP_SQRT_02 = 0.4472135955f; // sqrt(0.2)

__global__ void __launch_bounds__(MIP_BLOCK) mip_filter_kernel(const uint32_t P, const uint32_t C, const float* __restrict__ xyz, const float* __restrict__ views,
                                                                const float* __restrict__ intrinsics, uint32_t* __restrict__ max_bits, float* __restrict__ out)
{
    __shared__ uint32_t wave_max[MIP_BLOCK / 64];
    const uint32_t i = blockIdx.x * (uint32_t)MIP_BLOCK + threadIdx.x;
    const bool live = i < P;
    const size_t e = 3 * (size_t)(live ? i : 0);
    const float p0 = xyz[e], p1 = xyz[e + 1], p2 = xyz[e + 2];
    float distance = MIP_FAR;
    bool any = false;
    for (uint32_t c = 0; c < C; c++) { // (c is wave-uniform: M and K are scalar loads)
        const float* __restrict__ M = views + 16 * (size_t)c;
        const float* __restrict__ K = intrinsics + 4 * (size_t)c;
        const float x = __fmaf_rn(p2, M[8], __fmaf_rn(p1, M[4], __fmaf_rn(p0, M[0], M[12])));
        const float y = __fmaf_rn(p2, M[9], __fmaf_rn(p1, M[5], __fmaf_rn(p0, M[1], M[13])));
        const float z = __fmaf_rn(p2, M[10], __fmaf_rn(p1, M[6], __fmaf_rn(p0, M[2], M[14])));
        const float lim_x = __fmul_rn(__fmul_rn(MIP_HALF_SCREEN, K[2]), z), lim_y = __fmul_rn(__fmul_rn(MIP_HALF_SCREEN, K[3]), z);
        const bool valid = z > MIP_NEAR && fabsf(__fmul_rn(x, K[0])) <= lim_x && fabsf(__fmul_rn(y, K[1])) <= lim_y;
        distance = valid ? fminf(distance, z) : distance;
        any = any || valid;
    }
    any = any && live;
    if (live) out[i] = any ? distance : -1.0f;
    uint32_t m = any ? __float_as_uint(distance) : 0u; // (distance > 0.2: the unsigned order of the bits is the order of the floats)
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < MIP_BLOCK / 64; w++) m = max(m, wave_max[w]);
        if (m != 0u) atomicMax(max_bits, m);
    }
}

// out[i]: the distance of row i, or -1 where no camera sees it -> filter_3d[i]
__global__ void __launch_bounds__(MIP_BLOCK) mip_filter_finish_kernel(const uint32_t P, const uint32_t C, const float* __restrict__ intrinsics,
                                                                       const uint32_t* __restrict__ max_bits, float* __restrict__ out)
{
    __shared__ float wave_focal[MIP_BLOCK / 64];
    float focal = -INFINITY;
    for (uint32_t c = threadIdx.x; c < C; c += MIP_BLOCK) focal = fmaxf(focal, intrinsics[4 * (size_t)c]);
    for (int off = 32; off > 0; off >>= 1) focal = fmaxf(focal, __shfl_xor(focal, off, 64));
    if ((threadIdx.x & 63) == 0) wave_focal[threadIdx.x >> 6] = focal;
    __syncthreads();
    focal = fmaxf(fmaxf(wave_focal[0], wave_focal[1]), fmaxf(wave_focal[2], wave_focal[3]));
    static_assert(MIP_BLOCK / 64 == 4, "the four waves of a workgroup");
    const uint32_t i = blockIdx.x * (uint32_t)MIP_BLOCK + threadIdx.x;
    if (i >= P) return;
    const uint32_t bits = *max_bits;
    const float fill = bits != 0u ? __uint_as_float(bits) : MIP_FAR;
    const float d = out[i];
    out[i] = __fmul_rn(__fdiv_rn(d > 0.0f ? d : fill, focal), MIP_SQRT_02);
}

// ---- the filtered activations ----------------------------------------------------------------------------------------------------------------

struct MipRow { float e2[3], d[3], scl[3], r[3], sig, c, opa; };

__device__ __forceinline__ MipRow mip_row(const float* s, const float o, const float f)
{
    MipRow w;
    const float f2 = __fmul_rn(f, f);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const float ex = activate_scale(s[j]);
        w.e2[j] = __fmul_rn(ex, ex);
        w.d[j] = __fmaf_rn(ex, ex, f2);
        w.scl[j] = __fsqrt_rn(w.d[j]);
        w.r[j] = __fdiv_rn(w.e2[j], w.d[j]);
    }
    w.sig = activate_opacity(o);
    w.c = __fsqrt_rn(__fmul_rn(__fmul_rn(w.r[0], w.r[1]), w.r[2]));
    w.opa = __fmul_rn(w.sig, w.c);
    return w;
}

__device__ __forceinline__ void mip_forward_row(const float* s, const float o, const float f, float* scales, float& opacity)
{
    const MipRow w = mip_row(s, o, f);
#pragma unroll
    for (int j = 0; j < 3; j++) scales[j] = w.scl[j];
    opacity = w.opa;
}

// gs: the three upstream gradients of the scales, go: that of the opacity (zeros where absent)
__device__ __forceinline__ void mip_backward_row(const float* s, const float o, const float f, const float* gs, const float go, float* g_scaling, float& g_opacity)
{
    const MipRow w = mip_row(s, o, f);
    const float f2 = __fmul_rn(f, f), t = __fmul_rn(go, w.opa);
#pragma unroll
    for (int j = 0; j < 3; j++) g_scaling[j] = __fmaf_rn(gs[j], __fdiv_rn(w.e2[j], w.scl[j]), __fmul_rn(t, __fdiv_rn(f2, w.d[j])));
    g_opacity = __fmul_rn(__fmul_rn(__fmul_rn(go, w.c), w.sig), activate_opacity(-o)); // (1 - sig = sigmoid(-o))
}

__device__ __forceinline__ void unpack3(const float* __restrict__ p, const size_t t3, float* v)
{
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const f32x4 a = reinterpret_cast<const f32x4*>(p)[t3 + j];
#pragma unroll
        for (int e = 0; e < 4; e++) v[4 * j + e] = a[e];
    }
}

__device__ __forceinline__ void pack3(float* __restrict__ p, const size_t t3, const float* v)
{
#pragma unroll
    for (int j = 0; j < 3; j++) {
        f32x4 a;
#pragma unroll
        for (int e = 0; e < 4; e++) a[e] = v[4 * j + e];
        reinterpret_cast<f32x4*>(p)[t3 + j] = a;
    }
}

__device__ __forceinline__ void mip_forward_narrow(const size_t i, const float* __restrict__ scaling, const float* __restrict__ opacity, const float* __restrict__ filter,
                                                   float* __restrict__ scales, float* __restrict__ opacities)
{
    const float s[3] = {scaling[3 * i], scaling[3 * i + 1], scaling[3 * i + 2]};
    float out[3], o;
    mip_forward_row(s, opacity[i], filter[i], out, o);
#pragma unroll
    for (int j = 0; j < 3; j++) scales[3 * i + j] = out[j];
    opacities[i] = o;
}

// WIDE: thread t owns rows 4t .. 4t + 3 (all pointers 16-byte aligned), thread P / 4 the last P % 4; otherwise thread t owns row t
template <bool WIDE>
__global__ void __launch_bounds__(MIP_BLOCK) mip_activations_forward_kernel(const uint32_t P, const float* __restrict__ scaling, const float* __restrict__ opacity,
                                                                             const float* __restrict__ filter, float* __restrict__ scales, float* __restrict__ opacities)
{
    const uint32_t t = blockIdx.x * (uint32_t)MIP_BLOCK + threadIdx.x;
    if constexpr (WIDE) {
        const uint32_t groups = P >> 2;
        if (t < groups) {
            float s[12], out[12];
            unpack3(scaling, 3 * (size_t)t, s);
            const f32x4 o = reinterpret_cast<const f32x4*>(opacity)[t], f = reinterpret_cast<const f32x4*>(filter)[t];
            f32x4 oo;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                float v;
                mip_forward_row(s + 3 * g, o[g], f[g], out + 3 * g, v);
                oo[g] = v;
            }
            pack3(scales, 3 * (size_t)t, out);
            reinterpret_cast<f32x4*>(opacities)[t] = oo;
        } else if (t == groups) {
            for (uint32_t i = groups << 2; i < P; i++) mip_forward_narrow(i, scaling, opacity, filter, scales, opacities);
        }
    } else {
        if (t < P) mip_forward_narrow(t, scaling, opacity, filter, scales, opacities);
    }
}

__device__ __forceinline__ void mip_backward_narrow(const size_t i, const float* __restrict__ scaling, const float* __restrict__ opacity, const float* __restrict__ filter,
                                                    const float* __restrict__ g_scales, const float* __restrict__ g_opacities, float* __restrict__ g_scaling,
                                                    float* __restrict__ g_opacity)
{
    const float s[3] = {scaling[3 * i], scaling[3 * i + 1], scaling[3 * i + 2]};
    float gs[3] = {0.0f, 0.0f, 0.0f}, out[3], o;
    if (g_scales) {
#pragma unroll
        for (int j = 0; j < 3; j++) gs[j] = g_scales[3 * i + j];
    }
    mip_backward_row(s, opacity[i], filter[i], gs, g_opacities ? g_opacities[i] : 0.0f, out, o);
#pragma unroll
    for (int j = 0; j < 3; j++) g_scaling[3 * i + j] = out[j];
    g_opacity[i] = o;
}

// g_scales, g_opacities: either may be nullptr (zeros)
template <bool WIDE>
__global__ void __launch_bounds__(MIP_BLOCK) mip_activations_backward_kernel(const uint32_t P, const float* __restrict__ scaling, const float* __restrict__ opacity,
                                                                              const float* __restrict__ filter, const float* __restrict__ g_scales,
                                                                              const float* __restrict__ g_opacities, float* __restrict__ g_scaling, float* __restrict__ g_opacity)
{
    const uint32_t t = blockIdx.x * (uint32_t)MIP_BLOCK + threadIdx.x;
    if constexpr (WIDE) {
        const uint32_t groups = P >> 2;
        if (t < groups) {
            float s[12], gs[12], out[12];
            unpack3(scaling, 3 * (size_t)t, s);
            if (g_scales) unpack3(g_scales, 3 * (size_t)t, gs);
            else {
#pragma unroll
                for (int j = 0; j < 12; j++) gs[j] = 0.0f;
            }
            const f32x4 o = reinterpret_cast<const f32x4*>(opacity)[t], f = reinterpret_cast<const f32x4*>(filter)[t];
            f32x4 go = {0.0f, 0.0f, 0.0f, 0.0f}, oo;
            if (g_opacities) go = reinterpret_cast<const f32x4*>(g_opacities)[t];
#pragma unroll
            for (int g = 0; g < 4; g++) {
                float v;
                mip_backward_row(s + 3 * g, o[g], f[g], gs + 3 * g, go[g], out + 3 * g, v);
                oo[g] = v;
            }
            pack3(g_scaling, 3 * (size_t)t, out);
            reinterpret_cast<f32x4*>(g_opacity)[t] = oo;
        } else if (t == groups) {
            for (uint32_t i = groups << 2; i < P; i++) mip_backward_narrow(i, scaling, opacity, filter, g_scales, g_opacities, g_scaling, g_opacity);
        }
    } else {
        if (t < P) mip_backward_narrow(t, scaling, opacity, filter, g_scales, g_opacities, g_scaling, g_opacity);
    }
}

dim3 mip_grid(const int P, const bool wide)
{
    const uint32_t threads = wide ? ((uint32_t)P >> 2) + 1 : (uint32_t)P; // (wide: P / 4 groups and the thread of the tail)
    return dim3((threads + MIP_BLOCK - 1) / MIP_BLOCK);
}

} // namespace

int launch_mip_filter_3d(int P, int C, const float* xyz, const float* views, const float* intrinsics, void* workspace, float* filter_3d, hipStream_t st, hipError_t* err)
{
    uint32_t* const max_bits = static_cast<uint32_t*>(workspace);
    *err = hipMemsetAsync(max_bits, 0, sizeof(uint32_t), st); // (the running maximum starts below every distance)
    if (*err != hipSuccess) return 0;
    const dim3 grid(((uint32_t)P + MIP_BLOCK - 1) / MIP_BLOCK), block(MIP_BLOCK);
    hipLaunchKernelGGL(mip_filter_kernel, grid, block, 0, st, (uint32_t)P, (uint32_t)C, xyz, views, intrinsics, max_bits, filter_3d);
    *err = hipGetLastError();
    if (*err != hipSuccess) return 0;
    hipLaunchKernelGGL(mip_filter_finish_kernel, grid, block, 0, st, (uint32_t)P, (uint32_t)C, intrinsics, max_bits, filter_3d);
    *err = hipGetLastError();
    return *err == hipSuccess ? 2 : 1;
}

int launch_mip_activations_forward(int P, const float* scaling, const float* opacity, const float* filter_3d, float* scales, float* opacities, hipStream_t st,
                                   hipError_t* err)
{
    const bool wide = aligned16(scaling, opacity, filter_3d, scales, opacities);
    const dim3 grid = mip_grid(P, wide), block(MIP_BLOCK);
    if (wide) hipLaunchKernelGGL(mip_activations_forward_kernel<true>, grid, block, 0, st, (uint32_t)P, scaling, opacity, filter_3d, scales, opacities);
    else hipLaunchKernelGGL(mip_activations_forward_kernel<false>, grid, block, 0, st, (uint32_t)P, scaling, opacity, filter_3d, scales, opacities);
    *err = hipGetLastError();
    return *err == hipSuccess ? 1 : 0;
}

int launch_mip_activations_backward(int P, const float* scaling, const float* opacity, const float* filter_3d, const float* grad_scales, const float* grad_opacities,
                                    float* grad_scaling, float* grad_opacity, hipStream_t st, hipError_t* err)
{
    const bool wide = aligned16(scaling, opacity, filter_3d, grad_scales, grad_opacities, grad_scaling, grad_opacity); // (a null pointer counts as aligned)
    const dim3 grid = mip_grid(P, wide), block(MIP_BLOCK);
    if (wide)
        hipLaunchKernelGGL(mip_activations_backward_kernel<true>, grid, block, 0, st, (uint32_t)P, scaling, opacity, filter_3d, grad_scales, grad_opacities, grad_scaling,
                           grad_opacity);
    else
        hipLaunchKernelGGL(mip_activations_backward_kernel<false>, grid, block, 0, st, (uint32_t)P, scaling, opacity, filter_3d, grad_scales, grad_opacities, grad_scaling,
                           grad_opacity);
    *err = hipGetLastError();
    return *err == hipSuccess ? 1 : 0;
}

} // namespace stp
