// stp_activate.hip -- stp_activate_params: the activated copies of a trainer's raw parameters (no counterpart in the reference), for logging,
// export and tests.  The values are those the raw path of the rasterizer renders with, to the bit: the three functions of stp_activations.h,
// which preprocess_kernel and preprocess_backward_kernel call at their loads (stp_set_forward_raw_params / stp_set_backward_raw_params).
//
// HBM-streaming kernels flattened over elements: exp and sigmoid are elementwise, four floats per thread with 16-byte loads and stores where
// both pointers allow it; a quaternion is one 16-byte element.  One launch per pair of arrays given.
#include "stp_internal.h"
#include "stp_activations.h"

namespace stp {

namespace {

constexpr int ACT_BLOCK = 256;

enum ActKind { ACT_SCALE = 0, ACT_OPACITY = 1 };

template <int KIND>
__device__ __forceinline__ float activate_one(float x) { return KIND == ACT_SCALE ? activate_scale(x) : activate_opacity(x); }

// n floats, elementwise.  WIDE: thread t owns floats 4t .. 4t + 3 (both pointers 16-byte aligned), thread n / 4 the last n % 4
template <int KIND, bool WIDE>
__global__ void __launch_bounds__(ACT_BLOCK) activate_elements_kernel(const uint32_t n, const float* __restrict__ in, float* __restrict__ out)
{
    const uint32_t t = blockIdx.x * (uint32_t)ACT_BLOCK + threadIdx.x;
    if constexpr (WIDE) {
        const uint32_t groups = n >> 2;
        if (t < groups) {
            const float4 v = reinterpret_cast<const float4*>(in)[t];
            reinterpret_cast<float4*>(out)[t] = make_float4(activate_one<KIND>(v.x), activate_one<KIND>(v.y), activate_one<KIND>(v.z), activate_one<KIND>(v.w));
        } else if (t == groups) {
            for (uint32_t i = groups << 2; i < n; i++) out[i] = activate_one<KIND>(in[i]);
        }
    } else {
        if (t < n) out[t] = activate_one<KIND>(in[t]);
    }
}

// P quaternions, one per thread.  WIDE: 16-byte loads and stores
template <bool WIDE>
__global__ void __launch_bounds__(ACT_BLOCK) activate_rotations_kernel(const uint32_t P, const float* __restrict__ in, float* __restrict__ out)
{
    const uint32_t t = blockIdx.x * (uint32_t)ACT_BLOCK + threadIdx.x;
    if (t >= P) return;
    float4 q;
    if constexpr (WIDE) q = reinterpret_cast<const float4*>(in)[t];
    else q = make_float4(in[4 * (size_t)t], in[4 * (size_t)t + 1], in[4 * (size_t)t + 2], in[4 * (size_t)t + 3]);
    const float4 r = activate_rotation(q, nullptr);
    if constexpr (WIDE) reinterpret_cast<float4*>(out)[t] = r;
    else { out[4 * (size_t)t] = r.x; out[4 * (size_t)t + 1] = r.y; out[4 * (size_t)t + 2] = r.z; out[4 * (size_t)t + 3] = r.w; }
}

bool both_aligned16(const void* a, const void* b) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0; }

template <int KIND>
hipError_t launch_elements(uint32_t n, const float* in, float* out, hipStream_t st)
{
    const bool wide = both_aligned16(in, out);
    const uint32_t threads = wide ? (n >> 2) + 1 : n; // (wide: n / 4 groups and the thread of the tail)
    const dim3 grid((threads + ACT_BLOCK - 1) / ACT_BLOCK), block(ACT_BLOCK);
    if (wide) hipLaunchKernelGGL((activate_elements_kernel<KIND, true>), grid, block, 0, st, n, in, out);
    else hipLaunchKernelGGL((activate_elements_kernel<KIND, false>), grid, block, 0, st, n, in, out);
    return hipGetLastError();
}

} // namespace

int launch_activate_params(int P, const float* scaling, const float* rotation, const float* opacity, float* scales, float* rotations, float* opacities,
                           hipStream_t st, hipError_t* err)
{
    int launches = 0;
    *err = hipSuccess;
    if (scaling) {
        *err = launch_elements<ACT_SCALE>(3u * (uint32_t)P, scaling, scales, st);
        if (*err != hipSuccess) return launches;
        launches++;
    }
    if (rotation) {
        const dim3 grid(((uint32_t)P + ACT_BLOCK - 1) / ACT_BLOCK), block(ACT_BLOCK);
        if (both_aligned16(rotation, rotations)) hipLaunchKernelGGL(activate_rotations_kernel<true>, grid, block, 0, st, (uint32_t)P, rotation, rotations);
        else hipLaunchKernelGGL(activate_rotations_kernel<false>, grid, block, 0, st, (uint32_t)P, rotation, rotations);
        *err = hipGetLastError();
        if (*err != hipSuccess) return launches;
        launches++;
    }
    if (opacity) {
        *err = launch_elements<ACT_OPACITY>((uint32_t)P, opacity, opacities, st);
        if (*err != hipSuccess) return launches;
        launches++;
    }
    return launches;
}

} // namespace stp
