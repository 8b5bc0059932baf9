// stp_activations.h -- the three activations of a trainer's raw parameters (stp_set_forward_raw_params / stp_set_backward_raw_params /
// stp_activate_params), fixed to the float32 operation: every kernel that reads a raw array calls these, so the forward, the per-Gaussian
// backward and stp_activate_params agree to the bit.  expf is the one library call; every other step is a correctly rounded IEEE operation
// that no contraction setting can merge with its neighbours.
//   opacity   o = 1 / (1 + exp(-x))                                   torch.sigmoid
//   scale     s = exp(x)                                              torch.exp
//   rotation  q / max(|q|, 1e-12), |q| by a fixed chain of fmas       torch.nn.functional.normalize (eps = 1e-12)
#pragma once

#include <hip/hip_runtime.h>

namespace stp {

// the bits of the raw-parameter mask (include/stp_raster.h)
constexpr int RAW_OPACITY = 1, RAW_SCALE = 2, RAW_ROTATION = 4;
constexpr float kRawQuatEps = 1e-12f;

__device__ __forceinline__ float activate_opacity(float x) { return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-x))); }

__device__ __forceinline__ float activate_scale(float x) { return expf(x); }

// -> the normalised quaternion; *norm (may be nullptr): |q| as computed, BEFORE the clamp (the backward asks whether the clamp was active)
__device__ __forceinline__ float4 activate_rotation(float4 q, float* norm)
{
    float n = __fsqrt_rn(__fmaf_rn(q.w, q.w, __fmaf_rn(q.z, q.z, __fmaf_rn(q.y, q.y, __fmul_rn(q.x, q.x)))));
    if (norm) *norm = n;
    n = fmaxf(n, kRawQuatEps);
    return make_float4(__fdiv_rn(q.x, n), __fdiv_rn(q.y, n), __fdiv_rn(q.z, n), __fdiv_rn(q.w, n));
}

} // namespace stp
