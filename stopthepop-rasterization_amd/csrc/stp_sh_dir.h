// stp_sh_dir.h -- the derivative of one SH colour channel with respect to the unit view direction (reference backward.cu:62-134, the
// dRGBdx / dRGBdy / dRGBdz terms), shared by the two kernels that form it:
//   preprocess_backward_kernel (stp_backward.hip)  the legacy path: from the SH row it has staged in LDS
//   sh_color_kernel<.., STASH> (stp_preprocess.hip) the forward with stp_set_forward_sh_stash: from the row it has staged anyway, kept as nine
//                                                   floats per visible Gaussian for the backward to read back (36 B in the place of the 192 B row)
// Both include THIS text and compile it with the file's default contraction (no `#pragma clang fp contract` in here, and none may be added:
// sh_to_rgb's contract(off) is scoped to its own body and does not reach these functions).  A stashed value is the legacy backward's up to the
// fusion choices the compiler makes in the two kernels: equal bits at degree 1, an ulp apart now and then above it.  The three levels are functions of their own because the backward calls each inside the degree nesting it has always had.
#pragma once

#include "stp_device.h"

namespace stp {

constexpr int kShStashFloats = 9; // dx, dy, dz of the channels r, g, b: plane 3 * ch + {0, 1, 2} of the stash, P floats each

// the unit view direction of a Gaussian, v = mean - campos
__device__ __forceinline__ void sh_unit_dir(const float3 v, float& x, float& y, float& z)
{
    const float len = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    x = v.x / len; y = v.y / len; z = v.z / len;
}

// sh[k], k = 1 .. 15: the channel's coefficients, zero at and above min(M, (D + 1)^2)
__device__ __forceinline__ void sh_dir_deg1(const float* sh, float& dx, float& dy, float& dz)
{
    dx = -kSH_C1 * sh[3]; dy = -kSH_C1 * sh[1]; dz = kSH_C1 * sh[2];
}

__device__ __forceinline__ void sh_dir_deg2(const float x, const float y, const float z, const float* sh, float& dx, float& dy, float& dz)
{
    dx += kSH_C2[0] * y * sh[4] + kSH_C2[2] * 2.f * -x * sh[6] + kSH_C2[3] * z * sh[7] + kSH_C2[4] * 2.f * x * sh[8];
    dy += kSH_C2[0] * x * sh[4] + kSH_C2[1] * z * sh[5] + kSH_C2[2] * 2.f * -y * sh[6] + kSH_C2[4] * 2.f * -y * sh[8];
    dz += kSH_C2[1] * y * sh[5] + kSH_C2[2] * 2.f * 2.f * z * sh[6] + kSH_C2[3] * x * sh[7];
}

__device__ __forceinline__ void sh_dir_deg3(const float xx, const float yy, const float zz, const float xy, const float yz, const float xz,
                                            const float* sh, float& dx, float& dy, float& dz)
{
    dx += (kSH_C3[0] * sh[9] * 3.f * 2.f * xy + kSH_C3[1] * sh[10] * yz + kSH_C3[2] * sh[11] * -2.f * xy +
           kSH_C3[3] * sh[12] * -3.f * 2.f * xz + kSH_C3[4] * sh[13] * (-3.f * xx + 4.f * zz - yy) +
           kSH_C3[5] * sh[14] * 2.f * xz + kSH_C3[6] * sh[15] * 3.f * (xx - yy));
    dy += (kSH_C3[0] * sh[9] * 3.f * (xx - yy) + kSH_C3[1] * sh[10] * xz + kSH_C3[2] * sh[11] * (-3.f * yy + 4.f * zz - xx) +
           kSH_C3[3] * sh[12] * -3.f * 2.f * yz + kSH_C3[4] * sh[13] * -2.f * xy + kSH_C3[5] * sh[14] * -2.f * yz +
           kSH_C3[6] * sh[15] * -3.f * 2.f * xy);
    dz += (kSH_C3[1] * sh[10] * xy + kSH_C3[2] * sh[11] * 4.f * 2.f * yz + kSH_C3[3] * sh[12] * 3.f * (2.f * zz - xx - yy) +
           kSH_C3[4] * sh[13] * 4.f * 2.f * xz + kSH_C3[5] * sh[14] * (xx - yy));
}

// all active levels, in the backward's nesting (what the stashing forward evaluates)
__device__ __forceinline__ void sh_dir_derivative(const int D, const float x, const float y, const float z, const float* sh, float& dx, float& dy, float& dz)
{
    dx = 0; dy = 0; dz = 0;
    if (D > 0) {
        sh_dir_deg1(sh, dx, dy, dz);
        if (D > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            sh_dir_deg2(x, y, z, sh, dx, dy, dz);
            if (D > 2) sh_dir_deg3(xx, yy, zz, xy, yz, xz, sh, dx, dy, dz);
        }
    }
}

} // namespace stp
