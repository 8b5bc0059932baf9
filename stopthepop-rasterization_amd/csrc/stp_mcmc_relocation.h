// stp_mcmc_relocation.h -- one Gaussian's relocation (3DGS-MCMC's compute_relocation), shared by mcmc_relocation_kernel (stp_mcmc.hip) and the
// relocation / growth applies (stp_mcmc_relocate.hip): both give the same bits.  The evaluation order and the float64 steps are those documented
// at the top of stp_mcmc.hip; every float64 operation is an explicit intrinsic, so that the result does not hang on the including file's
// contraction setting.
#pragma once

#include <hip/hip_runtime.h>

namespace stp {

// a Gaussian of opacity o that is there `copies` times (already clamped to [1, 50]): o_new = 1 - (1 - o)^(1 / copies) and the coefficient
// o / denom of the scales, both in float64; the callers round (float)o_new and (float)(coef * (double)s) once
__device__ __forceinline__ void mcmc_relocation_row(const float opacity_old, const int copies, double& o_new, double& coef)
{
    const double o = (double)opacity_old;
    const double x = -expm1(__ddiv_rn(log1p(-o), (double)copies));
    double c = (double)copies, p = x, sum = 0.0;
    for (int k = 0; k < copies; k++) {
        sum = __dadd_rn(sum, __ddiv_rn(__dmul_rn(c, p), __dsqrt_rn((double)(k + 1))));
        c = __ddiv_rn(__dmul_rn(c, (double)(copies - k - 1)), (double)(k + 2));
        p = __dmul_rn(p, -x);
    }
    o_new = x;
    coef = __ddiv_rn(o, sum);
}

} // namespace stp
