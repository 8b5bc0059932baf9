// stp_adam_div.h -- the row index e / M of stp_adam.hip as a host-computed multiplier (plain C++: the kernel, its launcher and
// tests/cpp/adam_div_check.cpp include this one file).
//
// For a divisor M >= 2 let s be the integer with 2^s < M <= 2^(s+1) and mul = ceil(2^(32+s) / M) = (2^(32+s) + k) / M, 0 <= k < M.
// mul < 2^32 because 2^s < M.  For a dividend e < 2^31
//     e * mul / 2^(32+s) = e / M + e * k / (M * 2^(32+s)),     e * k < 2^31 * 2^(s+1) = 2^(32+s),
// so the second term is below 1 / M, the distance from e / M to the next integer is at least 1 / M, and
//     floor(e * mul / 2^(32+s)) = (mulhi(e, mul) >> s) = floor(e / M)     exactly, for EVERY e < 2^31.
// M == 1 has no such multiplier below 2^32 (it would be 2^32): mul = 0 marks it and the quotient is e itself.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define STP_ADAM_HD __host__ __device__ __forceinline__
#else
#define STP_ADAM_HD inline
#endif

namespace stp {

struct AdamDivisor { uint32_t mul, shift; };

inline AdamDivisor adam_divisor(uint32_t M) // M >= 1
{
    if (M <= 1) return {0u, 0u};
    uint32_t s = 0;
    while ((2ull << s) < M) s++; // 2^s < M <= 2^(s+1)
    const uint64_t pow = 1ull << (32 + s);
    return {(uint32_t)((pow + M - 1) / M), s};
}

STP_ADAM_HD uint32_t adam_div(uint32_t e, AdamDivisor d) // e < 2^31
{
#if defined(__HIP_DEVICE_COMPILE__)
    return d.mul ? (__umulhi(e, d.mul) >> d.shift) : e;
#else
    return d.mul ? (uint32_t)(((uint64_t)e * d.mul) >> 32) >> d.shift : e;
#endif
}

} // namespace stp
