// adam_div_check.cpp -- holds the row index of the sparse Adam kernel (csrc/stp_adam_div.h: a host-computed multiplier in the place of
// e / M) against the integer division, for M in 1..64 (and a few large M) and e within +-70 of every multiple of 2^16 up to 2^31 - 1,
// plus 0 and 2^31 - 1 themselves.  Host code only; tests/test_sparse_adam_cpu.py builds and runs it:
//     g++ -O2 -std=c++17 -I stopthepop-rasterization_amd/csrc tests/cpp/adam_div_check.cpp -o adam_div_check && ./adam_div_check
// Prints "ok <number of quotients checked>" and exits 0, or the first mismatch and exits 1.
#include <cstdint>
#include <cstdio>

#include "stp_adam_div.h"

int main()
{
    const uint32_t big[] = {65, 96, 127, 128, 129, 180, 255, 256, 257, 1000, 65535, 65536, 65537, 1u << 20, (1u << 30) - 1, 1u << 30, (1u << 30) + 1, 0x7FFFFFFEu, 0x7FFFFFFFu};
    uint64_t checked = 0;
    auto check_M = [&](uint32_t M) {
        const stp::AdamDivisor d = stp::adam_divisor(M);
        for (uint64_t c = 0; c <= (1ull << 31); c += (1ull << 16)) {
            for (int64_t off = -70; off <= 70; off++) {
                const int64_t e = (int64_t)c + off;
                if (e < 0 || e > 0x7FFFFFFFll) continue;
                const uint32_t got = stp::adam_div((uint32_t)e, d), want = (uint32_t)e / M;
                if (got != want) {
                    std::printf("mismatch: e = %lld, M = %u: got %u, want %u (mul %u, shift %u)\n", (long long)e, M, got, want, d.mul, d.shift);
                    return false;
                }
                checked++;
            }
        }
        return true;
    };
    for (uint32_t M = 1; M <= 64; M++)
        if (!check_M(M)) return 1;
    for (uint32_t M : big)
        if (!check_M(M)) return 1;
    std::printf("ok %llu\n", (unsigned long long)checked);
    return 0;
}
