// smart_philox.h -- the counter-based generator the units that draw share (smart_demcz.hip, smart_nsga2.hip, smart_error_model.hip):
// Philox4x32-10 (Salmon et al. 2011) and the 53-bit uniform made of two of its words.  What a counter's four words mean is
// the unit's own business (include/smart_amd.h says it per entry); the bits of a counter and key never depend on the
// launch.
#pragma once

#include <hip/hip_runtime.h>

namespace smart {

struct Philox4 {
    unsigned w[4];
};

__device__ inline Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// 53 bits of two words -> [0, 1): ((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53, exact
__device__ inline double u53(unsigned w0, unsigned w1)
{
    return (double)(((unsigned long long)(w0 >> 5) << 26) + (unsigned long long)(w1 >> 6)) * 0x1p-53;
}

// a word -> 0 .. n - 1: floor(w n / 2^32), exact
__device__ inline unsigned long long mulhi(unsigned w, unsigned long long n) { return ((unsigned long long)w * n) >> 32; }

} // namespace smart
