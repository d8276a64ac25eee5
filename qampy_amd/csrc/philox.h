// Counter-based random numbers shared by the generators (synth.hip, impair.hip): Philox4x32-10 and Box-Muller.  A draw is a function of
// (key, counter) alone, never of the launch geometry.
#pragma once
#include "common.h"

namespace qh {

struct Philox { unsigned x, y, z, w; };
__device__ __forceinline__ Philox philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox{c0, c1, c2, c3};
}
// two independent standard normals from two 32-bit words (Box-Muller)
__device__ __forceinline__ void gauss2(unsigned a, unsigned b, float &g0, float &g1)
{
    const float u = ((float)a + 1.0f) * 2.3283064365386963e-10f;           // (0, 1]
    const float v = (float)b * 2.3283064365386963e-10f;
    const float r = sqrtf(-2.0f * __logf(u));
    float s, c;
    __sincosf(6.283185307179586f * v, &s, &c);
    g0 = r * c; g1 = r * s;
}

}  // namespace qh
