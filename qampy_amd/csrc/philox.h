// Counter-based random numbers shared by the generators (synth.hip, impair.hip, txresp.hip): Philox4x32-10 and Box-Muller.  A draw is a function of
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

// The impairments' draws (impair.hip, txresp.hip): counter (sample index low word, high word, mode, stream), key = the seed.
constexpr unsigned IMP_STREAM_PHASE = 1u, IMP_STREAM_NOISE = 2u;
// The theory curves' draws: the Monte-Carlo noise of metrics.hip (counter: draw, SNR point) and the shaped source of source.hip (counter: sample, mode).
constexpr unsigned IMP_STREAM_MC = 3u, IMP_STREAM_SHAPE = 4u;
constexpr double IMP_TWO_PI = QH_TWO_PI;

// two independent standard normals of sample n of a mode, in the precision of the signal
__device__ __forceinline__ void imp_gauss(int64_t n, int mode, unsigned stream, unsigned k0, unsigned k1, float &g0, float &g1)
{
    const Philox p = philox4x32_10((unsigned)n, (unsigned)((uint64_t)n >> 32), (unsigned)mode, stream, k0, k1);
    gauss2(p.x, p.y, g0, g1);
}
__device__ __forceinline__ void imp_gauss(int64_t n, int mode, unsigned stream, unsigned k0, unsigned k1, double &g0, double &g1)
{
    const Philox p = philox4x32_10((unsigned)n, (unsigned)((uint64_t)n >> 32), (unsigned)mode, stream, k0, k1);
    const uint64_t a = (((uint64_t)p.x << 32) | p.y) >> 11, b = (((uint64_t)p.z << 32) | p.w) >> 11;
    const double u = ((double)a + 1.0) * 0x1p-53;                          // (0, 1]
    const double v = (double)b * 0x1p-53;                                  // [0, 1)
    const double r = sqrt(-2.0 * log(u));
    double s, c;
    sincos(IMP_TWO_PI * v, &s, &c);
    g0 = r * c; g1 = r * s;
}

}  // namespace qh
