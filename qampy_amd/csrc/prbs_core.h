// PRBS arithmetic shared by the host set-up and the kernels of source.hip (and by a host-only build: every function is plain C++).
//
// Both shift-register forms of qampy/core/pythran_dsp.py:156-178 put out a sequence c with a two-term recurrence over GF(2),
//     c[j + o] = c[j] ^ c[j + m],          characteristic polynomial p(x) = x^o + x^m + 1,
//   external XOR (prbs_ext, taps [o, k]): m = o - k, c[0 .. o) = the seed's bits 0 .. o-1 and output bit i is c[i + o];
//   internal XOR (prbs_int, mask 2^o + 2^k + 1): m = k and output bit i is c[i] - the register is seed(x) x^i mod (x^o + x^k + 1), the
//     output its top coefficient, a linear functional of a state that is multiplied by x per step.
// With r(x) = x^P mod p(x) = sum_j r_j x^j the recurrence gives c[P + t] = sum_j r_j c[j + t]: the o bits at ANY position P from the first
// 2o - 1 bits of c and one polynomial of degree < o.  x^P comes from square-and-multiply on <= 31-bit polynomials; the host reduces the
// call's start modulo the period 2^o - 1 (all four polynomials are primitive) and hands the kernel x^start and the table x^(2^j), so the
// work of a call does not depend on start.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define QH_HD __host__ __device__ __forceinline__
#else
#define QH_HD inline
#endif

namespace qh {

constexpr int PRBS_EXT = 0, PRBS_INT = 1;

struct PrbsParams {
    uint32_t jump[32];       // x^(2^j) mod p
    uint64_t init;           // bit j = c[j], j < 2o - 1
    uint32_t r0;             // x^(position of the call's first bit in c) mod p
    uint32_t flip;           // 0, or ~0 to complement the output
    int32_t o, m;
};

// a b mod p for polynomials of degree < o <= 31 (bit j = coefficient of x^j): shift, reduce, add - one bit of b per step
QH_HD uint32_t prbs_mulmod(uint32_t a, uint32_t b, int o, int m)
{
    const uint32_t full = (1u << o) | (1u << m) | 1u;
    uint32_t r = 0;
    for (int i = o - 1; i >= 0; i--) {
        r <<= 1;
        r ^= (0u - (r >> o)) & full;
        r ^= (0u - ((b >> i) & 1u)) & a;
    }
    return r;
}

// the o bits c[P .. P + o) from r = x^P mod p: bit t = parity(r & c[t .. t + o))
QH_HD uint32_t prbs_state(uint32_t r, uint64_t init, int o)
{
    uint32_t s = 0;
    for (int t = 0; t < o; t++) {
        const uint32_t x = r & (uint32_t)(init >> t);
#ifdef __HIP_DEVICE_COMPILE__
        s |= (uint32_t)(__popc(x) & 1) << t;
#else
        s |= (uint32_t)(__builtin_popcount(x) & 1) << t;
#endif
    }
    return s;
}

// Window of the sequence: bits [0, known) of v are c[q .. q + known), known >= o.  prbs_fill extends it to all 64 bits, o - m new bits per
// step (new bit q' needs c[q' - o] and c[q' - o + m], both below `known`); prbs_next hands out the low 32 bits and moves on.
QH_HD void prbs_fill(uint64_t &v, int &known, int o, int m)
{
    const uint64_t mask = ((uint64_t)1 << (o - m)) - 1;
    while (known < 64) {
        const int sh = known - o;
        v |= (((v >> sh) ^ (v >> (sh + m))) & mask) << known;
        known += o - m;
    }
    known = 64;
}
QH_HD uint32_t prbs_next(uint64_t &v, int &known, int o, int m)
{
    prbs_fill(v, known, o, m);
    const uint32_t w = (uint32_t)v;
    v >>= 32;
    known = 32;
    return w;
}

// Host set-up.  The caller has checked: order in {7, 15, 23, 31}, kind PRBS_EXT / PRBS_INT, 0 <= seed < 2^order, 0 <= start <= 2^62.
inline PrbsParams prbs_setup(int order, int kind, uint32_t seed, int64_t start, int invert)
{
    const int o = order, k = o == 7 ? 6 : o == 15 ? 14 : o == 23 ? 18 : 28;
    PrbsParams p;
    p.o = o;
    p.m = kind == PRBS_EXT ? o - k : k;
    p.flip = invert ? ~0u : 0u;
    uint64_t c = 0;
    if (kind == PRBS_EXT) {
        c = seed;
        for (int j = o; j < 2 * o - 1; j++) c |= (((c >> (j - o)) ^ (c >> (j - o + p.m))) & 1u) << j;
    } else {
        // prbs_int's update rule, 2o - 1 steps: shift, the bit that leaves is the output and folds the mask back in
        const uint64_t mask = ((uint64_t)1 << o) | ((uint64_t)1 << k) | 1u;
        uint64_t state = seed;
        for (int j = 0; j < 2 * o - 1; j++) {
            state <<= 1;
            const uint64_t x = state >> o;
            if (x) state ^= mask;
            c |= x << j;
        }
    }
    p.init = c;
    p.jump[0] = 2u;
    for (int j = 1; j < 32; j++) p.jump[j] = prbs_mulmod(p.jump[j - 1], p.jump[j - 1], o, p.m);
    const uint64_t period = ((uint64_t)1 << o) - 1;
    const uint32_t e = (uint32_t)(((uint64_t)start + (kind == PRBS_EXT ? (uint64_t)o : 0u)) % period);
    uint32_t r = 1u;
    for (int j = 0; j < 32; j++)
        if ((e >> j) & 1u) r = prbs_mulmod(r, p.jump[j], o, p.m);
    p.r0 = r;
    return p;
}

// The window at e bits past the call's first one.  (Splitting e into the workgroup's offset, whose products are scalar arithmetic, and the
// thread's was measured on the MI355X and did not pay: DESIGN.md 3.16.)
QH_HD void prbs_seek(const PrbsParams &p, uint32_t e, uint64_t &v, int &known)
{
    uint32_t r = p.r0;
#pragma unroll
    for (int j = 0; j < 32; j++)
        if ((e >> j) & 1u) r = prbs_mulmod(r, p.jump[j], p.o, p.m);
    v = prbs_state(r, p.init, p.o);
    known = p.o;
}

}  // namespace qh
