// Signal-quality metrics on the device: soft demapper (LLRs), GMI, MI, BER / SER / EVM of an aligned row and the
// data-aided SNR estimate.  Reference: pythran_dsp.soft_l_value_demapper / _minmax (qampy/core/pythran_dsp.py:87-131),
// estimate_snr (:244-286), cal_mi_mc / cal_mi_mc_fast (:289-313) and their callers cal_gmi / cal_mi / cal_ber / cal_evm
// (qampy/signals.py:340-560).
//
// Bit labels need no table: point g of the alphabet (coded order) carries Gray label g, bit k (MSB first) is
// (g >> (nbits - 1 - k)) & 1.  The kernels are templated on nbits (1..10, M up to 1024).  Up to nbits 8 the loops over the
// alphabet unroll fully, so each (bit, side) subset is fixed at compile time; above that they unroll by 8 and test the bits
// at run time (the same operations in the same order, a fraction of the code).
//
// Range of the exact LLR.  L = ln sum_{bit=1} exp(-snr d_g) - ln sum_{bit=0} exp(-snr d_g) (d_g = |s_g - r|^2).  In
// complex64 each (bit, side) sum is shifted by that subset's own minimum distance m, so its largest term is 1 and the sum
// never underflows: L = snr (m_0 - m_1) + ln S'_1 - ln S'_0 - nbits * M exp2 per symbol.  complex128 shifts by the global
// minimum only (M exp per symbol); its range then matches (and exceeds) the reference's unshifted double sums.
//
// Reductions are in double: per-block partials in a fixed order, then a fixed-order final sum (reduce_partials), so
// repeated calls give bit-identical results (the class statistics of the SNR estimate too: each class is added by one
// owner thread in index order).
#include "common.h"
#include "philox.h"
#include <algorithm>
#include <cmath>
#include <vector>

namespace qh {
namespace {

constexpr int MET_THREADS = 256, MET_MAXBLK = 1024, MET_NBMAX = 10;

// unroll factor of a loop over the 2^NB alphabet points: all of them up to 256 points, 8 at a time beyond
template <int NB> constexpr int unroll_points() { return NB <= 8 ? 1 << NB : 8; }
constexpr double LOG2E = 1.4426950408889634, LN2 = 0.6931471805599453;

template <typename R> __device__ __forceinline__ R hyp_(R a, R b);
template <> __device__ __forceinline__ float hyp_<float>(float a, float b) { return hypotf(a, b); }
template <> __device__ __forceinline__ double hyp_<double>(double a, double b) { return hypot(a, b); }
__device__ __forceinline__ float exp2_(float x) { return exp2f(x); }
__device__ __forceinline__ double exp2_(double x) { return exp2(x); }
__device__ __forceinline__ float log2_(float x) { return log2f(x); }
__device__ __forceinline__ double log2_(double x) { return log2(x); }

template <typename R> __device__ __forceinline__ R dist2(Cx<R> a, Cx<R> b)
{
    const R dx = a.re - b.re, dy = a.im - b.im;
    return dx * dx + dy * dy;
}

template <typename R> __device__ __forceinline__ Cx<R> rot90(Cx<R> x, int k)       // x * j^k
{
    switch (k & 3) {
    case 1: return Cx<R>{-x.im, x.re};
    case 2: return Cx<R>{-x.re, -x.im};
    case 3: return Cx<R>{x.im, -x.re};
    default: return x;
    }
}

// log2(1 + exp(x)) without overflow (softplus / ln 2)
__device__ __forceinline__ double softplus2(double x) { return (x > 0 ? x : 0.) * LOG2E + log1p(exp(-fabs(x))) * LOG2E; }

// Per-(bit, side) minimum distances, the global minimum and (DECIDE) the decision of ser.hip: first minimum of |r - s_g|
// (hypot, as det_symbol_argmin).  sy: the alphabet in LDS.
template <typename R, int NB, bool DECIDE> struct Scan {
    R m0[NB], m1[NB], dmin;
    int idx;
    __device__ __forceinline__ void run(Cx<R> r, const Cx<R> *sy)
    {
        constexpr int M = 1 << NB;
        const R inf = __builtin_inf();
#pragma unroll
        for (int k = 0; k < NB; k++) m0[k] = m1[k] = inf;
        dmin = inf;
        R hbest = inf;
        idx = 0;
#pragma unroll unroll_points<NB>()
        for (int g = 0; g < M; g++) {
            const Cx<R> s = sy[g];
            const R d = dist2(r, s);
#pragma unroll
            for (int k = 0; k < NB; k++) {
                if ((g >> (NB - 1 - k)) & 1) m1[k] = min_(m1[k], d);
                else m0[k] = min_(m0[k], d);
            }
            dmin = min_(dmin, d);
            if (DECIDE) {
                const R h = hyp_<R>(r.re - s.re, r.im - s.im);
                if (h < hbest) { hbest = h; idx = g; }
            }
        }
    }
};

// Exact LLRs of one symbol from its Scan (see the header comment for the shifts).  Also returns log2 of
// sum_g exp(-snr (d_g - dmin)), the sum the fast MI needs, at the cost of one more exp2 in complex64.
template <typename R, int NB, bool DECIDE>
__device__ __forceinline__ void llr_exact(Cx<R> r, const Cx<R> *sy, R snr, const Scan<R, NB, DECIDE> &sc, R *L, R *log2_all)
{
    constexpr int M = 1 << NB;
    constexpr bool PER_SUBSET = sizeof(R) == 4;
    const R t = snr * (R)LOG2E;
    R s0[NB], s1[NB];
#pragma unroll
    for (int k = 0; k < NB; k++) s0[k] = s1[k] = 0;
#pragma unroll unroll_points<NB>()
    for (int g = 0; g < M; g++) {
        const R d = dist2(r, sy[g]);
        if (PER_SUBSET) {
#pragma unroll
            for (int k = 0; k < NB; k++) {
                if ((g >> (NB - 1 - k)) & 1) s1[k] += exp2_((sc.m1[k] - d) * t);
                else s0[k] += exp2_((sc.m0[k] - d) * t);
            }
        } else {
            const R e = exp2_((sc.dmin - d) * t);
#pragma unroll
            for (int k = 0; k < NB; k++) {
                if ((g >> (NB - 1 - k)) & 1) s1[k] += e;
                else s0[k] += e;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NB; k++) {
        const R l = (R)LN2 * (log2_(s1[k]) - log2_(s0[k]));
        L[k] = PER_SUBSET ? snr * (sc.m0[k] - sc.m1[k]) + l : l;
    }
    if (PER_SUBSET) {     // bit 0's two sides cover the alphabet; the side holding the global minimum is already shifted by it
        *log2_all = sc.m0[0] <= sc.m1[0] ? log2_(s0[0] + s1[0] * exp2_((sc.dmin - sc.m1[0]) * t))
                                         : log2_(s1[0] + s0[0] * exp2_((sc.dmin - sc.m0[0]) * t));
    } else {
        *log2_all = log2_(s0[0] + s1[0]);
    }
}

// log2 sum_g exp(-(d_g - dmin) / N0) by its own loop (minmax LLRs and the host-array fast MI)
template <typename R, int NB>
__device__ __forceinline__ R log2_sum_loop(Cx<R> r, const Cx<R> *sy, R dmin, R n0inv_log2e)
{
    constexpr int M = 1 << NB;
    R s = 0;
#pragma unroll unroll_points<NB>()
    for (int g = 0; g < M; g++) s += exp2_((dmin - dist2(r, sy[g])) * n0inv_log2e);
    return log2_(s);
}

// Block sum of F per-thread doubles into partial[blockIdx.x * F + f] (fixed order: wave DPP tree, then waves 0..3)
template <int F> __device__ __forceinline__ void block_partials(double *acc, double *partial)
{
    __shared__ double wsum[MET_THREADS / 64][F];
#pragma unroll
    for (int f = 0; f < F; f++) {
        const double v = wave_sum(acc[f]);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][f] = v;
    }
    __syncthreads();
    if (threadIdx.x < F) {
        double s = 0;
        for (int w = 0; w < MET_THREADS / 64; w++) s += wsum[w][threadIdx.x];
        partial[(size_t)blockIdx.x * F + threadIdx.x] = s;
    }
}

template <typename R, int M> __device__ __forceinline__ void load_alphabet(Cx<R> *sy, const Cx<R> *alphabet)
{
    for (int g = threadIdx.x; g < M; g += blockDim.x) sy[g] = alphabet[g];
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------ kernels
// L (N, NB) float64: LLRs of every symbol (soft_l_value_demapper / _minmax)
template <typename R, int NB, bool MINMAX>
__global__ void __launch_bounds__(MET_THREADS) llr_kernel(const Cx<R> *E, int64_t N, const Cx<R> *alphabet, R snr, double *L)
{
    constexpr int M = 1 << NB;
    __shared__ Cx<R> sy[M];
    load_alphabet<R, M>(sy, alphabet);
    for (int64_t i = (int64_t)blockIdx.x * MET_THREADS + threadIdx.x; i < N; i += (int64_t)gridDim.x * MET_THREADS) {
        const Cx<R> r = ldg(E + i);
        Scan<R, NB, false> sc;
        sc.run(r, sy);
        R l[NB], la;
        if (MINMAX) {
#pragma unroll
            for (int k = 0; k < NB; k++) l[k] = snr * (sc.m0[k] - sc.m1[k]);
        } else {
            llr_exact<R, NB, false>(r, sy, snr, sc, l, &la);
        }
#pragma unroll
        for (int k = 0; k < NB; k++) L[(size_t)i * NB + k] = (double)l[k];
    }
}

// Fused pass over an aligned row: rx[i] * j^rot against alphabet[tx[i - lag]] for i in [i0, i1), i - lag in [0, ntx).
// partial fields: symbol errors, bit errors, compared, sum |t - r|^2, sum log2 sum_j exp(-(|r - s_j|^2 - |r - t|^2) snr),
// then per bit sum log2(1 + exp((-1)^b L)).  Transmitted indices outside [0, M) are skipped.
template <typename R, int NB, bool MINMAX>
__global__ void __launch_bounds__(MET_THREADS) metrics_kernel(const Cx<R> *E, int64_t i0, int64_t i1, int rot, int64_t lag, const int32_t *tx,
                                                              int64_t ntx, const Cx<R> *alphabet, R snr, double *partial)
{
    constexpr int M = 1 << NB, F = 5 + NB;
    __shared__ Cx<R> sy[M];
    load_alphabet<R, M>(sy, alphabet);
    double acc[F];
#pragma unroll
    for (int f = 0; f < F; f++) acc[f] = 0;
    const R t2 = snr * (R)LOG2E;
    for (int64_t i = i0 + (int64_t)blockIdx.x * MET_THREADS + threadIdx.x; i < i1; i += (int64_t)gridDim.x * MET_THREADS) {
        const int64_t it = i - lag;
        if (it < 0 || it >= ntx) continue;
        const int t = tx[it];
        if ((unsigned)t >= (unsigned)M) continue;
        const Cx<R> r = rot90(ldg(E + i), rot);
        Scan<R, NB, true> sc;
        sc.run(r, sy);
        acc[0] += sc.idx != t;
        acc[1] += __popc((unsigned)(sc.idx ^ t));
        acc[2] += 1;
        const R dt = dist2(r, sy[t]);
        acc[3] += (double)dt;
        R l[NB], la;
        if (MINMAX) {
#pragma unroll
            for (int k = 0; k < NB; k++) l[k] = snr * (sc.m0[k] - sc.m1[k]);
            la = log2_sum_loop<R, NB>(r, sy, sc.dmin, t2);
        } else {
            llr_exact<R, NB, true>(r, sy, snr, sc, l, &la);
        }
        acc[4] += (double)((dt - sc.dmin) * t2) + (double)la;
#pragma unroll
        for (int k = 0; k < NB; k++) acc[5 + k] += softplus2((t >> (NB - 1 - k)) & 1 ? -(double)l[k] : (double)l[k]);
    }
    block_partials<F>(acc, partial);
}

// cal_mi_mc_fast on host arrays: sum over l of log2 sum_j exp(-(|x_l - s_j|^2 - |x_l - t_l|^2) / N0)
template <typename R, int NB>
__global__ void __launch_bounds__(MET_THREADS) mi_fast_kernel(const Cx<R> *x, const Cx<R> *tx, int64_t L, const Cx<R> *alphabet, R n0inv, double *partial)
{
    constexpr int M = 1 << NB;
    __shared__ Cx<R> sy[M];
    load_alphabet<R, M>(sy, alphabet);
    double acc[1] = {0};
    const R t2 = n0inv * (R)LOG2E;
    for (int64_t l = (int64_t)blockIdx.x * MET_THREADS + threadIdx.x; l < L; l += (int64_t)gridDim.x * MET_THREADS) {
        const Cx<R> r = ldg(x + l);
        R dmin = __builtin_inf();
#pragma unroll unroll_points<NB>()
        for (int g = 0; g < M; g++) dmin = min_(dmin, dist2(r, sy[g]));
        acc[0] += (double)((dist2(r, ldg(tx + l)) - dmin) * t2) + (double)log2_sum_loop<R, NB>(r, sy, dmin, t2);
    }
    block_partials<1>(acc, partial);
}

// cal_mi_mc: sum over (i, l) of log2 sum_j exp(-(|s_i - s_j|^2 + 2 Re((s_i - s_j) n_l)) / N0), shifted by the largest exponent
template <typename R>
__global__ void __launch_bounds__(MET_THREADS) mi_mc_kernel(const Cx<R> *noise, int64_t L, const Cx<R> *alphabet, int M, R n0inv, double *partial)
{
    __shared__ Cx<R> sy[1 << MET_NBMAX];
    for (int g = threadIdx.x; g < M; g += blockDim.x) sy[g] = alphabet[g];
    __syncthreads();
    double acc[1] = {0};
    const int64_t P = L * M;
    for (int64_t p = (int64_t)blockIdx.x * MET_THREADS + threadIdx.x; p < P; p += (int64_t)gridDim.x * MET_THREADS) {
        const int i = (int)(p % M);
        const Cx<R> n = ldg(noise + p / M), si = sy[i];
        R amax = -__builtin_inf();
        for (int j = 0; j < M; j++) {
            const Cx<R> dd{si.re - sy[j].re, si.im - sy[j].im};
            amax = fmax(amax, -(dd.re * dd.re + dd.im * dd.im + 2 * (dd.re * n.re - dd.im * n.im)) * n0inv);
        }
        R s = 0;
        for (int j = 0; j < M; j++) {
            const Cx<R> dd{si.re - sy[j].re, si.im - sy[j].im};
            s += exp2_((-(dd.re * dd.re + dd.im * dd.im + 2 * (dd.re * n.re - dd.im * n.im)) * n0inv - amax) * (R)LOG2E);
        }
        acc[0] += (double)amax * LOG2E + (double)log2_(s);
    }
    block_partials<1>(acc, partial);
}

// 2^x for x <= 0 where a result below the smallest normal number may be flushed to zero: in float the bare instruction (exp2f spends a compare, a
// select, an add and a scaling on the subnormal range, which no sum here needs: its largest term is 1, or the sum is redone)
__device__ __forceinline__ float exp2_neg(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ double exp2_neg(double x) { return exp2(x); }

// Monte-Carlo GMI and MI of an alphabet over AWGN: cal_gmi_mc (pythran_dsp.py:181-197) and cal_mi_mc (:289-300) on the same draws.  With
// y = s_i + conj(z_l) the reference's exponent |s_i - s_j|^2 + 2 Re(z_l (s_i - s_j)) is |y - s_j|^2 - |z_l|^2, so its nbits * 2 * (M / 2) ratios of
// two sums per draw are the GMI terms of the synthetic received point y sent as point i: one sum over the alphabet, S_all, and its split into the
// (bit, side) sub-sums serve every bit, and log2(S_all / e_i) is cal_mi_mc's term.  A work item is (SNR point p = blockIdx.y, sent point i, draw l);
// the pairs (i, l) of a point are strided over the grid's x, so a capped grid loops.
//   partial fields per (block, p): sum log2(S_all / e_i), then per bit k sum log2(S_all / S_{k, side of i}).
// Shifts: every exponent is taken relative to the nearest point of y, so S_all lies in [1, M].  The side of the sent point can be far from y (a large
// draw): when one of its sums falls below TINY the item is redone with each own side shifted by that side's own nearest point, as the complex64 LLRs
// are, so no sum underflows whatever z holds.  Above TINY the largest term of the sum is a normal number with its full relative precision.
template <typename R, int NB>
__global__ void __launch_bounds__(MET_THREADS) awgn_mc_kernel(const Cx<R> *alphabet, const double *snr, const Cx<R> *z, int64_t ns, double *partial)
{
    constexpr int M = 1 << NB, F = 1 + NB, LB = NB < 6 ? NB : 6, HB = NB - LB, BLK = 1 << LB;
    const R TINY = sizeof(R) == 4 ? (R)0x1p-100 : (R)0x1p-900;
    __shared__ Cx<R> sy[M];
    load_alphabet<R, M>(sy, alphabet);
    const int p = blockIdx.y;
    const R t = (R)snr[p] * (R)LOG2E;
    const Cx<R> *zp = z + (size_t)p * ns;
    const R inf = __builtin_inf();
    double acc[F];
#pragma unroll
    for (int f = 0; f < F; f++) acc[f] = 0;
    const int64_t P = ns * M;
    for (int64_t q = (int64_t)blockIdx.x * MET_THREADS + threadIdx.x; q < P; q += (int64_t)gridDim.x * MET_THREADS) {
        const int i = (int)(q & (M - 1));
        const Cx<R> n = ldg(zp + (q >> NB)), si = sy[i];
        const Cx<R> y{si.re + n.re, si.im - n.im};
        R dmin = inf;
#pragma unroll 16
        for (int g = 0; g < M; g++) dmin = min_(dmin, dist2(y, sy[g]));
        // the alphabet in blocks of BLK = 2^LB points: inside a block the low LB label bits are fixed at compile time (the block unrolls), the
        // high HB bits are the block's number and take the block's sum
        R s0[NB], s1[NB];
#pragma unroll
        for (int k = 0; k < NB; k++) s0[k] = s1[k] = 0;
#pragma unroll 1
        for (int h = 0; h < (1 << HB); h++) {
            const Cx<R> *blk = sy + h * BLK;
            R sum = 0;
#pragma unroll
            for (int j = 0; j < BLK; j++) {
                const R e = exp2_neg((dmin - dist2(y, blk[j])) * t);
                sum += e;
#pragma unroll
                for (int k = 0; k < LB; k++) {
                    if ((j >> (LB - 1 - k)) & 1) s1[HB + k] += e;
                    else s0[HB + k] += e;
                }
            }
#pragma unroll
            for (int k = 0; k < HB; k++) {
                if ((h >> (HB - 1 - k)) & 1) s1[k] += sum;
                else s0[k] += sum;
            }
        }
        const R la = log2_(s0[NB - 1] + s1[NB - 1]);
        acc[0] += (double)((dist2(y, si) - dmin) * t) + (double)la;
        R own[NB], low = inf;
#pragma unroll
        for (int k = 0; k < NB; k++) {
            own[k] = (i >> (NB - 1 - k)) & 1 ? s1[k] : s0[k];
            low = min_(low, own[k]);
        }
        if (low >= TINY) {
#pragma unroll
            for (int k = 0; k < NB; k++) acc[1 + k] += (double)la - (double)log2_(own[k]);
        } else {                             // rare: per-side shifts; bit k of g ^ i is 0 on the sent point's side
            R m[NB];
#pragma unroll
            for (int k = 0; k < NB; k++) { m[k] = inf; own[k] = 0; }
#pragma unroll 1
            for (int g = 0; g < M; g++) {
                const R d = dist2(y, sy[g]);
#pragma unroll
                for (int k = 0; k < NB; k++) if ((((g ^ i) >> (NB - 1 - k)) & 1) == 0) m[k] = min_(m[k], d);
            }
#pragma unroll 1
            for (int g = 0; g < M; g++) {
                const R d = dist2(y, sy[g]);
#pragma unroll
                for (int k = 0; k < NB; k++) if ((((g ^ i) >> (NB - 1 - k)) & 1) == 0) own[k] += exp2_neg((m[k] - d) * t);
            }
#pragma unroll
            for (int k = 0; k < NB; k++) acc[1 + k] += (double)la - (double)log2_(own[k]) + ((double)m[k] - (double)dmin) * (double)t;
        }
    }
    block_partials<F>(acc, partial + (size_t)p * gridDim.x * F);
}

// z[p][l] = (g0 + j g1) sqrt(1 / (2 snr_p)), (g0, g1) the draw of counter (l, p, IMP_STREAM_MC): every SNR point its own noise, as the reference
// draws anew per call; the draws depend on (seed, p, l) alone.
template <typename R>
__global__ void __launch_bounds__(MET_THREADS) awgn_mc_noise_kernel(Cx<R> *z, const double *snr, int64_t ns, unsigned k0, unsigned k1)
{
    const int64_t l = (int64_t)blockIdx.x * MET_THREADS + threadIdx.x;
    if (l >= ns) return;
    const int p = blockIdx.y;
    const R sigma = (R)sqrt(1.0 / (2.0 * snr[p]));
    R g0, g1;
    imp_gauss(l, p, IMP_STREAM_MC, k0, k1, g0, g1);
    stg(z + (size_t)p * ns + l, Cx<R>{g0 * sigma, g1 * sigma});
}

// out[p] = [gmi, mi, gmi_per_bit ...] from the sums of point p over its count = M ns items
__global__ void __launch_bounds__(64) awgn_mc_finish_kernel(const double *sums, int nsnr, int nb, double count, double *out)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= nsnr) return;
    const double *s = sums + (size_t)p * (1 + nb);
    double *o = out + (size_t)p * (2 + nb), tot = 0;
    for (int k = 0; k < nb; k++) {
        o[2 + k] = 1.0 - s[1 + k] / count;
        tot += s[1 + k];
    }
    o[0] = (double)nb - tot / count;
    o[1] = (double)nb - s[0] / count;
}

// out[f] = sum over blocks of partial[b * F + f]: one wave per field, lane j adds blocks j, j + 64, ... in order (blockIdx.y: one such set of
// nblk partials and F outputs after another)
__global__ void __launch_bounds__(64) reduce_partials_kernel(const double *partial, int nblk, int F, double *out)
{
    const int f = blockIdx.x;
    partial += (size_t)blockIdx.y * nblk * F;
    out += (size_t)blockIdx.y * F;
    double s = 0;
    for (int b = threadIdx.x; b < nblk; b += 64) s += partial[(size_t)b * F + f];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[f] = s;
}

// SNR estimate, pass 1 (per class: count, sum re, sum im) and pass 2 (per class: sum |r - mu|^2), over the aligned row.
// Deterministic: the block stages 256 symbols in LDS; the block is P = 256 / S groups of S >= M threads (S = 64, 128 or 256), thread g of
// group q adds the staged symbols of class g in slice q of the tile in index order, and the P group sums are added in order at the end.
// Above 256 classes (C > 1, M <= 256 C) the block is one group and thread g owns the classes g, g + 256, ..., each in index order.
// Per-block sums go to partial[block][M][3] / [block][M]; labels outside [0, M) belong to no class.
template <typename R, bool PASS2, int C>
__global__ void __launch_bounds__(MET_THREADS) class_stats_kernel(const Cx<R> *E, int64_t i0, int64_t i1, int rot, int64_t lag, const int32_t *tx,
                                                                  int64_t ntx, int M, const double *mu, double *partial)
{
    constexpr int F = PASS2 ? 1 : 3;
    __shared__ int lab[MET_THREADS];
    __shared__ double v0[MET_THREADS], v1[MET_THREADS], acc[MET_THREADS][F];
    const int S = C > 1 || M > 128 ? 256 : M <= 64 ? 64 : 128, P = MET_THREADS / S, len = MET_THREADS / P;
    const int g = threadIdx.x % S, q = threadIdx.x / S;
    double a0[C], a1[C], a2[C];
#pragma unroll
    for (int c = 0; c < C; c++) a0[c] = a1[c] = a2[c] = 0;
    for (int64_t base = i0 + (int64_t)blockIdx.x * MET_THREADS; base < i1; base += (int64_t)gridDim.x * MET_THREADS) {
        const int64_t i = base + threadIdx.x, it = i - lag;
        int t = -1;
        double x0 = 0, x1 = 0;
        if (i < i1 && it >= 0 && it < ntx) {
            t = tx[it];
            if ((unsigned)t < (unsigned)M) {
                const Cx<R> r = rot90(ldg(E + i), rot);
                if (PASS2) {
                    const double dx = (double)r.re - mu[2 * t], dy = (double)r.im - mu[2 * t + 1];
                    x0 = dx * dx + dy * dy;
                } else {
                    x0 = (double)r.re; x1 = (double)r.im;
                }
            } else {
                t = -1;
            }
        }
        __syncthreads();                     // the previous tile is consumed
        lab[threadIdx.x] = t; v0[threadIdx.x] = x0; v1[threadIdx.x] = x1;
        __syncthreads();
        if (C == 1) {
            if (g < M) {
                for (int k = q * len; k < (q + 1) * len; k++) {
                    if (lab[k] != g) continue;
                    if (PASS2) { a0[0] += v0[k]; }
                    else { a0[0] += 1; a1[0] += v0[k]; a2[0] += v1[k]; }
                }
            }
        } else {
            for (int k = 0; k < MET_THREADS; k++) {
                const int l = lab[k];
                if (l < 0 || l % MET_THREADS != g) continue;
#pragma unroll
                for (int c = 0; c < C; c++) {        // constant register index: c = l / 256
                    if (l / MET_THREADS != c) continue;
                    if (PASS2) { a0[c] += v0[k]; }
                    else { a0[c] += 1; a1[c] += v0[k]; a2[c] += v1[k]; }
                }
            }
        }
    }
    if (C > 1) {                             // one group: the owner's sums are the block's
#pragma unroll
        for (int c = 0; c < C; c++) {
            const int cl = g + c * MET_THREADS;
            if (cl >= M) continue;
            double *p = partial + ((size_t)blockIdx.x * M + cl) * F;
            p[0] = a0[c];
            if (!PASS2) { p[1] = a1[c]; p[2] = a2[c]; }
        }
        return;
    }
    acc[threadIdx.x][0] = a0[0];
    if (!PASS2) { acc[threadIdx.x][1] = a1[0]; acc[threadIdx.x][2] = a2[0]; }
    __syncthreads();
    if (threadIdx.x < M) {
        double *p = partial + ((size_t)blockIdx.x * M + threadIdx.x) * F;
        for (int f = 0; f < F; f++) {
            double s = 0;
            for (int w = 0; w < P; w++) s += acc[w * S + threadIdx.x][f];
            p[f] = s;
        }
    }
}

// mu[t] = class mean from the pass-1 sums (0 / 0 = NaN for an empty class, as np.mean of an empty selection)
__global__ void class_mean_kernel(const double *sums, int M, double *mu)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < M) { mu[2 * t] = sums[3 * t + 1] / sums[3 * t]; mu[2 * t + 1] = sums[3 * t + 2] / sums[3 * t]; }
}

// label of tx[i]: index of the alphabet point it equals exactly, else -1 (estimate_snr selects with symbols_tx == gray_symbols[ind])
template <typename R>
__global__ void __launch_bounds__(MET_THREADS) exact_label_kernel(const Cx<R> *tx, int64_t n, const Cx<R> *alphabet, int M, int32_t *idx)
{
    const int64_t i = (int64_t)blockIdx.x * MET_THREADS + threadIdx.x;
    if (i >= n) return;
    const Cx<R> x = ldg(tx + i);
    int k = -1;
    for (int g = M - 1; g >= 0; g--) if (alphabet[g].re == x.re && alphabet[g].im == x.im) k = g;
    idx[i] = k;
}

// ------------------------------------------------------------------------------------------------ host side
unsigned grid_for(int64_t n)
{
    int64_t b = (n + MET_THREADS - 1) / MET_THREADS;
    return (unsigned)(b < 1 ? 1 : b > MET_MAXBLK ? MET_MAXBLK : b);
}

int nbits_of(int M)
{
    for (int nb = 1; nb <= MET_NBMAX; nb++) if (M == 1 << nb) return nb;
    return 0;
}

// dispatch a kernel templated on NB = 1..10
#define QH_NB_DISPATCH(nb, ...)                                                                                        \
    switch (nb) {                                                                                                       \
    case 1: { constexpr int NB = 1; __VA_ARGS__; } break;                                                                      \
    case 2: { constexpr int NB = 2; __VA_ARGS__; } break;                                                                      \
    case 3: { constexpr int NB = 3; __VA_ARGS__; } break;                                                                      \
    case 4: { constexpr int NB = 4; __VA_ARGS__; } break;                                                                      \
    case 5: { constexpr int NB = 5; __VA_ARGS__; } break;                                                                      \
    case 6: { constexpr int NB = 6; __VA_ARGS__; } break;                                                                      \
    case 7: { constexpr int NB = 7; __VA_ARGS__; } break;                                                                      \
    case 8: { constexpr int NB = 8; __VA_ARGS__; } break;                                                                      \
    case 9: { constexpr int NB = 9; __VA_ARGS__; } break;                                                                      \
    default: { constexpr int NB = 10; __VA_ARGS__; } break;                                                                    \
    }

// sum of F fields over nblk block partials into out (device), fixed order; batch: that many sets of partials and outputs, one behind the other
int reduce_fields(const double *partial, int nblk, int F, double *out, int batch = 1)
{
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(F, batch), dim3(64), 0, g_stream, partial, nblk, F, out);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

}  // namespace

template <typename R> int llr_dev(const void *E, int64_t N, int nbits, double snr, const void *alphabet, int M, int minmax, double *L)
{
    int rc = ensure_init();
    if (rc) return rc;
    const int nb = nbits_of(M);
    QH_REQUIRE(N >= 0 && nb > 0 && nbits == nb, "soft_l_value_demapper: M must be 2^nbits, nbits in 1..10");
    if (N == 0) return QH_OK;
    const unsigned g = grid_for(N);
    if (minmax) { QH_NB_DISPATCH(nb, hipLaunchKernelGGL((llr_kernel<R, NB, true>), dim3(g), dim3(MET_THREADS), 0, g_stream, (const Cx<R> *)E, N, (const Cx<R> *)alphabet, (R)snr, L)) }
    else { QH_NB_DISPATCH(nb, hipLaunchKernelGGL((llr_kernel<R, NB, false>), dim3(g), dim3(MET_THREADS), 0, g_stream, (const Cx<R> *)E, N, (const Cx<R> *)alphabet, (R)snr, L)) }
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R> int llr_host(const void *E, int64_t N, int nbits, double snr, const void *alphabet, int M, int minmax, double *L)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(N >= 0 && nbits_of(M) > 0 && nbits == nbits_of(M), "soft_l_value_demapper: M must be 2^nbits, nbits in 1..10");
    if (N == 0) return QH_OK;
    DevBuf dE, ds, dL;
    if ((rc = dE.from_host(E, (size_t)N * sizeof(Cx<R>)))) return rc;
    if ((rc = ds.from_host(alphabet, (size_t)M * sizeof(Cx<R>)))) return rc;
    if ((rc = dL.alloc((size_t)N * nbits * sizeof(double)))) return rc;
    if ((rc = llr_dev<R>(dE.p, N, nbits, snr, ds.p, M, minmax, (double *)dL.p))) return rc;
    if ((rc = dL.to_host(L, dL.n))) return rc;
    QH_HIP(hipStreamSynchronize(g_stream));
    return QH_OK;
}

template <typename R>
int metrics_dev(const void *E, int64_t N, const int32_t *idx_tx, int64_t ntx, const void *alphabet, int M, int rot, int64_t lag, int64_t trim,
                double snr, int minmax, int64_t *counts, double *sums)
{
    int rc = ensure_init();
    if (rc) return rc;
    const int nb = nbits_of(M);
    QH_REQUIRE(N > 0 && ntx > 0 && nb > 0 && trim >= 0 && 2 * trim < N, "metrics: bad sizes (M must be 2^nbits, nbits in 1..10)");
    QH_REQUIRE(std::min(N - trim, ntx + lag) > std::max(trim, lag), "metrics: the alignment leaves no overlap");
    const int F = 5 + nb;
    const unsigned g = grid_for(N - 2 * trim);
    void *buf = nullptr;
    if ((rc = scratch(Slot::METRICS, ((size_t)g + 1) * F * sizeof(double), &buf))) return rc;
    double *part = (double *)buf, *tot = part + (size_t)g * F;
    if (minmax) {
        QH_NB_DISPATCH(nb, hipLaunchKernelGGL((metrics_kernel<R, NB, true>), dim3(g), dim3(MET_THREADS), 0, g_stream, (const Cx<R> *)E, trim, N - trim, rot, lag,
                                               idx_tx, ntx, (const Cx<R> *)alphabet, (R)snr, part))
    } else {
        QH_NB_DISPATCH(nb, hipLaunchKernelGGL((metrics_kernel<R, NB, false>), dim3(g), dim3(MET_THREADS), 0, g_stream, (const Cx<R> *)E, trim, N - trim, rot, lag,
                                               idx_tx, ntx, (const Cx<R> *)alphabet, (R)snr, part))
    }
    QH_HIP(hipGetLastError());
    if ((rc = reduce_fields(part, (int)g, F, tot))) return rc;
    double h[5 + MET_NBMAX];
    QH_HIP(hipMemcpyAsync(h, tot, (size_t)F * sizeof(double), hipMemcpyDeviceToHost, g_stream));
    QH_HIP(hipStreamSynchronize(g_stream));
    for (int f = 0; f < 3; f++) counts[f] = (int64_t)h[f];
    for (int f = 3; f < F; f++) sums[f - 3] = h[f];
    return QH_OK;
}

// class statistics -> (snr, S0, N0) in result; L: the length the class fractions are taken over (the reference's signal_rx.shape[0])
template <typename R>
int snr_stats(const void *E, int64_t i0, int64_t i1, int rot, int64_t lag, const int32_t *idx_tx, int64_t ntx, int M, int64_t L, double *result)
{
    const unsigned g = grid_for(i1 - i0);
    void *buf = nullptr;
    const size_t np = (size_t)g * M * 3, nt = (size_t)M * 3 + (size_t)M * 2 + M;
    int rc;
    if ((rc = scratch(Slot::SNR_EST, (np + nt) * sizeof(double), &buf))) return rc;
    double *part = (double *)buf, *sums = part + np, *mu = sums + (size_t)M * 3, *sse = mu + (size_t)M * 2;
    if (M <= MET_THREADS) hipLaunchKernelGGL((class_stats_kernel<R, false, 1>), dim3(g), dim3(MET_THREADS), 0, g_stream, (const Cx<R> *)E, i0, i1, rot, lag,
                                             idx_tx, ntx, M, (const double *)nullptr, part);
    else hipLaunchKernelGGL((class_stats_kernel<R, false, (1 << MET_NBMAX) / MET_THREADS>), dim3(g), dim3(MET_THREADS), 0, g_stream, (const Cx<R> *)E, i0, i1,
                            rot, lag, idx_tx, ntx, M, (const double *)nullptr, part);
    QH_HIP(hipGetLastError());
    if ((rc = reduce_fields(part, (int)g, 3 * M, sums))) return rc;
    hipLaunchKernelGGL(class_mean_kernel, dim3((M + 63) / 64), dim3(64), 0, g_stream, (const double *)sums, M, mu);
    if (M <= MET_THREADS) hipLaunchKernelGGL((class_stats_kernel<R, true, 1>), dim3(g), dim3(MET_THREADS), 0, g_stream, (const Cx<R> *)E, i0, i1, rot, lag,
                                             idx_tx, ntx, M, (const double *)mu, part);
    else hipLaunchKernelGGL((class_stats_kernel<R, true, (1 << MET_NBMAX) / MET_THREADS>), dim3(g), dim3(MET_THREADS), 0, g_stream, (const Cx<R> *)E, i0, i1,
                            rot, lag, idx_tx, ntx, M, (const double *)mu, part);
    QH_HIP(hipGetLastError());
    if ((rc = reduce_fields(part, (int)g, M, sse))) return rc;
    std::vector<double> h(nt);
    QH_HIP(hipMemcpyAsync(h.data(), sums, nt * sizeof(double), hipMemcpyDeviceToHost, g_stream));
    QH_HIP(hipStreamSynchronize(g_stream));
    // estimate_snr (pythran_dsp.py:275-286), classes in alphabet order
    double in_pow = 0, N0 = 0;
    for (int t = 0; t < M; t++) {
        const double K = h[3 * t], Px = K / (double)L;
        const double mre = h[3 * M + 2 * t], mim = h[3 * M + 2 * t + 1];
        const double sigma = std::sqrt(h[5 * M + t] / K);
        N0 += sigma * sigma * Px;
        in_pow += (mre * mre + mim * mim) * Px;
    }
    result[0] = in_pow / N0; result[1] = in_pow; result[2] = N0;
    return QH_OK;
}

template <typename R>
int estimate_snr_dev(const void *E, int64_t N, const int32_t *idx_tx, int64_t ntx, const void *alphabet, int M, int rot, int64_t lag, int64_t trim,
                     double *result)
{
    (void)alphabet;
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(N > 0 && ntx > 0 && M >= 1 && M <= 1 << MET_NBMAX && trim >= 0 && 2 * trim < N, "estimate_snr: bad sizes (M <= 1024)");
    // compared symbols of the aligned overlap: the class fractions are taken over them
    const int64_t a = std::max(trim, lag), b = std::min(N - trim, ntx + lag);
    QH_REQUIRE(b > a, "estimate_snr: the alignment leaves no overlap");
    return snr_stats<R>(E, trim, N - trim, rot, lag, idx_tx, ntx, M, b - a, result);
}

template <typename R> int estimate_snr_host(const void *rx, int64_t N, const void *tx, int64_t ntx, const void *alphabet, int M, double *result)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(N > 0 && ntx == N && M >= 1 && M <= 1 << MET_NBMAX, "estimate_snr: signal_rx and symbols_tx need the same length, M <= 1024");
    DevBuf dE, dt, ds, di;
    if ((rc = dE.from_host(rx, (size_t)N * sizeof(Cx<R>)))) return rc;
    if ((rc = dt.from_host(tx, (size_t)N * sizeof(Cx<R>)))) return rc;
    if ((rc = ds.from_host(alphabet, (size_t)M * sizeof(Cx<R>)))) return rc;
    if ((rc = di.alloc((size_t)N * sizeof(int32_t)))) return rc;
    hipLaunchKernelGGL((exact_label_kernel<R>), dim3((unsigned)((N + MET_THREADS - 1) / MET_THREADS)), dim3(MET_THREADS), 0, g_stream, (const Cx<R> *)dt.p, N,
                       (const Cx<R> *)ds.p, M, (int32_t *)di.p);
    QH_HIP(hipGetLastError());
    return snr_stats<R>(dE.p, 0, N, 0, 0, (const int32_t *)di.p, N, M, N, result);
}

template <typename R> int mi_fast_host(const void *x, const void *tx, int64_t L, const void *alphabet, int M, double N0, double *mi)
{
    int rc = ensure_init();
    if (rc) return rc;
    const int nb = nbits_of(M);
    QH_REQUIRE(L > 0 && nb > 0, "cal_mi_mc_fast: M must be 2^nbits, nbits in 1..10");
    DevBuf dx, dt, ds, dp;
    const unsigned g = grid_for(L);
    if ((rc = dx.from_host(x, (size_t)L * sizeof(Cx<R>)))) return rc;
    if ((rc = dt.from_host(tx, (size_t)L * sizeof(Cx<R>)))) return rc;
    if ((rc = ds.from_host(alphabet, (size_t)M * sizeof(Cx<R>)))) return rc;
    if ((rc = dp.alloc(((size_t)g + 1) * sizeof(double)))) return rc;
    double *part = (double *)dp.p;
    QH_NB_DISPATCH(nb, hipLaunchKernelGGL((mi_fast_kernel<R, NB>), dim3(g), dim3(MET_THREADS), 0, g_stream, (const Cx<R> *)dx.p, (const Cx<R> *)dt.p, L,
                                           (const Cx<R> *)ds.p, (R)(1. / N0), part))
    QH_HIP(hipGetLastError());
    if ((rc = reduce_fields(part, (int)g, 1, part + g))) return rc;
    double s = 0;
    QH_HIP(hipMemcpyAsync(&s, part + g, sizeof(double), hipMemcpyDeviceToHost, g_stream));
    QH_HIP(hipStreamSynchronize(g_stream));
    *mi = std::log2((double)M) - s / (double)L;
    return QH_OK;
}

template <typename R> int mi_mc_host(const void *noise, int64_t L, const void *alphabet, int M, double N0, double *mi)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(L > 0 && M >= 1 && M <= 1 << MET_NBMAX, "cal_mi_mc: bad sizes (M <= 1024)");
    DevBuf dn, ds, dp;
    const unsigned g = grid_for(L * M);
    if ((rc = dn.from_host(noise, (size_t)L * sizeof(Cx<R>)))) return rc;
    if ((rc = ds.from_host(alphabet, (size_t)M * sizeof(Cx<R>)))) return rc;
    if ((rc = dp.alloc(((size_t)g + 1) * sizeof(double)))) return rc;
    double *part = (double *)dp.p;
    hipLaunchKernelGGL((mi_mc_kernel<R>), dim3(g), dim3(MET_THREADS), 0, g_stream, (const Cx<R> *)dn.p, L, (const Cx<R> *)ds.p, M, (R)(1. / N0), part);
    QH_HIP(hipGetLastError());
    if ((rc = reduce_fields(part, (int)g, 1, part + g))) return rc;
    double s = 0;
    QH_HIP(hipMemcpyAsync(&s, part + g, sizeof(double), hipMemcpyDeviceToHost, g_stream));
    QH_HIP(hipStreamSynchronize(g_stream));
    *mi = std::log2((double)M) - s / (double)M / (double)L;
    return QH_OK;
}

constexpr int MC_MAXSNR = 65535;                 // SNR points of one launch (the grid's y)
constexpr int64_t MC_MAXNS = (int64_t)1 << 31;    // draws per SNR point

static int awgn_mc_sizes(int nsnr, int64_t ns)
{
    QH_REQUIRE(nsnr >= 1 && nsnr <= MC_MAXSNR, "awgn_mc: between 1 and 65535 SNR points");
    QH_REQUIRE(ns >= 1 && ns <= MC_MAXNS, "awgn_mc: between 1 and 2^31 draws per SNR point");
    return QH_OK;
}

template <typename R> int awgn_mc_noise_dev(void *z, const double *snr, int nsnr, int64_t ns, uint64_t seed)
{
    int rc = awgn_mc_sizes(nsnr, ns);
    if (rc) return rc;
    QH_REQUIRE(z && snr, "awgn_mc_noise: z and snr must be given");
    if ((rc = ensure_init())) return rc;
    hipLaunchKernelGGL((awgn_mc_noise_kernel<R>), dim3((unsigned)((ns + MET_THREADS - 1) / MET_THREADS), nsnr), dim3(MET_THREADS), 0, g_stream, (Cx<R> *)z,
                       snr, ns, (unsigned)seed, (unsigned)(seed >> 32));
    QH_HIP(hipGetLastError());
    return QH_OK;
}

constexpr size_t MC_PARTIAL_DOUBLES = (size_t)1 << 22;      // most doubles of workgroup partials held at once (32 MiB)

// out (nsnr, 2 + nbits) = [gmi, mi, gmi per bit] of every SNR point, nothing read back.  The SNR points go through in batches whose partials fit
// MC_PARTIAL_DOUBLES - three launches per batch; a 31-point curve of 1024-QAM is one batch, 65535 points of it are 177 - and a point's result does
// not depend on the batch it falls into.
template <typename R> int awgn_mc_dev(const void *alphabet, int M, const double *snr, int nsnr, const void *z, int64_t ns, double *out)
{
    int rc = awgn_mc_sizes(nsnr, ns);
    if (rc) return rc;
    const int nb = nbits_of(M);
    QH_REQUIRE(nb > 0, "awgn_mc: M must be 2^nbits, nbits in 1..10");
    QH_REQUIRE(alphabet && snr && z && out, "awgn_mc: alphabet, snr, z and out must be given");
    if ((rc = ensure_init())) return rc;
    const int F = 1 + nb;
    const unsigned g = grid_for(ns * M);
    const int batch = (int)std::min<size_t>((size_t)nsnr, std::max<size_t>(1, MC_PARTIAL_DOUBLES / (((size_t)g + 1) * F)));
    void *buf = nullptr;
    if ((rc = scratch(Slot::AWGN_MC, ((size_t)g + 1) * batch * F * sizeof(double), &buf))) return rc;
    double *part = (double *)buf, *tot = part + (size_t)g * batch * F;
    for (int p0 = 0; p0 < nsnr; p0 += batch) {
        const int n = std::min(batch, nsnr - p0);
        QH_NB_DISPATCH(nb, hipLaunchKernelGGL((awgn_mc_kernel<R, NB>), dim3(g, n), dim3(MET_THREADS), 0, g_stream, (const Cx<R> *)alphabet, snr + p0,
                                               (const Cx<R> *)z + (size_t)p0 * ns, ns, part))
        QH_HIP(hipGetLastError());
        if ((rc = reduce_fields(part, (int)g, F, tot, n))) return rc;
        hipLaunchKernelGGL(awgn_mc_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, g_stream, (const double *)tot, n, nb, (double)ns * (double)M,
                           out + (size_t)p0 * (2 + nb));
        QH_HIP(hipGetLastError());
    }
    return QH_OK;
}

}  // namespace qh

extern "C" {
int qh_awgn_mc_noise_c64_dev(void *z, const double *snr, int nsnr, int64_t ns, uint64_t seed) { return qh::awgn_mc_noise_dev<float>(z, snr, nsnr, ns, seed); }
int qh_awgn_mc_noise_c128_dev(void *z, const double *snr, int nsnr, int64_t ns, uint64_t seed) { return qh::awgn_mc_noise_dev<double>(z, snr, nsnr, ns, seed); }
int qh_awgn_mc_c64_dev(const void *alphabet, int M, const double *snr, int nsnr, const void *z, int64_t ns, double *out)
{ return qh::awgn_mc_dev<float>(alphabet, M, snr, nsnr, z, ns, out); }
int qh_awgn_mc_c128_dev(const void *alphabet, int M, const double *snr, int nsnr, const void *z, int64_t ns, double *out)
{ return qh::awgn_mc_dev<double>(alphabet, M, snr, nsnr, z, ns, out); }
int qh_soft_l_value_demapper_c64(const void *rx, int64_t N, int nbits, double snr, const void *alphabet, int M, double *L)
{ return qh::llr_host<float>(rx, N, nbits, snr, alphabet, M, 0, L); }
int qh_soft_l_value_demapper_c128(const void *rx, int64_t N, int nbits, double snr, const void *alphabet, int M, double *L)
{ return qh::llr_host<double>(rx, N, nbits, snr, alphabet, M, 0, L); }
int qh_soft_l_value_demapper_minmax_c64(const void *rx, int64_t N, int nbits, double snr, const void *alphabet, int M, double *L)
{ return qh::llr_host<float>(rx, N, nbits, snr, alphabet, M, 1, L); }
int qh_soft_l_value_demapper_minmax_c128(const void *rx, int64_t N, int nbits, double snr, const void *alphabet, int M, double *L)
{ return qh::llr_host<double>(rx, N, nbits, snr, alphabet, M, 1, L); }
int qh_soft_l_value_demapper_c64_dev(const void *rx, int64_t N, int nbits, double snr, const void *alphabet, int M, int minmax, double *L)
{ return qh::llr_dev<float>(rx, N, nbits, snr, alphabet, M, minmax, L); }
int qh_soft_l_value_demapper_c128_dev(const void *rx, int64_t N, int nbits, double snr, const void *alphabet, int M, int minmax, double *L)
{ return qh::llr_dev<double>(rx, N, nbits, snr, alphabet, M, minmax, L); }
int qh_estimate_snr_c64(const void *rx, int64_t N, const void *tx, int64_t ntx, const void *alphabet, int M, double *result)
{ return qh::estimate_snr_host<float>(rx, N, tx, ntx, alphabet, M, result); }
int qh_estimate_snr_c128(const void *rx, int64_t N, const void *tx, int64_t ntx, const void *alphabet, int M, double *result)
{ return qh::estimate_snr_host<double>(rx, N, tx, ntx, alphabet, M, result); }
int qh_estimate_snr_c64_dev(const void *E, int64_t N, const int32_t *idx_tx, int64_t ntx, const void *alphabet, int M, int rot, int64_t lag,
                            int64_t trim, double *result)
{ return qh::estimate_snr_dev<float>(E, N, idx_tx, ntx, alphabet, M, rot, lag, trim, result); }
int qh_estimate_snr_c128_dev(const void *E, int64_t N, const int32_t *idx_tx, int64_t ntx, const void *alphabet, int M, int rot, int64_t lag,
                             int64_t trim, double *result)
{ return qh::estimate_snr_dev<double>(E, N, idx_tx, ntx, alphabet, M, rot, lag, trim, result); }
int qh_cal_mi_mc_c64(const void *noise, int64_t L, const void *alphabet, int M, double N0, double *mi)
{ return qh::mi_mc_host<float>(noise, L, alphabet, M, N0, mi); }
int qh_cal_mi_mc_c128(const void *noise, int64_t L, const void *alphabet, int M, double N0, double *mi)
{ return qh::mi_mc_host<double>(noise, L, alphabet, M, N0, mi); }
int qh_cal_mi_mc_fast_c64(const void *x, const void *tx, int64_t L, const void *alphabet, int M, double N0, double *mi)
{ return qh::mi_fast_host<float>(x, tx, L, alphabet, M, N0, mi); }
int qh_cal_mi_mc_fast_c128(const void *x, const void *tx, int64_t L, const void *alphabet, int M, double N0, double *mi)
{ return qh::mi_fast_host<double>(x, tx, L, alphabet, M, N0, mi); }
int qh_metrics_c64_dev(const void *E, int64_t N, const int32_t *idx_tx, int64_t ntx, const void *alphabet, int M, int rot, int64_t lag, int64_t trim,
                       double snr, int minmax, int64_t *counts, double *sums)
{ return qh::metrics_dev<float>(E, N, idx_tx, ntx, alphabet, M, rot, lag, trim, snr, minmax, counts, sums); }
int qh_metrics_c128_dev(const void *E, int64_t N, const int32_t *idx_tx, int64_t ntx, const void *alphabet, int M, int rot, int64_t lag, int64_t trim,
                        double snr, int minmax, int64_t *counts, double *sums)
{ return qh::metrics_dev<double>(E, N, idx_tx, ntx, alphabet, M, rot, lag, trim, snr, minmax, counts, sums); }
}
