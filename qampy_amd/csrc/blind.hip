// Blind signal quality of the rows of an (nrows, L) array already in HBM: nothing here needs the transmitted symbols
// (qampy/core/signal_quality.py:122-271 norm_to_s0, _cal_evm_blind / cal_evm, cal_snr_qam, cal_s0, cal_snr_blind_qpsk).
//
//   blind_moments   mean |E|^2, mean |E|^4, mean re, mean im of every row, or of every block of `block` samples of every row (a tail shorter
//                   than a block is left out).  Every term is formed in double from the sample (|E|^2 = fma(re, re, im im): the products of
//                   float input are exact) and summed in double.
//   blind_finish    (r2, r4, S1, S2, snr, s0) from the moments by the second / fourth-moment estimator of Gao and Tepedelenlioglu,
//                   k = r2^2 / r4,  S1 = 1 - 2 k - sqrt((2 - gamma)(2 k^2 - k)),  S2 = gamma k - 1,  snr = S1 / S2,  s0 = r2 / (1 + S2 / S1),
//                   on the device, so that s0 feeds the next two kernels without a round trip.  NaN / inf wherever the formula gives them.
//   scale_by_stat   out = E / sqrt(s0[row]), every quotient formed in double and rounded to the precision of the row (norm_to_s0); out may be E.
//   blind_evm       per row the sum over its samples of the smallest squared distance between E / sqrt(s0[row]) and a normalised alphabet
//                   (brute force over the M <= 1024 points, held in LDS), or of the squared distance to known / sqrt(s0_known[row]).  The
//                   distances are formed in the precision of the row, the sum in double.
//   qpsk_blind      P = mean |Eref|^2, var = P - |mean Eref|^2 and 10 log10(P / var) per row or block, Eref = (-E^4)^(1/4) on the principal
//                   branch.  arg(-E^4) / 4 = arg(E) + pi / 4 - q pi / 2 with the whole q that brings it into (-pi / 4, pi / 4]: Eref is
//                   E (1 + i) / sqrt 2 turned by quarter turns into that sector - two products and a sign choice, no angle is ever formed.
//
// One reduction serves all of them and repeats bit for bit.  A segment (a row or a block) is cut into nb <= 256 slices of at least 1024 samples;
// a workgroup of 256 threads sums one slice - every thread its samples in ascending order, wave_sum (DPP), the four wave totals in order - and
// writes its partial sums with plain stores (scratch slot Slot::BLIND).  A second launch, one wave per segment, adds the nb partials in a
// fixed order and applies what follows the sum.  No atomics anywhere.
//
// What bounds them: the moments, the scaling and the QPSK sums read (and the scaling writes) every sample once and do a dozen operations on
// it - memory traffic, and at a few million samples the latency of their two or three small launches.  The distance search does 5 vector operations per (sample, point); a thread keeps 4 samples against every alphabet read
// (a broadcast ds_read shared by the wave), so from a few tens of points on it runs at the vector issue rate.  DESIGN.md 3.20 has the times.
#include "common.h"
#include <cmath>

namespace qh {

constexpr int BL_T = 256;                // threads of a workgroup
constexpr int BL_NB = 256;               // most slices of a segment
constexpr int64_t BL_MIN = 1024;         // fewest samples of a slice before a segment is cut
constexpr int BL_M_MAX = 1024;           // most alphabet points (16 KiB of LDS in complex128)
constexpr int BL_S = 4;                  // samples a thread holds against one alphabet read
constexpr int BL_NSTAT = 6;              // r2, r4, S1, S2, snr, s0

struct BlSplit { int nb; int64_t chunk; };
static BlSplit bl_split(int64_t len)
{
    int64_t chunk = (len + BL_NB - 1) / BL_NB;
    if (chunk < BL_MIN) chunk = BL_MIN;
    return BlSplit{(int)((len + chunk - 1) / chunk), chunk};
}

// what a sample adds to the C sums of its slice
template <typename R> struct MomentTerms {
    static constexpr int C = 4;
    static __device__ __forceinline__ void add(Cx<R> v, double *s)
    {
        const double a = (double)v.re, b = (double)v.im;
        const double p = fma_(a, a, b * b);
        s[0] += p; s[1] = fma_(p, p, s[1]); s[2] += a; s[3] += b;
    }
};
template <typename R> struct QpskTerms {
    static constexpr int C = 3;
    static __device__ __forceinline__ void add(Cx<R> v, double *s)
    {
        const double a = (double)v.re, b = (double)v.im;
        const double c = 0.70710678118654752440;
        const double u = (a - b) * c, w = (a + b) * c;              // E (1 + i) / sqrt 2
        double er, ei;
        if (u > 0 && -u < w && w <= u) { er = u; ei = w; }           // (-pi/4, pi/4]
        else if (w > 0 && -w <= u && u < w) { er = w; ei = -u; }     // (pi/4, 3pi/4]: times -i
        else if (u < 0 && u <= w && w < -u) { er = -u; ei = -w; }    // (3pi/4, 5pi/4]: times -1
        else { er = -w; ei = u; }                                    // times i (and the origin)
        s[0] += fma_(a, a, b * b); s[1] += er; s[2] += ei;
    }
};

// grid (segments, nb): the sums of slice blockIdx.y of segment blockIdx.x -> part[(segment nb + slice) C + c].  Segment s is the block
// s % nblocks of row s / nblocks: seglen samples from sample (s % nblocks) seglen of the row.
template <typename R, typename T>
__global__ void __launch_bounds__(BL_T) blind_sums_kernel(const Cx<R> *__restrict__ E, int64_t L, int64_t nblocks, int64_t seglen, int64_t chunk,
                                                          double *__restrict__ part)
{
    __shared__ double red[BL_T / 64];
    const int64_t seg = blockIdx.x;
    const Cx<R> *x = E + (size_t)(seg / nblocks) * L + (size_t)(seg % nblocks) * seglen;
    const int64_t lo = (int64_t)blockIdx.y * chunk, hi = lo + chunk < seglen ? lo + chunk : seglen;
    double s[T::C];
#pragma unroll
    for (int c = 0; c < T::C; c++) s[c] = 0.;
#pragma unroll 4
    for (int64_t m = lo + threadIdx.x; m < hi; m += BL_T) T::add(ldg(x + m), s);
#pragma unroll
    for (int c = 0; c < T::C; c++) s[c] = block_sum<BL_T>(s[c], red);
    if (threadIdx.x < T::C) {
        double v = s[0];
#pragma unroll
        for (int c = 1; c < T::C; c++) v = (int)threadIdx.x == c ? s[c] : v;
        part[((size_t)seg * gridDim.y + blockIdx.y) * T::C + threadIdx.x] = v;
    }
}

// grid (segments), one wave: the segment's nb partials of C sums each, added in a fixed order and divided by den.  FIN 0: the C means
// -> out[segment C + c]; FIN 1 (C = 3, the QPSK sums): P, var, 10 log10(P / var) -> out[segment 3 + c].
template <int C, int FIN>
__global__ void __launch_bounds__(64) blind_combine_kernel(const double *__restrict__ part, int nb, double den, double *__restrict__ out)
{
    const double *p = part + (size_t)blockIdx.x * nb * C;
    double s[C];
#pragma unroll
    for (int c = 0; c < C; c++) s[c] = 0.;
    for (int b = threadIdx.x; b < nb; b += 64) {
#pragma unroll
        for (int c = 0; c < C; c++) s[c] += p[(size_t)b * C + c];
    }
#pragma unroll
    for (int c = 0; c < C; c++) s[c] = wave_sum(s[c]) / den;
    if (threadIdx.x != 0) return;
    double *o = out + (size_t)blockIdx.x * C;
    if (FIN == 1) {
        const double P = s[0], var = P - (s[1] * s[1] + s[2] * s[2]);
        o[0] = P; o[1] = var; o[2] = 10. * log10(P / var);
    } else {
#pragma unroll
        for (int c = 0; c < C; c++) o[c] = s[c];
    }
}

// one thread per segment: stats[i] = (r2, r4, S1, S2, snr, s0) from mom[i] = (mean |E|^2, mean |E|^4, ..); every operation rounded on its own
__global__ void __launch_bounds__(BL_T) blind_finish_kernel(const double *__restrict__ mom, int64_t n, double gamma, double *__restrict__ stats)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * BL_T + threadIdx.x;
    if (i >= n) return;
    const double r2 = mom[i * 4], r4 = mom[i * 4 + 1];
    const double k = r2 * r2 / r4;
    const double S1 = 1. - 2. * k - sqrt((2. - gamma) * (2. * k * k - k));
    const double S2 = gamma * k - 1.;
    double *o = stats + i * BL_NSTAT;
    o[0] = r2; o[1] = r4; o[2] = S1; o[3] = S2; o[4] = S1 / S2; o[5] = r2 / (1. + S2 / S1);
}

// v / norm, the quotient formed in double and rounded once to the precision of the row: the root of s0 never passes through float
template <typename R> __device__ __forceinline__ Cx<R> bl_scaled(Cx<R> v, double norm)
{
    return Cx<R>{(R)((double)v.re / norm), (R)((double)v.im / norm)};
}

// grid (blocks, nrows); out may be E: every thread reads a sample before it writes it
template <typename R>
__global__ void __launch_bounds__(BL_T) scale_by_stat_kernel(const Cx<R> *E, int64_t L, const double *__restrict__ stats, Cx<R> *out)
{
    const int row = blockIdx.y;
    const double norm = sqrt(stats[(size_t)row * BL_NSTAT + 5]);
    const Cx<R> *x = E + (size_t)row * L;
    Cx<R> *y = out + (size_t)row * L;
    for (int64_t m = (int64_t)blockIdx.x * BL_T + threadIdx.x; m < L; m += (int64_t)gridDim.x * BL_T) stg(y + m, bl_scaled(ldg(x + m), norm));
}

// grid (nb, nrows): slice blockIdx.x of row blockIdx.y -> part[row nb + slice], the sum of the squared distances of the slice's samples
template <typename R>
__global__ void __launch_bounds__(BL_T) blind_evm_kernel(const Cx<R> *__restrict__ E, int64_t L, int64_t chunk, const double *__restrict__ stats,
                                                         const Cx<R> *__restrict__ alphabet, int M, const Cx<R> *__restrict__ known,
                                                         const double *__restrict__ stats_known, double *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) Cx<R> al[BL_M_MAX];
    __shared__ double red[BL_T / 64];
    const int row = blockIdx.y, t = threadIdx.x;
    const double norm = sqrt(stats[(size_t)row * BL_NSTAT + 5]);
    const Cx<R> *x = E + (size_t)row * L;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < L ? lo + chunk : L;
    double acc = 0.;
    if (known) {
        const double normk = sqrt(stats_known[(size_t)row * BL_NSTAT + 5]);
        const Cx<R> *kx = known + (size_t)row * L;
#pragma unroll 4
        for (int64_t m = lo + t; m < hi; m += BL_T) {
            const Cx<R> v = bl_scaled(ldg(x + m), norm), k = bl_scaled(ldg(kx + m), normk);
            const R dr = k.re - v.re, di = k.im - v.im;
            acc += (double)(dr * dr + di * di);
        }
    } else {
        const int M4 = (M + 3) & ~3;                       // padded with copies of point 0: a minimum does not see them
        for (int j = t; j < M4; j += BL_T) al[j] = alphabet[j < M ? j : 0];
        __syncthreads();
        for (int64_t m0 = lo + t; m0 < hi; m0 += (int64_t)BL_T * BL_S) {
            R pr[BL_S], pi[BL_S], best[BL_S];
#pragma unroll
            for (int q = 0; q < BL_S; q++) {
                const int64_t m = m0 + (int64_t)q * BL_T;
                const Cx<R> v = bl_scaled(m < hi ? ldg(x + m) : Cx<R>{(R)0, (R)0}, norm);
                pr[q] = v.re; pi[q] = v.im;
                best[q] = (R)INFINITY;
            }
            for (int j = 0; j < M4; j += 4) {
#pragma unroll
                for (int jj = 0; jj < 4; jj++) {
                    const Cx<R> a = al[j + jj];
#pragma unroll
                    for (int q = 0; q < BL_S; q++) {
                        const R dr = pr[q] - a.re, di = pi[q] - a.im;
                        best[q] = min_(best[q], dr * dr + di * di);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < BL_S; q++) {
                // (a minimum drops a NaN; numpy's does not)
                const R d = (pr[q] != pr[q] || pi[q] != pi[q]) ? pr[q] + pi[q] : best[q];
                if (m0 + (int64_t)q * BL_T < hi) acc += (double)d;
            }
        }
    }
    acc = block_sum<BL_T>(acc, red);
    if (t == 0) part[(size_t)row * gridDim.x + blockIdx.x] = acc;
}

// ------------------------------------------------------------------------------------------------ host side
// rows or blocks: the number of segments per row and their length
static int bl_segments(const char *what, int nrows, int64_t L, int64_t block, int64_t *nblocks, int64_t *seglen)
{
    if (!(nrows >= 1 && nrows <= 65535 && L >= 1 && block >= 0 && block <= L)) {
        set_error(std::string(what) + ": 1 <= nrows <= 65535, L >= 1, 0 <= block <= L");
        return QH_ERR_ARG;
    }
    *nblocks = block > 0 ? L / block : 1;
    *seglen = block > 0 ? block : L;
    if (*nblocks * (int64_t)nrows > 0x7fffffffLL) { set_error(std::string(what) + ": too many blocks"); return QH_ERR_ARG; }
    return QH_OK;
}

template <typename R, typename T, int FIN> int blind_sums_dev(const char *what, const void *E, int nrows, int64_t L, int64_t block, double *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    if (!E || !out) { set_error(std::string(what) + ": null pointer"); return QH_ERR_ARG; }
    int64_t nblocks = 0, seglen = 0;
    if ((rc = bl_segments(what, nrows, L, block, &nblocks, &seglen))) return rc;
    const int64_t nseg = nblocks * nrows;
    const BlSplit sp = bl_split(seglen);
    void *part = nullptr;
    if ((rc = scratch(Slot::BLIND, (size_t)nseg * sp.nb * T::C * sizeof(double), &part))) return rc;
    hipLaunchKernelGGL((blind_sums_kernel<R, T>), dim3((unsigned)nseg, sp.nb), dim3(BL_T), 0, g_stream, (const Cx<R> *)E, L, nblocks, seglen, sp.chunk,
                       (double *)part);
    QH_HIP(hipGetLastError());
    hipLaunchKernelGGL((blind_combine_kernel<T::C, FIN>), dim3((unsigned)nseg), dim3(64), 0, g_stream, (const double *)part, sp.nb, (double)seglen, out);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

static int blind_finish_dev(const double *mom, int64_t n, double gamma, double *stats)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(mom && stats && n >= 1 && n <= 0x7fffffffLL, "blind_finish: bad arguments");
    QH_REQUIRE(std::isfinite(gamma), "blind_finish: gamma must be finite");
    hipLaunchKernelGGL(blind_finish_kernel, dim3((unsigned)((n + BL_T - 1) / BL_T)), dim3(BL_T), 0, g_stream, mom, n, gamma, stats);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R> int scale_by_stat_dev(const void *E, int nrows, int64_t L, const double *stats, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(E && stats && out && nrows >= 1 && nrows <= 65535 && L >= 1, "scale_by_stat: bad arguments");
    int64_t nblk = (L + BL_T * 8 - 1) / (BL_T * 8);
    if (nblk > 4096) nblk = 4096;
    hipLaunchKernelGGL((scale_by_stat_kernel<R>), dim3((unsigned)nblk, nrows), dim3(BL_T), 0, g_stream, (const Cx<R> *)E, L, stats, (Cx<R> *)out);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R> int blind_evm_dev(const void *E, int nrows, int64_t L, const double *stats, const void *alphabet, int M, const void *known,
                                        const double *stats_known, double *evm_sum)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(E && stats && evm_sum && nrows >= 1 && nrows <= 65535 && L >= 1, "blind_evm: bad arguments");
    if (known) QH_REQUIRE(stats_known, "blind_evm: known symbols come with their own stats");
    else QH_REQUIRE(alphabet && M >= 1 && M <= BL_M_MAX, "blind_evm: an alphabet of 1 .. 1024 points");
    const BlSplit sp = bl_split(L);
    void *part = nullptr;
    if ((rc = scratch(Slot::BLIND, (size_t)nrows * sp.nb * sizeof(double), &part))) return rc;
    hipLaunchKernelGGL((blind_evm_kernel<R>), dim3(sp.nb, nrows), dim3(BL_T), 0, g_stream, (const Cx<R> *)E, L, sp.chunk, stats, (const Cx<R> *)alphabet,
                       known ? 0 : M, (const Cx<R> *)known, stats_known, (double *)part);
    QH_HIP(hipGetLastError());
    hipLaunchKernelGGL((blind_combine_kernel<1, 0>), dim3(nrows), dim3(64), 0, g_stream, (const double *)part, sp.nb, 1., evm_sum);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

}  // namespace qh

extern "C" {
int qh_blind_moments_c64_dev(const void *E, int nrows, int64_t L, int64_t block, double *mom)
{ return qh::blind_sums_dev<float, qh::MomentTerms<float>, 0>("blind_moments", E, nrows, L, block, mom); }
int qh_blind_moments_c128_dev(const void *E, int nrows, int64_t L, int64_t block, double *mom)
{ return qh::blind_sums_dev<double, qh::MomentTerms<double>, 0>("blind_moments", E, nrows, L, block, mom); }
int qh_blind_finish_dev(const double *mom, int64_t n, double gamma, double *stats) { return qh::blind_finish_dev(mom, n, gamma, stats); }
int qh_scale_by_stat_c64_dev(const void *E, int nrows, int64_t L, const double *stats, void *out)
{ return qh::scale_by_stat_dev<float>(E, nrows, L, stats, out); }
int qh_scale_by_stat_c128_dev(const void *E, int nrows, int64_t L, const double *stats, void *out)
{ return qh::scale_by_stat_dev<double>(E, nrows, L, stats, out); }
int qh_blind_evm_c64_dev(const void *E, int nrows, int64_t L, const double *stats, const void *alphabet, int M, const void *known,
                         const double *stats_known, double *evm_sum)
{ return qh::blind_evm_dev<float>(E, nrows, L, stats, alphabet, M, known, stats_known, evm_sum); }
int qh_blind_evm_c128_dev(const void *E, int nrows, int64_t L, const double *stats, const void *alphabet, int M, const void *known,
                          const double *stats_known, double *evm_sum)
{ return qh::blind_evm_dev<double>(E, nrows, L, stats, alphabet, M, known, stats_known, evm_sum); }
int qh_qpsk_blind_c64_dev(const void *E, int nrows, int64_t L, int64_t block, double *out)
{ return qh::blind_sums_dev<float, qh::QpskTerms<float>, 1>("qpsk_blind", E, nrows, L, block, out); }
int qh_qpsk_blind_c128_dev(const void *E, int nrows, int64_t L, int64_t block, double *out)
{ return qh::blind_sums_dev<double, qh::QpskTerms<double>, 1>("qpsk_blind", E, nrows, L, block, out); }
}
