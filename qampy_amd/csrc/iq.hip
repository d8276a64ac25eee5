// IQ conditioning of every row of an (nmodes, L) complex array in HBM (qampy/core/analog_frontend.py:30-52 comp_IQ_inbalance, :91-132
// orthonormalize_signal): both are affine maps of (I, Q) whose coefficients follow from ten sums per row.
//
//   moments   per row sum I, sum Q, sum I^2, sum Q^2, sum I Q over all samples and over every os-th sample, in double: a workgroup sums a
//             tile of IQ_TILE samples in a fixed order (thread-strided, then a tree in LDS), a second launch sums the tile totals of a row in
//             a fixed order.  No atomics: a repeated call is bit-identical.
//   coeffs    one workgroup turns the moments into y = A (I, Q)^T + b per row: coef[row] = (a00, a01, a10, a11, b0, b1), nothing read back.
//   affine    one point-wise pass, evaluated in double, stored in the signal's precision; `out` may be `E`.
//
// The tile totals live in scratch slot Slot::IQ.  The derivation of the two maps is in DESIGN.md 3.14.
#include "common.h"
#include <cmath>

namespace qh {

constexpr int IQ_TILE = 4096, IQ_T = 256, IQ_NMOM = 10;
enum { IQ_ORTHONORMALIZE = 0, IQ_IMBALANCE = 1, IQ_CENTRE = 2 };

// fixed-order tree over the workgroup's IQ_NMOM-vectors; the totals are in s[0 .. IQ_NMOM - 1] of thread 0's slot
__device__ __forceinline__ void iq_block_reduce(double (*s)[IQ_NMOM], const double *v)
{
    for (int q = 0; q < IQ_NMOM; q++) s[threadIdx.x][q] = v[q];
    __syncthreads();
    for (int h = IQ_T / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h)
            for (int q = 0; q < IQ_NMOM; q++) s[threadIdx.x][q] += s[threadIdx.x + h][q];
        __syncthreads();
    }
}

// grid (tiles, nmodes); part (nmodes, tiles, IQ_NMOM)
template <typename R>
__global__ void __launch_bounds__(IQ_T) iq_moments_tile_kernel(const Cx<R> *__restrict__ E, int64_t L, int os, double *__restrict__ part)
{
    __shared__ double s[IQ_T][IQ_NMOM];
    const size_t row = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * IQ_TILE;
    const Cx<R> *x = E + row * L;
    double v[IQ_NMOM];
    for (int q = 0; q < IQ_NMOM; q++) v[q] = 0.0;
    for (int t = threadIdx.x; t < IQ_TILE; t += IQ_T) {
        const int64_t n = base + t;
        if (n >= L) break;
        const Cx<R> e = ldg(x + n);
        const double I = (double)e.re, Q = (double)e.im;
        v[0] += I; v[1] += Q; v[2] += I * I; v[3] += Q * Q; v[4] += I * Q;
        if (n % os == 0) { v[5] += I; v[6] += Q; v[7] += I * I; v[8] += Q * Q; v[9] += I * Q; }
    }
    iq_block_reduce(s, v);
    if (threadIdx.x < IQ_NMOM) part[(row * gridDim.x + blockIdx.x) * IQ_NMOM + threadIdx.x] = s[0][threadIdx.x];
}

// grid (nmodes); mom (nmodes, IQ_NMOM)
__global__ void __launch_bounds__(IQ_T) iq_moments_final_kernel(const double *__restrict__ part, int64_t tiles, double *__restrict__ mom)
{
    __shared__ double s[IQ_T][IQ_NMOM];
    const size_t row = blockIdx.x;
    double v[IQ_NMOM];
    for (int q = 0; q < IQ_NMOM; q++) v[q] = 0.0;
    for (int64_t t = threadIdx.x; t < tiles; t += IQ_T)
        for (int q = 0; q < IQ_NMOM; q++) v[q] += part[(row * tiles + t) * IQ_NMOM + q];
    iq_block_reduce(s, v);
    if (threadIdx.x < IQ_NMOM) mom[row * IQ_NMOM + threadIdx.x] = s[0][threadIdx.x];
}

// one workgroup; coef (nmodes, 6)
__global__ void __launch_bounds__(IQ_T) iq_coeffs_kernel(const double *__restrict__ mom, int nmodes, int64_t L, int os, int kind, double *__restrict__ coef)
{
    if (kind == IQ_ORTHONORMALIZE) {
        const double n = (double)L, ns = (double)((L + os - 1) / os);
        for (int row = threadIdx.x; row < nmodes; row += IQ_T) {
            const double *m = mom + (size_t)row * IQ_NMOM;
            const double mI = m[0] / n, mQ = m[1] / n;
            const double PI = m[2] / n - mI * mI, PQ = m[3] / n - mQ * mQ, PIQ = m[4] / n - mI * mQ;      // powers of the centred rails
            const double a = 1.0 / sqrt(PI), d = 1.0 / sqrt(PQ), g = PIQ / (PI * sqrt(PQ));
            const double sI = m[5] / ns, sQ = m[6] / ns;                                                  // means of every os-th sample
            const double VI = m[7] / ns - sI * sI, VQ = m[8] / ns - sQ * sQ, VIQ = m[9] / ns - sI * sQ;
            const double p = a * a * VI + d * d * VQ - 2.0 * d * g * VIQ + g * g * VI;                     // mean |.|^2 of every os-th output
            const double s = 1.0 / sqrt(p);
            double *c = coef + (size_t)row * 6;
            c[0] = s * a; c[1] = 0.0; c[2] = -s * g; c[3] = s * d;
            c[4] = -(c[0] * sI); c[5] = -(c[2] * sI + c[3] * sQ);
        }
        return;
    }
    // pooled over all rows, summed in row order by every thread alike
    double t[5] = {0, 0, 0, 0, 0};
    for (int row = 0; row < nmodes; row++)
        for (int q = 0; q < 5; q++) t[q] += mom[(size_t)row * IQ_NMOM + q];
    const double n = (double)L * (double)nmodes;
    const double mI = t[0] / n, mQ = t[1] / n;
    double c0 = 1.0, c1 = 0.0, c2 = 0.0, c3 = 1.0;
    if (kind == IQ_IMBALANCE) {
        const double SII = t[2] - n * mI * mI, SQQ = t[3] - n * mQ * mQ, SIQ = t[4] - n * mI * mQ;
        const double sn = -(SIQ / SII), cs = sqrt(1.0 - sn * sn);          // sin, cos of arcsin(-sum IQ / sum I^2)
        const double SQb = (SQQ + 2.0 * sn * SIQ + sn * sn * SII) / (cs * cs);
        const double g = sqrt(SII / SQb);
        c2 = g * sn / cs; c3 = g / cs;
    }
    for (int row = threadIdx.x; row < nmodes; row += IQ_T) {
        double *c = coef + (size_t)row * 6;
        c[0] = c0; c[1] = c1; c[2] = c2; c[3] = c3;
        c[4] = -(c0 * mI + c1 * mQ); c[5] = -(c2 * mI + c3 * mQ);
    }
}

// grid (ceil(L / 1024), nmodes)
template <typename R>
__global__ void __launch_bounds__(IQ_T) iq_affine_kernel(const Cx<R> *E, int64_t L, const double *__restrict__ coef, Cx<R> *out)
{
    const size_t row = blockIdx.y;
    const double *c = coef + row * 6;
    const double a00 = c[0], a01 = c[1], a10 = c[2], a11 = c[3], b0 = c[4], b1 = c[5];
    const int64_t base = (int64_t)blockIdx.x * 1024;
    for (int t = threadIdx.x; t < 1024; t += IQ_T) {
        const int64_t n = base + t;
        if (n >= L) break;
        const Cx<R> e = ldg(E + row * L + n);
        const double I = (double)e.re, Q = (double)e.im;
        stg(out + row * L + n, Cx<R>{(R)(a00 * I + a01 * Q + b0), (R)(a10 * I + a11 * Q + b1)});
    }
}

template <typename R> int iq_moments_dev(const void *E, int nmodes, int64_t L, int os, double *mom)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 1 && os >= 1, "iq_moments: bad sizes");
    QH_REQUIRE(E && mom, "iq_moments: E and mom must be given");
    const int64_t tiles = (L + IQ_TILE - 1) / IQ_TILE;
    QH_REQUIRE(tiles <= 0x7fffffffLL, "iq_moments: L too long");
    void *part = nullptr;
    if ((rc = scratch(Slot::IQ, (size_t)nmodes * tiles * IQ_NMOM * sizeof(double), &part))) return rc;
    hipLaunchKernelGGL((iq_moments_tile_kernel<R>), dim3((unsigned)tiles, nmodes), dim3(IQ_T), 0, g_stream, (const Cx<R> *)E, L, os, (double *)part);
    hipLaunchKernelGGL(iq_moments_final_kernel, dim3(nmodes), dim3(IQ_T), 0, g_stream, (const double *)part, tiles, mom);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

static int iq_coeffs_dev(const double *mom, int nmodes, int64_t L, int os, int kind, double *coef)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 1 && os >= 1, "iq_coeffs: bad sizes");
    QH_REQUIRE(kind >= IQ_ORTHONORMALIZE && kind <= IQ_CENTRE, "iq_coeffs: kind is 0 (orthonormalize), 1 (imbalance) or 2 (centre)");
    QH_REQUIRE(mom && coef, "iq_coeffs: mom and coef must be given");
    hipLaunchKernelGGL(iq_coeffs_kernel, dim3(1), dim3(IQ_T), 0, g_stream, mom, nmodes, L, os, kind, coef);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R> int iq_affine_dev(const void *E, int nmodes, int64_t L, const double *coef, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 1, "iq_affine: bad sizes");
    QH_REQUIRE(E && coef && out, "iq_affine: E, coef and out must be given");
    const int64_t blocks = (L + 1023) / 1024;
    QH_REQUIRE(blocks <= 0x7fffffffLL, "iq_affine: L too long");
    hipLaunchKernelGGL((iq_affine_kernel<R>), dim3((unsigned)blocks, nmodes), dim3(IQ_T), 0, g_stream, (const Cx<R> *)E, L, coef, (Cx<R> *)out);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

}  // namespace qh

extern "C" {
int qh_iq_moments_c64_dev(const void *E, int nmodes, int64_t L, int os, double *mom) { return qh::iq_moments_dev<float>(E, nmodes, L, os, mom); }
int qh_iq_moments_c128_dev(const void *E, int nmodes, int64_t L, int os, double *mom) { return qh::iq_moments_dev<double>(E, nmodes, L, os, mom); }
int qh_iq_coeffs_dev(const double *mom, int nmodes, int64_t L, int os, int kind, double *coef) { return qh::iq_coeffs_dev(mom, nmodes, L, os, kind, coef); }
int qh_iq_affine_c64_dev(const void *E, int nmodes, int64_t L, const double *coef, void *out) { return qh::iq_affine_dev<float>(E, nmodes, L, coef, out); }
int qh_iq_affine_c128_dev(const void *E, int nmodes, int64_t L, const double *coef, void *out) { return qh::iq_affine_dev<double>(E, nmodes, L, coef, out); }
}
