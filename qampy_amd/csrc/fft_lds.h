// Stockham autosort FFT in LDS, shared by the kernels that transform one block per workgroup (cd.hip, foe.hip, fft.hip, impair.hip): every pass reads
// its butterflies' inputs from LDS into registers, runs radix-8/4/2 butterflies there and writes the results back in place (a barrier
// between the reads and the writes, so one N-point buffer suffices).  `tw` is the table W_N^m = exp(-2 pi i m / N), m = 0 .. N - 1, of
// the transform's own size, in the signal's precision.
#pragma once
#include "common.h"

namespace qh {

constexpr int CD_T = 256;                 // threads per workgroup

template <typename R> __device__ __forceinline__ Cx<R> mul_mi(Cx<R> a) { return Cx<R>{a.im, -a.re}; }     // a * (-i)

// The table of the units that form it on the device (foe.hip, fft.hip): tab[m] = exp(-2 pi i m / n), m = 0 .. n - 1 (n a power of two: m / n
// is exact).  grid (n / 256 rounded up).  (`static`: two translation units instantiate it.)
template <typename R> static __global__ void __launch_bounds__(256) twiddle_kernel(Cx<R> *tab, int n)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    double sn, cs;
    sincospi(-2.0 * ((double)m / (double)n), &sn, &cs);
    stg(tab + m, Cx<R>{(R)cs, (R)sn});
}

// forward DFTs in registers: y[s] = sum_r v[r] exp(-2 pi i r s / RAD)
template <typename R> __device__ __forceinline__ void dft2(Cx<R> &a, Cx<R> &b)
{
    const Cx<R> t = a;
    a = cadd(t, b); b = csub(t, b);
}
template <typename R> __device__ __forceinline__ void dft4(Cx<R> &a0, Cx<R> &a1, Cx<R> &a2, Cx<R> &a3)
{
    const Cx<R> t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), t3 = mul_mi(csub(a1, a3));
    a0 = cadd(t0, t2); a2 = csub(t0, t2); a1 = cadd(t1, t3); a3 = csub(t1, t3);
}
template <typename R, int RAD> __device__ __forceinline__ void dft(Cx<R> *v)
{
    if constexpr (RAD == 2) {
        dft2(v[0], v[1]);
    } else if constexpr (RAD == 4) {
        dft4(v[0], v[1], v[2], v[3]);
    } else {
        static_assert(RAD == 8, "radix 2, 4 or 8");
        const R h = (R)0.70710678118654752440;
        dft4(v[0], v[2], v[4], v[6]);                 // even samples -> E0..E3 in v[0], v[2], v[4], v[6]
        dft4(v[1], v[3], v[5], v[7]);                 // odd samples  -> O0..O3 in v[1], v[3], v[5], v[7]
        const Cx<R> o1 = Cx<R>{h * (v[3].re + v[3].im), h * (v[3].im - v[3].re)};        // O1 * exp(-i pi / 4)
        const Cx<R> o2 = mul_mi(v[5]);                                                     // O2 * exp(-i pi / 2)
        const Cx<R> o3 = Cx<R>{h * (v[7].im - v[7].re), -h * (v[7].re + v[7].im)};       // O3 * exp(-3 i pi / 4)
        const Cx<R> e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6], o0 = v[1];
        v[0] = cadd(e0, o0); v[4] = csub(e0, o0);
        v[1] = cadd(e1, o1); v[5] = csub(e1, o1);
        v[2] = cadd(e2, o2); v[6] = csub(e2, o2);
        v[3] = cadd(e3, o3); v[7] = csub(e3, o3);
    }
}

// One Stockham pass of radix RAD over sub-transforms of length NS * RAD (NS = product of the earlier radices):
//   butterfly j (0 <= j < N / RAD), k = j mod NS:  v[r] = x[j + r N / RAD] * W_{NS RAD}^{r k};  v = DFT_RAD(v);
//   y[(j / NS) NS RAD + k + s NS] = v[s]
template <typename R, int N, int RAD, int NS>
__device__ __forceinline__ void fft_pass(Cx<R> *buf, const Cx<R> *__restrict__ tw)
{
    constexpr int NB = N / RAD, PER = (NB + CD_T - 1) / CD_T;
    Cx<R> v[PER][RAD];
#pragma unroll
    for (int p = 0; p < PER; p++) {
        const int j = threadIdx.x + p * CD_T;
        if (NB % CD_T == 0 || j < NB) {
#pragma unroll
            for (int r = 0; r < RAD; r++) v[p][r] = buf[j + r * NB];
        }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < PER; p++) {
        const int j = threadIdx.x + p * CD_T;
        if (NB % CD_T == 0 || j < NB) {
            const int k = j % NS;
            if constexpr (NS > 1) {
#pragma unroll
                for (int r = 1; r < RAD; r++) v[p][r] = cmul(v[p][r], ldg(tw + r * k * (N / (NS * RAD))));
            }
            dft<R, RAD>(v[p]);
            const int d = (j / NS) * NS * RAD + k;
#pragma unroll
            for (int s = 0; s < RAD; s++) buf[d + s * NS] = v[p][s];
        }
    }
    __syncthreads();
}

// radix plan: log2 N = 3a + b -> radix 8 while more than two radix-8 passes' worth of bits remain, then 8 / 4 / 4,4 at the end
template <typename R, int N, int NS>
__device__ __forceinline__ void fft_from(Cx<R> *buf, const Cx<R> *__restrict__ tw)
{
    constexpr int REM = N / NS;
    if constexpr (REM == 1) {
        return;
    } else if constexpr (REM == 2) {
        fft_pass<R, N, 2, NS>(buf, tw);
    } else if constexpr (REM == 4 || REM == 16) {
        fft_pass<R, N, 4, NS>(buf, tw);
        fft_from<R, N, NS * 4>(buf, tw);
    } else {
        fft_pass<R, N, 8, NS>(buf, tw);
        fft_from<R, N, NS * 8>(buf, tw);
    }
}

}  // namespace qh
