// One block of one row through a static filter in LDS: load (with its halo) -> forward FFT -> * H -> inverse FFT -> store.  Shared by the
// dispersion filter (cd.hip) and the PMD filter (impair.hip), which differ in how a sample of the block is formed and in the response a
// row sees - a compile-time source policy:
//
//   PlainRow   the row itself, response H (cd.hip)
//   PmdRow     row `row` of R(theta) E formed from the two input rows, response H (row 0) or conj H (row 1); circular mode only
//
// The table `tab` holds the twiddles W_N^m, then H with the 1/N of the inverse transform folded in (filter_table).  Boundary modes and block
// sizes are described in cd.hip.
#pragma once
#include "fft_lds.h"
#include <cmath>

namespace qh {

// circular_only: the kernel is instantiated without its linear mode.  whole_loop: a whole row (N == L) is loaded by a loop of its own; without it
// the row goes through the block loop at base 0 - the same samples, and at N = 8192 ten vector registers less in the PMD instantiation
template <typename R> struct PlainRow {
    static constexpr bool circular_only = false, whole_loop = true;
    __device__ __forceinline__ Cx<R> load(const Cx<R> *E, int64_t L, int row, int64_t p) const { return ldg(E + (size_t)row * L + p); }
    __device__ __forceinline__ Cx<R> filter(int, Cx<R> x, Cx<R> h) const { return cmul(x, h); }
};
template <typename R> struct PmdRow {
    static constexpr bool circular_only = true, whole_loop = false;
    R c, s;                                                                 // cos, sin of theta
    __device__ __forceinline__ Cx<R> load(const Cx<R> *E, int64_t L, int row, int64_t p) const
    {
        const R a = row == 0 ? c : s, b = row == 0 ? -s : c;                // the row of R(theta)
        const Cx<R> u = ldg(E + p), v = ldg(E + L + p);
        return Cx<R>{a * u.re + b * v.re, a * u.im + b * v.im};
    }
    // x H (row 0) or x conj H (row 1); the products are fused as the compiler fused them in this filter's first form, spelled out so that
    // the bits do not follow the compiler's choice
    __device__ __forceinline__ Cx<R> filter(int row, Cx<R> x, Cx<R> h) const
    {
        if (row) h.im = -h.im;
        return Cx<R>{fma_(x.re, h.re, -(x.im * h.im)), fma_(x.re, h.im, x.im * h.re)};
    }
};

// grid (blocks, nmodes).  mode 0: circular; `whole` (N == L): one transform per row.  mode 1: linear, blocks of parity `parity`
// (blockIdx.x -> block 2 blockIdx.x + parity); `nb` = L // n.
template <typename R, int N, typename Src>
__global__ void __launch_bounds__(CD_T) block_filter_kernel(const Cx<R> *__restrict__ E, Cx<R> *__restrict__ out, int64_t L, int64_t Lout,
                                                            const Cx<R> *__restrict__ tab, Src src, int mode, int whole, int64_t nb, int parity)
{
    extern __shared__ __attribute__((aligned(16))) char smem_bf[];
    Cx<R> *buf = reinterpret_cast<Cx<R> *>(smem_bf);
    const Cx<R> *tw = tab, *H = tab + N;
    constexpr int n = N / 2, q = N / 4;
    const int row = blockIdx.y;
    Cx<R> *y = out + (size_t)row * Lout;
    const Cx<R> zero{(R)0, (R)0};
    const bool circular = Src::circular_only || mode == 0;
    int64_t blk;
    if (circular) {
        blk = blockIdx.x;
        if (whole && Src::whole_loop) {
            for (int t = threadIdx.x; t < N; t += CD_T) buf[t] = src.load(E, L, row, t);
        } else {
            int64_t base = 0;                                               // whole: L == N, p = t
            if (!whole) {
                base = (blk * n - q) % L;
                if (base < 0) base += L;
            }
            for (int t = threadIdx.x; t < N; t += CD_T) {
                int64_t p = base + t;
                if (p >= L) p = L >= N ? p - L : p % L;
                buf[t] = src.load(E, L, row, p);
            }
        }
    } else {
        blk = 2 * (int64_t)blockIdx.x + parity;
        const int64_t s = blk * n - q;
        for (int t = threadIdx.x; t < N; t += CD_T) buf[t] = (t >= q && t < q + n) ? src.load(E, L, row, s + t) : zero;
    }
    __syncthreads();
    fft_from<R, N, 1>(buf, tw);
    for (int t = threadIdx.x; t < N; t += CD_T) {
        const Cx<R> v = src.filter(row, buf[t], ldg(H + t));
        buf[t] = Cx<R>{v.re, -v.im};
    }
    __syncthreads();
    fft_from<R, N, 1>(buf, tw);
    if (circular) {
        const int off = whole ? 0 : q, keep = whole ? N : n;
        for (int t = threadIdx.x; t < keep; t += CD_T) {
            const int64_t p = blk * (whole ? N : n) + t;
            if (p < L) {
                const Cx<R> v = buf[off + t];
                stg(y + p, Cx<R>{v.re, -v.im});
            }
        }
    } else {
        const int64_t s = blk * n - q;
        // odd blocks: a sample was written by an even neighbour unless it lies right of the centre of the last block and that
        // block is odd
        const bool right_even = blk + 1 < nb;
        for (int t = threadIdx.x; t < N; t += CD_T) {
            const int64_t p = s + t;
            if (p < 0 || p >= Lout) continue;
            const Cx<R> b = buf[t];
            Cx<R> v{b.re, -b.im};
            if (parity && (t < n || right_even)) {
                const Cx<R> a = ldg(y + p);
                v = Cx<R>{a.re + v.re, a.im + v.im};
            }
            stg(y + p, v);
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
// Twiddles of the N-point transform, then H[k] = exp(j phase(k)) / N on numpy's fftfreq grid (k = -N/2 .. N/2 - 1 in fftfreq order), formed in
// double - the phase reduced modulo 2 pi before its sine and cosine - and cast to the signal's precision.  `key` names what `phase` depends on;
// N and the precision are added here.
template <typename R, typename P> int filter_table(TableCache &cache, Slot slot, int N, std::string key, P phase, const Cx<R> **tab)
{
    key_add(key, N);
    key_add(key, (int)sizeof(R));
    auto fill = [&](char *host) {
        Cx<R> *h = reinterpret_cast<Cx<R> *>(host);
        for (int m = 0; m < N; m++) {
            const double a = -QH_TWO_PI * (double)m / (double)N;
            h[m] = Cx<R>{(R)cos(a), (R)sin(a)};
            const double ph = remainder(phase(m < N / 2 ? m : m - N), QH_TWO_PI);
            h[N + m] = Cx<R>{(R)(cos(ph) / N), (R)(sin(ph) / N)};
        }
    };
    return cache.get(slot, key, 2 * (size_t)N * sizeof(Cx<R>), fill, (const void **)tab);
}

template <typename R, int N, typename Src>
int block_filter_launch(const Cx<R> *E, Cx<R> *out, int nmodes, int64_t L, int64_t Lout, const Cx<R> *tab, Src src, int mode)
{
    const size_t lds = (size_t)N * sizeof(Cx<R>);
    int rc = dyn_lds(block_filter_kernel<R, N, Src>, lds);
    if (rc) return rc;
    constexpr int64_t n = N / 2;
    if (mode == 0) {
        const int whole = L == N;
        const int64_t nblk = whole ? 1 : (L + n - 1) / n;
        hipLaunchKernelGGL((block_filter_kernel<R, N, Src>), dim3((unsigned)nblk, nmodes), dim3(CD_T), lds, g_stream, E, out, L, L, tab, src, 0, whole, nblk, 0);
        QH_HIP(hipGetLastError());
    } else {
        const int64_t nb = L / n;
        for (int parity = 0; parity < 2; parity++) {
            const int64_t cnt = (nb - parity + 1) / 2;
            if (cnt <= 0) continue;
            hipLaunchKernelGGL((block_filter_kernel<R, N, Src>), dim3((unsigned)cnt, nmodes), dim3(CD_T), lds, g_stream, E, out, L, Lout, tab, src, 1, 0, nb, parity);
            QH_HIP(hipGetLastError());
        }
    }
    return QH_OK;
}

// N: a power of two from 256 to 8192 (the caller checks)
template <typename R, typename Src>
int block_filter(int N, const Cx<R> *E, Cx<R> *out, int nmodes, int64_t L, int64_t Lout, const Cx<R> *tab, Src src, int mode)
{
    switch (N) {
    case 256: return block_filter_launch<R, 256>(E, out, nmodes, L, Lout, tab, src, mode);
    case 512: return block_filter_launch<R, 512>(E, out, nmodes, L, Lout, tab, src, mode);
    case 1024: return block_filter_launch<R, 1024>(E, out, nmodes, L, Lout, tab, src, mode);
    case 2048: return block_filter_launch<R, 2048>(E, out, nmodes, L, Lout, tab, src, mode);
    case 4096: return block_filter_launch<R, 4096>(E, out, nmodes, L, Lout, tab, src, mode);
    default: return block_filter_launch<R, 8192>(E, out, nmodes, L, Lout, tab, src, mode);
    }
}

}  // namespace qh
