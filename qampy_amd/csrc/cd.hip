// Static all-pass filtering of every row of an (nmodes, L) array: chromatic-dispersion compensation and emulation
// (qampy/core/equalisation/equalisation.py:596-669 CDcomp, qampy/core/impairments.py:673-703 add_dispersion).
//
//   H(w) = exp(j (c2 w^2 + c1 w + c0)) / N,   w = 2 pi k / N on numpy's fftfreq grid of the block size N (rad / sample, [-pi, pi))
//
// One workgroup transforms one block of one row: load (with its halo) -> forward FFT -> * H -> inverse FFT -> store.  The FFT is a
// Stockham autosort in LDS: every pass reads its butterflies' inputs from LDS into registers, runs radix-8/4 butterflies there
// and writes the results back in place (a barrier between the reads and the writes, so one N-point buffer suffices).  The
// inverse transform is conj(FFT(conj(.))), with the conjugations folded into the multiply by H and the store.
//
// Sizes: N = 256 .. 8192, a power of two, for both precisions.  One buffer of N complex values: 64 KiB (complex64) or 128 KiB
// (complex128) at N = 8192; complex128 at 16384 would need 256 KiB against 160 KiB of LDS per CU.
//
// Twiddles W_N^m and H (1/N of the inverse folded in) come from tables formed on the host in double precision - the phase of
// H reduced modulo 2 pi in double before its sine and cosine - cast to the signal's precision and uploaded once per
// (N, c2, c1, c0, dtype) into scratch slot 15.
//
// Boundary modes:
//   circular (0)  overlap-save.  Block j keeps output samples [j n, (j + 1) n), n = N / 2, of a transform over input positions
//                 j n - N/4 .. j n + n + N/4 - 1, taken modulo L (any L >= 1; the last block may be partial).  N == L: one
//                 transform per row, no overlap.
//   linear (1)    the reference's zero-padded overlap-add: block j holds input [j n, (j + 1) n) at offset N/4 of N zeros, its N
//                 outputs land at j n - N/4 ..; output length n (L // n).  Every output sample is the sum of two blocks' outputs.
//                 Even blocks are written first (their outputs tile the row without overlap), then the odd blocks add theirs
//                 in a second launch on the same stream: no atomics and no scratch; the sum of two terms is exact in either
//                 order, so the result is that of the reference's accumulation.
#include "common.h"
#include "fft_lds.h"
#include <cmath>
#include <vector>

namespace qh {

constexpr int CD_NMIN = 256, CD_NMAX = 8192;

// grid (blocks, nmodes).  mode 0: circular; `whole` (N == L): one transform per row.  mode 1: linear, blocks of parity `parity`
// (blockIdx.x -> block 2 blockIdx.x + parity); `nb` = L // n.
template <typename R, int N>
__global__ void __launch_bounds__(CD_T) cd_filter_kernel(const Cx<R> *__restrict__ E, Cx<R> *__restrict__ out, int64_t L, int64_t Lout,
                                                         const Cx<R> *__restrict__ tab, int mode, int whole, int64_t nb, int parity)
{
    extern __shared__ __attribute__((aligned(16))) char smem_cd[];
    Cx<R> *buf = reinterpret_cast<Cx<R> *>(smem_cd);
    const Cx<R> *tw = tab, *H = tab + N;
    constexpr int n = N / 2, q = N / 4;
    const int row = blockIdx.y;
    const Cx<R> *x = E + (size_t)row * L;
    Cx<R> *y = out + (size_t)row * Lout;
    const Cx<R> zero{(R)0, (R)0};
    int64_t blk;
    if (mode == 0) {
        blk = blockIdx.x;
        if (whole) {
            for (int t = threadIdx.x; t < N; t += CD_T) buf[t] = ldg(x + t);
        } else {
            int64_t base = (blk * n - q) % L;
            if (base < 0) base += L;
            for (int t = threadIdx.x; t < N; t += CD_T) {
                int64_t p = base + t;
                if (p >= L) p = L >= N ? p - L : p % L;
                buf[t] = ldg(x + p);
            }
        }
    } else {
        blk = 2 * (int64_t)blockIdx.x + parity;
        const int64_t s = blk * n - q;
        for (int t = threadIdx.x; t < N; t += CD_T) buf[t] = (t >= q && t < q + n) ? ldg(x + s + t) : zero;
    }
    __syncthreads();
    fft_from<R, N, 1>(buf, tw);
    for (int t = threadIdx.x; t < N; t += CD_T) {
        const Cx<R> v = cmul(buf[t], ldg(H + t));
        buf[t] = Cx<R>{v.re, -v.im};
    }
    __syncthreads();
    fft_from<R, N, 1>(buf, tw);
    if (mode == 0) {
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
struct CdTable {
    int N = 0, rsize = 0;
    double c2 = 0, c1 = 0, c0 = 0;
    void *dev = nullptr;
    unsigned epoch = 0;
    std::vector<char> host;                // kept alive for the asynchronous upload
};
static thread_local CdTable g_cd;

template <typename R> static int cd_table(int N, double c2, double c1, double c0, const Cx<R> **tab)
{
    const size_t bytes = 2 * (size_t)N * sizeof(Cx<R>);
    void *p = nullptr;
    int rc;
    if (g_cd.dev && g_cd.N == N && g_cd.rsize == (int)sizeof(R) && g_cd.c2 == c2 && g_cd.c1 == c1 && g_cd.c0 == c0 && g_cd.epoch == scratch_epoch()) {
        if ((rc = scratch(15, bytes, &p))) return rc;
        if (p == g_cd.dev) { *tab = (const Cx<R> *)p; return QH_OK; }
    }
    // a new table: whatever still reads the old one (a launch on another of this thread's streams) finishes first
    if (g_cd.dev) QH_HIP(hipDeviceSynchronize());
    if ((rc = scratch(15, bytes, &p))) return rc;
    g_cd.host.resize(bytes);
    Cx<R> *h = reinterpret_cast<Cx<R> *>(g_cd.host.data());
    for (int m = 0; m < N; m++) {
        const double a = -QH_TWO_PI * (double)m / (double)N;
        h[m] = Cx<R>{(R)cos(a), (R)sin(a)};
        const int k = m < N / 2 ? m : m - N;                              // fftfreq order
        const double w = QH_TWO_PI * (double)k / (double)N;
        const double ph = remainder(c2 * w * w + c1 * w + c0, QH_TWO_PI);
        h[N + m] = Cx<R>{(R)(cos(ph) / N), (R)(sin(ph) / N)};
    }
    QH_HIP(hipMemcpyAsync(p, h, bytes, hipMemcpyHostToDevice, g_stream));
    g_cd.N = N; g_cd.rsize = (int)sizeof(R); g_cd.c2 = c2; g_cd.c1 = c1; g_cd.c0 = c0; g_cd.dev = p; g_cd.epoch = scratch_epoch();
    *tab = (const Cx<R> *)p;
    return QH_OK;
}

template <typename R, int N>
static int cd_launch(const Cx<R> *E, Cx<R> *out, int nmodes, int64_t L, int64_t Lout, const Cx<R> *tab, int mode)
{
    const size_t lds = (size_t)N * sizeof(Cx<R>);
    int rc = dyn_lds(cd_filter_kernel<R, N>, lds);
    if (rc) return rc;
    constexpr int64_t n = N / 2;
    if (mode == 0) {
        const int whole = L == N;
        const int64_t nblk = whole ? 1 : (L + n - 1) / n;
        hipLaunchKernelGGL((cd_filter_kernel<R, N>), dim3((unsigned)nblk, nmodes), dim3(CD_T), lds, g_stream, E, out, L, L, tab, 0, whole, nblk, 0);
        QH_HIP(hipGetLastError());
    } else {
        const int64_t nb = L / n;
        for (int parity = 0; parity < 2; parity++) {
            const int64_t cnt = (nb - parity + 1) / 2;
            if (cnt <= 0) continue;
            hipLaunchKernelGGL((cd_filter_kernel<R, N>), dim3((unsigned)cnt, nmodes), dim3(CD_T), lds, g_stream, E, out, L, Lout, tab, 1, 0, nb, parity);
            QH_HIP(hipGetLastError());
        }
    }
    return QH_OK;
}

static bool cd_size_ok(int N) { return N >= CD_NMIN && N <= CD_NMAX && (N & (N - 1)) == 0; }

template <typename R>
int cd_filter_dev(const void *E, int nmodes, int64_t L, int N, double c2, double c1, double c0, int mode, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(cd_size_ok(N), "cd_filter: N must be a power of two from 256 to 8192");
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 0, "cd_filter: bad sizes");
    QH_REQUIRE(mode == 0 || mode == 1, "cd_filter: mode is 0 (circular) or 1 (linear)");
    QH_REQUIRE(std::isfinite(c2) && std::isfinite(c1) && std::isfinite(c0), "cd_filter: coefficients must be finite");
    QH_REQUIRE(E && out && E != out, "cd_filter: out must be a buffer other than E");
    const int64_t Lout = mode == 0 ? L : (L / (N / 2)) * (N / 2);
    if (Lout == 0) return QH_OK;
    QH_REQUIRE(mode == 1 || (L + N / 2 - 1) / (N / 2) <= 0x7fffffffLL, "cd_filter: L too long");
    const Cx<R> *tab;
    if ((rc = cd_table<R>(N, c2, c1, c0, &tab))) return rc;
    const Cx<R> *e = (const Cx<R> *)E;
    Cx<R> *o = (Cx<R> *)out;
    switch (N) {
    case 256: return cd_launch<R, 256>(e, o, nmodes, L, Lout, tab, mode);
    case 512: return cd_launch<R, 512>(e, o, nmodes, L, Lout, tab, mode);
    case 1024: return cd_launch<R, 1024>(e, o, nmodes, L, Lout, tab, mode);
    case 2048: return cd_launch<R, 2048>(e, o, nmodes, L, Lout, tab, mode);
    case 4096: return cd_launch<R, 4096>(e, o, nmodes, L, Lout, tab, mode);
    default: return cd_launch<R, 8192>(e, o, nmodes, L, Lout, tab, mode);
    }
}

template <typename R>
int cd_filter_host(const void *E, int nmodes, int64_t L, int N, double c2, double c1, double c0, int mode, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(cd_size_ok(N), "cd_filter: N must be a power of two from 256 to 8192");
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 0, "cd_filter: bad sizes");
    QH_REQUIRE(mode == 0 || mode == 1, "cd_filter: mode is 0 (circular) or 1 (linear)");
    const int64_t Lout = mode == 0 ? L : (L / (N / 2)) * (N / 2);
    if (Lout == 0) return QH_OK;
    DevBuf dE, dout;
    if ((rc = dE.from_host(E, (size_t)nmodes * L * sizeof(Cx<R>)))) return rc;
    if ((rc = dout.alloc((size_t)nmodes * Lout * sizeof(Cx<R>)))) return rc;
    if ((rc = cd_filter_dev<R>(dE.p, nmodes, L, N, c2, c1, c0, mode, dout.p))) return rc;
    if ((rc = dout.to_host(out, dout.n))) return rc;
    QH_HIP(hipStreamSynchronize(g_stream));
    return QH_OK;
}

}  // namespace qh

extern "C" {
int qh_cd_filter_c64(const void *E, int nmodes, int64_t L, int N, double c2, double c1, double c0, int mode, void *out)
{ return qh::cd_filter_host<float>(E, nmodes, L, N, c2, c1, c0, mode, out); }
int qh_cd_filter_c128(const void *E, int nmodes, int64_t L, int N, double c2, double c1, double c0, int mode, void *out)
{ return qh::cd_filter_host<double>(E, nmodes, L, N, c2, c1, c0, mode, out); }
int qh_cd_filter_c64_dev(const void *E, int nmodes, int64_t L, int N, double c2, double c1, double c0, int mode, void *out)
{ return qh::cd_filter_dev<float>(E, nmodes, L, N, c2, c1, c0, mode, out); }
int qh_cd_filter_c128_dev(const void *E, int nmodes, int64_t L, int N, double c2, double c1, double c0, int mode, void *out)
{ return qh::cd_filter_dev<double>(E, nmodes, L, N, c2, c1, c0, mode, out); }
}
