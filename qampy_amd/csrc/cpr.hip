// Feed-forward carrier recovery on gfx950: Viterbi-Viterbi for M-PSK and 16-QAM by QPSK partitioning, without leaving device memory.
//
// Reference behaviour:
//   qampy/core/phaserecovery.py:40-79    viterbiviterbi(E, N, M): z = exp(j angle(E))^M, sums over every window of N samples, np.unwrap of
//                                        their angles, trace = (unwrapped - pi) / M, E * exp(-j trace) on the centre of every window
//   qampy/core/phaserecovery.py:292-382  partition_16qam / phase_partition_16qam: ring thresholds from cal_s0(E, 1.32), one fourth-power
//                                        estimate per block of Nblock samples, np.unwrap over the row, trace = unwrapped / 4 - pi / 4
//
// Both are a raw angle per output (V&V) or per block (partition), np.unwrap and a de-rotation.  np.unwrap is an exact integer prefix sum K of
// wrap counts c_k = -1 where theta_k - theta_(k-1) > pi, +1 where it is < -pi, else 0 (+-pi itself: 0, as numpy), taken in the three-phase form
// of unwrap_scan.h.  The angles are kept in double in scratch; the trace is formed in double and rounded once to the signal's real type.
//
// Viterbi-Viterbi, three launches, E read twice and written once:
//   vv_theta_kernel   one workgroup per chunk of UW_CHUNK outputs: z of the chunk, of the output in front of it and of their N - 1 halo
//                     (in the signal's precision; a zero sample gives z = 1), an inclusive prefix of z over the tile in DOUBLE in LDS, window
//                     sums as prefix differences (a tile holds at most 2048 unit vectors: 2048 eps = 5e-13 at N = 1), theta = atan2, the wrap
//                     counts of the chunk - the count of the chunk's first output from the tile's own angle of the output in front, which is
//                     stored per chunk so that the apply kernel repeats exactly this decision - and their sum
//   unwrap_scan_kernel
//   vv_apply_kernel   prefix of the wrap counts inside the chunk, trace = (theta + 2 pi K - pi) / M, de-rotation of the window centres
//                     (by the trace with K reduced modulo M, which is the same rotation at a small argument), zero edges.
// Bound: HBM - 16 B of field in, 8 out, 16 of theta and 4 (8) of trace per complex64 (complex128: 32, 16, 16, 8) sample, and the halo
// (N - 1) / UW_CHUNK of a second read that mostly hits the cache.
//
// QPSK partition, six launches: p16_moments_kernel (row sums of |E|^2 and |E|^4 in double, P16_PARTS partial sums per row),
// p16_theta_kernel (every workgroup sums the partials in the same order -> the same S0 and ring thresholds everywhere; one wave per block:
// classes decided in double, fourth powers in the signal's precision, block sums in double, theta_b), p16_jump_kernel (chunk sums of the wrap
// counts over the blocks), unwrap_scan_kernel, p16_unwrap_kernel (K_b) and p16_apply_kernel (trace and de-rotation of every sample).  The four
// kernels in the middle touch one value per BLOCK; the field is read three times (the two passes of p16_theta_kernel over a block: the
// second from the cache) and written once.
// The complex minimum is a discontinuity of the estimator itself: Re A - Re B = 2 Im(E^4) sin(4 phi) vanishes for a class-2 sample on an axis
// or a diagonal, and which of the two is taken there - a step of 2 |E|^4 in the block sum - hangs on the last bit of a rounding, in numpy as
// here.
#include "common.h"
#include "unwrap_scan.h"

namespace qh {

constexpr int VV_NMAX = 1024, VV_MMAX = 64;
constexpr int VV_TILE = 2 * UW_CHUNK;                 // z values of a tile, at most: UW_CHUNK + 1 outputs and N - 1 <= UW_CHUNK - 1 of halo
constexpr int VV_ROWS = VV_TILE / UW_THREADS;
constexpr int P16_NBLOCK_MAX = 4096;
constexpr int P16_PARTS = 256;                        // partial moment sums per row, at most
constexpr int P16_SPAN_MIN = 4096;                    // samples per partial sum, at least
constexpr int P16_WAVES = UW_THREADS / 64;
static_assert(VV_NMAX <= UW_CHUNK, "the halo of a V&V tile must fit the second half of the tile");
static_assert(P16_PARTS <= UW_THREADS, "one partial sum per thread");

// (x / |x|)^M in the precision of x; zero -> 1 (np.angle(0) = 0)
template <typename R> __device__ __forceinline__ Cx<R> unit_pow(Cx<R> x, int M)
{
    const R m = abs_(x.re) > abs_(x.im) ? abs_(x.re) : abs_(x.im);
    if (m == (R)0) return Cx<R>{(R)1, (R)0};
    const R a = x.re / m, b = x.im / m;                     // (scaled first: no under- or overflow of the square)
    const R inv = (R)1 / sqrt(fma_(a, a, b * b));
    Cx<R> u{a * inv, b * inv}, r{(R)1, (R)0};
    for (; M; M >>= 1) {
        if (M & 1) r = cmul(r, u);
        u = cmul(u, u);
    }
    return r;
}

// De-rotation by a trace: x * exp(-j p)
template <typename R> __device__ __forceinline__ Cx<R> derotate(Cx<R> x, R p)
{
    R sn, cs;
    sincos_<R>(p, &sn, &cs);
    return Cx<R>{fma_(x.re, cs, x.im * sn), fma_(x.im, cs, -(x.re * sn))};
}

// ------------------------------------------------------------------------------------------------ Viterbi-Viterbi
template <typename R>
__global__ void __launch_bounds__(UW_THREADS) vv_theta_kernel(const Cx<R> *__restrict__ E, int64_t L, int N, int M, int64_t nout, int64_t nchunk,
                                                              double *__restrict__ theta, int *__restrict__ chunk_sum, int *__restrict__ first_jump)
{
    extern __shared__ __attribute__((aligned(16))) char vv_smem[];
    double2 *Q = reinterpret_cast<double2 *>(vv_smem);  // [nrows * UW_THREADS + 1]: Q[i] = z[0] + .. + z[i - 1] of the tile
    __shared__ double2 wtot[VV_ROWS][UW_THREADS / 64];
    __shared__ double th[UW_CHUNK + 1];                // th[li]: angle of output base - 1 + li
    __shared__ int red[UW_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t mode = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * UW_CHUNK;
    const int64_t j0 = base - 1;                       // tile entry i is sample j0 + i: the output in front of the chunk comes first
    const Cx<R> *e = E + mode * L;
    const int nz = UW_CHUNK + N;                       // entries in use: UW_CHUNK + 1 outputs and their halo
    const int nrows = (nz + UW_THREADS - 1) / UW_THREADS;
    double2 incl[VV_ROWS];
#pragma unroll
    for (int r = 0; r < VV_ROWS; r++) {
        if (r < nrows) {                               // (workgroup-uniform)
            const int i = r * UW_THREADS + tid;
            const int64_t j = j0 + i;
            double2 z{0., 0.};
            if (i < nz && j >= 0 && j < L) {
                const Cx<R> p = unit_pow<R>(ldg(e + j), M);
                z.x = (double)p.re; z.y = (double)p.im;
            }
            for (int o = 1; o < 64; o <<= 1) {
                const double tx = __shfl_up(z.x, o), ty = __shfl_up(z.y, o);
                if (lane >= o) { z.x += tx; z.y += ty; }
            }
            incl[r] = z;
            if (lane == 63) wtot[r][wave] = z;
        }
    }
    __syncthreads();
    double2 carry{0., 0.};
#pragma unroll
    for (int r = 0; r < VV_ROWS; r++) {
        if (r < nrows) {
            double2 off = carry;
            for (int w = 0; w < UW_THREADS / 64; w++) {
                const double2 t = wtot[r][w];
                if (w < wave) { off.x += t.x; off.y += t.y; }
                carry.x += t.x; carry.y += t.y;
            }
            Q[r * UW_THREADS + tid + 1] = double2{off.x + incl[r].x, off.y + incl[r].y};
        }
    }
    if (tid == 0) Q[0] = double2{0., 0.};
    __syncthreads();
    for (int li = tid; li <= UW_CHUNK; li += UW_THREADS) {
        const int64_t k = j0 + li;
        double t = 0.;
        if (k >= 0 && k < nout) {
            const double2 a = Q[li], b = Q[li + N];    // li + N <= UW_CHUNK + N = nz <= nrows * UW_THREADS
            t = atan2(b.y - a.y, b.x - a.x);
            if (li >= 1) theta[mode * nout + k] = t;
        }
        th[li] = t;
    }
    __syncthreads();
    const int s = block_sum_int(strided_wrap_counts(th, base, nout, first_jump + mode * nchunk + blockIdx.x), red);
    if (tid == 0) chunk_sum[mode * nchunk + blockIdx.x] = s;
}

template <typename R>
__global__ void __launch_bounds__(UW_THREADS) vv_apply_kernel(const Cx<R> *__restrict__ E, int64_t L, int N, int M, int64_t nout, int64_t nchunk,
                                                              const double *__restrict__ theta, const int *__restrict__ chunk_off,
                                                              const int *__restrict__ first_jump, R *__restrict__ trace, Cx<R> *__restrict__ Eout)
{
    __shared__ double th[UW_CHUNK];
    __shared__ int corr[UW_CHUNK];
    __shared__ int wsum[UW_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t mode = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * UW_CHUNK;
    const int64_t o = (N - 1) / 2;                     // output k is the centre of window k: sample o + k
#pragma unroll
    for (int r = 0; r < UW_PER_THREAD; r++) {
        const int el = r * UW_THREADS + tid;
        const int64_t k = base + el;
        th[el] = k < nout ? theta[mode * nout + k] : 0.;
    }
    __syncthreads();
    int jmp[UW_PER_THREAD];
    owned_wrap_counts(th, base, nout, first_jump + mode * nchunk + blockIdx.x, jmp);
    chunk_prefix(jmp, chunk_off[mode * nchunk + blockIdx.x], corr, wsum);
    const Cx<R> *e = E + mode * L;
    Cx<R> *out = Eout + mode * L;
#pragma unroll
    for (int r = 0; r < UW_PER_THREAD; r++) {
        const int el = r * UW_THREADS + tid;
        const int64_t k = base + el;
        if (k < nout) {
            const int K = corr[el];
            trace[mode * nout + k] = (R)((th[el] + 2 * QH_PI * (double)K - QH_PI) / (double)M);
            // exp(-j trace) does not change when K changes by M: the argument stays within (-2 pi, 2 pi) and keeps its digits
            const int Km = ((K % M) + M) % M;
            const R p = (R)((th[el] + 2 * QH_PI * (double)Km - QH_PI) / (double)M);
            stg(out + o + k, derotate<R>(ldg(e + o + k), p));
        }
    }
    // the N - 1 samples that are no window's centre
    if (blockIdx.x == 0)
        for (int64_t i = tid; i < o; i += UW_THREADS) stg(out + i, Cx<R>{(R)0, (R)0});
    if (blockIdx.x == nchunk - 1)
        for (int64_t i = o + nout + tid; i < L; i += UW_THREADS) stg(out + i, Cx<R>{(R)0, (R)0});
}

template <typename R>
int vv_recover_dev(const void *E, int nmodes, int64_t L, int N, int M, void *trace, void *Eout)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 1, "vv_recover: bad sizes");
    QH_REQUIRE(M >= 2 && M <= VV_MMAX, "vv_recover: M must be between 2 and 64");
    QH_REQUIRE(N >= 1 && N <= VV_NMAX && N <= L, "vv_recover: N must be between 1 and min(L, 1024)");
    QH_REQUIRE(E && trace && Eout, "vv_recover: E, trace and Eout must be given");
    const int64_t nout = L - N + 1, nchunk = (nout + UW_CHUNK - 1) / UW_CHUNK;
    QH_REQUIRE(nchunk <= 0x7fffffff, "vv_recover: row too long");
    // scratch: theta | chunk sums | wrap count of every chunk's first output
    UnwrapScratch us;
    if ((rc = unwrap_scratch(Slot::CPR, nmodes, nchunk, (size_t)nmodes * nout * sizeof(double), &us))) return rc;
    double *theta = (double *)us.base;
    int *csum = us.csum, *first = us.first;
    const dim3 grid((unsigned)nchunk, nmodes);
    const size_t lds = ((size_t)(UW_CHUNK + N + UW_THREADS - 1) / UW_THREADS * UW_THREADS + 1) * sizeof(double2);      // <= 32 KiB + 16
    hipLaunchKernelGGL((vv_theta_kernel<R>), grid, dim3(UW_THREADS), lds, g_stream, (const Cx<R> *)E, L, N, M, nout, nchunk, theta, csum, first);
    hipLaunchKernelGGL(unwrap_scan_kernel, dim3(nmodes), dim3(1024), 0, g_stream, csum, nchunk);
    hipLaunchKernelGGL((vv_apply_kernel<R>), grid, dim3(UW_THREADS), 0, g_stream, (const Cx<R> *)E, L, N, M, nout, nchunk, (const double *)theta,
                       (const int *)csum, (const int *)first, (R *)trace, (Cx<R> *)Eout);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

// ------------------------------------------------------------------------------------------------ 16-QAM by QPSK partitioning
template <typename R>
__global__ void __launch_bounds__(UW_THREADS) p16_moments_kernel(const Cx<R> *__restrict__ E, int64_t L, int64_t span, int nparts, double *__restrict__ part)
{
    __shared__ double red[P16_WAVES][2];
    const Cx<R> *e = E + (int64_t)blockIdx.y * L;
    const int64_t n0 = (int64_t)blockIdx.x * span, n1 = n0 + span < L ? n0 + span : L;
    double s2 = 0., s4 = 0.;
    for (int64_t n = n0 + threadIdx.x; n < n1; n += 4 * UW_THREADS) {
        Cx<R> x[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int64_t i = n + (int64_t)q * UW_THREADS;
            x[q] = i < n1 ? ldg(e + i) : Cx<R>{(R)0, (R)0};
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const double p = (double)x[q].re * (double)x[q].re + (double)x[q].im * (double)x[q].im;
            s2 += p;
            s4 += p * p;
        }
    }
    block_sum2<UW_THREADS>(s2, s4, red);
    if (threadIdx.x == 0) {
        double *o = part + ((int64_t)blockIdx.y * nparts + blockIdx.x) * 2;
        o[0] = s2; o[1] = s4;
    }
}

template <typename R> struct P16Args {
    const Cx<R> *E;
    const double *part;      // (nmodes, nparts, 2)
    double *theta;           // (nmodes, nb)
    int64_t L, nb;
    int Nblock, nparts, G;   // G: consecutive blocks per wave
    R cphi, sphi;            // exp(j (pi / 4 + atan(1 / 3)))
};

template <typename R>
__global__ void __launch_bounds__(UW_THREADS) p16_theta_kernel(P16Args<R> a)
{
    __shared__ double red[P16_WAVES][2];
    __shared__ double ring[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t mode = blockIdx.y;
    {
        // S0 of cal_s0(E, 1.32) - gamma = 25 / 33 for that "order" - and the rings half way between the three radii of 16-QAM
        double s2 = 0., s4 = 0.;
        if (tid < a.nparts) {
            const double *p = a.part + (mode * a.nparts + tid) * 2;
            s2 = p[0]; s4 = p[1];
        }
        block_sum2<UW_THREADS>(s2, s4, red);
        if (tid == 0) {
            const double gamma = 25. / 33., r2 = s2 / (double)a.L, r4 = s4 / (double)a.L, q = r2 * r2 / r4;
            const double S1 = 1 - 2 * q - sqrt((2 - gamma) * (2 * q * q - q));
            const double S2 = gamma * q - 1;
            const double S0 = r2 / (1 + S2 / S1);
            ring[0] = (sqrt(S0 / 5) + sqrt(S0)) / 2;
            ring[1] = (sqrt(9 * S0 / 5) + sqrt(S0)) / 2;
        }
        __syncthreads();
    }
    const double inner = ring[0], outer = ring[1];
    const Cx<R> *e = a.E + mode * a.L;
    const Cx<R> rp{a.cphi, a.sphi}, rm{a.cphi, -a.sphi};
    for (int g = 0; g < a.G; g++) {
        const int64_t b = ((int64_t)blockIdx.x * P16_WAVES + wave) * a.G + g;
        if (b >= a.nb) break;                          // (wave-uniform)
        const int64_t n0 = b * a.Nblock, n1 = n0 + a.Nblock < a.L ? n0 + a.Nblock : a.L;
        auto class1 = [&](Cx<R> x) {
            const double mag = sqrt((double)x.re * (double)x.re + (double)x.im * (double)x.im);
            return mag < inner || mag > outer;
        };
        double s1r = 0., s1i = 0.;
        for (int64_t n = n0 + lane; n < n1; n += 64) {
            const Cx<R> x = ldg(e + n);
            if (class1(x)) {
                const Cx<R> p = pow4(x);
                s1r += (double)p.re; s1i += (double)p.im;
            }
        }
        wave_sum2(s1r, s1i);
        double mr = 0., mi = 0.;
        for (int64_t n = n0 + lane; n < n1; n += 64) {
            const Cx<R> x = ldg(e + n);
            if (!class1(x)) {
                const Cx<R> wp = pow4(cmul(x, rp)), wm = pow4(cmul(x, rm));
                const double Ar = s1r - (double)wp.re, Ai = s1i - (double)wp.im, Br = s1r - (double)wm.re, Bi = s1i - (double)wm.im;
                const bool takeB = Br < Ar || (Br == Ar && Bi < Ai);       // numpy's complex minimum: real part first, a tie keeps the first
                mr += takeB ? Br : Ar;
                mi += takeB ? Bi : Ai;
            }
        }
        wave_sum2(mr, mi);
        if (lane == 0) a.theta[mode * a.nb + b] = atan2(s1i + mi, s1r + mr);
    }
}

__global__ void __launch_bounds__(UW_THREADS) p16_jump_kernel(const double *__restrict__ theta, int64_t nb, int64_t nchunk, int *__restrict__ chunk_sum)
{
    __shared__ int red[UW_THREADS / 64];
    const int64_t mode = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * UW_CHUNK;
    const double *th = theta + mode * nb;
    int s = 0;
    for (int r = 0; r < UW_PER_THREAD; r++) {
        const int64_t k = base + threadIdx.x + (int64_t)r * UW_THREADS;
        if (k >= 1 && k < nb) s += wrap_count(th[k - 1], th[k]);
    }
    s = block_sum_int(s, red);
    if (threadIdx.x == 0) chunk_sum[mode * nchunk + blockIdx.x] = s;
}

__global__ void __launch_bounds__(UW_THREADS) p16_unwrap_kernel(const double *__restrict__ theta, int64_t nb, int64_t nchunk, const int *__restrict__ chunk_off,
                                                                int *__restrict__ Kb)
{
    __shared__ int corr[UW_CHUNK];
    __shared__ int wsum[UW_THREADS / 64];
    const int64_t mode = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * UW_CHUNK;
    const double *th = theta + mode * nb;
    int jmp[UW_PER_THREAD];
    int local = 0;
#pragma unroll
    for (int r = 0; r < UW_PER_THREAD; r++) {
        const int64_t k = base + threadIdx.x * UW_PER_THREAD + r;
        if (k >= 1 && k < nb) local += wrap_count(th[k - 1], th[k]);
        jmp[r] = local;
    }
    chunk_prefix(jmp, chunk_off[mode * nchunk + blockIdx.x], corr, wsum);
#pragma unroll
    for (int r = 0; r < UW_PER_THREAD; r++) {
        const int el = r * UW_THREADS + threadIdx.x;
        const int64_t k = base + el;
        if (k < nb) Kb[mode * nb + k] = corr[el];
    }
}

template <typename R>
__global__ void __launch_bounds__(UW_THREADS) p16_apply_kernel(const Cx<R> *__restrict__ E, int64_t L, int Nblock, int64_t nb, const double *__restrict__ theta,
                                                               const int *__restrict__ Kb, R *__restrict__ trace, Cx<R> *__restrict__ Eout)
{
    const int64_t mode = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * UW_CHUNK;
#pragma unroll
    for (int r = 0; r < UW_PER_THREAD; r++) {
        const int64_t n = base + r * UW_THREADS + threadIdx.x;
        if (n < L) {
            const int64_t b = n / Nblock;
            const double t = theta[mode * nb + b];
            const int K = Kb[mode * nb + b];
            trace[mode * L + n] = (R)(t / 4 + (QH_PI / 2) * (double)K - QH_PI / 4);
            const R p = (R)(t / 4 + (QH_PI / 2) * (double)(K & 3) - QH_PI / 4);      // the same rotation: K changes by a multiple of 4
            stg(Eout + mode * L + n, derotate<R>(ldg(E + mode * L + n), p));
        }
    }
}

template <typename R>
int partition16_recover_dev(const void *E, int nmodes, int64_t L, int Nblock, void *trace, void *Eout)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 1, "partition16_recover: bad sizes");
    QH_REQUIRE(Nblock >= 1 && Nblock <= P16_NBLOCK_MAX, "partition16_recover: Nblock must be between 1 and 4096");
    QH_REQUIRE(E && trace && Eout, "partition16_recover: E, trace and Eout must be given");
    const int64_t nb = (L + Nblock - 1) / Nblock, nchunk = (nb + UW_CHUNK - 1) / UW_CHUNK, nsamp = (L + UW_CHUNK - 1) / UW_CHUNK;
    int64_t np = (L + P16_SPAN_MIN - 1) / P16_SPAN_MIN;
    if (np > P16_PARTS) np = P16_PARTS;
    const int nparts = (int)np;
    int64_t span = (L + nparts - 1) / nparts;
    const int G = Nblock >= UW_CHUNK ? 1 : UW_CHUNK / Nblock;
    const int64_t ngroups = (nb + (int64_t)P16_WAVES * G - 1) / ((int64_t)P16_WAVES * G);
    QH_REQUIRE(ngroups <= 0x7fffffff && nsamp <= 0x7fffffff, "partition16_recover: row too long");
    // scratch: partial moments | theta_b | K_b | chunk sums
    ScratchLayout lay;
    const size_t o_part = lay.take((size_t)nmodes * nparts * 2 * sizeof(double)), o_theta = lay.take((size_t)nmodes * nb * sizeof(double)),
                 o_K = lay.take((size_t)nmodes * nb * sizeof(int)), o_sum = lay.take((size_t)nmodes * nchunk * sizeof(int));
    void *sb = nullptr;
    if ((rc = scratch(Slot::CPR, lay.total, &sb))) return rc;
    double *part = (double *)((char *)sb + o_part), *theta = (double *)((char *)sb + o_theta);
    int *Kb = (int *)((char *)sb + o_K), *csum = (int *)((char *)sb + o_sum);
    const double phi = QH_PI / 4 + atan(1. / 3.);
    P16Args<R> a;
    a.E = (const Cx<R> *)E; a.part = part; a.theta = theta; a.L = L; a.nb = nb; a.Nblock = Nblock; a.nparts = nparts; a.G = G;
    a.cphi = (R)cos(phi); a.sphi = (R)sin(phi);
    hipLaunchKernelGGL((p16_moments_kernel<R>), dim3(nparts, nmodes), dim3(UW_THREADS), 0, g_stream, (const Cx<R> *)E, L, span, nparts, part);
    hipLaunchKernelGGL((p16_theta_kernel<R>), dim3((unsigned)ngroups, nmodes), dim3(UW_THREADS), 0, g_stream, a);
    hipLaunchKernelGGL(p16_jump_kernel, dim3((unsigned)nchunk, nmodes), dim3(UW_THREADS), 0, g_stream, (const double *)theta, nb, nchunk, csum);
    hipLaunchKernelGGL(unwrap_scan_kernel, dim3(nmodes), dim3(1024), 0, g_stream, csum, nchunk);
    hipLaunchKernelGGL(p16_unwrap_kernel, dim3((unsigned)nchunk, nmodes), dim3(UW_THREADS), 0, g_stream, (const double *)theta, nb, nchunk, (const int *)csum, Kb);
    hipLaunchKernelGGL((p16_apply_kernel<R>), dim3((unsigned)nsamp, nmodes), dim3(UW_THREADS), 0, g_stream, (const Cx<R> *)E, L, Nblock, nb, (const double *)theta,
                       (const int *)Kb, (R *)trace, (Cx<R> *)Eout);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

}  // namespace qh

extern "C" {
int qh_vv_recover_c64_dev(const void *E, int nmodes, int64_t L, int N, int M, void *trace, void *Eout)
{ return qh::vv_recover_dev<float>(E, nmodes, L, N, M, trace, Eout); }
int qh_vv_recover_c128_dev(const void *E, int nmodes, int64_t L, int N, int M, void *trace, void *Eout)
{ return qh::vv_recover_dev<double>(E, nmodes, L, N, M, trace, Eout); }
int qh_partition16_recover_c64_dev(const void *E, int nmodes, int64_t L, int Nblock, void *trace, void *Eout)
{ return qh::partition16_recover_dev<float>(E, nmodes, L, Nblock, trace, Eout); }
int qh_partition16_recover_c128_dev(const void *E, int nmodes, int64_t L, int Nblock, void *trace, void *Eout)
{ return qh::partition16_recover_dev<double>(E, nmodes, L, Nblock, trace, Eout); }
}
