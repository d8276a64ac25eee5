// Blind frequency-offset estimate of every row of an (nmodes, L) array from the spectral peak of its fourth power
// (qampy/core/phaserecovery.py:385-433 find_freq_offset), without leaving device memory:
//
//   X_b = FFT_N(x[b N : (b + 1) N] ** 4),  b = 0 .. B - 1      block 0 zero-padded when L < N; B > 1 needs B N <= L
//   P[k] = sum_b |X_b[k]|^2                                     accumulated per bin in block order, in the signal's real type
//   bin  = first maximum of P (np.argmax);  stats = (bin, P[bin], sum_k P[k]) in double
//   fo   = fftfreq(N, 1 / os)[bin] / 4 in double; on request every row is replaced by the mean over the rows (summed in row order)
//
// B = 1 is the reference's estimator, B > 1 a Welch average over the capture.  N = 2^8 .. 2^20.
//
// N <= 8192: one workgroup transforms one block of one row with the Stockham LDS transform of fft_lds.h.
// N >  8192: four-step, N = N1 N2 with N1 = 2^floor(log2(N) / 2) (128 .. 1024) and N2 = N / N1 (128 .. 1024):
//   step 1  a workgroup loads FOE_C neighbouring columns n2 of the (N1, N2) view of a block (x[n1 N2 + n2] ** 4), transforms each over n1,
//           multiplies by the inter-step twiddle W_N^(k1 n2) - its turn k1 n2 / N is exact in double and below one; sine and cosine in
//           double - and stores T[k1][n2]
//   step 2  a workgroup transforms one row T[k1][:] over n2 and stores |.|^2 at [k1][k2]: bin k = k1 + N1 k2.
// The power spectrum is kept in that (k1, k2) order (the natural order when N1 = 1); the peak search compares natural bin numbers and the
// optional spectrum output is transposed on its way out.
//
// A call proceeds in chunks of c blocks, c = max(1, min(B, FOE_CHUNK / (nmodes N))): the per-block powers (nmodes c N reals) and the
// four-step intermediate T (nmodes c N complex values) never exceed the blocks they come from (c N <= L whenever B N <= L; one zero-padded
// block otherwise).  Tables, accumulator, partial results and intermediates live in scratch slot Slot::FOE.  The tables W_N1^m and
// W_N2^m are formed on the device in double at every call (at most 8192 + 1024 entries): nothing is cached across calls and nothing is
// copied from the host.  No atomics: a repeated call is bit-identical.  Every launch is bounded by the call's arguments alone.
#include "common.h"
#include "fft_lds.h"

namespace qh {

constexpr int FOE_LG_MIN = 8, FOE_LG_MAX = 20, FOE_LG_SINGLE = 13;     // N = 2^8 .. 2^20; one LDS transform up to 2^13
constexpr int FOE_C = 8;                                               // columns per workgroup in step 1
constexpr int64_t FOE_CHUNK = (int64_t)1 << 22;                        // elements of intermediate per chunk of blocks
constexpr int FOE_PARTS = 256;                                         // partial results per row in the peak search, at most

// grid (transforms per row, nmodes).  FOURTH: transform blockIdx.x is block b0 + blockIdx.x of row blockIdx.y of E, raised to the fourth power,
// zero beyond the row's end.  Otherwise it is the blockIdx.x-th run of N values of the row's intermediate.  Pb: |X|^2, same layout as the grid.
template <typename R, int N, bool FOURTH>
__global__ void __launch_bounds__(CD_T) foe_fft_kernel(const Cx<R> *__restrict__ in, int64_t L, int64_t b0, const Cx<R> *__restrict__ tw, R *__restrict__ Pb)
{
    extern __shared__ __attribute__((aligned(16))) char smem_foe[];
    Cx<R> *buf = reinterpret_cast<Cx<R> *>(smem_foe);
    const size_t slot = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if constexpr (FOURTH) {
        const int64_t s = (b0 + blockIdx.x) * (int64_t)N;
        const int64_t valid = L - s;                                   // samples of the row from s on (may exceed N: only N are read)
        const Cx<R> *x = in + (size_t)blockIdx.y * L + s;
        for (int t = threadIdx.x; t < N; t += CD_T) buf[t] = t < valid ? pow4(ldg(x + t)) : Cx<R>{(R)0, (R)0};
    } else {
        const Cx<R> *x = in + slot * N;
        for (int t = threadIdx.x; t < N; t += CD_T) buf[t] = ldg(x + t);
    }
    __syncthreads();
    fft_from<R, N, 1>(buf, tw);
    R *p = Pb + slot * N;
    for (int t = threadIdx.x; t < N; t += CD_T) {
        const Cx<R> v = buf[t];
        p[t] = v.re * v.re + v.im * v.im;
    }
}

// Step 1 of the four-step transform.  grid (N2 / FOE_C, blocks of the chunk, nmodes); T (nmodes, blocks, N1, N2).
template <typename R, int N1>
__global__ void __launch_bounds__(CD_T) foe_step1_kernel(const Cx<R> *__restrict__ E, int64_t L, int64_t b0, int N2, const Cx<R> *__restrict__ tw1, Cx<R> *__restrict__ T)
{
    extern __shared__ __attribute__((aligned(16))) char smem_foe[];
    Cx<R> *buf = reinterpret_cast<Cx<R> *>(smem_foe);
    constexpr int LD = N1 + 1;                                         // a column's stride in LDS: the FOE_C columns of one n1 fall on different banks
    const int64_t N = (int64_t)N1 * N2;
    const int c0 = blockIdx.x * FOE_C;
    const int64_t s = (b0 + blockIdx.y) * N;
    const int64_t valid = L - s;
    const Cx<R> *x = E + (size_t)blockIdx.z * L + s;
    for (int i = threadIdx.x; i < N1 * FOE_C; i += CD_T) {
        const int c = i % FOE_C, n1 = i / FOE_C;
        const int64_t n = (int64_t)n1 * N2 + c0 + c;                   // < N by construction
        buf[c * LD + n1] = n < valid ? pow4(ldg(x + n)) : Cx<R>{(R)0, (R)0};
    }
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < FOE_C; c++) fft_from<R, N1, 1>(buf + c * LD, tw1);
    Cx<R> *t = T + ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * N;
    for (int i = threadIdx.x; i < N1 * FOE_C; i += CD_T) {
        const int c = i % FOE_C, k1 = i / FOE_C;
        double turns = (double)((int64_t)k1 * (c0 + c)) / (double)N;   // exact, in [0, 1)
        turns -= rint(turns);
        double sn, cs;
        sincospi(-2.0 * turns, &sn, &cs);
        stg(t + (size_t)k1 * N2 + c0 + c, cmul(buf[c * LD + k1], Cx<R>{(R)cs, (R)sn}));
    }
}

// P[row][j] = (first ? 0 : P[row][j]) + sum_b Pb[row][b][j], b in order.  grid (N / 256, nmodes)
template <typename R>
__global__ void __launch_bounds__(256) foe_accum_kernel(const R *__restrict__ Pb, int N, int nb, int first, R *__restrict__ P)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const size_t row = blockIdx.y;
    R acc = first ? (R)0 : P[row * N + j];
    for (int b = 0; b < nb; b++) acc += Pb[(row * nb + b) * N + j];
    P[row * N + j] = acc;
}

// the larger value wins, of equal values the lower bin (np.argmax: the first maximum)
__device__ __forceinline__ void peak_merge(double &v, int &k, double v2, int k2)
{
    if (v2 > v || (v2 == v && k2 < k)) { v = v2; k = k2; }
}
// tree over the 256 threads' (value, bin, sum) in LDS, in a fixed order; the result is in entry 0
__device__ __forceinline__ void peak_block_reduce(double *sv, int *sk, double *ss, double v, int k, double sum)
{
    sv[threadIdx.x] = v; sk[threadIdx.x] = k; ss[threadIdx.x] = sum;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) {
            double a = sv[threadIdx.x];
            int ka = sk[threadIdx.x];
            peak_merge(a, ka, sv[threadIdx.x + h], sk[threadIdx.x + h]);
            sv[threadIdx.x] = a; sk[threadIdx.x] = ka;
            ss[threadIdx.x] += ss[threadIdx.x + h];
        }
        __syncthreads();
    }
}

// First level: part p of row r covers `per` consecutive positions q of the stored spectrum; position q = k1 N2 + k2 is bin k1 + N1 k2.
// grid (N / per, nmodes); part (nmodes, gridDim.x, 3) doubles: value, bin, sum.
template <typename R>
__global__ void __launch_bounds__(256) foe_peak_partial_kernel(const R *__restrict__ P, int N, int lgN2, int N1, int per, double *__restrict__ part)
{
    __shared__ double sv[256], ss[256];
    __shared__ int sk[256];
    const size_t row = blockIdx.y;
    const int base = blockIdx.x * per, m2 = (1 << lgN2) - 1;
    double v = -1.0, sum = 0.0;
    int k = 0x7fffffff;
    for (int j = threadIdx.x; j < per; j += 256) {
        const int q = base + j;
        const double pv = (double)P[row * N + q];
        sum += pv;
        peak_merge(v, k, pv, (q >> lgN2) + N1 * (q & m2));
    }
    peak_block_reduce(sv, sk, ss, v, k, sum);
    if (threadIdx.x == 0) {
        double *o = part + (row * gridDim.x + blockIdx.x) * 3;
        o[0] = sv[0]; o[1] = (double)sk[0]; o[2] = ss[0];
    }
}

// Second level, one workgroup, the rows in turn: stats[row] = (bin, P[bin], sum P), fo[row] = (bin < N / 2 ? bin : bin - N) * step / 4 with
// step = 1 / (N (1 / os)) formed by the caller as numpy's fftfreq forms it; `average`: every fo[row] becomes sum_rows fo / nmodes.
__global__ void __launch_bounds__(256) foe_peak_final_kernel(const double *__restrict__ part, int nparts, int nmodes, int N, double step, int average,
                                                             double *__restrict__ fo, double *__restrict__ stats)
{
    __shared__ double sv[256], ss[256];
    __shared__ int sk[256];
    __shared__ double mean;
    double total = 0.0;
    for (int row = 0; row < nmodes; row++) {
        double v = -1.0, sum = 0.0;
        int k = 0x7fffffff;
        if ((int)threadIdx.x < nparts) {
            const double *p = part + ((size_t)row * nparts + threadIdx.x) * 3;
            v = p[0]; k = (int)p[1]; sum = p[2];
        }
        peak_block_reduce(sv, sk, ss, v, k, sum);
        if (threadIdx.x == 0) {
            int bin = sk[0];
            if (bin < 0 || bin >= N) bin = 0;                          // (a row of NaNs has no maximum)
            const double f = (double)(bin < N / 2 ? bin : bin - N) * step / 4.0;
            stats[3 * (size_t)row] = (double)bin; stats[3 * (size_t)row + 1] = sv[0]; stats[3 * (size_t)row + 2] = ss[0];
            fo[row] = f;
            total += f;
        }
        __syncthreads();
    }
    if (!average) return;
    if (threadIdx.x == 0) mean = total / (double)nmodes;
    __syncthreads();
    for (int row = threadIdx.x; row < nmodes; row += 256) fo[row] = mean;
}

// out[row][k] = P[row][(k mod N1) N2 + k / N1]: the stored spectrum in bin order.  grid (N / 256, nmodes)
template <typename R>
__global__ void __launch_bounds__(256) foe_spectrum_kernel(const R *__restrict__ P, int N, int lgN1, int lgN2, R *__restrict__ out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    const size_t row = blockIdx.y;
    out[row * N + k] = P[row * N + ((size_t)(k & ((1 << lgN1) - 1)) << lgN2) + (k >> lgN1)];
}

// ------------------------------------------------------------------------------------------------ host side
template <typename R, int N, bool FOURTH>
static int foe_fft_launch(const Cx<R> *in, int64_t L, int64_t b0, int64_t count, int nmodes, const Cx<R> *tw, R *Pb)
{
    const size_t lds = (size_t)N * sizeof(Cx<R>);
    int rc = dyn_lds(foe_fft_kernel<R, N, FOURTH>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL((foe_fft_kernel<R, N, FOURTH>), dim3((unsigned)count, nmodes), dim3(CD_T), lds, g_stream, in, L, b0, tw, Pb);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R, int N1>
static int foe_step1_launch(const Cx<R> *E, int64_t L, int64_t b0, int nb, int nmodes, int N2, const Cx<R> *tw1, Cx<R> *T)
{
    const size_t lds = (size_t)FOE_C * (N1 + 1) * sizeof(Cx<R>);
    int rc = dyn_lds(foe_step1_kernel<R, N1>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL((foe_step1_kernel<R, N1>), dim3(N2 / FOE_C, nb, nmodes), dim3(CD_T), lds, g_stream, E, L, b0, N2, tw1, T);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R>
int find_freq_offset_dev(const void *E, int nmodes, int64_t L, int os, int fft_size, int blocks, int average, double *fo, double *stats, void *spectrum)
{
    int rc = ensure_init();
    if (rc) return rc;
    int lg = 0;
    while (lg < 30 && (1 << lg) < fft_size) lg++;
    QH_REQUIRE(fft_size == (1 << lg) && lg >= FOE_LG_MIN && lg <= FOE_LG_MAX, "find_freq_offset: fft_size must be a power of two from 2^8 to 2^20");
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 1 && os >= 1, "find_freq_offset: bad sizes");
    QH_REQUIRE(blocks >= 1 && (blocks == 1 || (int64_t)blocks * fft_size <= L), "find_freq_offset: blocks >= 1, and more than one block needs blocks * fft_size <= L");
    QH_REQUIRE(E && fo, "find_freq_offset: E and fo_out must be given");
    const int N = fft_size;
    const int lgN1 = lg > FOE_LG_SINGLE ? lg / 2 : 0, lgN2 = lg - lgN1;
    const int N1 = 1 << lgN1, N2 = 1 << lgN2;
    int64_t chunk = FOE_CHUNK / ((int64_t)nmodes * N);
    if (chunk > blocks) chunk = blocks;
    if (chunk < 1) chunk = 1;
    const int per = N / FOE_PARTS >= 256 ? N / FOE_PARTS : 256, nparts = N / per;
    // scratch: W_N1 | W_N2 | P | partial results | stats | per-block powers | four-step intermediate
    ScratchLayout lay;
    const size_t o_tw1 = lay.take((size_t)N1 * sizeof(Cx<R>)), o_tw2 = lay.take((size_t)N2 * sizeof(Cx<R>)), o_P = lay.take((size_t)nmodes * N * sizeof(R)),
                 o_part = lay.take((size_t)nmodes * nparts * 3 * sizeof(double)), o_stats = lay.take((size_t)nmodes * 3 * sizeof(double)),
                 o_Pb = lay.take((size_t)nmodes * chunk * N * sizeof(R)), o_T = lay.take(N1 > 1 ? (size_t)nmodes * chunk * N * sizeof(Cx<R>) : 0);
    void *base = nullptr;
    if ((rc = scratch(Slot::FOE, lay.total, &base))) return rc;
    char *sb = (char *)base;
    Cx<R> *tw1 = (Cx<R> *)(sb + o_tw1), *tw2 = (Cx<R> *)(sb + o_tw2), *T = (Cx<R> *)(sb + o_T);
    R *P = (R *)(sb + o_P), *Pb = (R *)(sb + o_Pb);
    double *part = (double *)(sb + o_part);
    if (!stats) stats = (double *)(sb + o_stats);
    const Cx<R> *e = (const Cx<R> *)E;
    if (N1 > 1) hipLaunchKernelGGL((twiddle_kernel<R>), dim3((N1 + 255) / 256), dim3(256), 0, g_stream, tw1, N1);
    hipLaunchKernelGGL((twiddle_kernel<R>), dim3((N2 + 255) / 256), dim3(256), 0, g_stream, tw2, N2);
    QH_HIP(hipGetLastError());
    for (int64_t b0 = 0; b0 < blocks; b0 += chunk) {
        const int nb = (int)(blocks - b0 < chunk ? blocks - b0 : chunk);
        if (N1 == 1) {
            switch (N) {
            case 256: rc = foe_fft_launch<R, 256, true>(e, L, b0, nb, nmodes, tw2, Pb); break;
            case 512: rc = foe_fft_launch<R, 512, true>(e, L, b0, nb, nmodes, tw2, Pb); break;
            case 1024: rc = foe_fft_launch<R, 1024, true>(e, L, b0, nb, nmodes, tw2, Pb); break;
            case 2048: rc = foe_fft_launch<R, 2048, true>(e, L, b0, nb, nmodes, tw2, Pb); break;
            case 4096: rc = foe_fft_launch<R, 4096, true>(e, L, b0, nb, nmodes, tw2, Pb); break;
            default: rc = foe_fft_launch<R, 8192, true>(e, L, b0, nb, nmodes, tw2, Pb); break;
            }
            if (rc) return rc;
        } else {
            switch (N1) {
            case 128: rc = foe_step1_launch<R, 128>(e, L, b0, nb, nmodes, N2, tw1, T); break;
            case 256: rc = foe_step1_launch<R, 256>(e, L, b0, nb, nmodes, N2, tw1, T); break;
            case 512: rc = foe_step1_launch<R, 512>(e, L, b0, nb, nmodes, N2, tw1, T); break;
            default: rc = foe_step1_launch<R, 1024>(e, L, b0, nb, nmodes, N2, tw1, T); break;
            }
            if (rc) return rc;
            const int64_t count = (int64_t)nb * N1;                    // rows T[k1][:] of the chunk's blocks, per mode
            switch (N2) {
            case 128: rc = foe_fft_launch<R, 128, false>(T, 0, 0, count, nmodes, tw2, Pb); break;
            case 256: rc = foe_fft_launch<R, 256, false>(T, 0, 0, count, nmodes, tw2, Pb); break;
            case 512: rc = foe_fft_launch<R, 512, false>(T, 0, 0, count, nmodes, tw2, Pb); break;
            default: rc = foe_fft_launch<R, 1024, false>(T, 0, 0, count, nmodes, tw2, Pb); break;
            }
            if (rc) return rc;
        }
        hipLaunchKernelGGL((foe_accum_kernel<R>), dim3(N / 256, nmodes), dim3(256), 0, g_stream, (const R *)Pb, N, nb, b0 == 0 ? 1 : 0, P);
        QH_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL((foe_peak_partial_kernel<R>), dim3(nparts, nmodes), dim3(256), 0, g_stream, (const R *)P, N, lgN2, N1, per, part);
    const double d = 1.0 / (double)os, step = 1.0 / ((double)N * d);   // numpy.fft.fftfreq(N, 1 / os): k * (1 / (N d))
    hipLaunchKernelGGL(foe_peak_final_kernel, dim3(1), dim3(256), 0, g_stream, (const double *)part, nparts, nmodes, N, step, average ? 1 : 0, fo, stats);
    if (spectrum) hipLaunchKernelGGL((foe_spectrum_kernel<R>), dim3(N / 256, nmodes), dim3(256), 0, g_stream, (const R *)P, N, lgN1, lgN2, (R *)spectrum);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R>
int find_freq_offset_host(const void *E, int nmodes, int64_t L, int os, int fft_size, int blocks, int average, double *fo, double *stats, void *spectrum)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 1 && fft_size >= 1 && fft_size <= (1 << FOE_LG_MAX), "find_freq_offset: bad sizes");
    QH_REQUIRE(E && fo, "find_freq_offset: E and fo_out must be given");
    DevBuf dE, dfo, dst, dsp;
    if ((rc = dE.from_host(E, (size_t)nmodes * L * sizeof(Cx<R>)))) return rc;
    if ((rc = dfo.alloc((size_t)nmodes * sizeof(double)))) return rc;
    if ((rc = dst.alloc((size_t)nmodes * 3 * sizeof(double)))) return rc;
    if (spectrum && (rc = dsp.alloc((size_t)nmodes * fft_size * sizeof(R)))) return rc;
    if ((rc = find_freq_offset_dev<R>(dE.p, nmodes, L, os, fft_size, blocks, average, (double *)dfo.p, (double *)dst.p, spectrum ? dsp.p : nullptr))) return rc;
    if ((rc = dfo.to_host(fo, dfo.n))) return rc;
    if (stats && (rc = dst.to_host(stats, dst.n))) return rc;
    if (spectrum && (rc = dsp.to_host(spectrum, dsp.n))) return rc;
    QH_HIP(hipStreamSynchronize(g_stream));
    return QH_OK;
}

}  // namespace qh

extern "C" {
int qh_find_freq_offset_c64_dev(const void *E, int nmodes, int64_t L, int os, int fft_size, int blocks, int average, double *fo_out, double *stats_out,
                                void *spectrum_out)
{ return qh::find_freq_offset_dev<float>(E, nmodes, L, os, fft_size, blocks, average, fo_out, stats_out, spectrum_out); }
int qh_find_freq_offset_c128_dev(const void *E, int nmodes, int64_t L, int os, int fft_size, int blocks, int average, double *fo_out, double *stats_out,
                                 void *spectrum_out)
{ return qh::find_freq_offset_dev<double>(E, nmodes, L, os, fft_size, blocks, average, fo_out, stats_out, spectrum_out); }
int qh_find_freq_offset_c64(const void *E, int nmodes, int64_t L, int os, int fft_size, int blocks, int average, double *fo_out, double *stats_out,
                            void *spectrum_out)
{ return qh::find_freq_offset_host<float>(E, nmodes, L, os, fft_size, blocks, average, fo_out, stats_out, spectrum_out); }
int qh_find_freq_offset_c128(const void *E, int nmodes, int64_t L, int os, int fft_size, int blocks, int average, double *fo_out, double *stats_out,
                             void *spectrum_out)
{ return qh::find_freq_offset_host<double>(E, nmodes, L, os, fft_size, blocks, average, fo_out, stats_out, spectrum_out); }
}
