// Synchronisation of a received row with a transmitted one in HBM: what find_sequence_offset / find_sequence_offset_complex /
// sync_and_adjust (qampy/core/ber_functions.py:33-160) do on the host with scipy's fftconvolve.
//
//   xcorr     cc = fftconvolve(x, conj(y)[::-1], "full") of every row of x: one streaming kernel writes the reversed conjugate of y, then
//             three power-of-two transforms of size P >= nx + ny - 1 (fft.hip): y's, the rows' and the inverse one, which multiplies by y's
//             transform as it loads the spectrum and stores only the nx + ny - 1 values that exist.  The zero padding is the transforms'
//             load functor, not a pass.  Bound by HBM: per row about 6 P complex values moved (four-step sizes), 2 P up to P = 2^13.
//   peak      first maximum of |cc| over [0, n) and the maxima of Re, Im, -Re, -Im (the four quarter-turn hypotheses), two launches: one
//             partial per tile of PK_TILE values (shuffles inside a wave, LDS across the four waves), then one workgroup over the partials.
//             Magnitudes are compared squared, in the field's real type.  Every comparison carries the index and a tie goes to the lower one, so the order of the reduction does not matter and the
//             result is np.argmax's; a NaN magnitude beats every number (np.argmax takes the first NaN) and turns the maxima into NaN (np.max).
//             One read of cc: bound by HBM.
//   gather    out[i] = j^turns src[(i - offset) mod nsrc]: roll, roll and cut, periodic extension of sync_and_adjust in one formula; the
//             rotation is a swap and a sign.  One read, one write.
//   labels    out[i] = alphabet[idx[i]], 0 for a label outside [0, M).
//
// No atomics: a repeated call is bit-identical.  Scratch slot Slot::SYNC: reversed y (P) | spectra (rows, P); Slot::PEAK: the partials.
// Grow-only, so a call at a shape seen before allocates nothing.  Every launch is bounded by the call's arguments alone.
#include "common.h"
#include <cmath>

namespace qh {

constexpr int SY_T = 256;                   // threads of every kernel here
constexpr int PK_PER = 16;                  // values per thread of the peak search's first stage
constexpr int PK_TILE = SY_T * PK_PER;      // values per workgroup
constexpr int PK_F = 6;                     // doubles of a partial and of a result row: index, max Re, max Im, max -Re, max -Im, |cc| there
constexpr int SY_LG_MIN = 8, SY_LG_MAX = 24;
constexpr int64_t SY_NMAX = (int64_t)1 << 31;      // longest row of the gather and the label kernels (and largest |offset|)

template <typename R> __device__ __forceinline__ Cx<R> sy_rot90(Cx<R> x, int k)       // x * j^k
{
    switch (k & 3) {
    case 1: return Cx<R>{-x.im, x.re};
    case 2: return Cx<R>{-x.re, -x.im};
    case 3: return Cx<R>{x.im, -x.re};
    default: return x;
    }
}

// yrev[i] = conj(y[ny - 1 - i]), i < ny
template <typename R> __global__ void __launch_bounds__(SY_T) sync_reverse_kernel(const Cx<R> *__restrict__ y, int64_t ny, Cx<R> *__restrict__ yrev)
{
    const int64_t i = (int64_t)blockIdx.x * SY_T + threadIdx.x;
    if (i >= ny) return;
    const Cx<R> v = ldg(y + (ny - 1 - i));
    stg(yrev + i, Cx<R>{v.re, -v.im});
}

// ---------------------------------------------------------------------------------------------- peak search
// candidate (magnitude, index) a against b: a NaN beats a number, a larger number a smaller one, the lower index an equal one
template <typename R> __device__ __forceinline__ bool pk_better(R ma, int64_t ia, R mb, int64_t ib)
{
    const bool na = ma != ma, nb = mb != mb;
    if (na != nb) return na;
    if (!na && ma != mb) return ma > mb;
    return ia < ib;
}
// np.max of two: the larger, NaN if either is
template <typename R> __device__ __forceinline__ R pk_max(R a, R b) { return (b > a || b != b) ? b : a; }

template <typename R> struct Peak {
    R m;                 // squared magnitude at idx
    int64_t idx;
    R d[4];              // max Re, max Im, max -Re, max -Im
};

template <typename R> __device__ __forceinline__ void pk_merge(Peak<R> &a, const Peak<R> &b)
{
    if (pk_better(b.m, b.idx, a.m, a.idx)) { a.m = b.m; a.idx = b.idx; }
#pragma unroll
    for (int k = 0; k < 4; k++) a.d[k] = pk_max(a.d[k], b.d[k]);
}

// all 256 threads' candidates into thread 0's: shuffles inside each wave64, LDS across the four waves
template <typename R> __device__ __forceinline__ void pk_block_reduce(Peak<R> &p)
{
    for (int o = 32; o > 0; o >>= 1) {
        Peak<R> q;
        q.m = __shfl_down(p.m, o);
        q.idx = __shfl_down(p.idx, o);
#pragma unroll
        for (int k = 0; k < 4; k++) q.d[k] = __shfl_down(p.d[k], o);
        pk_merge(p, q);
    }
    __shared__ Peak<R> part[SY_T / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < SY_T / 64; w++) pk_merge(p, part[w]);
}

template <typename R> __device__ __forceinline__ Peak<R> pk_empty()
{
    const R ninf = -(R)INFINITY;
    return Peak<R>{(R)-1, INT64_MAX, {ninf, ninf, ninf, ninf}};      // any magnitude (>= 0 or NaN) beats -1
}

// a partial keeps the squared magnitude (a value of type R, exact in a double); the result row holds the magnitude
template <typename R, bool FINAL> __device__ __forceinline__ void pk_write(double *o, const Peak<R> &p)
{
    o[0] = (double)p.idx; o[1] = (double)p.d[0]; o[2] = (double)p.d[1]; o[3] = (double)p.d[2]; o[4] = (double)p.d[3];
    o[5] = FINAL ? sqrt((double)p.m) : (double)p.m;
}

// stage one.  grid (tiles, rows); part (rows, tiles, PK_F)
template <typename R> __global__ void __launch_bounds__(SY_T) sync_peak_tile_kernel(const Cx<R> *__restrict__ cc, int64_t n, double *__restrict__ part)
{
    const Cx<R> *row = cc + (size_t)blockIdx.y * n;
    const int64_t t0 = (int64_t)blockIdx.x * PK_TILE;
    Peak<R> p = pk_empty<R>();
#pragma unroll 4
    for (int k = 0; k < PK_PER; k++) {
        const int64_t i = t0 + (int64_t)k * SY_T + threadIdx.x;
        if (i < n) {
            const Cx<R> v = ldg(row + i);
            Peak<R> q{v.re * v.re + v.im * v.im, i, {v.re, v.im, -v.re, -v.im}};
            pk_merge(p, q);
        }
    }
    pk_block_reduce(p);
    if (threadIdx.x == 0) pk_write<R, false>(part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * PK_F, p);
}

// stage two.  grid (rows): one workgroup over the `tiles` partials of its row
template <typename R> __global__ void __launch_bounds__(SY_T) sync_peak_final_kernel(const double *__restrict__ part, int tiles, double *__restrict__ res)
{
    const double *row = part + (size_t)blockIdx.x * tiles * PK_F;
    Peak<R> p = pk_empty<R>();
    for (int t = threadIdx.x; t < tiles; t += SY_T) {
        const double *q = row + (size_t)t * PK_F;
        Peak<R> c{(R)q[5], (int64_t)q[0], {(R)q[1], (R)q[2], (R)q[3], (R)q[4]}};         // the doubles hold values of type R: exact
        pk_merge(p, c);
    }
    pk_block_reduce(p);
    if (threadIdx.x == 0) pk_write<R, true>(res + (size_t)blockIdx.x * PK_F, p);
}

// ---------------------------------------------------------------------------------------------- gather
// GA_PER consecutive strides of the grid per thread: one 64-bit remainder per thread, then a step and a wrap
constexpr int GA_PER = 4;

template <typename T, bool ROT>
__global__ void __launch_bounds__(SY_T) sync_gather_kernel(const T *__restrict__ src, int64_t nsrc, int64_t offset, int turns, int64_t nout, T *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * SY_T, step = stride % nsrc;
    int64_t i = (int64_t)blockIdx.x * SY_T + threadIdx.x;
    if (i >= nout) return;
    int64_t j = (i - offset) % nsrc;
    if (j < 0) j += nsrc;
    for (int k = 0; k < GA_PER && i < nout; k++, i += stride) {
        if constexpr (ROT) stg(out + i, sy_rot90(ldg(src + j), turns));
        else out[i] = src[j];
        j += step;
        if (j >= nsrc) j -= nsrc;
    }
}

template <typename R>
__global__ void __launch_bounds__(SY_T) sync_labels_kernel(const int32_t *__restrict__ idx, int64_t n, const Cx<R> *__restrict__ alphabet, int M, Cx<R> *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * SY_T + threadIdx.x;
    if (i >= n) return;
    const int32_t k = idx[i];
    stg(out + i, (k >= 0 && k < M) ? ldg(alphabet + k) : Cx<R>{(R)0, (R)0});
}

// ------------------------------------------------------------------------------------------------ host side
template <typename R> int xcorr_dev(const void *x, int nx_rows, int64_t nx, const void *y, int64_t ny, void *cc)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nx >= 1 && ny >= 1 && nx <= ((int64_t)1 << SY_LG_MAX) && ny <= ((int64_t)1 << SY_LG_MAX) && nx + ny - 1 <= ((int64_t)1 << SY_LG_MAX),
               "xcorr: nx and ny must be at least 1 and nx + ny - 1 at most 2^24");
    QH_REQUIRE(nx_rows >= 1 && nx_rows <= 65535, "xcorr: bad number of rows");
    QH_REQUIRE(x && y && cc, "xcorr: x, y and cc must be given");
    const int64_t n = nx + ny - 1;
    int lg = SY_LG_MIN;
    while (((int64_t)1 << lg) < n) lg++;
    const int64_t P = (int64_t)1 << lg;
    ScratchLayout lay;
    const size_t o_y = lay.take((size_t)P * sizeof(Cx<R>)), o_spec = lay.take((size_t)nx_rows * P * sizeof(Cx<R>));
    void *base = nullptr;
    if ((rc = scratch(Slot::SYNC, lay.total, &base))) return rc;
    Cx<R> *yrev = (Cx<R> *)((char *)base + o_y), *spec = (Cx<R> *)((char *)base + o_spec);
    hipLaunchKernelGGL((sync_reverse_kernel<R>), dim3((unsigned)((ny + SY_T - 1) / SY_T)), dim3(SY_T), 0, g_stream, (const Cx<R> *)y, ny, yrev);
    QH_HIP(hipGetLastError());
    return fft_correlate_pow2<R>(x, nx_rows, nx, yrev, ny, P, spec, cc, n);
}

template <typename R> int xcorr_peak_dev(const void *cc, int rows, int64_t n, double *res)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(rows >= 1 && rows <= 65535 && n >= 1 && n <= ((int64_t)1 << (SY_LG_MAX + 1)), "xcorr_peak: bad sizes");
    QH_REQUIRE(cc && res, "xcorr_peak: cc and res must be given");
    const int tiles = (int)((n + PK_TILE - 1) / PK_TILE);
    void *part = nullptr;
    if ((rc = scratch(Slot::PEAK, (size_t)rows * tiles * PK_F * sizeof(double), &part))) return rc;
    hipLaunchKernelGGL((sync_peak_tile_kernel<R>), dim3(tiles, rows), dim3(SY_T), 0, g_stream, (const Cx<R> *)cc, n, (double *)part);
    hipLaunchKernelGGL((sync_peak_final_kernel<R>), dim3(rows), dim3(SY_T), 0, g_stream, (const double *)part, tiles, res);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename T, bool ROT> int cyclic_gather_dev(const void *src, int64_t nsrc, int64_t offset, int turns, int64_t nout, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nsrc >= 1 && nout >= 1 && nsrc <= SY_NMAX && nout <= SY_NMAX && offset >= -SY_NMAX && offset <= SY_NMAX, "cyclic_gather: bad sizes");
    QH_REQUIRE(src && out && src != out, "cyclic_gather: src and out must be given and differ");
    const int64_t per = (int64_t)SY_T * GA_PER;
    hipLaunchKernelGGL((sync_gather_kernel<T, ROT>), dim3((unsigned)((nout + per - 1) / per)), dim3(SY_T), 0, g_stream, (const T *)src, nsrc, offset, turns & 3,
                       nout, (T *)out);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R> int labels_to_symbols_dev(const int32_t *idx, int64_t n, const void *alphabet, int M, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(n >= 1 && n <= SY_NMAX && M >= 1, "labels_to_symbols: bad sizes");
    QH_REQUIRE(idx && alphabet && out, "labels_to_symbols: idx, alphabet and out must be given");
    hipLaunchKernelGGL((sync_labels_kernel<R>), dim3((unsigned)((n + SY_T - 1) / SY_T)), dim3(SY_T), 0, g_stream, idx, n, (const Cx<R> *)alphabet, M, (Cx<R> *)out);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

}  // namespace qh

extern "C" {
int qh_xcorr_c64_dev(const void *x, int nx_rows, int64_t nx, const void *y, int64_t ny, void *cc) { return qh::xcorr_dev<float>(x, nx_rows, nx, y, ny, cc); }
int qh_xcorr_c128_dev(const void *x, int nx_rows, int64_t nx, const void *y, int64_t ny, void *cc) { return qh::xcorr_dev<double>(x, nx_rows, nx, y, ny, cc); }
int qh_xcorr_peak_c64_dev(const void *cc, int rows, int64_t n, double *res) { return qh::xcorr_peak_dev<float>(cc, rows, n, res); }
int qh_xcorr_peak_c128_dev(const void *cc, int rows, int64_t n, double *res) { return qh::xcorr_peak_dev<double>(cc, rows, n, res); }
int qh_cyclic_gather_c64_dev(const void *src, int64_t nsrc, int64_t offset, int turns, int64_t nout, void *out)
{ return qh::cyclic_gather_dev<qh::Cx<float>, true>(src, nsrc, offset, turns, nout, out); }
int qh_cyclic_gather_c128_dev(const void *src, int64_t nsrc, int64_t offset, int turns, int64_t nout, void *out)
{ return qh::cyclic_gather_dev<qh::Cx<double>, true>(src, nsrc, offset, turns, nout, out); }
int qh_cyclic_gather_i32_dev(const int32_t *src, int64_t nsrc, int64_t offset, int64_t nout, int32_t *out)
{ return qh::cyclic_gather_dev<int32_t, false>(src, nsrc, offset, 0, nout, out); }
int qh_labels_to_symbols_c64_dev(const int32_t *idx, int64_t n, const void *alphabet, int M, void *out) { return qh::labels_to_symbols_dev<float>(idx, n, alphabet, M, out); }
int qh_labels_to_symbols_c128_dev(const int32_t *idx, int64_t n, const void *alphabet, int M, void *out) { return qh::labels_to_symbols_dev<double>(idx, n, alphabet, M, out); }
}
