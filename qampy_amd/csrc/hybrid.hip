// Time-domain hybrid QAM on rows already in HBM: two formats interleaved in a fixed frame (qampy/signals.py:1182-1427 TDHQAMSymbols; the
// reference builds such a signal but cannot take it apart or measure it - DESIGN.md 3.21 has the semantics fixed here).
//
// A frame is fM positions: position n of a row carries format 1 when n % fM < fM1, else format 2 (fM2 = fM - fM1 of them).  Format-2 symbols
// are stored divided by sqrt(powratio), so that both alphabets keep the same spacing.
//
//   assemble     out[f fM + p] = part1[f fM1 + p] (p < fM1) or part2[f fM2 + p - fM1] / sqrt(powratio); optionally the labels of the parts are
//                laid out the same way.  The quotient is numpy's complex-by-real one: the product with 1 / sqrt(powratio), formed in double and
//                rounded once to the precision of the row.
//   class sums   S[row][r] = sum of |x_n| over n = r (mod fM), |x| = sqrt(re^2 + im^2) in double.  A workgroup takes a tile of TDH_TILE samples
//                whatever fM is: its 256 threads are G = 256 / fM groups of fM, thread (q, r) adds the occurrences q, q + G, .. of residue r
//                inside the tile in ascending order, the G group sums are added in order, and the tile's fM sums go out with plain stores.  The
//                residue of a tile's first sample is (tile TDH_TILE) % fM: fM need not divide the tile.  A second launch, one wave per
//                (residue, row), adds the tile sums in a fixed order.  No atomics: a repeated call gives the same bits.
//   align        one workgroup per row: m_j = sum over the residues r of the higher-order format of S[(r + j) % fM], j < fM (r ascending), and
//                shift = the first j whose m_j is strictly largest, written to HBM as int32.
//   split        part1[k] = x[(idx1[k] + shift) % L], part2[k] = x[(idx2[k] + shift) % L] sqrt(powratio) (the product in double, rounded once).
//   metrics      per row and format: symbol errors, bit errors (popc(decision ^ label): the alphabets are in bit-label order), symbols compared
//                and the sum of |r - s_label|^2, r the sample at (n + shift) % L, times sqrt(powratio) in format 2.  Both alphabets (runtime
//                M1, M2 <= 1024) sit in LDS; the format-1 symbols and the format-2 symbols are walked in two loops, so a wave never mixes
//                alphabets, and a thread holds TDH_S samples against every alphabet read.  The decision is the nearest point by squared
//                distance in the precision of the row, the first on a tie.  Labels outside [0, M) are skipped.  Sums in double: workgroup
//                partials in a fixed order, then a fixed-order reduction.
//
// What bounds them: assemble, split and the class sums move every sample once and do one integer division on it - memory traffic, at a few
// million samples the latency of their one or two launches; the metrics pass does 7 vector operations per (sample, point) and runs at the
// vector issue rate from a few tens of points on.  profiles/hybrid_timings.md has the times.
#include "common.h"
#include <cmath>

namespace qh {

constexpr int TDH_T = 256;               // threads of a workgroup
constexpr int TDH_TILE = 4096;           // samples of a row per workgroup of the class sums
constexpr int TDH_FM_MAX = 256;          // longest frame
constexpr int TDH_M_MAX = 1024;          // most points of an alphabet
constexpr int TDH_S = 4;                 // samples a thread holds against one alphabet read
constexpr int TDH_MAXBLK = 1024;         // most workgroups per row of the metrics pass
constexpr int TDH_F = 8;                 // sums per row: (symbol errors, bit errors, compared, squared error) of format 1, then of format 2
constexpr int64_t TDH_LMAX = 0x7fffffffLL;

// a sample's place in the parts: frame f, position p of n = f fM + p
struct TdhGeom { unsigned fM, fM1, fM2; };

template <typename R> __device__ __forceinline__ Cx<R> tdh_scaled(Cx<R> v, double s)
{
    return Cx<R>{(R)((double)v.re * s), (R)((double)v.im * s)};
}

// grid (blocks, nmodes)
template <typename R>
__global__ void __launch_bounds__(TDH_T) tdh_assemble_kernel(const Cx<R> *__restrict__ p1, const Cx<R> *__restrict__ p2, const int32_t *__restrict__ l1,
                                                             const int32_t *__restrict__ l2, unsigned nframes, TdhGeom g, double inv_root,
                                                             Cx<R> *__restrict__ out, int32_t *__restrict__ idx)
{
    const unsigned L = nframes * g.fM, n = blockIdx.x * TDH_T + threadIdx.x;
    if (n >= L) return;
    const size_t row = blockIdx.y;
    const unsigned f = n / g.fM, p = n - f * g.fM;
    if (p < g.fM1) {
        const size_t k = row * ((size_t)nframes * g.fM1) + (size_t)f * g.fM1 + p;
        stg(out + row * L + n, ldg(p1 + k));
        if (idx) idx[row * L + n] = l1[k];
    } else {
        const size_t k = row * ((size_t)nframes * g.fM2) + (size_t)f * g.fM2 + (p - g.fM1);
        stg(out + row * L + n, tdh_scaled(ldg(p2 + k), inv_root));
        if (idx) idx[row * L + n] = l2[k];
    }
}

// grid (tiles, nmodes): part[(row tiles + tile) fM + r]
template <typename R>
__global__ void __launch_bounds__(TDH_T) tdh_class_tile_kernel(const Cx<R> *__restrict__ E, unsigned L, unsigned fM, double *__restrict__ part)
{
    __shared__ double grp[TDH_T];
    const unsigned t = threadIdx.x, G = TDH_T / fM;
    const unsigned lo = blockIdx.x * (unsigned)TDH_TILE, len = L - lo < (unsigned)TDH_TILE ? L - lo : (unsigned)TDH_TILE;
    const Cx<R> *x = E + (size_t)blockIdx.y * L + lo;
    double s = 0.;
    if (t < G * fM) {
        const unsigned q = t / fM, r = t - q * fM;
        const unsigned first = (r + fM - lo % fM) % fM;           // the first sample of the tile with residue r
        const unsigned step = G * fM;
#pragma unroll 4
        for (unsigned p = first + q * fM; p < len; p += step) {
            const Cx<R> v = ldg(x + p);
            const double a = (double)v.re, b = (double)v.im;
            s += sqrt(fma_(a, a, b * b));
        }
    }
    grp[t] = s;
    __syncthreads();
    if (t < fM) {
        double tot = 0.;
        for (unsigned q = 0; q < G; q++) tot += grp[q * fM + t];
        part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * fM + t] = tot;
    }
}

// grid (fM, nmodes), one wave: sums[row fM + r] = the tiles' sums of residue r, lane j adds the tiles j, j + 64, .. in order
__global__ void __launch_bounds__(64) tdh_class_combine_kernel(const double *__restrict__ part, int ntiles, double *__restrict__ sums)
{
    const unsigned r = blockIdx.x, fM = gridDim.x;
    const double *p = part + (size_t)blockIdx.y * ntiles * fM + r;
    double s = 0.;
    for (int b = threadIdx.x; b < ntiles; b += 64) s += p[(size_t)b * fM];
    s = wave_sum(s);
    if (threadIdx.x == 0) sums[(size_t)blockIdx.y * fM + r] = s;
}

// grid (nmodes): residues [h0, h1) carry the higher-order format
__global__ void __launch_bounds__(TDH_T) tdh_align_kernel(const double *__restrict__ sums, int fM, int h0, int h1, int32_t *__restrict__ shift)
{
    __shared__ double S[TDH_FM_MAX], m[TDH_FM_MAX];
    const int j = threadIdx.x;
    if (j < fM) S[j] = sums[(size_t)blockIdx.x * fM + j];
    __syncthreads();
    if (j < fM) {
        double a = 0.;
        for (int r = h0; r < h1; r++) {
            int k = r + j;
            if (k >= fM) k -= fM;
            a += S[k];
        }
        m[j] = a;
    }
    __syncthreads();
    if (j == 0) {
        int best = 0;
        double top = m[0];
        for (int k = 1; k < fM; k++) if (m[k] > top) { top = m[k]; best = k; }
        shift[blockIdx.x] = best;
    }
}

// the cyclic shift of a row, brought into [0, L)
__device__ __forceinline__ unsigned tdh_shift(const int32_t *shift_dev, int shift_host, unsigned row, unsigned L)
{
    const long long s = shift_dev ? (long long)shift_dev[row] : (long long)shift_host;
    const long long m = s % (long long)L;
    return (unsigned)(m < 0 ? m + L : m);
}
__device__ __forceinline__ unsigned tdh_wrap(unsigned n, unsigned sh, unsigned L)
{
    const unsigned long long v = (unsigned long long)n + sh;
    return (unsigned)(v >= L ? v - L : v);
}

// grid (blocks, nmodes)
template <typename R>
__global__ void __launch_bounds__(TDH_T) tdh_split_kernel(const Cx<R> *__restrict__ E, unsigned L, TdhGeom g, double root, const int32_t *__restrict__ shift_dev,
                                                          int shift_host, Cx<R> *__restrict__ p1, Cx<R> *__restrict__ p2)
{
    const unsigned n = blockIdx.x * TDH_T + threadIdx.x;
    if (n >= L) return;
    const unsigned row = blockIdx.y, nframes = L / g.fM;
    const Cx<R> v = ldg(E + (size_t)row * L + tdh_wrap(n, tdh_shift(shift_dev, shift_host, row, L), L));
    const unsigned f = n / g.fM, p = n - f * g.fM;
    if (p < g.fM1) stg(p1 + (size_t)row * ((size_t)nframes * g.fM1) + (size_t)f * g.fM1 + p, v);
    else stg(p2 + (size_t)row * ((size_t)nframes * g.fM2) + (size_t)f * g.fM2 + (p - g.fM1), tdh_scaled(v, root));
}

// The symbols k = k0 + q TDH_T (q < TDH_S) of one format: fc positions per frame from position off on, decided against the M points of al (LDS,
// padded to a multiple of 4 with copies of point 0, which a strict comparison never picks); acc[0..3] take the four sums.
template <typename R>
__device__ __forceinline__ void tdh_format_pass(const Cx<R> *__restrict__ x, const int32_t *__restrict__ tx, unsigned L, unsigned sh, unsigned fM, unsigned fc,
                                                unsigned off, unsigned nsym, double scale, bool scaled, const Cx<R> *al, int M, double *acc)
{
    const int M4 = (M + 3) & ~3;
    const R inf = __builtin_inf();
    for (unsigned k0 = blockIdx.x * (unsigned)(TDH_T * TDH_S) + threadIdx.x; k0 < nsym; k0 += gridDim.x * (unsigned)(TDH_T * TDH_S)) {
        R pr[TDH_S], pi[TDH_S], best[TDH_S];
        int bi[TDH_S], lab[TDH_S];
#pragma unroll
        for (int q = 0; q < TDH_S; q++) {
            const unsigned k = k0 + (unsigned)q * TDH_T;
            Cx<R> v{(R)0, (R)0};
            lab[q] = -1;
            if (k < nsym) {
                const unsigned f = k / fc, n = f * fM + off + (k - f * fc);
                v = ldg(x + tdh_wrap(n, sh, L));
                if (scaled) v = tdh_scaled(v, scale);
                lab[q] = tx[n];
            }
            pr[q] = v.re; pi[q] = v.im;
            best[q] = inf; bi[q] = 0;
        }
        for (int j = 0; j < M4; j += 4) {
#pragma unroll
            for (int jj = 0; jj < 4; jj++) {
                const Cx<R> a = al[j + jj];
#pragma unroll
                for (int q = 0; q < TDH_S; q++) {
                    const R dr = pr[q] - a.re, di = pi[q] - a.im;
                    const R d = dr * dr + di * di;
                    if (d < best[q]) { best[q] = d; bi[q] = j + jj; }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < TDH_S; q++) {
            const int t = lab[q];
            if ((unsigned)t >= (unsigned)M) continue;            // no symbol here, or a label outside the alphabet
            const Cx<R> s = al[t];
            const R dr = pr[q] - s.re, di = pi[q] - s.im;
            acc[0] += bi[q] != t;
            acc[1] += __popc((unsigned)(bi[q] ^ t));
            acc[2] += 1;
            acc[3] += (double)(dr * dr + di * di);
        }
    }
}

// grid (blocks, nmodes): part[(row blocks + block) TDH_F + f]
template <typename R>
__global__ void __launch_bounds__(TDH_T) tdh_metrics_kernel(const Cx<R> *__restrict__ E, unsigned L, TdhGeom g, double root, const int32_t *__restrict__ shift_dev,
                                                            int shift_host, const int32_t *__restrict__ idx_tx, const Cx<R> *__restrict__ alphabet1, int M1,
                                                            const Cx<R> *__restrict__ alphabet2, int M2, double *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) Cx<R> al1[TDH_M_MAX], al2[TDH_M_MAX];
    __shared__ double wsum[TDH_T / 64][TDH_F];
    const unsigned row = blockIdx.y, t = threadIdx.x;
    for (int j = t; j < ((M1 + 3) & ~3); j += TDH_T) al1[j] = alphabet1[j < M1 ? j : 0];
    for (int j = t; j < ((M2 + 3) & ~3); j += TDH_T) al2[j] = alphabet2[j < M2 ? j : 0];
    __syncthreads();
    const unsigned nframes = L / g.fM, sh = tdh_shift(shift_dev, shift_host, row, L);
    const Cx<R> *x = E + (size_t)row * L;
    const int32_t *tx = idx_tx + (size_t)row * L;
    double acc[TDH_F];
#pragma unroll
    for (int f = 0; f < TDH_F; f++) acc[f] = 0.;
    tdh_format_pass<R>(x, tx, L, sh, g.fM, g.fM1, 0u, nframes * g.fM1, 1., false, al1, M1, acc);
    tdh_format_pass<R>(x, tx, L, sh, g.fM, g.fM2, g.fM1, nframes * g.fM2, root, true, al2, M2, acc + 4);
#pragma unroll
    for (int f = 0; f < TDH_F; f++) {
        const double v = wave_sum(acc[f]);
        if ((t & 63) == 0) wsum[t >> 6][f] = v;
    }
    __syncthreads();
    if (t < TDH_F) {
        double s = 0.;
        for (int w = 0; w < TDH_T / 64; w++) s += wsum[w][t];
        part[((size_t)row * gridDim.x + blockIdx.x) * TDH_F + t] = s;
    }
}

// grid (TDH_F, nmodes), one wave: out[row TDH_F + f] = the workgroups' partials of field f, lane j adds the blocks j, j + 64, .. in order
__global__ void __launch_bounds__(64) tdh_reduce_kernel(const double *__restrict__ part, int nblk, double *__restrict__ out)
{
    const int f = blockIdx.x;
    const double *p = part + (size_t)blockIdx.y * nblk * TDH_F + f;
    double s = 0.;
    for (int b = threadIdx.x; b < nblk; b += 64) s += p[(size_t)b * TDH_F];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[(size_t)blockIdx.y * TDH_F + f] = s;
}

// ------------------------------------------------------------------------------------------------ host side
static int tdh_geometry(const char *what, int nmodes, int64_t L, int fM, int fM1, TdhGeom *g)
{
    const std::string w(what);
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535, w + ": 1 <= nmodes <= 65535");
    QH_REQUIRE(fM >= 2 && fM <= TDH_FM_MAX, w + ": a frame of 2 .. 256 symbols");
    QH_REQUIRE(fM1 >= 1 && fM1 < fM, w + ": both formats need a place in the frame (1 <= fM1 < fM)");
    QH_REQUIRE(L >= fM && L <= TDH_LMAX, w + ": a row of at least one frame and at most 2^31 - 1 symbols");
    QH_REQUIRE(L % fM == 0, w + ": the row must hold whole frames (L % fM == 0)");
    *g = TdhGeom{(unsigned)fM, (unsigned)fM1, (unsigned)(fM - fM1)};
    return QH_OK;
}

static int tdh_powratio(const char *what, double powratio)
{
    QH_REQUIRE(std::isfinite(powratio) && powratio > 0, std::string(what) + ": powratio must be positive and finite");
    return QH_OK;
}

static unsigned tdh_blocks(int64_t L) { return (unsigned)((L + TDH_T - 1) / TDH_T); }

template <typename R>
int tdh_assemble_dev(const void *part1, const void *part2, const int32_t *lab1, const int32_t *lab2, int nmodes, int64_t nframes, int fM, int fM1,
                     double powratio, void *out, int32_t *idx_out)
{
    int rc;
    TdhGeom g;
    QH_REQUIRE(nframes >= 1 && nframes <= TDH_LMAX / TDH_FM_MAX, "tdh_assemble: nframes must be positive (and nframes * fM below 2^31)");
    if ((rc = tdh_geometry("tdh_assemble", nmodes, nframes * (int64_t)fM, fM, fM1, &g))) return rc;
    if ((rc = tdh_powratio("tdh_assemble", powratio))) return rc;
    QH_REQUIRE(part1 && part2 && out, "tdh_assemble: null pointer");
    QH_REQUIRE(out != part1 && out != part2, "tdh_assemble: out must not be one of the parts");
    QH_REQUIRE((idx_out != nullptr) == (lab1 != nullptr) && (lab1 != nullptr) == (lab2 != nullptr), "tdh_assemble: the label rows of both parts and idx_out come together");
    if ((rc = ensure_init())) return rc;
    hipLaunchKernelGGL((tdh_assemble_kernel<R>), dim3(tdh_blocks(nframes * fM), nmodes), dim3(TDH_T), 0, g_stream, (const Cx<R> *)part1, (const Cx<R> *)part2,
                       lab1, lab2, (unsigned)nframes, g, 1.0 / std::sqrt(powratio), (Cx<R> *)out, idx_out);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R> int tdh_class_sums_dev(const void *E, int nmodes, int64_t L, int fM, double *sums)
{
    int rc;
    TdhGeom g;
    if ((rc = tdh_geometry("tdh_class_sums", nmodes, L, fM, 1, &g))) return rc;
    QH_REQUIRE(E && sums, "tdh_class_sums: null pointer");
    if ((rc = ensure_init())) return rc;
    const int ntiles = (int)((L + TDH_TILE - 1) / TDH_TILE);
    void *part = nullptr;
    if ((rc = scratch(Slot::HYBRID, (size_t)nmodes * ntiles * fM * sizeof(double), &part))) return rc;
    hipLaunchKernelGGL((tdh_class_tile_kernel<R>), dim3(ntiles, nmodes), dim3(TDH_T), 0, g_stream, (const Cx<R> *)E, (unsigned)L, (unsigned)fM, (double *)part);
    QH_HIP(hipGetLastError());
    hipLaunchKernelGGL(tdh_class_combine_kernel, dim3(fM, nmodes), dim3(64), 0, g_stream, (const double *)part, ntiles, sums);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

static int tdh_align_dev(const double *sums, int nmodes, int fM, int fM1, int high_first, int32_t *shift)
{
    int rc;
    TdhGeom g;
    if ((rc = tdh_geometry("tdh_align", nmodes, fM, fM, fM1, &g))) return rc;
    QH_REQUIRE(sums && shift, "tdh_align: null pointer");
    if ((rc = ensure_init())) return rc;
    hipLaunchKernelGGL(tdh_align_kernel, dim3(nmodes), dim3(TDH_T), 0, g_stream, sums, fM, high_first ? 0 : fM1, high_first ? fM1 : fM, shift);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R>
int tdh_split_dev(const void *E, int nmodes, int64_t L, int fM, int fM1, double powratio, const int32_t *shift_dev, int shift_host, void *part1, void *part2)
{
    int rc;
    TdhGeom g;
    if ((rc = tdh_geometry("tdh_split", nmodes, L, fM, fM1, &g))) return rc;
    if ((rc = tdh_powratio("tdh_split", powratio))) return rc;
    QH_REQUIRE(E && part1 && part2, "tdh_split: null pointer");
    QH_REQUIRE(part1 != E && part2 != E && part1 != part2, "tdh_split: the parts must not be E (the gather is cyclic) nor each other");
    if ((rc = ensure_init())) return rc;
    hipLaunchKernelGGL((tdh_split_kernel<R>), dim3(tdh_blocks(L), nmodes), dim3(TDH_T), 0, g_stream, (const Cx<R> *)E, (unsigned)L, g, std::sqrt(powratio),
                       shift_dev, shift_host, (Cx<R> *)part1, (Cx<R> *)part2);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R>
int tdh_metrics_dev(const void *E, int nmodes, int64_t L, int fM, int fM1, double powratio, const int32_t *shift_dev, int shift_host, const int32_t *idx_tx,
                    const void *alphabet1, int M1, const void *alphabet2, int M2, double *sums)
{
    int rc;
    TdhGeom g;
    if ((rc = tdh_geometry("tdh_metrics", nmodes, L, fM, fM1, &g))) return rc;
    if ((rc = tdh_powratio("tdh_metrics", powratio))) return rc;
    QH_REQUIRE(E && idx_tx && alphabet1 && alphabet2 && sums, "tdh_metrics: null pointer");
    QH_REQUIRE(M1 >= 1 && M1 <= TDH_M_MAX && M2 >= 1 && M2 <= TDH_M_MAX, "tdh_metrics: alphabets of 1 .. 1024 points");
    if ((rc = ensure_init())) return rc;
    const int64_t most = (L / fM) * (int64_t)(g.fM1 > g.fM2 ? g.fM1 : g.fM2);
    int64_t nblk = (most + TDH_T * TDH_S - 1) / (TDH_T * TDH_S);
    if (nblk > TDH_MAXBLK) nblk = TDH_MAXBLK;
    void *part = nullptr;
    if ((rc = scratch(Slot::HYBRID, (size_t)nmodes * nblk * TDH_F * sizeof(double), &part))) return rc;
    hipLaunchKernelGGL((tdh_metrics_kernel<R>), dim3((unsigned)nblk, nmodes), dim3(TDH_T), 0, g_stream, (const Cx<R> *)E, (unsigned)L, g, std::sqrt(powratio),
                       shift_dev, shift_host, idx_tx, (const Cx<R> *)alphabet1, M1, (const Cx<R> *)alphabet2, M2, (double *)part);
    QH_HIP(hipGetLastError());
    hipLaunchKernelGGL(tdh_reduce_kernel, dim3(TDH_F, nmodes), dim3(64), 0, g_stream, (const double *)part, (int)nblk, sums);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

}  // namespace qh

extern "C" {
int qh_tdh_assemble_c64_dev(const void *part1, const void *part2, const int32_t *lab1, const int32_t *lab2, int nmodes, int64_t nframes, int fM, int fM1,
                            double powratio, void *out, int32_t *idx_out)
{ return qh::tdh_assemble_dev<float>(part1, part2, lab1, lab2, nmodes, nframes, fM, fM1, powratio, out, idx_out); }
int qh_tdh_assemble_c128_dev(const void *part1, const void *part2, const int32_t *lab1, const int32_t *lab2, int nmodes, int64_t nframes, int fM, int fM1,
                             double powratio, void *out, int32_t *idx_out)
{ return qh::tdh_assemble_dev<double>(part1, part2, lab1, lab2, nmodes, nframes, fM, fM1, powratio, out, idx_out); }
int qh_tdh_class_sums_c64_dev(const void *E, int nmodes, int64_t L, int fM, double *sums) { return qh::tdh_class_sums_dev<float>(E, nmodes, L, fM, sums); }
int qh_tdh_class_sums_c128_dev(const void *E, int nmodes, int64_t L, int fM, double *sums) { return qh::tdh_class_sums_dev<double>(E, nmodes, L, fM, sums); }
int qh_tdh_align_dev(const double *sums, int nmodes, int fM, int fM1, int high_first, int32_t *shift)
{ return qh::tdh_align_dev(sums, nmodes, fM, fM1, high_first, shift); }
int qh_tdh_split_c64_dev(const void *E, int nmodes, int64_t L, int fM, int fM1, double powratio, const int32_t *shift_dev, int shift_host, void *part1,
                         void *part2)
{ return qh::tdh_split_dev<float>(E, nmodes, L, fM, fM1, powratio, shift_dev, shift_host, part1, part2); }
int qh_tdh_split_c128_dev(const void *E, int nmodes, int64_t L, int fM, int fM1, double powratio, const int32_t *shift_dev, int shift_host, void *part1,
                          void *part2)
{ return qh::tdh_split_dev<double>(E, nmodes, L, fM, fM1, powratio, shift_dev, shift_host, part1, part2); }
int qh_tdh_metrics_c64_dev(const void *E, int nmodes, int64_t L, int fM, int fM1, double powratio, const int32_t *shift_dev, int shift_host,
                           const int32_t *idx_tx, const void *alphabet1, int M1, const void *alphabet2, int M2, double *sums)
{ return qh::tdh_metrics_dev<float>(E, nmodes, L, fM, fM1, powratio, shift_dev, shift_host, idx_tx, alphabet1, M1, alphabet2, M2, sums); }
int qh_tdh_metrics_c128_dev(const void *E, int nmodes, int64_t L, int fM, int fM1, double powratio, const int32_t *shift_dev, int shift_host,
                            const int32_t *idx_tx, const void *alphabet1, int M1, const void *alphabet2, int M2, double *sums)
{ return qh::tdh_metrics_dev<double>(E, nmodes, L, fM, fM1, powratio, shift_dev, shift_host, idx_tx, alphabet1, M1, alphabet2, M2, sums); }
}
