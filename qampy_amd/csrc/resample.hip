// Rational polyphase FIR resampling of every row of an (nmodes, L) array, and the per-row renormalisation that goes with it
// (qampy/core/resample.py:37-127 resample_poly / rrcos_resample, qampy/core/filter.py:177-212 rrcos_pulseshaping).
//
//   y[k] = g * sum_m h[k down + half - m up] x[m],   half = (T - 1) / 2,   x zero outside [0, L),   k = 0 .. Lout - 1
//
// in polyphase form:  p = (k down + half) % up,  m0 = (k down + half) / up,  y[k] = g sum_{j < J} h[p + j up] x[m0 - j],  J = ceil(T / up).
// g = up is scipy's resample_poly(window = h), g = 1 the zero-insertion / fftconvolve('same') / decimation path, up = down = 1 a plain
// 'same' convolution.  Real taps, given in double on the host, cast to the signal's precision; accumulation in that precision by FMA,
// j ascending, every output on its own: no atomics, bit-identical from call to call.
//
// Supported: 1 <= up, down <= 64, 1 <= ntaps <= 8191, 1 <= nmodes <= 65535, Lout <= ceil(L up / down), out another buffer than E.
//
// Layout.  The host reorders the taps phase-major, tab[p][j] = h[p + j up] (zero-padded to J), and uploads the table once per distinct
// (taps, up, precision) into scratch slot Slot::RESAMPLE_TABLE; the taps are part of the table's key.  A workgroup owns a tile of
// up * G * 4 consecutive outputs of one row.  Thread (i, g), i = t % up the fast index, keeps the 4 outputs k = K0 + (r G + g) up + i,
// r = 0 .. 3, in registers: they share the phase p, so one coefficient read feeds 4 complex FMAs, their inputs lie r G down samples apart,
// and for each r a wave stores a contiguous run of outputs.  The sum over j runs in chunks of JC taps per phase; for each chunk the
// workgroup stages in LDS
//   ts[p][jj]  the slice tab[p][jc + jj] of the phase table, rows of JC + 1 words (odd: lanes of different p on different banks; lanes
//              of the same p read one address, a broadcast),
//   xs[u]      the input samples m0(K0) - jc - JC + 1 + u, u < G 4 down + JC + 1: the tile's span with a halo of JC samples, zeros
//              where the row ends, so the inner loop has no bounds test.  Lanes i, i + 1 of one g read samples about down / up
//              apart, lanes of successive g samples `down` apart (the layout follows the sample index, so it cannot be padded
//              per lane; bank conflicts of these reads have not been counted).
// G = min(256 / up, 2048 / (4 down)) (at least 1) and JC = min(J rounded up to 4, 1024, 4096 / up rounded down to 4) keep a workgroup
// within 41 KiB (complex64) / 82 KiB (complex128) of LDS, so the whole supported range runs in one form.
//
// What bounds it: every FMA pair needs its own input sample from LDS (one ds_read_b64 of a complex64 per two fp32 FMAs), so a long
// filter runs at the LDS read rate, about a quarter of the fp32 FMA rate; a short one (J of a few tens) at the HBM rate of reading L
// and writing Lout samples per row.  DESIGN.md 3.8 has the measured times beside both floors.
//
// Renormalisation (the reference's renormalise=True: normalise_and_center(out) * sqrt(mean |in|^2)), without the host:
//   row_moments   mean re, mean im, mean |.|^2 of every row, accumulated in double: RM_NB partial sums per row in a fixed order (scratch
//                 slot Slot::ROW_MOMENTS), then one wave per row adds them, again in a fixed order.  3 doubles per row in device memory.
//   center_scale  x <- (x - mean) sqrt(P / (mean |x|^2 - |mean|^2)) in place, the moments read from device memory; P is the mean
//                 |.|^2 of a second moments buffer (the input's), or a given target power when that pointer is NULL.
#include "common.h"
#include <cmath>

namespace qh {

constexpr int RS_MAXF = 64, RS_MAXTAPS = 8191;      // caps of up / down and of ntaps
constexpr int RS_T = 256;                           // most threads of a workgroup
constexpr int RS_R = 4;                             // outputs of one phase per thread
constexpr int RS_XSPAN = 2048;                      // most input samples a tile spans (less halo)
constexpr int RS_JCMAX = 1024, RS_TABMAX = 4096;    // most taps per phase and most table words staged at a time

// grid (tiles, nmodes), up * G threads rounded up to whole waves
template <typename R>
__global__ void __launch_bounds__(RS_T) resample_kernel(const Cx<R> *__restrict__ E, Cx<R> *__restrict__ out, int64_t L, int64_t Lout,
                                                        const R *__restrict__ tab, int up, int down, int half, int J, int JC, int G, R gain)
{
    extern __shared__ __attribute__((aligned(16))) char smem_rs[];
    const int JCP = JC + 1, XW = G * RS_R * down + JC + 1;
    Cx<R> *xs = reinterpret_cast<Cx<R> *>(smem_rs);
    R *ts = reinterpret_cast<R *>(xs + XW);
    const int t = threadIdx.x, nthr = blockDim.x;
    const Cx<R> *x = E + (size_t)blockIdx.y * L;
    Cx<R> *y = out + (size_t)blockIdx.y * Lout;
    const int64_t K0 = (int64_t)blockIdx.x * ((int64_t)up * G * RS_R);
    const int64_t M0 = (K0 * down + half) / up;                    // m0 of the tile's first output
    const bool active = t < up * G;
    const int i = t % up, g = t / up;
    const int64_t k0 = K0 + (int64_t)g * up + i;
    const int64_t a0 = k0 * down + half;
    const int p = (int)(a0 % up);
    const int b0 = active ? (int)(a0 / up - M0) + JC - 1 : JC - 1;   // xs index of x[m0] at jj = 0, r = 0
    const R *trow = ts + (active ? p : 0) * JCP;
    const int rstep = G * down;
    Cx<R> acc[RS_R];
#pragma unroll
    for (int r = 0; r < RS_R; r++) acc[r] = Cx<R>{(R)0, (R)0};
    const Cx<R> zero{(R)0, (R)0};

    for (int jc = 0; jc < J; jc += JC) {
        if (jc) __syncthreads();
        for (int e = t; e < up * JC; e += nthr) {
            const int pp = e / JC, jj = e - pp * JC;
            ts[pp * JCP + jj] = jc + jj < J ? tab[(size_t)pp * J + jc + jj] : (R)0;
        }
        const int64_t mb = M0 - jc - JC + 1;
        for (int u = t; u < XW; u += nthr) {
            const int64_t m = mb + u;
            xs[u] = (m >= 0 && m < L) ? ldg(x + m) : zero;
        }
        __syncthreads();
        if (active) {
            for (int jj = 0; jj < JC; jj += 4) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const R c = trow[jj + q];
#pragma unroll
                    for (int r = 0; r < RS_R; r++) {
                        const Cx<R> v = xs[b0 + r * rstep - jj - q];
                        acc[r].re = fma_(c, v.re, acc[r].re);
                        acc[r].im = fma_(c, v.im, acc[r].im);
                    }
                }
            }
        }
    }
    if (active) {
#pragma unroll
        for (int r = 0; r < RS_R; r++) {
            const int64_t k = k0 + (int64_t)r * G * up;
            if (k < Lout) stg(y + k, Cx<R>{gain * acc[r].re, gain * acc[r].im});
        }
    }
}

// ------------------------------------------------------------------------------------------------ per-row moments, centre and scale
constexpr int RM_NB = 128, RM_T = 256;             // partial sums per row; threads per workgroup

// grid (nb, nmodes): partial sums of re, im, |.|^2 over the slice [b chunk, (b + 1) chunk) of a row -> part[(row nb + b) 3 + c]
template <typename R>
__global__ void __launch_bounds__(RM_T) row_moments_part_kernel(const Cx<R> *__restrict__ E, int64_t L, int64_t chunk, double *__restrict__ part)
{
    __shared__ double red[3][RM_T / 64];
    const Cx<R> *x = E + (size_t)blockIdx.y * L;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < L ? lo + chunk : L;
    double sr = 0, si = 0, sq = 0;
    for (int64_t m = lo + threadIdx.x; m < hi; m += RM_T) {
        const Cx<R> v = ldg(x + m);
        const double a = (double)v.re, b = (double)v.im;
        sr += a; si += b; sq = fma_(a, a, fma_(b, b, sq));
    }
    sr = wave_sum(sr); si = wave_sum(si); sq = wave_sum(sq);
    const int w = threadIdx.x / 64;
    if (threadIdx.x % 64 == 0) { red[0][w] = sr; red[1][w] = si; red[2][w] = sq; }
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = 0;
        for (int q = 0; q < RM_T / 64; q++) s += red[threadIdx.x][q];
        part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3 + threadIdx.x] = s;
    }
}

// grid (nmodes), one wave: mom[row 3 + c] = (sum of the row's nb partial sums) / L
__global__ void __launch_bounds__(64) row_moments_final_kernel(const double *__restrict__ part, int nb, int64_t L, double *__restrict__ mom)
{
    const double *pr = part + (size_t)blockIdx.x * nb * 3;
    double s[3] = {0, 0, 0};
    for (int b = threadIdx.x; b < nb; b += 64)
        for (int c = 0; c < 3; c++) s[c] += pr[b * 3 + c];
    for (int c = 0; c < 3; c++) s[c] = wave_sum(s[c]);
    if (threadIdx.x < 3) mom[(size_t)blockIdx.x * 3 + threadIdx.x] = (threadIdx.x == 0 ? s[0] : threadIdx.x == 1 ? s[1] : s[2]) / (double)L;
}

// grid (blocks, nmodes)
template <typename R>
__global__ void __launch_bounds__(RM_T) center_scale_kernel(Cx<R> *__restrict__ X, int64_t L, const double *__restrict__ mom,
                                                            const double *__restrict__ mom_in, double target)
{
    const int row = blockIdx.y;
    const double mr = mom[row * 3], mi = mom[row * 3 + 1];
    const double var = mom[row * 3 + 2] - (mr * mr + mi * mi);
    const double P = mom_in ? mom_in[row * 3 + 2] : target;
    const double s = sqrt(P / var);
    Cx<R> *x = X + (size_t)row * L;
    for (int64_t m = (int64_t)blockIdx.x * RM_T + threadIdx.x; m < L; m += (int64_t)gridDim.x * RM_T) {
        const Cx<R> v = ldg(x + m);
        stg(x + m, Cx<R>{(R)(((double)v.re - mr) * s), (R)(((double)v.im - mi) * s)});
    }
}

// ------------------------------------------------------------------------------------------------ host side
static thread_local TableCache g_rs;

template <typename R> static int rs_table(const double *h, int ntaps, int up, int J, const R **tab)
{
    std::string key;
    key_add(key, up);
    key_add(key, (int)sizeof(R));
    key.append(reinterpret_cast<const char *>(h), (size_t)ntaps * sizeof(double));
    return g_rs.get(Slot::RESAMPLE_TABLE, key, (size_t)up * J * sizeof(R), [=](char *host) {
        R *pm = reinterpret_cast<R *>(host);
        for (int ph = 0; ph < up; ph++)
            for (int j = 0; j < J; j++) {
                const int idx = ph + j * up;
                pm[(size_t)ph * J + j] = idx < ntaps ? (R)h[idx] : (R)0;
            }
    }, (const void **)tab);
}

static int rs_check(int nmodes, int64_t L, const double *h, int ntaps, int up, int down, double gain, int64_t Lout)
{
    QH_REQUIRE(up >= 1 && up <= RS_MAXF && down >= 1 && down <= RS_MAXF, "resample: up and down must be from 1 to 64");
    QH_REQUIRE(ntaps >= 1 && ntaps <= RS_MAXTAPS && h, "resample: ntaps must be from 1 to 8191");
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 0 && L <= (int64_t)1 << 48, "resample: bad sizes");
    QH_REQUIRE(std::isfinite(gain), "resample: gain must be finite");
    QH_REQUIRE(Lout >= 0 && Lout <= (L * up + down - 1) / down, "resample: Lout is longer than ceil(L up / down)");
    return QH_OK;
}

template <typename R>
int resample_dev(const void *E, int nmodes, int64_t L, const double *h, int ntaps, int up, int down, double gain, int64_t Lout, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    if ((rc = rs_check(nmodes, L, h, ntaps, up, down, gain, Lout))) return rc;
    QH_REQUIRE(E && out && E != out, "resample: out must be a buffer other than E");
    if (Lout == 0) return QH_OK;
    const int J = (ntaps + up - 1) / up;
    int G = RS_T / up;
    const int gx = RS_XSPAN / (RS_R * down);
    if (G > gx) G = gx;
    if (G < 1) G = 1;
    int JC = (J + 3) & ~3;
    if (JC > RS_JCMAX) JC = RS_JCMAX;
    if (JC > ((RS_TABMAX / up) & ~3)) JC = (RS_TABMAX / up) & ~3;
    const int64_t tile = (int64_t)up * G * RS_R, ntiles = (Lout + tile - 1) / tile;
    QH_REQUIRE(ntiles <= 0x7fffffffLL, "resample: Lout too long");
    const R *tab;
    if ((rc = rs_table<R>(h, ntaps, up, J, &tab))) return rc;
    const size_t lds = (size_t)(G * RS_R * down + JC + 1) * sizeof(Cx<R>) + (size_t)up * (JC + 1) * sizeof(R);
    if ((rc = dyn_lds(resample_kernel<R>, lds))) return rc;
    const int nthr = (up * G + 63) / 64 * 64;
    hipLaunchKernelGGL((resample_kernel<R>), dim3((unsigned)ntiles, nmodes), dim3(nthr), lds, g_stream, (const Cx<R> *)E, (Cx<R> *)out, L, Lout,
                       tab, up, down, (ntaps - 1) / 2, J, JC, G, (R)gain);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R>
int resample_host(const void *E, int nmodes, int64_t L, const double *h, int ntaps, int up, int down, double gain, int64_t Lout, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    if ((rc = rs_check(nmodes, L, h, ntaps, up, down, gain, Lout))) return rc;
    QH_REQUIRE(E && out && E != out, "resample: out must be a buffer other than E");
    if (Lout == 0) return QH_OK;
    DevBuf dE, dout;
    if ((rc = dE.from_host(E, (size_t)nmodes * L * sizeof(Cx<R>)))) return rc;
    if ((rc = dout.alloc((size_t)nmodes * Lout * sizeof(Cx<R>)))) return rc;
    if ((rc = resample_dev<R>(dE.p, nmodes, L, h, ntaps, up, down, gain, Lout, dout.p))) return rc;
    if ((rc = dout.to_host(out, dout.n))) return rc;
    QH_HIP(hipStreamSynchronize(g_stream));
    return QH_OK;
}

template <typename R> int row_moments_dev(const void *E, int nmodes, int64_t L, double *mom)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(E && mom && nmodes >= 1 && nmodes <= 65535 && L >= 1, "row_moments: bad arguments");
    int64_t chunk = (L + RM_NB - 1) / RM_NB;
    if (chunk < RM_T) chunk = RM_T;
    const int nb = (int)((L + chunk - 1) / chunk);
    void *part = nullptr;
    if ((rc = scratch(Slot::ROW_MOMENTS, (size_t)nmodes * nb * 3 * sizeof(double), &part))) return rc;
    hipLaunchKernelGGL((row_moments_part_kernel<R>), dim3(nb, nmodes), dim3(RM_T), 0, g_stream, (const Cx<R> *)E, L, chunk, (double *)part);
    QH_HIP(hipGetLastError());
    hipLaunchKernelGGL(row_moments_final_kernel, dim3(nmodes), dim3(64), 0, g_stream, (const double *)part, nb, L, mom);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R> int center_scale_dev(void *X, int nmodes, int64_t L, const double *mom, const double *mom_in, double target)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(X && mom && nmodes >= 1 && nmodes <= 65535 && L >= 1, "center_scale: bad arguments");
    QH_REQUIRE(mom_in || (std::isfinite(target) && target >= 0), "center_scale: the target power must be finite and not negative");
    int64_t nblk = (L + RM_T * 8 - 1) / (RM_T * 8);
    if (nblk > 4096) nblk = 4096;
    hipLaunchKernelGGL((center_scale_kernel<R>), dim3((unsigned)nblk, nmodes), dim3(RM_T), 0, g_stream, (Cx<R> *)X, L, mom, mom_in, target);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

}  // namespace qh

extern "C" {
int qh_resample_c64(const void *E, int nmodes, int64_t L, const double *h, int ntaps, int up, int down, double gain, int64_t Lout, void *out)
{ return qh::resample_host<float>(E, nmodes, L, h, ntaps, up, down, gain, Lout, out); }
int qh_resample_c128(const void *E, int nmodes, int64_t L, const double *h, int ntaps, int up, int down, double gain, int64_t Lout, void *out)
{ return qh::resample_host<double>(E, nmodes, L, h, ntaps, up, down, gain, Lout, out); }
int qh_resample_c64_dev(const void *E, int nmodes, int64_t L, const double *h, int ntaps, int up, int down, double gain, int64_t Lout, void *out)
{ return qh::resample_dev<float>(E, nmodes, L, h, ntaps, up, down, gain, Lout, out); }
int qh_resample_c128_dev(const void *E, int nmodes, int64_t L, const double *h, int ntaps, int up, int down, double gain, int64_t Lout, void *out)
{ return qh::resample_dev<double>(E, nmodes, L, h, ntaps, up, down, gain, Lout, out); }
int qh_row_moments_c64_dev(const void *E, int nmodes, int64_t L, double *mom) { return qh::row_moments_dev<float>(E, nmodes, L, mom); }
int qh_row_moments_c128_dev(const void *E, int nmodes, int64_t L, double *mom) { return qh::row_moments_dev<double>(E, nmodes, L, mom); }
int qh_center_scale_c64_dev(void *X, int nmodes, int64_t L, const double *mom, const double *mom_in, double target)
{ return qh::center_scale_dev<float>(X, nmodes, L, mom, mom_in, target); }
int qh_center_scale_c128_dev(void *X, int nmodes, int64_t L, const double *mom, const double *mom_in, double target)
{ return qh::center_scale_dev<double>(X, nmodes, L, mom, mom_in, target); }
}
