// Nonlinear fibre on a field that already lies in HBM: symmetric split-step Fourier propagation of the (Manakov) nonlinear Schroedinger
// equation over `nspans` identical amplified spans, and its algebraic inverse, digital back-propagation.
//
// A span is a list of step lengths dz[0 .. n - 1] (metres).  With f = fftfreq(L, 1 / fs), kappa = 1 (one row) or 8 / 9 (two rows):
//
//   D(h)   every row becomes ifft(exp(-2 pi i t) . fft(row)), t = pi beta2 h f^2 turns, formed and reduced modulo one in double
//   N(h)   P[n] = sum_m |E[m, n]|^2, phi[n] = kappa gamma pscale h_eff P[n], h_eff = (1 - exp(-alpha h)) / alpha (h when alpha == 0),
//          E[m, n] <- a exp(+j phi[n]) E[m, n], a = exp(-alpha h / 2)
//   span   D(dz[0] / 2), then for i = 0 .. n - 1: N(dz[i]), D(dz[i] / 2 + dz[i + 1] / 2) (the last one D(dz[n - 1] / 2)): n point-wise
//          launches and n + 1 filters; half steps are merged inside a span, never across spans.
//   amplify   the last N of a span also multiplies by exp(+alpha span / 2), the lumped amplifier, folded into a.
//   noise     (ase_w > 0, forward only) that launch then adds sigma w[m, n], sigma^2 = ase_w / pscale, w the unit draw of impair.hip's
//             point-wise pass (philox.h imp_gauss, stream 2) under the key seed + s for span s.
//   pscale    watts per unit of |E|^2, fixed once at the start of the call and kept on the device: given, or P / sum_m mean_n |E[m, n]|^2 for a
//             launch power P over all rows (two launches: partials, then the total; double, fixed order, no atomics).
//   backward  the step list reversed, beta2, gamma and alpha negated; with amplify the factor exp(-alpha span / 2) goes in front of the first N of
//             a span, before its power is taken.  That is the exact inverse of the noise-free forward call with the same arguments.
//
// Everything N(h) needs folds into two scalars, so one kernel serves every case: E <- a' exp(j c pscale P) E with a' = a (times the lumped
// factor) and c = +-kappa gamma h_eff (times the lumped factor squared, backward).  The filters are qh_spectral_filter_*_dev with a complex table
// (kind 6): fft.hip applies the table as its inverse transform loads the spectrum.  A table exp(-2 pi i t) is formed on the device for one length h;
// two tables live in the slot and one is formed again only when the length it is for changes (least recently used goes), so a span of equal steps
// forms two tables per call, h / 2 and h.
//
// Scratch slot Slot::FIBRE: power partials | pscale | table 0 (L) | table 1 (L).  The whole loop over spans and steps is enqueued on the current
// stream by the host; nothing is read back; no atomics: a repeated call is bit-identical.  out may be E: the first filter reads E and writes
// out, everything after it works on out in place, and a thread of the point-wise kernel reads the samples it writes.
#include "common.h"
#include "philox.h"
#include <cmath>

namespace qh {

constexpr int FIB_T = 256, FIB_U = 4;          // a thread handles FIB_U groups of V neighbouring sample positions, FIB_T V apart (coalesced)
constexpr int FIB_MAX = 4096;                  // most steps per span, most spans

// the lengths fft.hip transforms (its fft_length_ok)
static bool fibre_length_ok(int64_t L)
{
    if (L < 2) return false;
    if ((L & (L - 1)) == 0 && L >= 256) return L <= ((int64_t)1 << 24);
    return L <= ((int64_t)1 << 23);
}

// V neighbouring samples of one row as one load / store: 16 bytes per lane with V = 2 (complex64) or V = 1 (complex128); V = 1 in complex64 is
// the 8-byte form for rows that are not 16-byte aligned (odd L, or an odd offset of the caller's pointers)
template <typename R, int V> __device__ __forceinline__ void fib_load(const Cx<R> *p, Cx<R> (&x)[V])
{
    if constexpr (V == 2) {
        const float4 v = *reinterpret_cast<const float4 *>(p);
        x[0] = Cx<R>{v.x, v.y}; x[1] = Cx<R>{v.z, v.w};
    } else {
        x[0] = ldg(p);
    }
}
template <typename R, int V> __device__ __forceinline__ void fib_store(Cx<R> *p, const Cx<R> (&x)[V])
{
    if constexpr (V == 2) {
        float4 v; v.x = x[0].re; v.y = x[0].im; v.z = x[1].re; v.w = x[1].im;
        *reinterpret_cast<float4 *>(p) = v;
    } else {
        stg(p, x[0]);
    }
}

// The nonlinear step, grid (ceil(L / (FIB_T FIB_U V))): out[m, n] = a exp(j coef pscale P[n]) E[m, n] (+ sigma w[m, n]), P[n] = sum_m |E[m, n]|^2.
// All NM rows of a sample position belong to one thread: one power, one sine and cosine.  sigma = sigma_w / sqrt(pscale), sigma_w = sqrt(ase_w).
// NOISE is a template parameter: the launches without noise carry no trace of it.  out == E is allowed.
template <typename R, int NM, bool NOISE, int V>
__global__ void __launch_bounds__(FIB_T) fibre_nl_kernel(const Cx<R> *E, Cx<R> *out, int64_t L, R a, double coef, const double *__restrict__ pscale,
                                                         double sigma_w, unsigned k0, unsigned k1)
{
    const double ps = pscale[0];
    const R c = (R)(coef * ps);
    const R sg = NOISE ? (R)(sigma_w / sqrt(ps)) : (R)0;
    const R s_iq = (R)0.70710678118654752440;                              // the unit draw of impair_pointwise_kernel: sigma = 1 split over I and Q
    const int64_t n0 = ((int64_t)blockIdx.x * (FIB_T * FIB_U) + threadIdx.x) * V;
    Cx<R> x[FIB_U][NM][V];
#pragma unroll
    for (int u = 0; u < FIB_U; u++) {
        const int64_t n = n0 + (int64_t)u * (FIB_T * V);
        if (n < L) {                                                       // V == 2 only with even L: n + 1 < L too
#pragma unroll
            for (int m = 0; m < NM; m++) fib_load<R, V>(E + (size_t)m * L + n, x[u][m]);
        }
    }
#pragma unroll
    for (int u = 0; u < FIB_U; u++) {
        const int64_t n = n0 + (int64_t)u * (FIB_T * V);
        if (n >= L) break;
#pragma unroll
        for (int v = 0; v < V; v++) {
            R P = (R)0;
#pragma unroll
            for (int m = 0; m < NM; m++) P = fma_(x[u][m][v].re, x[u][m][v].re, fma_(x[u][m][v].im, x[u][m][v].im, P));
            R sn, cs;
            sincos_<R>(c * P, &sn, &cs);                                   // accurate for any argument: no reduction of its own needed
            const R rr = a * cs, ri = a * sn;
#pragma unroll
            for (int m = 0; m < NM; m++) {
                const Cx<R> e = x[u][m][v];
                Cx<R> y{e.re * rr - e.im * ri, e.re * ri + e.im * rr};
                if constexpr (NOISE) {
                    R g0, g1;
                    imp_gauss(n + v, m, IMP_STREAM_NOISE, k0, k1, g0, g1);
                    y = Cx<R>{fma_(sg, s_iq * g0, y.re), fma_(sg, s_iq * g1, y.im)};
                }
                x[u][m][v] = y;
            }
        }
#pragma unroll
        for (int m = 0; m < NM; m++) fib_store<R, V>(out + (size_t)m * L + n, x[u][m]);
    }
}

// tab[k] = exp(-2 pi i t), t = c f^2 with f = kk df, kk numpy's fftfreq numerator; c = pi beta2 h.  Double throughout, cast at the store.
template <typename R> __global__ void __launch_bounds__(FIB_T) fibre_table_kernel(Cx<R> *__restrict__ tab, int64_t L, double df, double c)
{
    const int64_t k = (int64_t)blockIdx.x * FIB_T + threadIdx.x;
    if (k >= L) return;
    const int64_t kk = k < (L - 1) / 2 + 1 ? k : k - L;
    const double f = (double)kk * df;
    double t = c * (f * f);
    t -= rint(t);
    double sn, cs;
    sincospi(-2.0 * t, &sn, &cs);
    stg(tab + k, Cx<R>{(R)cs, (R)sn});
}

// pscale, launch 1, grid (nb): part[b] = the sum of |E|^2 over every row of the block's FIB_T FIB_U sample positions, terms and sums in double
template <typename R>
__global__ void __launch_bounds__(FIB_T) fibre_power_kernel(const Cx<R> *__restrict__ E, int nmodes, int64_t L, double *__restrict__ part)
{
    __shared__ double red[FIB_T / 64];
    double q = 0;
    for (int u = 0; u < FIB_U; u++) {
        const int64_t n = (int64_t)blockIdx.x * (FIB_T * FIB_U) + u * FIB_T + threadIdx.x;
        if (n >= L) break;
        for (int m = 0; m < nmodes; m++) {
            const Cx<R> v = ldg(E + (size_t)m * L + n);
            q = fma_((double)v.re, (double)v.re, fma_((double)v.im, (double)v.im, q));
        }
    }
    q = block_sum<FIB_T>(q, red);
    if (threadIdx.x == 0) part[blockIdx.x] = q;
}

// pscale, launch 2, one workgroup: pscale = power / (sum_m mean_n |E[m, n]|^2) from the partials in a fixed order (derive != 0), or power itself
__global__ void __launch_bounds__(FIB_T) fibre_pscale_kernel(const double *__restrict__ part, int64_t nb, int64_t L, int derive, double power,
                                                             double *__restrict__ pscale)
{
    __shared__ double red[FIB_T / 64];
    double s = 0;
    if (derive)
        for (int64_t i = threadIdx.x; i < nb; i += FIB_T) s += part[i];
    s = block_sum<FIB_T>(s, red);
    if (threadIdx.x == 0) pscale[0] = derive ? power / (s / (double)L) : power;
}

// ------------------------------------------------------------------------------------------------ host side
static int fibre_filter(float, const void *E, int nm, int64_t L, const void *H, void *out) { return qh_spectral_filter_c64_dev(E, nm, L, 6, 0, 0, 0, 0, 0, H, out); }
static int fibre_filter(double, const void *E, int nm, int64_t L, const void *H, void *out) { return qh_spectral_filter_c128_dev(E, nm, L, 6, 0, 0, 0, 0, 0, H, out); }

template <typename R, int NM, bool NOISE, int V>
static void fibre_nl_launch(const Cx<R> *E, Cx<R> *out, int64_t L, double a, double coef, const double *pscale, double sigma_w, uint64_t seed)
{
    const int64_t per = (int64_t)FIB_T * FIB_U * V;
    hipLaunchKernelGGL((fibre_nl_kernel<R, NM, NOISE, V>), dim3((unsigned)((L + per - 1) / per)), dim3(FIB_T), 0, g_stream, E, out, L, (R)a, coef, pscale,
                       sigma_w, (unsigned)seed, (unsigned)(seed >> 32));
}

template <typename R> static int fibre_nl(const Cx<R> *E, Cx<R> *out, int nm, int64_t L, double a, double coef, const double *pscale, bool noise, double sigma_w, uint64_t seed)
{
    // 16 bytes per lane: complex128 always; complex64 two samples at a time when every row starts on 16 bytes
    if constexpr (sizeof(R) == 4) {
        if ((L & 1) == 0 && (((uintptr_t)E | (uintptr_t)out) & 15) == 0) {
            if (nm == 1) noise ? fibre_nl_launch<R, 1, true, 2>(E, out, L, a, coef, pscale, sigma_w, seed) : fibre_nl_launch<R, 1, false, 2>(E, out, L, a, coef, pscale, sigma_w, seed);
            else noise ? fibre_nl_launch<R, 2, true, 2>(E, out, L, a, coef, pscale, sigma_w, seed) : fibre_nl_launch<R, 2, false, 2>(E, out, L, a, coef, pscale, sigma_w, seed);
            QH_HIP(hipGetLastError());
            return QH_OK;
        }
    }
    if (nm == 1) noise ? fibre_nl_launch<R, 1, true, 1>(E, out, L, a, coef, pscale, sigma_w, seed) : fibre_nl_launch<R, 1, false, 1>(E, out, L, a, coef, pscale, sigma_w, seed);
    else noise ? fibre_nl_launch<R, 2, true, 1>(E, out, L, a, coef, pscale, sigma_w, seed) : fibre_nl_launch<R, 2, false, 1>(E, out, L, a, coef, pscale, sigma_w, seed);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

// the two dispersion tables of a call: which length each holds and which was used last
template <typename R> struct FibreTables {
    Cx<R> *tab[2] = {nullptr, nullptr};
    double h[2] = {0, 0};
    bool full[2] = {false, false};
    int last = 1;
    int64_t L = 0;
    double df = 0, b2 = 0;
    // the table for length h; formed (one launch) unless one of the two holds it
    int get(double hh, const Cx<R> **t)
    {
        for (int i = 0; i < 2; i++)
            if (full[i] && h[i] == hh) { last = i; *t = tab[i]; return QH_OK; }
        const int i = !full[0] ? 0 : (!full[1] ? 1 : 1 - last);
        hipLaunchKernelGGL((fibre_table_kernel<R>), dim3((unsigned)((L + FIB_T - 1) / FIB_T)), dim3(FIB_T), 0, g_stream, tab[i], L, df, QH_PI * b2 * hh);
        QH_HIP(hipGetLastError());
        full[i] = true; h[i] = hh; last = i; *t = tab[i];
        return QH_OK;
    }
};

template <typename R>
int fibre_ssfm_dev(const void *E, int nmodes, int64_t L, double fs, double beta2, double gamma, double alpha, const double *dz, int nsteps, int nspans,
                   int backward, int amplify, int power_mode, double power, double ase_w, uint64_t seed, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nmodes == 1 || nmodes == 2, "fibre_ssfm: one row, or two (Manakov)");
    QH_REQUIRE(fibre_length_ok(L), "fibre_ssfm: L must be a power of two from 2^8 to 2^24, or any other length from 2 to 2^23");
    QH_REQUIRE(E && out && dz, "fibre_ssfm: E, out and the step lengths must be given");
    QH_REQUIRE(nsteps >= 1 && nsteps <= FIB_MAX && nspans >= 1 && nspans <= FIB_MAX, "fibre_ssfm: 1 to 4096 steps per span, 1 to 4096 spans");
    QH_REQUIRE(std::isfinite(fs) && fs > 0 && std::isfinite(beta2) && std::isfinite(gamma) && std::isfinite(alpha), "fibre_ssfm: fs must be positive, beta2, gamma and alpha finite");
    double span = 0;
    for (int i = 0; i < nsteps; i++) {
        QH_REQUIRE(std::isfinite(dz[i]) && dz[i] > 0, "fibre_ssfm: every step length must be finite and positive");
        span += dz[i];
    }
    QH_REQUIRE(power_mode == 0 || power_mode == 1, "fibre_ssfm: power_mode is 0 (power is pscale) or 1 (power is the launch power in watts)");
    QH_REQUIRE(std::isfinite(power) && power > 0, "fibre_ssfm: the power must be finite and positive");
    QH_REQUIRE(std::isfinite(ase_w) && ase_w >= 0, "fibre_ssfm: the amplifier noise power must be finite and not negative");
    QH_REQUIRE(!(backward && ase_w != 0), "fibre_ssfm: back-propagation adds no amplifier noise");
    QH_REQUIRE(std::isfinite(exp(fabs(alpha) * span)), "fibre_ssfm: the loss of a span overflows");

    const int64_t nb = (L + FIB_T * FIB_U - 1) / (FIB_T * FIB_U);
    ScratchLayout lay;
    const size_t o_part = lay.take((size_t)nb * sizeof(double)), o_ps = lay.take(sizeof(double)), o_t0 = lay.take((size_t)L * sizeof(Cx<R>)),
                 o_t1 = lay.take((size_t)L * sizeof(Cx<R>));
    void *base = nullptr;
    if ((rc = scratch(Slot::FIBRE, lay.total, &base))) return rc;
    double *part = (double *)((char *)base + o_part), *pscale = (double *)((char *)base + o_ps);
    FibreTables<R> tabs;
    tabs.tab[0] = (Cx<R> *)((char *)base + o_t0); tabs.tab[1] = (Cx<R> *)((char *)base + o_t1);
    tabs.L = L;
    tabs.df = 1.0 / ((double)L * (1.0 / fs));                              // numpy's fftfreq(L, 1 / fs) spacing
    const double sgn = backward ? -1.0 : 1.0;
    tabs.b2 = sgn * beta2;

    const Cx<R> *src = (const Cx<R> *)E;
    Cx<R> *dst = (Cx<R> *)out;
    if (power_mode == 1) {
        hipLaunchKernelGGL((fibre_power_kernel<R>), dim3((unsigned)nb), dim3(FIB_T), 0, g_stream, src, nmodes, L, part);
        QH_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(fibre_pscale_kernel, dim3(1), dim3(FIB_T), 0, g_stream, (const double *)part, nb, L, power_mode, power, pscale);
    QH_HIP(hipGetLastError());

    std::vector<double> h(dz, dz + nsteps);                                // the steps in the order they are walked
    if (backward) for (int i = 0; i < nsteps / 2; i++) std::swap(h[i], h[nsteps - 1 - i]);
    const double kappa = nmodes == 2 ? 8.0 / 9.0 : 1.0, al = sgn * alpha, sigma_w = sqrt(ase_w);
    const Cx<R> *tab;
    for (int s = 0; s < nspans; s++) {
        if ((rc = tabs.get(h[0] / 2, &tab))) return rc;
        if ((rc = fibre_filter(R(), src, nmodes, L, tab, dst))) return rc;
        src = dst;
        for (int i = 0; i < nsteps; i++) {
            const double heff = al == 0 ? h[i] : -expm1(-al * h[i]) / al;
            double a = exp(-al * h[i] / 2), pre = 1.0;
            if (amplify && !backward && i == nsteps - 1) a *= exp(alpha * span / 2);
            if (amplify && backward && i == 0) pre = exp(-alpha * span / 2);
            const bool noise = ase_w > 0 && i == nsteps - 1;
            if ((rc = fibre_nl<R>(dst, dst, nmodes, L, a * pre, sgn * kappa * gamma * heff * pre * pre, pscale, noise, sigma_w, seed + (uint64_t)s))) return rc;
            if ((rc = tabs.get(h[i] / 2 + (i + 1 < nsteps ? h[i + 1] / 2 : 0.0), &tab))) return rc;
            if ((rc = fibre_filter(R(), dst, nmodes, L, tab, dst))) return rc;
        }
    }
    return QH_OK;
}

// the nonlinear step on its own (one launch): what a measurement, or a caller with a step rule of its own, builds on
template <typename R> int fibre_nl_dev(const void *E, int nmodes, int64_t L, double a, double coef, const double *pscale, double sigma_w, uint64_t seed, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nmodes == 1 || nmodes == 2, "fibre_nl: one row, or two (Manakov)");
    QH_REQUIRE(L >= 1 && L <= ((int64_t)1 << 24), "fibre_nl: L must be from 1 to 2^24");
    QH_REQUIRE(E && out && pscale, "fibre_nl: E, out and pscale must be given");
    QH_REQUIRE(std::isfinite(a) && std::isfinite(coef) && std::isfinite(sigma_w) && sigma_w >= 0, "fibre_nl: a and coef must be finite, sigma_w finite and not negative");
    return fibre_nl<R>((const Cx<R> *)E, (Cx<R> *)out, nmodes, L, a, coef, pscale, sigma_w > 0, sigma_w, seed);
}

}  // namespace qh

extern "C" {
int qh_fibre_nl_c64_dev(const void *E, int nmodes, int64_t L, double a, double coef, const double *pscale, double sigma_w, uint64_t seed, void *out)
{ return qh::fibre_nl_dev<float>(E, nmodes, L, a, coef, pscale, sigma_w, seed, out); }
int qh_fibre_nl_c128_dev(const void *E, int nmodes, int64_t L, double a, double coef, const double *pscale, double sigma_w, uint64_t seed, void *out)
{ return qh::fibre_nl_dev<double>(E, nmodes, L, a, coef, pscale, sigma_w, seed, out); }
int qh_fibre_ssfm_c64_dev(const void *E, int nmodes, int64_t L, double fs, double beta2, double gamma, double alpha, const double *dz, int nsteps, int nspans,
                          int backward, int amplify, int power_mode, double power, double ase_w, uint64_t seed, void *out)
{ return qh::fibre_ssfm_dev<float>(E, nmodes, L, fs, beta2, gamma, alpha, dz, nsteps, nspans, backward, amplify, power_mode, power, ase_w, seed, out); }
int qh_fibre_ssfm_c128_dev(const void *E, int nmodes, int64_t L, double fs, double beta2, double gamma, double alpha, const double *dz, int nsteps, int nspans,
                           int backward, int amplify, int power_mode, double power, double ase_w, uint64_t seed, void *out)
{ return qh::fibre_ssfm_dev<double>(E, nmodes, L, fs, beta2, gamma, alpha, dz, nsteps, nspans, backward, amplify, power_mode, power, ase_w, seed, out); }
}
