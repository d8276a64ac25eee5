// Channel impairments on a field that already lies in HBM (qampy/core/impairments.py:29-328): additive white Gaussian noise, laser phase
// noise, a carrier offset, first-order PMD, a rotation of the two polarisations and a whole-sample delay per mode.
//
// Fused point-wise pass (the hot path), every term optional:
//
//   out[m, n] = x[m, n] exp(j (phi[m, n] + 2 pi n f)) + sigma w[m, n]
//
//   w      complex Gaussian noise of unit variance, split over I and Q: counter-based Philox4x32-10 keyed by the seed, counter (sample
//          index low word, high word, mode, stream), stream 2 for the noise and 1 for the phase increments - a draw depends on
//          (seed, mode, n) alone.  complex64: Box-Muller on two 32-bit words with the fast float intrinsics (philox.h gauss2);
//          complex128: uniforms of 53 bits from two words each, Box-Muller in double.
//   sigma  given by the caller, or factor sqrt(p) with p = mean |x|^2 over ALL modes (np.mean(abs(sig)**2) of change_snr) reduced on the
//          device: per-tile partial sums in double, then the final kernel; it never leaves the device.
//   phi    a Wiener process per mode, increments N(0, var), accumulated like np.cumsum: per-tile totals, one exclusive scan of the totals,
//          then the prefix inside the tile - every sum in double for both precisions.
//   f      turns per sample; n f is formed in double and reduced modulo one turn before the sine and cosine.
//
// Launches with every term on: (1) per-tile phase totals and power partials, (2) scan of the totals and the final of the power, (3) the
// pass itself.  Without phase noise and without a device-side sigma the pass is the only launch.  No atomics: a repeated call is
// bit-identical.
//
// PMD: R(-theta) diag(H, conj H) R(theta) with H = exp(-j w dgd / 2).  R commutes with the transform, so a workgroup rotates its block of
// one row on load, transforms it in LDS, multiplies by H (row 0) or conj H (row 1), transforms back and stores - cd.hip's kernel with another
// source policy (block_filter.h PmdRow); a second point-wise launch rotates by -theta in place.  Block sizes and boundary rule of cd.hip's
// circular mode: a row length that is a power of two from 256 to 8192 is one exact transform per row, every other length overlap-save with
// N = 8192 (N / 2 kept, N / 4 of halo on each side, the input taken modulo L).
#include "block_filter.h"
#include "philox.h"

namespace qh {

constexpr int IMP_T = 256, IMP_PER = 4, IMP_TILE = IMP_T * IMP_PER;     // a workgroup covers IMP_TILE samples of one mode, a thread IMP_PER neighbours
constexpr int PMD_N = 8192;

template <typename R> __device__ __forceinline__ double imp_increment(int64_t n, int mode, unsigned k0, unsigned k1, double sphase)
{
    R g0, g1;
    imp_gauss(n, mode, IMP_STREAM_PHASE, k0, k1, g0, g1);
    return sphase * (double)g0;
}

// launch 1, grid (ntiles, nmodes): tot[mode][tile] = sum of the tile's phase increments, pw[mode][tile] = sum of the tile's |x|^2
template <typename R>
__global__ void __launch_bounds__(IMP_T) impair_part_kernel(const Cx<R> *__restrict__ E, int64_t L, int do_phase, int do_power, double sphase, unsigned k0,
                                                            unsigned k1, double *__restrict__ tot, double *__restrict__ pw)
{
    __shared__ double red[IMP_T / 64];
    const int mode = blockIdx.y;
    const size_t slot = (size_t)mode * gridDim.x + blockIdx.x;
    double s = 0, q = 0;
    for (int i = 0; i < IMP_PER; i++) {
        const int64_t n = (int64_t)blockIdx.x * IMP_TILE + i * IMP_T + threadIdx.x;
        if (n >= L) break;
        if (do_phase) s += imp_increment<R>(n, mode, k0, k1, sphase);
        if (do_power) {
            const Cx<R> v = ldg(E + (size_t)mode * L + n);
            q = fma_((double)v.re, (double)v.re, fma_((double)v.im, (double)v.im, q));
        }
    }
    if (do_phase) { s = block_sum<IMP_T>(s, red); if (threadIdx.x == 0) tot[slot] = s; }
    if (do_power) { q = block_sum<IMP_T>(q, red); if (threadIdx.x == 0) pw[slot] = q; }
}

// launch 2, grid (nmodes): the mode's tile totals become their exclusive prefix sums; workgroup 0 also forms sig[0] = factor sqrt(mean |x|^2)
// over every mode
__global__ void __launch_bounds__(IMP_T) impair_scan_kernel(double *__restrict__ tot, const double *__restrict__ pw, int64_t ntiles, int nmodes, int64_t L,
                                                            int do_phase, int do_power, double factor, double *__restrict__ sig)
{
    __shared__ double sh[IMP_T];
    if (do_phase) {
        double *t = tot + (size_t)blockIdx.x * ntiles;
        const int64_t per = (ntiles + IMP_T - 1) / IMP_T, lo = threadIdx.x * per, hi = lo + per < ntiles ? lo + per : ntiles;
        double s = 0;
        for (int64_t i = lo; i < hi; i++) s += t[i];
        sh[threadIdx.x] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            double acc = 0;
            for (int i = 0; i < IMP_T; i++) { const double v = sh[i]; sh[i] = acc; acc += v; }
        }
        __syncthreads();
        double acc = sh[threadIdx.x];
        for (int64_t i = lo; i < hi; i++) { const double v = t[i]; t[i] = acc; acc += v; }
        __syncthreads();
    }
    if (do_power && blockIdx.x == 0) {
        const int64_t cnt = ntiles * nmodes;
        double s = 0;
        for (int64_t i = threadIdx.x; i < cnt; i += IMP_T) s += pw[i];
        sh[threadIdx.x] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            double acc = 0;
            for (int i = 0; i < IMP_T; i++) acc += sh[i];
            sig[0] = factor * sqrt(acc / ((double)nmodes * (double)L));
        }
    }
}

// launch 3, grid (ntiles, nmodes).  E == nullptr: only the phase is written (trace).  out == E is allowed: a thread reads the elements it writes.
template <typename R>
__global__ void __launch_bounds__(IMP_T) impair_pointwise_kernel(const Cx<R> *E, Cx<R> *out, int64_t L, int do_phase, int cumulative, int do_freq, int noise_mode,
                                                                 double sigma, const double *__restrict__ sig, double sphase, double fturns, unsigned k0,
                                                                 unsigned k1, const double *__restrict__ tile_off, double *__restrict__ trace)
{
    __shared__ double wt[IMP_T / 64];
    const int mode = blockIdx.y;
    const int64_t n0 = (int64_t)blockIdx.x * IMP_TILE + (int64_t)threadIdx.x * IMP_PER;
    double phi[IMP_PER] = {0, 0, 0, 0};
    if (do_phase) {
        double inc[IMP_PER], run = 0;
#pragma unroll
        for (int i = 0; i < IMP_PER; i++) {
            inc[i] = n0 + i < L ? imp_increment<R>(n0 + i, mode, k0, k1, sphase) : 0.0;
            run += inc[i];
            phi[i] = run;                                               // inclusive, like np.cumsum
        }
        if (cumulative) {
            const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
            double v = run;
            for (int o = 1; o < 64; o <<= 1) {
                const double u = __shfl_up(v, o);
                if (lane >= o) v += u;
            }
            if (lane == 63) wt[wave] = v;
            __syncthreads();
            double base = tile_off[(size_t)mode * gridDim.x + blockIdx.x];
            for (int w = 0; w < wave; w++) base += wt[w];
            base += v - run;
#pragma unroll
            for (int i = 0; i < IMP_PER; i++) phi[i] += base;
        } else {
#pragma unroll
            for (int i = 0; i < IMP_PER; i++) phi[i] = inc[i];
        }
        if (trace) {
#pragma unroll
            for (int i = 0; i < IMP_PER; i++)
                if (n0 + i < L) trace[(size_t)mode * L + n0 + i] = phi[i];
        }
    }
    if (!E) return;
    double sg = noise_mode == 2 ? sig[0] : sigma;
    const R s_iq = (R)(sg * 0.70710678118654752440);
    const bool noisy = noise_mode != 0 && sg != 0.0;
#pragma unroll
    for (int i = 0; i < IMP_PER; i++) {
        const int64_t n = n0 + i;
        if (n >= L) break;
        Cx<R> x = ldg(E + (size_t)mode * L + n);
        if (do_phase || do_freq) {
            double turns = do_phase ? phi[i] * (1.0 / IMP_TWO_PI) : 0.0;
            if (do_freq) {
                double ft = (double)n * fturns;
                ft -= rint(ft);
                turns += ft;
            }
            turns -= rint(turns);
            R sn, cs;
            if constexpr (sizeof(R) == 4) sincosf((float)(IMP_TWO_PI * turns), &sn, &cs);
            else sincos(IMP_TWO_PI * turns, &sn, &cs);
            x = Cx<R>{x.re * cs - x.im * sn, x.re * sn + x.im * cs};
        }
        if (noisy) {
            R g0, g1;
            imp_gauss(n, mode, IMP_STREAM_NOISE, k0, k1, g0, g1);
            x = Cx<R>{fma_(s_iq, g0, x.re), fma_(s_iq, g1, x.im)};
        }
        stg(out + (size_t)mode * L + n, x);
    }
}

// out[0] = c x[0] - s x[1], out[1] = s x[0] + c x[1] (rotate_field); out == E is allowed.  grid (blocks)
template <typename R>
__global__ void __launch_bounds__(IMP_T) rotate_field_kernel(const Cx<R> *E, Cx<R> *out, int64_t L, R c, R s)
{
    const int64_t n = (int64_t)blockIdx.x * IMP_T + threadIdx.x;
    if (n >= L) return;
    const Cx<R> u = ldg(E + n), v = ldg(E + L + n);
    stg(out + n, Cx<R>{c * u.re - s * v.re, c * u.im - s * v.im});
    stg(out + L + n, Cx<R>{s * u.re + c * v.re, s * u.im + c * v.im});
}

// ------------------------------------------------------------------------------------------------ host side
// E == nullptr: phase only (trace must be given).  noise_mode 0: none; 1: sigma = noise; 2: sigma = noise sqrt(mean |E|^2 over all modes)
template <typename R>
int impair_pointwise_dev(const void *E, int nmodes, int64_t L, int noise_mode, double noise, int have_phase, double phase_var, int cumulative, int have_freq,
                         double freq, uint64_t seed, double *trace, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 0 && (L + IMP_TILE - 1) / IMP_TILE <= 0x7fffffffLL, "impair_pointwise: bad sizes");
    QH_REQUIRE(noise_mode >= 0 && noise_mode <= 2, "impair_pointwise: noise_mode is 0 (none), 1 (sigma given) or 2 (sigma relative to the signal's rms)");
    QH_REQUIRE(noise_mode == 0 || (std::isfinite(noise) && noise >= 0), "impair_pointwise: the noise strength must be finite and not negative");
    QH_REQUIRE(!have_phase || (std::isfinite(phase_var) && phase_var >= 0), "impair_pointwise: the variance of the phase increments must be finite and not negative");
    QH_REQUIRE(!have_freq || std::isfinite(freq), "impair_pointwise: the carrier offset must be finite");
    QH_REQUIRE(E ? out != nullptr : (trace != nullptr && have_phase), "impair_pointwise: E and out, or a trace of the phase alone");
    QH_REQUIRE(!trace || have_phase, "impair_pointwise: a trace needs phase noise");
    if (L == 0) return QH_OK;
    const int64_t ntiles = (L + IMP_TILE - 1) / IMP_TILE;
    const int scan = have_phase && cumulative, power = E && noise_mode == 2;
    ScratchLayout lay;
    const size_t o_tot = lay.take((size_t)nmodes * ntiles * sizeof(double)), o_pw = lay.take((size_t)nmodes * ntiles * sizeof(double)), o_sig = lay.take(sizeof(double));
    void *base = nullptr;
    if ((rc = scratch(Slot::IMPAIR, lay.total, &base))) return rc;
    double *tot = (double *)((char *)base + o_tot), *pw = (double *)((char *)base + o_pw), *sig = (double *)((char *)base + o_sig);
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    const double sphase = have_phase ? sqrt(phase_var) : 0.0;
    const dim3 grid((unsigned)ntiles, nmodes);
    if (scan || power) {
        hipLaunchKernelGGL((impair_part_kernel<R>), grid, dim3(IMP_T), 0, g_stream, (const Cx<R> *)E, L, scan, power, sphase, k0, k1, tot, pw);
        hipLaunchKernelGGL(impair_scan_kernel, dim3(nmodes), dim3(IMP_T), 0, g_stream, tot, (const double *)pw, ntiles, nmodes, L, scan, power, noise, sig);
        QH_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL((impair_pointwise_kernel<R>), grid, dim3(IMP_T), 0, g_stream, (const Cx<R> *)E, (Cx<R> *)out, L, have_phase ? 1 : 0, cumulative ? 1 : 0,
                       have_freq ? 1 : 0, noise_mode, noise, (const double *)sig, sphase, have_freq ? freq : 0.0, k0, k1, (const double *)tot, trace);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R>
int impair_pointwise_host(const void *E, int nmodes, int64_t L, int noise_mode, double noise, int have_phase, double phase_var, int have_freq, double freq,
                          uint64_t seed, double *trace, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(E && out && nmodes >= 1 && nmodes <= 65535 && L >= 0, "impair_pointwise: bad arguments");
    if (L == 0) return QH_OK;
    DevBuf dE, dtr;
    const size_t bytes = (size_t)nmodes * L * sizeof(Cx<R>);
    if ((rc = dE.from_host(E, bytes))) return rc;
    if (trace && (rc = dtr.alloc((size_t)nmodes * L * sizeof(double)))) return rc;
    if ((rc = impair_pointwise_dev<R>(dE.p, nmodes, L, noise_mode, noise, have_phase, phase_var, 1, have_freq, freq, seed, trace ? (double *)dtr.p : nullptr, dE.p)))
        return rc;
    if ((rc = dE.to_host(out, bytes))) return rc;
    if (trace && (rc = dtr.to_host(trace, dtr.n))) return rc;
    QH_HIP(hipStreamSynchronize(g_stream));
    return QH_OK;
}

template <typename R> int rotate_field_dev(const void *E, int nmodes, int64_t L, double theta, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nmodes == 2, "rotate_field: a rotation of the polarisations needs two modes");
    QH_REQUIRE(E && out && L >= 0 && (L + IMP_T - 1) / IMP_T <= 0x7fffffffLL && std::isfinite(theta), "rotate_field: bad arguments");
    if (L == 0) return QH_OK;
    hipLaunchKernelGGL((rotate_field_kernel<R>), dim3((unsigned)((L + IMP_T - 1) / IMP_T)), dim3(IMP_T), 0, g_stream, (const Cx<R> *)E, (Cx<R> *)out, L,
                       (R)cos(theta), (R)sin(theta));
    QH_HIP(hipGetLastError());
    return QH_OK;
}

// twiddles of the block transform and H[k] = exp(-j pi dgd k / N) / N on the fftfreq grid (dgd in samples), uploaded once per
// (N, dgd, precision) into scratch slot Slot::PMD
static thread_local TableCache g_pmd;

template <typename R> static int pmd_table(int N, double dgd, const Cx<R> **tab)
{
    std::string key;
    key_add(key, dgd);
    return filter_table<R>(g_pmd, Slot::PMD, N, key, [=](int k) { return -QH_PI * dgd * (double)k / (double)N; }, tab);
}

// dgd in samples (t_dgd fs)
template <typename R> int apply_pmd_dev(const void *E, int nmodes, int64_t L, double theta, double dgd, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nmodes == 2, "apply_pmd: first-order PMD needs two modes");
    QH_REQUIRE(E && out && E != out, "apply_pmd: out must be a buffer other than E");
    QH_REQUIRE(L >= 0 && (L + PMD_N / 2 - 1) / (PMD_N / 2) <= 0x7fffffffLL && (L + IMP_T - 1) / IMP_T <= 0x7fffffffLL, "apply_pmd: bad sizes");
    QH_REQUIRE(std::isfinite(theta) && std::isfinite(dgd), "apply_pmd: theta and the delay must be finite");
    if (L == 0) return QH_OK;
    const bool whole = L >= 256 && L <= PMD_N && (L & (L - 1)) == 0;
    const int N = whole ? (int)L : PMD_N;
    const Cx<R> *tab;
    if ((rc = pmd_table<R>(N, dgd, &tab))) return rc;
    Cx<R> *o = (Cx<R> *)out;
    const R c = (R)cos(theta), s = (R)sin(theta);
    if ((rc = block_filter<R>(N, (const Cx<R> *)E, o, 2, L, L, tab, PmdRow<R>{c, s}, 0))) return rc;
    // R(-theta), in place
    hipLaunchKernelGGL((rotate_field_kernel<R>), dim3((unsigned)((L + IMP_T - 1) / IMP_T)), dim3(IMP_T), 0, g_stream, (const Cx<R> *)o, o, L, c, -s);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R> int apply_pmd_host(const void *E, int nmodes, int64_t L, double theta, double dgd, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nmodes == 2, "apply_pmd: first-order PMD needs two modes");
    QH_REQUIRE(E && out && L >= 0, "apply_pmd: bad arguments");
    if (L == 0) return QH_OK;
    DevBuf dE, dout;
    const size_t bytes = 2 * (size_t)L * sizeof(Cx<R>);
    if ((rc = dE.from_host(E, bytes))) return rc;
    if ((rc = dout.alloc(bytes))) return rc;
    if ((rc = apply_pmd_dev<R>(dE.p, 2, L, theta, dgd, dout.p))) return rc;
    if ((rc = dout.to_host(out, bytes))) return rc;
    QH_HIP(hipStreamSynchronize(g_stream));
    return QH_OK;
}

// np.roll of every row by delays[row] whole samples (host array): two copies per row on the stream
static int modal_delay_dev(const void *E, int nmodes, int64_t L, const int64_t *delays, void *out, size_t esize)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(E && out && E != out && delays && nmodes >= 1 && L >= 0, "modal_delay: out must be a buffer other than E, one delay per mode");
    if (L == 0) return QH_OK;
    for (int m = 0; m < nmodes; m++) {
        int64_t d = delays[m] % L;
        if (d < 0) d += L;
        const char *x = (const char *)E + (size_t)m * L * esize;
        char *y = (char *)out + (size_t)m * L * esize;
        QH_HIP(hipMemcpyAsync(y + (size_t)d * esize, x, (size_t)(L - d) * esize, hipMemcpyDeviceToDevice, g_stream));
        if (d) QH_HIP(hipMemcpyAsync(y, x + (size_t)(L - d) * esize, (size_t)d * esize, hipMemcpyDeviceToDevice, g_stream));
    }
    return QH_OK;
}

}  // namespace qh

extern "C" {
int qh_impair_pointwise_c64_dev(const void *E, int nmodes, int64_t L, int noise_mode, double noise, int have_phase, double phase_var, int have_freq, double freq,
                                uint64_t seed, double *trace, void *out)
{ return qh::impair_pointwise_dev<float>(E, nmodes, L, noise_mode, noise, have_phase, phase_var, 1, have_freq, freq, seed, trace, out); }
int qh_impair_pointwise_c128_dev(const void *E, int nmodes, int64_t L, int noise_mode, double noise, int have_phase, double phase_var, int have_freq, double freq,
                                 uint64_t seed, double *trace, void *out)
{ return qh::impair_pointwise_dev<double>(E, nmodes, L, noise_mode, noise, have_phase, phase_var, 1, have_freq, freq, seed, trace, out); }
int qh_impair_pointwise_c64(const void *E, int nmodes, int64_t L, int noise_mode, double noise, int have_phase, double phase_var, int have_freq, double freq,
                            uint64_t seed, double *trace, void *out)
{ return qh::impair_pointwise_host<float>(E, nmodes, L, noise_mode, noise, have_phase, phase_var, have_freq, freq, seed, trace, out); }
int qh_impair_pointwise_c128(const void *E, int nmodes, int64_t L, int noise_mode, double noise, int have_phase, double phase_var, int have_freq, double freq,
                             uint64_t seed, double *trace, void *out)
{ return qh::impair_pointwise_host<double>(E, nmodes, L, noise_mode, noise, have_phase, phase_var, have_freq, freq, seed, trace, out); }
int qh_phase_noise_c64_dev(double *out, int nmodes, int64_t L, double phase_var, uint64_t seed, int cumulative)
{ return qh::impair_pointwise_dev<float>(nullptr, nmodes, L, 0, 0.0, 1, phase_var, cumulative, 0, 0.0, seed, out, nullptr); }
int qh_phase_noise_c128_dev(double *out, int nmodes, int64_t L, double phase_var, uint64_t seed, int cumulative)
{ return qh::impair_pointwise_dev<double>(nullptr, nmodes, L, 0, 0.0, 1, phase_var, cumulative, 0, 0.0, seed, out, nullptr); }
int qh_rotate_field_c64_dev(const void *E, int nmodes, int64_t L, double theta, void *out) { return qh::rotate_field_dev<float>(E, nmodes, L, theta, out); }
int qh_rotate_field_c128_dev(const void *E, int nmodes, int64_t L, double theta, void *out) { return qh::rotate_field_dev<double>(E, nmodes, L, theta, out); }
int qh_apply_pmd_c64_dev(const void *E, int nmodes, int64_t L, double theta, double dgd, void *out) { return qh::apply_pmd_dev<float>(E, nmodes, L, theta, dgd, out); }
int qh_apply_pmd_c128_dev(const void *E, int nmodes, int64_t L, double theta, double dgd, void *out) { return qh::apply_pmd_dev<double>(E, nmodes, L, theta, dgd, out); }
int qh_apply_pmd_c64(const void *E, int nmodes, int64_t L, double theta, double dgd, void *out) { return qh::apply_pmd_host<float>(E, nmodes, L, theta, dgd, out); }
int qh_apply_pmd_c128(const void *E, int nmodes, int64_t L, double theta, double dgd, void *out) { return qh::apply_pmd_host<double>(E, nmodes, L, theta, dgd, out); }
int qh_modal_delay_c64_dev(const void *E, int nmodes, int64_t L, const int64_t *delays, void *out) { return qh::modal_delay_dev(E, nmodes, L, delays, out, 8); }
int qh_modal_delay_c128_dev(const void *E, int nmodes, int64_t L, const int64_t *delays, void *out) { return qh::modal_delay_dev(E, nmodes, L, delays, out, 16); }
}
