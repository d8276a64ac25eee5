// Digital pre-compensation on gfx950 without leaving device memory: the pattern index of every symbol, the look-up table of the average error per
// pattern and its application, the arcsin that undoes the modulator's sine, and the regularised inverse of the DAC's low-pass as a table of bins.
//
// Reference behaviour:
//   qampy/core/digital_pre_compensation.py:98-131   find_sym_patterns: np.argmin(|x - levels|) per symbol, then the window of mem_len decisions that starts
//                                                   mem_len // 2 symbols back (cal_lut: idx = nonzero(idx_data) - mem_len // 2 into the wrapped rolling window)
//   qampy/core/digital_pre_compensation.py:133-191  cal_lut: err = tx - rx at the positions of idx_data, averaged per pattern, I and Q on their own
//   qampy/core/pythran_dsp.py:201-240               cal_lut_avg: sums / max(counts, 1)
//   qampy/core/digital_pre_compensation.py:40-56    comp_mod_sin: 2 vpi asin(x) per rail
//   qampy/core/digital_pre_compensation.py:58-96    comp_dac_resp: p_f = n_f conj(d_f) / (n_f |d_f|^2 + alpha)
//
// Pattern index, one launch: a workgroup decides the level of the PC_TILE symbols of its tile and of the mem_len - 1 around them ONCE, keeps the
// decisions in LDS as 16-bit numbers and every thread then folds the mem_len decisions of its window, p = sum_j lev[(i - mem_len / 2 + j) mod L]
// M^(mem_len - 1 - j).  Sorted rail levels are searched by bisection, a complex alphabet by a linear scan of the squared distances (both from LDS up to
// PC_LDS_LEVELS entries, from global memory above); the first minimum wins a tie and a NaN sample gets level 0, as np.argmin gives.  The alphabet's
// distances are dr^2 + di^2 in double where numpy compares hypot(dr, di): exact ties fall alike, but two points whose distances differ by less than
// the rounding of either form (about 1e-16 of the distance) may be ordered differently - a sample that close to a boundary has no decision to keep.  The same kernel, with the table in place of the
// index rows, is the fused pre-distortion: no index row is written.  8 B in and 8 B out per complex64 symbol: HBM traffic is the floor.
//
// Look-up table, bit-identical on every call: a float sum by atomics depends on the order of arrival, so the errors are summed as 64-bit integers in
// fixed point.  lut_max_kernel / lut_scale_kernel: max |err| of a row over the selected positions, 2^E just above it, and the scale 2^s with
// s = 62 - ceil(log2(L + 1)) - E: every |err 2^s| is below 2^(62 - ceil(log2(L + 1))) and no sum of L of them leaves 63 bits.  With L <= 2^24 a sample keeps
// at least 37 bits below the largest error.  lut_accum_kernel: integer atomic adds - into tables private to the workgroup in LDS while N <= PC_LDS_N,
// flushed once per workgroup with global atomics; straight into the global tables above that.  The sums live in the (nmodes, N) complex128 output
// itself (16 B per entry = two 64-bit sums); lut_final_kernel turns them into averages in place: (double)sum 2^-s / max(count, 1) for the real
// parts and (double)sum 2^-s (1 / max(count, 1)) for the imaginary parts - the two roundings numpy makes when the reference divides the complex
// 1j sum_Q by the counts.
#include "common.h"
#include <cmath>

namespace qh {
namespace {

constexpr int PC_THREADS = 256;
constexpr int PC_TILE = 1024;                          // symbols per workgroup of the pattern kernels
constexpr int PC_MEM_MAX = 15;                         // longest pattern
constexpr int PC_M_MAX = 4096;                         // most levels of a rail, most points of an alphabet
constexpr int PC_LDS_LEVELS = 256;                     // rails of up to this many levels are searched in LDS
constexpr int64_t PC_N_MAX = (int64_t)1 << 24;         // largest table
constexpr int PC_LDS_N = 2048;                         // largest table a workgroup keeps in LDS (24 B per entry)
constexpr int PC_LUT_CHUNK = 16384;                    // symbols per workgroup of the accumulation
constexpr int PC_MAX_TILE = 4096;                      // symbols per workgroup of the max |err| pass
constexpr int64_t PC_LUT_LMAX = (int64_t)1 << 24;      // longest row of the table's accumulation
constexpr int64_t PC_ROW_MAX = (int64_t)1 << 40;
constexpr int PC_SOS_MAX = 4;

// rails: li (mi sorted levels) and lq (mq); alphabet: al (mc points, re / im pairs), li == nullptr
struct Levels { const double *li, *lq, *al; int mi, mq, mc, mem_len; };

// np.argmin(|x - lv|) over sorted levels: bisection to the neighbours of x, then down while a level below is no farther (only rounding, or an
// infinite x, makes it so): the first minimum.  A NaN compares false everywhere: level 0.
__device__ __forceinline__ int nearest_level(const double *lv, int M, double x)
{
    int lo = -1, hi = M;                               // lv[lo] <= x < lv[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (lv[mid] <= x) lo = mid; else hi = mid;
    }
    int c = lo < 0 ? 0 : lo;
    double d = fabs(x - lv[c]);
    if (lo >= 0 && lo + 1 < M) {
        const double d1 = fabs(x - lv[lo + 1]);
        if (d1 < d) { c = lo + 1; d = d1; }
    }
    while (c > 0 && fabs(x - lv[c - 1]) <= d) c--;
    return c;
}

// first minimum of the squared distance to the points (re[k stride], im[k stride])
__device__ __forceinline__ int nearest_point(const double *re, const double *im, int stride, int M, double xr, double xi)
{
    int c = 0;
    double best = 0.;
    for (int k = 0; k < M; k++) {
        const double dr = xr - re[k * stride], di = xi - im[k * stride], d = dr * dr + di * di;
        if (k == 0 || d < best) { best = d; c = k; }
    }
    return c;
}

// MODE 0: idx_I / idx_Q (nmodes, L) int32, either may be nullptr.  MODE 1: out = E + gain (ea[p_I].re + 1j ea[p_Q].im), ea (nmodes, N) complex128.
template <typename R, int MODE>
__global__ void __launch_bounds__(PC_THREADS) pattern_kernel(const Cx<R> *__restrict__ E, int64_t L, Levels lv, int32_t *__restrict__ idx_I, int32_t *__restrict__ idx_Q,
                                                             const double *__restrict__ ea, int64_t N, double gain, Cx<R> *__restrict__ out)
{
    __shared__ uint16_t sI[PC_TILE + PC_MEM_MAX - 1], sQ[PC_TILE + PC_MEM_MAX - 1];
    __shared__ double tI[PC_LDS_LEVELS], tQ[PC_LDS_LEVELS];
    const int tid = threadIdx.x;
    const int64_t mode = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * PC_TILE;
    const bool rails = lv.li != nullptr;
    const bool lds = rails ? lv.mi <= PC_LDS_LEVELS && lv.mq <= PC_LDS_LEVELS : lv.mc <= PC_LDS_LEVELS;       // (uniform)
    if (lds) {                                         // rails: the two tables; alphabet: its real parts in tI, its imaginary parts in tQ
        if (rails) {
            for (int k = tid; k < lv.mi; k += PC_THREADS) tI[k] = lv.li[k];
            for (int k = tid; k < lv.mq; k += PC_THREADS) tQ[k] = lv.lq[k];
        } else {
            for (int k = tid; k < lv.mc; k += PC_THREADS) { tI[k] = lv.al[2 * k]; tQ[k] = lv.al[2 * k + 1]; }
        }
        __syncthreads();
    }
    const int cnt = (int)(L - base < PC_TILE ? L - base : PC_TILE);
    const int ne = cnt + lv.mem_len - 1;
    const int64_t first = base - lv.mem_len / 2;
    for (int e = tid; e < ne; e += PC_THREADS) {
        int64_t p = (first + e) % L;
        if (p < 0) p += L;
        const Cx<R> x = ldg(E + mode * L + p);
        int a, b;
        if (rails && lds) { a = nearest_level(tI, lv.mi, (double)x.re); b = nearest_level(tQ, lv.mq, (double)x.im); }
        else if (rails) { a = nearest_level(lv.li, lv.mi, (double)x.re); b = nearest_level(lv.lq, lv.mq, (double)x.im); }
        else if (lds) { a = b = nearest_point(tI, tQ, 1, lv.mc, (double)x.re, (double)x.im); }
        else { a = b = nearest_point(lv.al, lv.al + 1, 2, lv.mc, (double)x.re, (double)x.im); }
        sI[e] = (uint16_t)a;
        sQ[e] = (uint16_t)b;
    }
    __syncthreads();
    const int64_t MI = rails ? lv.mi : lv.mc, MQ = rails ? lv.mq : lv.mc;
    for (int k = tid; k < cnt; k += PC_THREADS) {
        int64_t pI = 0, pQ = 0;
        for (int j = 0; j < lv.mem_len; j++) {
            pI = pI * MI + sI[k + j];
            pQ = pQ * MQ + sQ[k + j];
        }
        const int64_t at = mode * L + base + k;
        if constexpr (MODE == 0) {
            if (idx_I) idx_I[at] = (int32_t)pI;
            if (idx_Q) idx_Q[at] = (int32_t)pQ;
        } else {
            const Cx<R> x = ldg(E + at);
            const double cr = pI < N ? ea[2 * (mode * N + pI)] : 0., ci = pQ < N ? ea[2 * (mode * N + pQ) + 1] : 0.;
            stg(out + at, Cx<R>{(R)((double)x.re + gain * cr), (R)((double)x.im + gain * ci)});
        }
    }
}

// out = sig + gain (ea[idx_I].re + 1j ea[idx_Q].im), in double, rounded once; an index outside the table adds nothing.  (out may be sig)
// One sample per thread here and in mod_sin_kernel: with two complex64 per thread (16 B per lane, one float4 each way) both kernels took 14 - 35 %
// longer at 2 x 2^22 samples - they wait on the dependent table reads and on the double asin, not on the width of their accesses.
template <typename R>
__global__ void __launch_bounds__(PC_THREADS) lut_apply_kernel(const Cx<R> *sig, int64_t L, const double *__restrict__ ea, int64_t N, const int32_t *__restrict__ idx_I,
                                                               const int32_t *__restrict__ idx_Q, double gain, Cx<R> *out)
{
    const int64_t i = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= L) return;
    const int64_t mode = blockIdx.y, at = mode * L + i;
    const int64_t a = idx_I[at], b = idx_Q[at];
    const double cr = a >= 0 && a < N ? ea[2 * (mode * N + a)] : 0., ci = b >= 0 && b < N ? ea[2 * (mode * N + b) + 1] : 0.;
    const Cx<R> x = ldg(sig + at);
    stg(out + at, Cx<R>{(R)((double)x.re + gain * cr), (R)((double)x.im + gain * ci)});
}

// ------------------------------------------------------------------------------------------------ look-up table
__device__ __forceinline__ double block_max(double m, double *red)
{
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = PC_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

template <typename R>
__global__ void __launch_bounds__(PC_THREADS) lut_max_kernel(const Cx<R> *__restrict__ tx, const Cx<R> *__restrict__ rx, int64_t L, const uint8_t *__restrict__ mask,
                                                             int64_t mstride, double *__restrict__ part)
{
    __shared__ double red[PC_THREADS];
    const int64_t mode = blockIdx.y, base = (int64_t)blockIdx.x * PC_MAX_TILE;
    double m = 0.;
    for (int k = threadIdx.x; k < PC_MAX_TILE; k += PC_THREADS) {
        const int64_t i = base + k;
        if (i >= L) break;
        if (mask && !mask[mode * mstride + i]) continue;
        const Cx<R> a = ldg(tx + mode * L + i), b = ldg(rx + mode * L + i);
        m = fmax(m, fmax(fabs((double)a.re - (double)b.re), fabs((double)a.im - (double)b.im)));      // (fmax drops a NaN)
    }
    m = block_max(m, red);
    if (threadIdx.x == 0) part[mode * gridDim.x + blockIdx.x] = m;
}

// scale[mode] = {2^s, 2^-s}; hb = ceil(log2(L + 1)).  An error that is not finite, or beyond 2^900, leaves s = 0 and entries without meaning.
__global__ void __launch_bounds__(PC_THREADS) lut_scale_kernel(const double *__restrict__ part, int64_t ntiles, int hb, double *__restrict__ scale)
{
    __shared__ double red[PC_THREADS];
    double m = 0.;
    for (int64_t k = threadIdx.x; k < ntiles; k += PC_THREADS) m = fmax(m, part[(int64_t)blockIdx.x * ntiles + k]);
    m = block_max(m, red);
    if (threadIdx.x == 0) {
        int s = 0;
        if (m > 0. && m < 0x1p900) {
            int e;
            frexp(m, &e);                              // m < 2^e
            s = 62 - hb - e;
            if (s > 1000) s = 1000;
        }
        scale[2 * blockIdx.x] = ldexp(1., s);
        scale[2 * blockIdx.x + 1] = ldexp(1., -s);
    }
}

__device__ __forceinline__ void add64(unsigned long long *p, long long v) { atomicAdd(p, (unsigned long long)v); }

// sums (nmodes, N, 2) 64-bit integers (the output's own storage), nI / nQ (nmodes, N) int32; all zero before the launch
template <typename R, bool LDS>
__global__ void __launch_bounds__(PC_THREADS) lut_accum_kernel(const Cx<R> *__restrict__ tx, const Cx<R> *__restrict__ rx, int64_t L, const int32_t *__restrict__ idx_I,
                                                               const int32_t *__restrict__ idx_Q, const uint8_t *__restrict__ mask, int64_t mstride, int64_t N,
                                                               const double *__restrict__ scale, unsigned long long *sums, unsigned int *nI, unsigned int *nQ)
{
    __shared__ unsigned long long sS[LDS ? 2 * PC_LDS_N : 2];
    __shared__ unsigned int sC[LDS ? 2 * PC_LDS_N : 2];
    const int64_t mode = blockIdx.y, base = (int64_t)blockIdx.x * PC_LUT_CHUNK;
    const int n = (int)N;
    if constexpr (LDS) {
        for (int k = threadIdx.x; k < 2 * n; k += PC_THREADS) { sS[k] = 0; sC[k] = 0; }
        __syncthreads();
    }
    const double sc = scale[2 * mode];
    unsigned long long *gs = sums + mode * N * 2;
    unsigned int *gI = nI + mode * N, *gQ = nQ + mode * N;
    for (int k = threadIdx.x; k < PC_LUT_CHUNK; k += PC_THREADS) {
        const int64_t i = base + k;
        if (i >= L) break;
        if (mask && !mask[mode * mstride + i]) continue;
        const Cx<R> a = ldg(tx + mode * L + i), b = ldg(rx + mode * L + i);
        const long long qr = llrint(((double)a.re - (double)b.re) * sc), qi = llrint(((double)a.im - (double)b.im) * sc);
        const int64_t pI = idx_I[mode * L + i], pQ = idx_Q[mode * L + i];
        if (pI >= 0 && pI < N) {
            if constexpr (LDS) { add64(&sS[2 * pI], qr); atomicAdd(&sC[2 * pI], 1u); }
            else { add64(&gs[2 * pI], qr); atomicAdd(&gI[pI], 1u); }
        }
        if (pQ >= 0 && pQ < N) {
            if constexpr (LDS) { add64(&sS[2 * pQ + 1], qi); atomicAdd(&sC[2 * pQ + 1], 1u); }
            else { add64(&gs[2 * pQ + 1], qi); atomicAdd(&gQ[pQ], 1u); }
        }
    }
    if constexpr (LDS) {
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += PC_THREADS) {
            if (sC[2 * k]) { add64(&gs[2 * k], (long long)sS[2 * k]); atomicAdd(&gI[k], sC[2 * k]); }
            if (sC[2 * k + 1]) { add64(&gs[2 * k + 1], (long long)sS[2 * k + 1]); atomicAdd(&gQ[k], sC[2 * k + 1]); }
        }
    }
}

// in place: entry p of ea holds two 64-bit sums and leaves as sum 2^-s / max(count, 1) per rail
__global__ void __launch_bounds__(PC_THREADS) lut_final_kernel(double *ea, int64_t N, const double *__restrict__ scale, const unsigned int *__restrict__ nI,
                                                               const unsigned int *__restrict__ nQ)
{
    const int64_t p = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x;
    if (p >= N) return;
    const int64_t mode = blockIdx.y, at = mode * N + p;
    const double inv = scale[2 * mode + 1];
    const long long *s = reinterpret_cast<const long long *>(ea) + 2 * at;
    const long long sr = s[0], si = s[1];
    const unsigned int cI = nI[at], cQ = nQ[at];
    ea[2 * at] = (double)sr * inv / (double)(cI ? cI : 1u);
    ea[2 * at + 1] = (double)si * inv * (1. / (double)(cQ ? cQ : 1u));      // numpy divides the complex 1j sum_Q by n as a product with 1 / n
}

// ------------------------------------------------------------------------------------------------ arcsin
// a value beyond +-clip goes to +-clip first (clip > 0); a NaN stays one, and asin outside [-1, 1] gives one
__device__ __forceinline__ double clamp_keep_nan(double x, double c) { return x > c ? c : (x < -c ? -c : x); }

template <typename R>
__global__ void __launch_bounds__(PC_THREADS) mod_sin_kernel(const Cx<R> *sig, int64_t total, double vr, double vi, double clip, Cx<R> *out)
{
    const int64_t i = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= total) return;
    const Cx<R> x = ldg(sig + i);
    double xr = (double)x.re, xi = (double)x.im;
    if (clip > 0.) { xr = clamp_keep_nan(xr, clip); xi = clamp_keep_nan(xi, clip); }
    const double oi = 2. * vi * asin(xi);
    // numpy forms re + 1j im with im as a complex number: a NaN of the quadrature rail lands in the real part too (0 NaN), not the other way round
    stg(out + i, Cx<R>{(R)(2. * vr * asin(xr) + 0. * oi), (R)oi});
}

// ------------------------------------------------------------------------------------------------ DAC pre-emphasis table
struct DacArgs { int64_t n; double fb, fs, beta, c; int nsec; double sos[PC_SOS_MAX][6]; };

// n_f and d_f of bin k, the arithmetic of the frequency grid and of the band edges written as numpy evaluates it (a bin on an edge falls as there)
__device__ __forceinline__ void dac_bin(const DacArgs &a, int64_t k, double *nf, double *dr, double *di)
{
    const int64_t kk = k < (a.n + 1) / 2 ? k : k - a.n;
    const double f = fabs((double)kk * (1.0 / (double)a.n) * a.fs);
    const double T = 1.0 / a.fb, lo = (1. - a.beta) / (2. * T), hi = (1. + a.beta) / (2. * T);
    double rc = 0.;
    if (f <= lo) rc = T;
    else if (f <= hi) rc = T / 2. * (1. + cos(QH_PI * T / a.beta * (f - lo)));
    *nf = rc / T;
    double s1, c1;
    sincospi(2. * (double)k / (double)a.n, &s1, &c1);
    const double c2 = c1 * c1 - s1 * s1, s2 = 2. * s1 * c1;
    double hr = 1., hi_ = 0.;
    for (int s = 0; s < a.nsec; s++) {
        const double *q = a.sos[s];
        const double nr = q[0] + q[1] * c1 + q[2] * c2, ni = -(q[1] * s1 + q[2] * s2);
        const double er = q[3] + q[4] * c1 + q[5] * c2, ei = -(q[4] * s1 + q[5] * s2);
        const double den = er * er + ei * ei;
        const double gr = (nr * er + ni * ei) / den, gi = (ni * er - nr * ei) / den;
        const double t = hr * gr - hi_ * gi;
        hi_ = hr * gi + hi_ * gr;
        hr = t;
    }
    *dr = hr;
    *di = hi_;
}

// part[tile] = sum over the tile's bins of |d_f|^2 n_f df, in a fixed order
__global__ void __launch_bounds__(PC_THREADS) dac_part_kernel(DacArgs a, double *__restrict__ part)
{
    __shared__ double red[PC_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * PC_TILE;
    const double df = a.fs / (double)a.n;
    double s = 0.;
    for (int k = threadIdx.x; k < PC_TILE; k += PC_THREADS) {
        if (base + k >= a.n) break;
        double nf, dr, di;
        dac_bin(a, base + k, &nf, &dr, &di);
        s += (dr * dr + di * di) * nf * df;
    }
    s = block_sum<PC_THREADS>(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// part[ntiles] = alpha = c sum of the tile shares, one workgroup, a fixed order
__global__ void __launch_bounds__(PC_THREADS) dac_alpha_kernel(double c, double *__restrict__ part, int64_t ntiles)
{
    __shared__ double red[PC_THREADS / 64];
    double s = 0.;
    for (int64_t k = threadIdx.x; k < ntiles; k += PC_THREADS) s += part[k];
    s = block_sum<PC_THREADS>(s, red);
    if (threadIdx.x == 0) part[ntiles] = c * s;
}

template <typename R>
__global__ void __launch_bounds__(PC_THREADS) dac_table_kernel(DacArgs a, const double *__restrict__ part, int64_t ntiles, Cx<R> *__restrict__ pf)
{
    const double alpha = part[ntiles];
    const int64_t base = (int64_t)blockIdx.x * PC_TILE;
    for (int k = threadIdx.x; k < PC_TILE; k += PC_THREADS) {
        if (base + k >= a.n) break;
        double nf, dr, di;
        dac_bin(a, base + k, &nf, &dr, &di);
        const double den = nf * (dr * dr + di * di) + alpha;
        stg(pf + base + k, Cx<R>{(R)(nf * dr / den), (R)(-nf * di / den)});
    }
}

// ------------------------------------------------------------------------------------------------ host side
inline bool grid_ok(int64_t n, int per) { return (n + per - 1) / per <= 0x7fffffffLL; }

// checks the level tables and the pattern length; *N = MI^mem_len
int levels_args(const char *who, const double *lev_I, int MI, const double *lev_Q, int MQ, const double *alphabet, int M, int mem_len, Levels *lv, int64_t *N)
{
    const bool rails = alphabet == nullptr;
    bool ok = mem_len >= 1 && mem_len <= PC_MEM_MAX;
    if (rails) ok = ok && lev_I && lev_Q && MI >= 2 && MI <= PC_M_MAX && MQ >= 2 && MQ <= MI;
    else ok = ok && !lev_I && !lev_Q && M >= 2 && M <= PC_M_MAX;
    int64_t n = 1;
    for (int j = 0; ok && j < mem_len; j++) {
        n *= rails ? MI : M;
        ok = n <= PC_N_MAX;
    }
    if (!ok) {
        set_error(std::string(who) + ": two sorted rail tables (2 <= MQ <= MI <= 4096) or one alphabet (2 <= M <= 4096), 1 <= mem_len <= 15 and M^mem_len <= 2^24");
        return QH_ERR_ARG;
    }
    lv->li = lev_I; lv->lq = lev_Q; lv->al = alphabet;
    lv->mi = MI; lv->mq = MQ; lv->mc = M; lv->mem_len = mem_len;
    *N = n;
    return QH_OK;
}

template <typename R>
int pattern_index_dev(const void *E, int nmodes, int64_t L, const double *lev_I, int MI, const double *lev_Q, int MQ, const double *alphabet, int M, int mem_len,
                      int32_t *idx_I, int32_t *idx_Q)
{
    int rc = ensure_init();
    if (rc) return rc;
    Levels lv;
    int64_t N;
    if ((rc = levels_args("pattern_index", lev_I, MI, lev_Q, MQ, alphabet, M, mem_len, &lv, &N))) return rc;
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 1 && L <= PC_ROW_MAX && grid_ok(L, PC_TILE), "pattern_index: bad sizes");
    QH_REQUIRE(E && (idx_I || idx_Q), "pattern_index: E and one of idx_I and idx_Q must be given");
    hipLaunchKernelGGL((pattern_kernel<R, 0>), dim3((unsigned)((L + PC_TILE - 1) / PC_TILE), nmodes), dim3(PC_THREADS), 0, g_stream, (const Cx<R> *)E, L, lv, idx_I, idx_Q,
                       (const double *)nullptr, (int64_t)0, 0., (Cx<R> *)nullptr);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R>
int lut_predistort_dev(const void *sig, int nmodes, int64_t L, const double *lev_I, int MI, const double *lev_Q, int MQ, const double *alphabet, int M, int mem_len,
                       const void *ea, int64_t N, double gain, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    Levels lv;
    int64_t need;
    if ((rc = levels_args("lut_predistort", lev_I, MI, lev_Q, MQ, alphabet, M, mem_len, &lv, &need))) return rc;
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 1 && L <= PC_ROW_MAX && grid_ok(L, PC_TILE), "lut_predistort: bad sizes");
    QH_REQUIRE(N == need, "lut_predistort: the table must hold M^mem_len entries");
    QH_REQUIRE(sig && ea && out && out != sig && std::isfinite(gain), "lut_predistort: sig, ea and out must be given, out another buffer than sig, gain finite");
    hipLaunchKernelGGL((pattern_kernel<R, 1>), dim3((unsigned)((L + PC_TILE - 1) / PC_TILE), nmodes), dim3(PC_THREADS), 0, g_stream, (const Cx<R> *)sig, L, lv,
                       (int32_t *)nullptr, (int32_t *)nullptr, (const double *)ea, N, gain, (Cx<R> *)out);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R>
int lut_apply_dev(const void *sig, int nmodes, int64_t L, const void *ea, int64_t N, const int32_t *idx_I, const int32_t *idx_Q, double gain, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 1 && L <= PC_ROW_MAX && grid_ok(L, PC_THREADS) && N >= 1 && N <= PC_N_MAX, "lut_apply: bad sizes");
    QH_REQUIRE(sig && ea && idx_I && idx_Q && out && std::isfinite(gain), "lut_apply: sig, ea, idx_I, idx_Q and out must be given, gain finite");
    hipLaunchKernelGGL((lut_apply_kernel<R>), dim3((unsigned)((L + PC_THREADS - 1) / PC_THREADS), nmodes), dim3(PC_THREADS), 0, g_stream, (const Cx<R> *)sig, L,
                       (const double *)ea, N, idx_I, idx_Q, gain, (Cx<R> *)out);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R>
int lut_accumulate_dev(const void *tx, const void *rx, int nmodes, int64_t L, const int32_t *idx_I, const int32_t *idx_Q, const uint8_t *mask, int mask_rows, int64_t N,
                       void *ea, int32_t *nI, int32_t *nQ)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 1 && L <= PC_LUT_LMAX && N >= 1 && N <= PC_N_MAX, "lut_accumulate: bad sizes (1 <= L <= 2^24, 1 <= N <= 2^24)");
    QH_REQUIRE(tx && rx && idx_I && idx_Q && ea && nI && nQ, "lut_accumulate: tx, rx, idx_I, idx_Q, ea, nI and nQ must be given");
    QH_REQUIRE(!mask || mask_rows == 1 || mask_rows == nmodes, "lut_accumulate: the mask is (L) or (nmodes, L)");
    const int64_t ntiles = (L + PC_MAX_TILE - 1) / PC_MAX_TILE, nchunk = (L + PC_LUT_CHUNK - 1) / PC_LUT_CHUNK;
    ScratchLayout lay;
    const size_t o_part = lay.take((size_t)nmodes * ntiles * sizeof(double)), o_scale = lay.take((size_t)nmodes * 2 * sizeof(double));
    void *base = nullptr;
    if ((rc = scratch(Slot::PRECOMP, lay.total, &base))) return rc;
    double *part = (double *)((char *)base + o_part), *scale = (double *)((char *)base + o_scale);
    int hb = 0;
    while (((int64_t)1 << hb) < L + 1) hb++;
    const int64_t mstride = mask && mask_rows == nmodes && nmodes > 1 ? L : 0;
    QH_HIP(hipMemsetAsync(ea, 0, (size_t)nmodes * N * 16, g_stream));
    QH_HIP(hipMemsetAsync(nI, 0, (size_t)nmodes * N * sizeof(int32_t), g_stream));
    QH_HIP(hipMemsetAsync(nQ, 0, (size_t)nmodes * N * sizeof(int32_t), g_stream));
    hipLaunchKernelGGL((lut_max_kernel<R>), dim3((unsigned)ntiles, nmodes), dim3(PC_THREADS), 0, g_stream, (const Cx<R> *)tx, (const Cx<R> *)rx, L, mask, mstride, part);
    hipLaunchKernelGGL(lut_scale_kernel, dim3(nmodes), dim3(PC_THREADS), 0, g_stream, (const double *)part, ntiles, hb, scale);
    const dim3 grid((unsigned)nchunk, nmodes);
    if (N <= PC_LDS_N)
        hipLaunchKernelGGL((lut_accum_kernel<R, true>), grid, dim3(PC_THREADS), 0, g_stream, (const Cx<R> *)tx, (const Cx<R> *)rx, L, idx_I, idx_Q, mask, mstride, N,
                           (const double *)scale, (unsigned long long *)ea, (unsigned int *)nI, (unsigned int *)nQ);
    else
        hipLaunchKernelGGL((lut_accum_kernel<R, false>), grid, dim3(PC_THREADS), 0, g_stream, (const Cx<R> *)tx, (const Cx<R> *)rx, L, idx_I, idx_Q, mask, mstride, N,
                           (const double *)scale, (unsigned long long *)ea, (unsigned int *)nI, (unsigned int *)nQ);
    hipLaunchKernelGGL(lut_final_kernel, dim3((unsigned)((N + PC_THREADS - 1) / PC_THREADS), nmodes), dim3(PC_THREADS), 0, g_stream, (double *)ea, N, (const double *)scale,
                       (const unsigned int *)nI, (const unsigned int *)nQ);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R>
int comp_mod_sin_dev(const void *sig, int nmodes, int64_t L, double vpi_re, double vpi_im, double clip, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 1 && L <= PC_ROW_MAX && grid_ok((int64_t)nmodes * L, PC_THREADS), "comp_mod_sin: bad sizes");
    QH_REQUIRE(sig && out && std::isfinite(vpi_re) && std::isfinite(vpi_im) && clip >= 0. && std::isfinite(clip),
               "comp_mod_sin: sig and out must be given, vpi finite, clip 0 (none) or positive");
    const int64_t total = (int64_t)nmodes * L;
    hipLaunchKernelGGL((mod_sin_kernel<R>), dim3((unsigned)((total + PC_THREADS - 1) / PC_THREADS)), dim3(PC_THREADS), 0, g_stream, (const Cx<R> *)sig, total, vpi_re, vpi_im,
                       clip, (Cx<R> *)out);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R>
int dac_preemphasis_table_dev(int64_t n, double fb, double fs, double beta, double c, const double *sos, int nsec, void *pf)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(n >= 1 && n <= PC_N_MAX, "dac_preemphasis_table: 1 <= sim_len <= 2^24");
    QH_REQUIRE(std::isfinite(fb) && fb > 0. && std::isfinite(fs) && fs > 0. && beta >= 0. && beta <= 1. && std::isfinite(c) && c >= 0.,
               "dac_preemphasis_table: fb and fs positive, 0 <= beta <= 1, the noise factor finite and not negative");
    QH_REQUIRE(sos && nsec >= 1 && nsec <= PC_SOS_MAX && pf, "dac_preemphasis_table: 1 to 4 sections and the table must be given");
    DacArgs a;
    a.n = n; a.fb = fb; a.fs = fs; a.beta = beta; a.c = c; a.nsec = nsec;
    for (int s = 0; s < PC_SOS_MAX; s++)
        for (int j = 0; j < 6; j++) {
            a.sos[s][j] = s < nsec ? sos[6 * s + j] : 0.;
            QH_REQUIRE(std::isfinite(a.sos[s][j]), "dac_preemphasis_table: the section coefficients must be finite");
        }
    const int64_t ntiles = (n + PC_TILE - 1) / PC_TILE;
    void *base = nullptr;
    if ((rc = scratch(Slot::PRECOMP, (size_t)(ntiles + 1) * sizeof(double), &base))) return rc;
    hipLaunchKernelGGL(dac_part_kernel, dim3((unsigned)ntiles), dim3(PC_THREADS), 0, g_stream, a, (double *)base);
    hipLaunchKernelGGL(dac_alpha_kernel, dim3(1), dim3(PC_THREADS), 0, g_stream, a.c, (double *)base, ntiles);
    hipLaunchKernelGGL((dac_table_kernel<R>), dim3((unsigned)ntiles), dim3(PC_THREADS), 0, g_stream, a, (const double *)base, ntiles, (Cx<R> *)pf);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

}  // namespace
}  // namespace qh

extern "C" {
int qh_pattern_index_c64_dev(const void *E, int nmodes, int64_t L, const double *lev_I, int MI, const double *lev_Q, int MQ, const double *alphabet, int M, int mem_len,
                             int32_t *idx_I, int32_t *idx_Q)
{ return qh::pattern_index_dev<float>(E, nmodes, L, lev_I, MI, lev_Q, MQ, alphabet, M, mem_len, idx_I, idx_Q); }
int qh_pattern_index_c128_dev(const void *E, int nmodes, int64_t L, const double *lev_I, int MI, const double *lev_Q, int MQ, const double *alphabet, int M, int mem_len,
                              int32_t *idx_I, int32_t *idx_Q)
{ return qh::pattern_index_dev<double>(E, nmodes, L, lev_I, MI, lev_Q, MQ, alphabet, M, mem_len, idx_I, idx_Q); }
int qh_lut_accumulate_c64_dev(const void *tx, const void *rx, int nmodes, int64_t L, const int32_t *idx_I, const int32_t *idx_Q, const uint8_t *mask, int mask_rows,
                              int64_t N, void *ea, int32_t *nI, int32_t *nQ)
{ return qh::lut_accumulate_dev<float>(tx, rx, nmodes, L, idx_I, idx_Q, mask, mask_rows, N, ea, nI, nQ); }
int qh_lut_accumulate_c128_dev(const void *tx, const void *rx, int nmodes, int64_t L, const int32_t *idx_I, const int32_t *idx_Q, const uint8_t *mask, int mask_rows,
                               int64_t N, void *ea, int32_t *nI, int32_t *nQ)
{ return qh::lut_accumulate_dev<double>(tx, rx, nmodes, L, idx_I, idx_Q, mask, mask_rows, N, ea, nI, nQ); }
int qh_lut_apply_c64_dev(const void *sig, int nmodes, int64_t L, const void *ea, int64_t N, const int32_t *idx_I, const int32_t *idx_Q, double gain, void *out)
{ return qh::lut_apply_dev<float>(sig, nmodes, L, ea, N, idx_I, idx_Q, gain, out); }
int qh_lut_apply_c128_dev(const void *sig, int nmodes, int64_t L, const void *ea, int64_t N, const int32_t *idx_I, const int32_t *idx_Q, double gain, void *out)
{ return qh::lut_apply_dev<double>(sig, nmodes, L, ea, N, idx_I, idx_Q, gain, out); }
int qh_lut_predistort_c64_dev(const void *sig, int nmodes, int64_t L, const double *lev_I, int MI, const double *lev_Q, int MQ, const double *alphabet, int M, int mem_len,
                              const void *ea, int64_t N, double gain, void *out)
{ return qh::lut_predistort_dev<float>(sig, nmodes, L, lev_I, MI, lev_Q, MQ, alphabet, M, mem_len, ea, N, gain, out); }
int qh_lut_predistort_c128_dev(const void *sig, int nmodes, int64_t L, const double *lev_I, int MI, const double *lev_Q, int MQ, const double *alphabet, int M, int mem_len,
                               const void *ea, int64_t N, double gain, void *out)
{ return qh::lut_predistort_dev<double>(sig, nmodes, L, lev_I, MI, lev_Q, MQ, alphabet, M, mem_len, ea, N, gain, out); }
int qh_comp_mod_sin_c64_dev(const void *sig, int nmodes, int64_t L, double vpi_re, double vpi_im, double clip, void *out)
{ return qh::comp_mod_sin_dev<float>(sig, nmodes, L, vpi_re, vpi_im, clip, out); }
int qh_comp_mod_sin_c128_dev(const void *sig, int nmodes, int64_t L, double vpi_re, double vpi_im, double clip, void *out)
{ return qh::comp_mod_sin_dev<double>(sig, nmodes, L, vpi_re, vpi_im, clip, out); }
int qh_dac_preemphasis_table_c64_dev(int64_t sim_len, double fb, double fs, double beta, double noise, const double *sos, int nsec, void *p_f)
{ return qh::dac_preemphasis_table_dev<float>(sim_len, fb, fs, beta, noise, sos, nsec, p_f); }
int qh_dac_preemphasis_table_c128_dev(int64_t sim_len, double fb, double fs, double beta, double noise, const double *sos, int nsec, void *p_f)
{ return qh::dac_preemphasis_table_dev<double>(sim_len, fb, fs, beta, noise, sos, nsec, p_f); }
}
