// Transmitter response on a field that already lies in HBM (qampy/core/impairments.py:370-671, qampy/core/filter.py:86-147): the DAC - clip,
// quantise, ENOB noise, a Bessel / Butterworth low-pass as second-order sections -, an ideal amplifier and the IQ modulator.
//
// Row extrema (2 launches): ext[m] = (max |re|, max |im|) of row m in double - per-tile maxima, then one workgroup per row.  A maximum does
// not depend on the order, so the result is bit-reproducible.  The consumers form the maximum of a row and of the whole field from it.
//
// DAC point-wise pass (1 launch): clip, quantise, noise, each optional, in double up to the noise, which is added in the precision of the
// signal exactly as impair.hip adds it (same Philox stream: a draw depends on (seed, mode, n) only).  One extrema pass in front serves all
// three stages: after clipping every row's maximum is min(1 / clip_rat, 1), after quantising (1 - delta / 2) max_swing.
//
// Sections filter (3 launches), scipy.signal.sosfilt with zero initial state, exact and parallel in time.  A lane owns SOS_C consecutive
// samples, a workgroup of one wave SOS_W * SOS_C.  Coefficients and state are double in both precisions.
//   (1) every lane runs the cascade over its chunk from a zero state; a log-step scan over the wave with P^(2^d), P = M^SOS_C the
//       zero-input transition of the cascade over one chunk, leaves the tile's end state from a zero start in the last lane.
//   (2) one wave per row carries the tile states: a lane walks its run of tiles with Q = P^SOS_W, the wave scans with (Q^run)^(2^d), the
//       lane walks again and leaves every tile's true start state.
//   (3) every lane repeats (1) with the tile's start state folded into lane 0, takes its own start state from its left neighbour, runs its
//       chunk again and writes.
// A lane's chunk is contiguous, so a tile goes through LDS in blocks of SOS_J samples per lane: the wave loads 64 runs of SOS_J samples
// (128 bytes of complex64 each) and every lane reads its own run.  The matrices travel as kernel arguments (at most 3744 bytes).
// Samples past the end of a row enter as zeros: a partial chunk's end state feeds only lanes that own nothing.
//
// Modulator (1 launch): an optional amplifier x / max * tgt_v with the maximum over all rows, then modulator_response.  Every angle is
// formed in double as turns and reduced modulo one turn before the sine and cosine, in both precisions.
#include "common.h"
#include "philox.h"
#include <cmath>

namespace qh {

constexpr int TX_T = 256, TX_PER = 4, TX_TILE = TX_T * TX_PER;          // the point-wise passes: impair.hip's geometry
constexpr int EXT_PER = 16, EXT_TILE = TX_T * EXT_PER;                  // samples of one row per workgroup of the extrema pass
constexpr int TX_MAXMODES = 1024;                                       // every workgroup reads all row extrema
constexpr int SOS_C = 128, SOS_W = 64, SOS_J = 16, SOS_T = SOS_C * SOS_W, SOS_MAXSEC = 4;

// ------------------------------------------------------------------------------------------------ extrema
__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// grid (ntiles, nmodes): part[mode][tile] = (max |re|, max |im|) of the tile
template <typename R> __global__ void __launch_bounds__(TX_T) extrema_part_kernel(const Cx<R> *__restrict__ E, int64_t L, double *__restrict__ part)
{
    __shared__ double red[2][TX_T / 64];
    const int mode = blockIdx.y;
    double a = 0, b = 0;
    for (int i = 0; i < EXT_PER; i++) {
        const int64_t n = (int64_t)blockIdx.x * EXT_TILE + i * TX_T + threadIdx.x;
        if (n >= L) break;
        const Cx<R> v = ldg(E + (size_t)mode * L + n);
        a = fmax(a, (double)abs_(v.re));
        b = fmax(b, (double)abs_(v.im));
    }
    a = wave_max(a); b = wave_max(b);
    if (threadIdx.x % 64 == 0) { red[0][threadIdx.x / 64] = a; red[1][threadIdx.x / 64] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < TX_T / 64; q++) { a = fmax(a, red[0][q]); b = fmax(b, red[1][q]); }
        double *p = part + 2 * ((size_t)mode * gridDim.x + blockIdx.x);
        p[0] = a; p[1] = b;
    }
}

// grid (nmodes): ext[mode] = the maxima over the row's tiles
__global__ void __launch_bounds__(TX_T) extrema_final_kernel(const double *__restrict__ part, int64_t ntiles, double *__restrict__ ext)
{
    __shared__ double red[2][TX_T / 64];
    const double *p = part + 2 * (size_t)blockIdx.x * ntiles;
    double a = 0, b = 0;
    for (int64_t i = threadIdx.x; i < ntiles; i += TX_T) { a = fmax(a, p[2 * i]); b = fmax(b, p[2 * i + 1]); }
    a = wave_max(a); b = wave_max(b);
    if (threadIdx.x % 64 == 0) { red[0][threadIdx.x / 64] = a; red[1][threadIdx.x / 64] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < TX_T / 64; q++) { a = fmax(a, red[0][q]); b = fmax(b, red[1][q]); }
        ext[2 * blockIdx.x] = a; ext[2 * blockIdx.x + 1] = b;
    }
}

// (maximum of the row, maximum over all rows) from the extrema buffer
__device__ __forceinline__ void ext_maxima(const double *__restrict__ ext, int nmodes, int mode, double &row, double &all)
{
    row = fmax(ext[2 * mode], ext[2 * mode + 1]);
    all = 0;
    for (int m = 0; m < nmodes; m++) all = fmax(all, fmax(ext[2 * m], ext[2 * m + 1]));
}

// ------------------------------------------------------------------------------------------------ DAC, point-wise
struct DacPrm {
    int clip, nbits, noise;          // stages; nbits 0: no quantiser
    double inv_clip;                 // 1 / clip_rat
    double enob_pow;                 // 2^(enob - 1)
    unsigned k0, k1;
};

// number of thresholds -1 + k delta, k = 1 .. 2^n - 1, that are <= u (np.digitize(..., right=False)): floor((u + 1) / delta), put right
// against the exact thresholds where u + 1 rounded, and clamped
__device__ __forceinline__ double dac_level(double u, double half, double delta, double top)
{
    double k = floor((u + 1.0) * half);
    k = fmin(fmax(k, -1.0), top + 1.0);
    const double t = fma(k, delta, -1.0);                               // exact: a multiple of delta of magnitude <= 1
    if (u < t) k -= 1.0;
    else if (u >= t + delta) k += 1.0;
    k = fmin(fmax(k, 0.0), top);
    return fma(k, delta, -1.0 + 0.5 * delta);
}

// grid (ntiles, nmodes); out == E is allowed: a thread reads the elements it writes
template <typename R>
__global__ void __launch_bounds__(TX_T) dac_pointwise_kernel(const Cx<R> *E, Cx<R> *out, int64_t L, int nmodes, const double *__restrict__ ext, DacPrm p)
{
    const int mode = blockIdx.y;
    double rm, gm;
    ext_maxima(ext, nmodes, mode, rm, gm);
    const double c_rm = rm;
    if (p.clip) rm = gm = fmin(p.inv_clip, 1.0);
    const double q_rm = rm, q_gm = gm;
    const double half = ldexp(1.0, p.nbits - 1), delta = 1.0 / half, top = 2.0 * half - 1.0;
    if (p.nbits) rm = gm = (1.0 - 0.5 * delta) * q_gm;
    const double d_enob = gm / p.enob_pow;
    const double sg = p.noise ? sqrt(2.0 * (d_enob * d_enob) / 12.0) : 0.0;
    const R s_iq = (R)(sg * 0.70710678118654752440);
    const bool noisy = p.noise && sg != 0.0;
    const int64_t n0 = (int64_t)blockIdx.x * TX_TILE + (int64_t)threadIdx.x * TX_PER;
#pragma unroll
    for (int i = 0; i < TX_PER; i++) {
        const int64_t n = n0 + i;
        if (n >= L) break;
        Cx<R> x = ldg(E + (size_t)mode * L + n);
        if (p.clip || p.nbits) {
            double vr = (double)x.re, vi = (double)x.im;
            if (p.clip) {
                vr = vr / c_rm * p.inv_clip; vi = vi / c_rm * p.inv_clip;
                vr = copysign(fmin(fabs(vr), 1.0), vr); vi = copysign(fmin(fabs(vi), 1.0), vi);
            }
            if (p.nbits) {
                vr = dac_level(vr / q_rm, half, delta, top) * q_gm;
                vi = dac_level(vi / q_rm, half, delta, top) * q_gm;
            }
            x = Cx<R>{(R)vr, (R)vi};
        }
        if (noisy) {
            R g0, g1;
            imp_gauss(n, mode, IMP_STREAM_NOISE, p.k0, p.k1, g0, g1);
            x = Cx<R>{fma_(s_iq, g0, x.re), fma_(s_iq, g1, x.im)};
        }
        stg(out + (size_t)mode * L + n, x);
    }
}

// ------------------------------------------------------------------------------------------------ amplifier and modulator
struct ModPrm {
    int amp;
    double tgt;                      // amplifier: x / max * tgt
    double dr, di;                   // dcbias of I and Q
    double gr, gi;                   // gfactr of I and Q
    double pr, mr, pi, mi;           // (1 + cfactr) / 4 and (1 - cfactr) / 4, I and Q: turns per volt
    double ar, ai, br, bi;           // what multiplies the I and the Q arm: outer bias, outer gain and the arms' -1 / (1 + gfactr)
};

template <typename R> __device__ __forceinline__ void sincos_turns(double t, double &s, double &c)
{
    t -= rint(t);
    if constexpr (sizeof(R) == 4) {
        float sf, cf;
        sincosf((float)(IMP_TWO_PI * t), &sf, &cf);
        s = sf; c = cf;
    } else sincos(IMP_TWO_PI * t, &s, &c);
}

// exp(j pi v (1 + c) / 2) + g exp(-j pi v (1 - c) / 2)
template <typename R> __device__ __forceinline__ void mzm_arm(double v, double kp, double km, double g, double &re, double &im)
{
    double s1, c1, s2, c2;
    sincos_turns<R>(v * kp, s1, c1);
    sincos_turns<R>(v * km, s2, c2);
    re = fma(g, c2, c1);
    im = fma(-g, s2, s1);
}

template <typename R>
__global__ void __launch_bounds__(TX_T) modulator_kernel(const Cx<R> *E, Cx<R> *out, int64_t L, int nmodes, const double *__restrict__ ext, ModPrm p)
{
    const int mode = blockIdx.y;
    double rm = 1, gm = 1;
    if (p.amp) ext_maxima(ext, nmodes, mode, rm, gm);
    const int64_t n0 = (int64_t)blockIdx.x * TX_TILE + (int64_t)threadIdx.x * TX_PER;
#pragma unroll
    for (int i = 0; i < TX_PER; i++) {
        const int64_t n = n0 + i;
        if (n >= L) break;
        const Cx<R> x = ldg(E + (size_t)mode * L + n);
        double vr = (double)x.re, vi = (double)x.im;
        if (p.amp) { vr = vr / gm * p.tgt; vi = vi / gm * p.tgt; }
        vr += p.dr; vi += p.di;
        double ir, ii, qr, qi;
        mzm_arm<R>(vr, p.pr, p.mr, p.gr, ir, ii);
        mzm_arm<R>(vi, p.pi, p.mi, p.gi, qr, qi);
        const double yr = p.ar * ir - p.ai * ii + p.br * qr - p.bi * qi;
        const double yi = p.ar * ii + p.ai * ir + p.br * qi + p.bi * qr;
        stg(out + (size_t)mode * L + n, Cx<R>{(R)yr, (R)yi});
    }
}

// ------------------------------------------------------------------------------------------------ sections filter
template <int NS> struct SosCoef { double c[NS][5]; };                  // b0 b1 b2 a1 a2 of every section (a0 = 1)
template <int NS> struct SosPow { double m[7][4 * NS * NS]; };          // seven (2 NS) x (2 NS) matrices, row-major

// one sample through the cascade (direct form II transposed, the recurrence of scipy's sosfilt); x becomes the output
template <int NS> __device__ __forceinline__ void sos_step(const SosCoef<NS> &k, double (&z)[2 * NS], double &x)
{
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const double y = fma(k.c[s][0], x, z[2 * s]);
        z[2 * s] = fma(k.c[s][1], x, fma(-k.c[s][3], y, z[2 * s + 1]));
        z[2 * s + 1] = fma(k.c[s][2], x, -k.c[s][4] * y);
        x = y;
    }
}

// acc += M v
template <int NS> __device__ __forceinline__ void sos_matvec_add(const double *M, const double (&v)[2 * NS], double (&acc)[2 * NS])
{
#pragma unroll
    for (int r = 0; r < 2 * NS; r++) {
        double a = acc[r];
#pragma unroll
        for (int c = 0; c < 2 * NS; c++) a = fma(M[r * 2 * NS + c], v[c], a);
        acc[r] = a;
    }
}

// inclusive scan over the wave: afterwards lane k holds sum_{i <= k} (m[0])^(k - i) v_i, given m[d] = (m[0])^(2^d)
template <int NS> __device__ __forceinline__ void sos_wave_scan(const SosPow<NS> &pw, int lane, double (&zr)[2 * NS], double (&zi)[2 * NS])
{
#pragma unroll
    for (int d = 0; d < 6; d++) {
        double ur[2 * NS], ui[2 * NS];
#pragma unroll
        for (int i = 0; i < 2 * NS; i++) { ur[i] = __shfl_up(zr[i], 1 << d); ui[i] = __shfl_up(zi[i], 1 << d); }
        if (lane >= (1 << d)) {
            sos_matvec_add<NS>(pw.m[d], ur, zr);
            sos_matvec_add<NS>(pw.m[d], ui, zi);
        }
    }
}

// the lane's chunk of the tile that starts at sample `base` of the row x, SOS_J samples per lane at a time through LDS
template <typename R, int NS, bool WRITE>
__device__ __forceinline__ void sos_pass(const Cx<R> *x, Cx<R> *y, int64_t base, int64_t L, Cx<R> *buf, const SosCoef<NS> &k, double (&zr)[2 * NS],
                                         double (&zi)[2 * NS])
{
    const int lane = threadIdx.x;
    for (int jb = 0; jb < SOS_C / SOS_J; jb++) {
        if (base + (int64_t)jb * SOS_J >= L) break;                    // uniform: the first lane's samples of this block lie past the row already
#pragma unroll
        for (int i = 0; i < SOS_J; i++) {
            const int e = lane + SOS_W * i, q = e / SOS_J, jj = e % SOS_J;
            const int64_t n = base + (int64_t)q * SOS_C + jb * SOS_J + jj;
            buf[q * (SOS_J + 1) + jj] = n < L ? ldg(x + n) : Cx<R>{(R)0, (R)0};
        }
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < SOS_J; jj++) {
            const Cx<R> v = buf[lane * (SOS_J + 1) + jj];
            double xr = (double)v.re, xi = (double)v.im;
            sos_step<NS>(k, zr, xr);
            sos_step<NS>(k, zi, xi);
            if (WRITE) buf[lane * (SOS_J + 1) + jj] = Cx<R>{(R)xr, (R)xi};
        }
        __syncthreads();
        if (WRITE) {
#pragma unroll
            for (int i = 0; i < SOS_J; i++) {
                const int e = lane + SOS_W * i, q = e / SOS_J, jj = e % SOS_J;
                const int64_t n = base + (int64_t)q * SOS_C + jb * SOS_J + jj;
                if (n < L) stg(y + n, buf[q * (SOS_J + 1) + jj]);
            }
            __syncthreads();
        }
    }
}

// launches (1) and (3), grid (ntiles, nmodes), one wave.  WRITE = false: st[mode][tile] = the tile's end state from a zero start.
// WRITE = true: st[mode][tile] is the tile's start state; the filtered tile goes to out (out == E is allowed: a workgroup has read its
// tile before it writes the block it then reads again, and touches no other tile).
template <typename R, int NS, bool WRITE>
__global__ void __launch_bounds__(SOS_W) sos_tile_kernel(const Cx<R> *E, Cx<R> *out, int64_t L, SosCoef<NS> k, SosPow<NS> pw, double *st)
{
    __shared__ Cx<R> buf[SOS_W * (SOS_J + 1)];
    const int lane = threadIdx.x, mode = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * SOS_T;
    const Cx<R> *x = E + (size_t)mode * L;
    double *s = st + ((size_t)mode * gridDim.x + blockIdx.x) * 4 * NS;
    double zr[2 * NS], zi[2 * NS];
#pragma unroll
    for (int i = 0; i < 2 * NS; i++) zr[i] = zi[i] = 0;
    sos_pass<R, NS, false>(x, nullptr, base, L, buf, k, zr, zi);
    if (WRITE) {
        double sr[2 * NS], si[2 * NS];
#pragma unroll
        for (int i = 0; i < 2 * NS; i++) { sr[i] = s[i]; si[i] = s[2 * NS + i]; }
        if (lane == 0) {
            sos_matvec_add<NS>(pw.m[0], sr, zr);
            sos_matvec_add<NS>(pw.m[0], si, zi);
        }
        sos_wave_scan<NS>(pw, lane, zr, zi);
#pragma unroll
        for (int i = 0; i < 2 * NS; i++) {
            const double ur = __shfl_up(zr[i], 1), ui = __shfl_up(zi[i], 1);
            zr[i] = lane ? ur : sr[i];
            zi[i] = lane ? ui : si[i];
        }
        sos_pass<R, NS, true>(x, out + (size_t)mode * L, base, L, buf, k, zr, zi);
    } else {
        sos_wave_scan<NS>(pw, lane, zr, zi);
        if (lane == SOS_W - 1) {
#pragma unroll
            for (int i = 0; i < 2 * NS; i++) { s[i] = zr[i]; s[2 * NS + i] = zi[i]; }
        }
    }
}

// launch (2), grid (nmodes), one wave: st[mode][tile] end states from a zero start -> true start states.  Lane k owns the tiles
// [k per, (k + 1) per); pw.m[6] = Q, the transition over one tile, pw.m[d] = (Q^per)^(2^d).
template <int NS> __global__ void __launch_bounds__(SOS_W) sos_carry_kernel(double *st, int64_t ntiles, int64_t per, SosPow<NS> pw)
{
    const int lane = threadIdx.x;
    double *row = st + (size_t)blockIdx.x * ntiles * 4 * NS;
    const int64_t lo = lane * per < ntiles ? lane * per : ntiles, hi = lo + per < ntiles ? lo + per : ntiles;
    double zr[2 * NS], zi[2 * NS];
#pragma unroll
    for (int i = 0; i < 2 * NS; i++) zr[i] = zi[i] = 0;
    for (int64_t t = lo; t < hi; t++) {
        double nr[2 * NS], ni[2 * NS];
#pragma unroll
        for (int i = 0; i < 2 * NS; i++) { nr[i] = row[t * 4 * NS + i]; ni[i] = row[t * 4 * NS + 2 * NS + i]; }
        sos_matvec_add<NS>(pw.m[6], zr, nr);
        sos_matvec_add<NS>(pw.m[6], zi, ni);
#pragma unroll
        for (int i = 0; i < 2 * NS; i++) { zr[i] = nr[i]; zi[i] = ni[i]; }
    }
    sos_wave_scan<NS>(pw, lane, zr, zi);
#pragma unroll
    for (int i = 0; i < 2 * NS; i++) {
        const double ur = __shfl_up(zr[i], 1), ui = __shfl_up(zi[i], 1);
        zr[i] = lane ? ur : 0.0;
        zi[i] = lane ? ui : 0.0;
    }
    for (int64_t t = lo; t < hi; t++) {
        double nr[2 * NS], ni[2 * NS];
#pragma unroll
        for (int i = 0; i < 2 * NS; i++) {
            nr[i] = row[t * 4 * NS + i]; ni[i] = row[t * 4 * NS + 2 * NS + i];
            row[t * 4 * NS + i] = zr[i]; row[t * 4 * NS + 2 * NS + i] = zi[i];
        }
        sos_matvec_add<NS>(pw.m[6], zr, nr);
        sos_matvec_add<NS>(pw.m[6], zi, ni);
#pragma unroll
        for (int i = 0; i < 2 * NS; i++) { zr[i] = nr[i]; zi[i] = ni[i]; }
    }
}

// ------------------------------------------------------------------------------------------------ host side
static bool tx_sizes_ok(int nmodes, int64_t L) { return nmodes >= 1 && nmodes <= TX_MAXMODES && L >= 0 && (L + TX_TILE - 1) / TX_TILE <= 0x7fffffffLL; }

// scratch slot Slot::TXRESP: the row extrema a call forms for itself (own_extrema), at its base | the tile extrema, at *part
static int extrema_scratch(int nmodes, int64_t ntiles, void **base, double **part)
{
    ScratchLayout lay;
    lay.take(2 * (size_t)nmodes * sizeof(double));
    const size_t o_part = lay.take(2 * (size_t)nmodes * ntiles * sizeof(double));
    int rc = scratch(Slot::TXRESP, lay.total, base);
    if (rc) return rc;
    *part = (double *)((char *)*base + o_part);
    return QH_OK;
}

// ext: nmodes pairs of doubles on the device
template <typename R> int row_extrema_dev(const void *E, int nmodes, int64_t L, double *ext)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(E && ext && tx_sizes_ok(nmodes, L) && L >= 1, "row_extrema: E, ext, 1 to 1024 modes, at least one sample");
    const int64_t ntiles = (L + EXT_TILE - 1) / EXT_TILE;
    void *base = nullptr;
    double *part = nullptr;
    if ((rc = extrema_scratch(nmodes, ntiles, &base, &part))) return rc;
    hipLaunchKernelGGL((extrema_part_kernel<R>), dim3((unsigned)ntiles, nmodes), dim3(TX_T), 0, g_stream, (const Cx<R> *)E, L, part);
    hipLaunchKernelGGL(extrema_final_kernel, dim3(nmodes), dim3(TX_T), 0, g_stream, (const double *)part, ntiles, ext);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

// the extrema a call forms for itself live at the head of the scratch slot whose tail holds the tile maxima
template <typename R> static int own_extrema(const void *E, int nmodes, int64_t L, const double **ext)
{
    void *base = nullptr;
    double *part = nullptr;
    int rc = extrema_scratch(nmodes, (L + EXT_TILE - 1) / EXT_TILE, &base, &part);
    if (rc) return rc;
    *ext = (const double *)base;
    return row_extrema_dev<R>(E, nmodes, L, (double *)base);
}

// stages: bit 0 clip, bit 1 quantise, bit 2 ENOB noise.  ext: the row extrema of E, or nullptr (formed here).
template <typename R>
int dac_pointwise_dev(const void *E, int nmodes, int64_t L, const double *ext, int stages, double clip_rat, int quant_bits, double enob, uint64_t seed, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(E && out && tx_sizes_ok(nmodes, L), "dac_pointwise: E, out, 1 to 1024 modes");
    QH_REQUIRE(stages >= 0 && stages <= 7, "dac_pointwise: stages is a mask of 1 (clip), 2 (quantise), 4 (ENOB noise)");
    QH_REQUIRE(!(stages & 1) || (std::isfinite(clip_rat) && clip_rat > 0), "dac_pointwise: clip_rat must be positive");
    QH_REQUIRE(!(stages & 2) || (quant_bits >= 1 && quant_bits <= 16), "dac_pointwise: 1 to 16 quantiser bits");
    QH_REQUIRE(!(stages & 4) || (std::isfinite(enob) && enob > 0), "dac_pointwise: enob must be positive");
    if (L == 0) return QH_OK;
    if (!stages) {
        if (out != E) QH_HIP(hipMemcpyAsync(out, E, (size_t)nmodes * L * sizeof(Cx<R>), hipMemcpyDeviceToDevice, g_stream));
        return QH_OK;
    }
    if (!ext && (rc = own_extrema<R>(E, nmodes, L, &ext))) return rc;
    DacPrm p;
    p.clip = stages & 1; p.nbits = (stages & 2) ? quant_bits : 0; p.noise = (stages & 4) ? 1 : 0;
    p.inv_clip = p.clip ? 1.0 / clip_rat : 1.0;
    p.enob_pow = p.noise ? exp2(enob - 1.0) : 1.0;
    p.k0 = (unsigned)seed; p.k1 = (unsigned)(seed >> 32);
    hipLaunchKernelGGL((dac_pointwise_kernel<R>), dim3((unsigned)((L + TX_TILE - 1) / TX_TILE), nmodes), dim3(TX_T), 0, g_stream, (const Cx<R> *)E, (Cx<R> *)out, L,
                       nmodes, ext, p);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

// prm: dcbias re, im, gfactr re, im, cfactr re, im, dcbias_out, gfactr_out (host).  have_amp: x / max * tgt_v first, the maximum over all
// rows from ext (nullptr: formed here).
template <typename R> int modulator_dev(const void *E, int nmodes, int64_t L, const double *ext, int have_amp, double tgt_v, const double *prm, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(E && out && prm && tx_sizes_ok(nmodes, L), "modulator: E, out, the parameters, 1 to 1024 modes");
    for (int i = 0; i < 8; i++) QH_REQUIRE(std::isfinite(prm[i]), "modulator: the parameters must be finite");
    QH_REQUIRE(!have_amp || std::isfinite(tgt_v), "modulator: the target voltage must be finite");
    if (L == 0) return QH_OK;
    if (have_amp && !ext && (rc = own_extrema<R>(E, nmodes, L, &ext))) return rc;
    ModPrm p;
    p.amp = have_amp ? 1 : 0; p.tgt = tgt_v;
    p.dr = prm[0]; p.di = prm[1]; p.gr = prm[2]; p.gi = prm[3];
    p.pr = (1 + prm[4]) / 4; p.mr = (1 - prm[4]) / 4; p.pi = (1 + prm[5]) / 4; p.mi = (1 - prm[5]) / 4;
    const double d = prm[6], go = prm[7];
    const double ca = cos(QH_PI / 4 - QH_PI * d / 2), sa = sin(QH_PI / 4 - QH_PI * d / 2), cb = cos(QH_PI / 4 + QH_PI * d / 2), sb = sin(QH_PI / 4 + QH_PI * d / 2);
    const double fa = -1.0 / ((1 + go) * (1 + p.gr)), fb = -go / ((1 + go) * (1 + p.gi));
    p.ar = fa * ca; p.ai = fa * sa; p.br = fb * cb; p.bi = fb * sb;
    hipLaunchKernelGGL((modulator_kernel<R>), dim3((unsigned)((L + TX_TILE - 1) / TX_TILE), nmodes), dim3(TX_T), 0, g_stream, (const Cx<R> *)E, (Cx<R> *)out, L, nmodes,
                       ext, p);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

// The powers of the transition matrix are formed in extended precision and rounded once: for a narrow low-pass its entries reach 1e9 and
// cancel in every product, and squaring in double loses seven digits (the filtered field is then off by 3e-12 of the input rms, not 5e-14).
typedef long double xreal;
constexpr int SOS_NN = 4 * SOS_MAXSEC * SOS_MAXSEC;
// C = A B, n x n row-major
static void mat_mul(const xreal *A, const xreal *B, xreal *C, int n)
{
    xreal T[SOS_NN];
    for (int r = 0; r < n; r++)
        for (int c = 0; c < n; c++) {
            xreal a = 0;
            for (int k = 0; k < n; k++) a += A[r * n + k] * B[k * n + c];
            T[r * n + c] = a;
        }
    for (int i = 0; i < n * n; i++) C[i] = T[i];
}
// m[d] = A^(2^d), d = 0 .. 5; next = A^64
static void mat_squares(const xreal *A, xreal (*m)[SOS_NN], xreal *next, int n)
{
    for (int i = 0; i < n * n; i++) m[0][i] = A[i];
    for (int d = 1; d < 6; d++) mat_mul(m[d - 1], m[d - 1], m[d], n);
    mat_mul(m[5], m[5], next, n);
}
static void mat_power(const xreal *A, int64_t e, xreal *out, int n)
{
    xreal b[SOS_NN], r[SOS_NN];
    for (int i = 0; i < n * n; i++) { b[i] = A[i]; r[i] = (i / n == i % n) ? 1.0L : 0.0L; }
    for (; e > 0; e >>= 1) {
        if (e & 1) mat_mul(r, b, r, n);
        mat_mul(b, b, b, n);
    }
    for (int i = 0; i < n * n; i++) out[i] = r[i];
}

template <typename R, int NS> static int sosfilt_launch(const Cx<R> *E, Cx<R> *out, int nmodes, int64_t L, const double *sos, const double *P)
{
    constexpr int n = 2 * NS;
    SosCoef<NS> k;
    for (int s = 0; s < NS; s++) {
        k.c[s][0] = sos[6 * s]; k.c[s][1] = sos[6 * s + 1]; k.c[s][2] = sos[6 * s + 2]; k.c[s][3] = sos[6 * s + 4]; k.c[s][4] = sos[6 * s + 5];
    }
    const int64_t ntiles = (L + SOS_T - 1) / SOS_T, per = (ntiles + SOS_W - 1) / SOS_W;
    xreal P0[SOS_NN], wave[6][SOS_NN], Q[SOS_NN], Rp[SOS_NN], carry[6][SOS_NN], unused[SOS_NN];
    for (int i = 0; i < n * n; i++) P0[i] = P[i];
    mat_squares(P0, wave, Q, n);
    mat_power(Q, per, Rp, n);
    mat_squares(Rp, carry, unused, n);
    SosPow<NS> pt, pc;
    for (int d = 0; d < 6; d++)
        for (int i = 0; i < n * n; i++) { pt.m[d][i] = (double)wave[d][i]; pc.m[d][i] = (double)carry[d][i]; }
    for (int i = 0; i < n * n; i++) { pt.m[6][i] = (double)Q[i]; pc.m[6][i] = (double)Q[i]; }
    void *base = nullptr;
    int rc;
    if ((rc = scratch(Slot::SOS, (size_t)nmodes * ntiles * 2 * n * sizeof(double), &base))) return rc;
    double *st = (double *)base;
    const dim3 grid((unsigned)ntiles, nmodes);
    if (ntiles > 1) {
        hipLaunchKernelGGL((sos_tile_kernel<R, NS, false>), grid, dim3(SOS_W), 0, g_stream, E, (Cx<R> *)nullptr, L, k, pt, st);
        hipLaunchKernelGGL((sos_carry_kernel<NS>), dim3(nmodes), dim3(SOS_W), 0, g_stream, st, ntiles, per, pc);
    } else
        QH_HIP(hipMemsetAsync(st, 0, (size_t)nmodes * 2 * n * sizeof(double), g_stream));      // one tile: it starts from the zero state
    hipLaunchKernelGGL((sos_tile_kernel<R, NS, true>), grid, dim3(SOS_W), 0, g_stream, E, out, L, k, pt, st);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

// sos: nsec rows of b0 b1 b2 a0 a1 a2 with a0 = 1 (host); P: the (2 nsec)^2 zero-input transition of the cascade over SOS_C samples (host)
template <typename R> int sosfilt_dev(const void *E, int nmodes, int64_t L, const double *sos, int nsec, const double *P, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(E && out && sos && P && nmodes >= 1 && nmodes <= 65535 && L >= 0 && (L + SOS_T - 1) / SOS_T <= 0x7fffffffLL, "sosfilt: bad arguments");
    QH_REQUIRE(nsec >= 1 && nsec <= SOS_MAXSEC, "sosfilt: 1 to 4 sections");
    for (int i = 0; i < 6 * nsec; i++) QH_REQUIRE(std::isfinite(sos[i]), "sosfilt: the coefficients must be finite");
    for (int i = 0; i < 4 * nsec * nsec; i++) QH_REQUIRE(std::isfinite(P[i]), "sosfilt: the transition matrix must be finite");
    for (int s = 0; s < nsec; s++) QH_REQUIRE(sos[6 * s + 3] == 1.0, "sosfilt: every section is normalised to a0 = 1");
    if (L == 0) return QH_OK;
    const Cx<R> *e = (const Cx<R> *)E;
    Cx<R> *o = (Cx<R> *)out;
    switch (nsec) {
    case 1: return sosfilt_launch<R, 1>(e, o, nmodes, L, sos, P);
    case 2: return sosfilt_launch<R, 2>(e, o, nmodes, L, sos, P);
    case 3: return sosfilt_launch<R, 3>(e, o, nmodes, L, sos, P);
    default: return sosfilt_launch<R, 4>(e, o, nmodes, L, sos, P);
    }
}

}  // namespace qh

extern "C" {
int qh_sos_geometry(int *chunk, int *tile)
{
    if (chunk) *chunk = qh::SOS_C;
    if (tile) *tile = qh::SOS_T;
    return QH_OK;
}
int qh_row_extrema_c64_dev(const void *E, int nmodes, int64_t L, double *ext) { return qh::row_extrema_dev<float>(E, nmodes, L, ext); }
int qh_row_extrema_c128_dev(const void *E, int nmodes, int64_t L, double *ext) { return qh::row_extrema_dev<double>(E, nmodes, L, ext); }
int qh_dac_pointwise_c64_dev(const void *E, int nmodes, int64_t L, const double *ext, int stages, double clip_rat, int quant_bits, double enob, uint64_t seed,
                             void *out)
{ return qh::dac_pointwise_dev<float>(E, nmodes, L, ext, stages, clip_rat, quant_bits, enob, seed, out); }
int qh_dac_pointwise_c128_dev(const void *E, int nmodes, int64_t L, const double *ext, int stages, double clip_rat, int quant_bits, double enob, uint64_t seed,
                              void *out)
{ return qh::dac_pointwise_dev<double>(E, nmodes, L, ext, stages, clip_rat, quant_bits, enob, seed, out); }
int qh_sosfilt_c64_dev(const void *E, int nmodes, int64_t L, const double *sos, int nsec, const double *P, void *out)
{ return qh::sosfilt_dev<float>(E, nmodes, L, sos, nsec, P, out); }
int qh_sosfilt_c128_dev(const void *E, int nmodes, int64_t L, const double *sos, int nsec, const double *P, void *out)
{ return qh::sosfilt_dev<double>(E, nmodes, L, sos, nsec, P, out); }
int qh_modulator_c64_dev(const void *E, int nmodes, int64_t L, const double *ext, int have_amp, double tgt_v, const double *prm, void *out)
{ return qh::modulator_dev<float>(E, nmodes, L, ext, have_amp, tgt_v, prm, out); }
int qh_modulator_c128_dev(const void *E, int nmodes, int64_t L, const double *ext, int have_amp, double tgt_v, const double *prm, void *out)
{ return qh::modulator_dev<double>(E, nmodes, L, ext, have_amp, tgt_v, prm, out); }
}
