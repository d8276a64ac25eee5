// Whole-row transforms of an (nmodes, L) complex array in HBM, and the spectral multiply between a forward and an inverse one:
//
//   fft      X[k] = sum_n x[n] exp(-2 pi i n k / L)            numpy's sign; the inverse carries 1 / L
//   filter   y = ifft(H . fft(x)),  H formed on the device in double from a handful of parameters, or a caller's table
//
// Three paths by length, all on the Stockham LDS core of fft_lds.h:
//   L = 2^8 .. 2^13        one workgroup per row.
//   L = 2^14 .. 2^24       four-step, L = N1 N2 with N1 = 2^floor(lg / 2), N2 = L / N1 (both 128 .. 4096): a workgroup of step 1 transforms
//                          FFT_COLS neighbouring columns n2 of the (N1, N2) view over n1, multiplies by W_L^(k1 n2) - the turn k1 n2 / L is
//                          exact in double, sine and cosine in double - and stores T[k1][n2]; a workgroup of step 2 transforms FFT_COLS
//                          neighbouring rows T[k1][:] over n2 and stores bin k1 + N1 k2: natural order, the transpose is in that store.
//   every other L, 2 .. 2^23   Bluestein on M = 2^m >= max(256, 2 L - 1): X[k] = w[k] sum_n (x[n] w[n]) conj(w)[k - n], w[n] = exp(-i pi n^2 / L),
//                          n^2 taken modulo 2 L in 64-bit integers and the turn reduced in double before its sine and cosine; the circular
//                          convolution is two transforms of size M by the two paths above.  The chirp and the transform of its filter are
//                          formed on the device at every call: nothing is cached across calls, nothing of length L comes from the host.
//
// Every transform kernel reads through one load functor and writes through one store functor; conjugations (the inverse is
// conj(FFT(conj(.))) / L), zero padding, the chirp products, the 1 / L and the multiply by H live there, so a Bluestein transform is two
// passes over HBM per size-M transform and the filter costs no pass of its own: H is applied as the inverse transform loads the spectrum.
//
// A kernel of one transform has read all of its input before the next one writes (single workgroup: into LDS before the first store;
// four-step: step 1 reads the input, step 2 writes the output; Bluestein: the first transform reads the input, the second writes), so
// `out` may be the very buffer `E`.  Partial overlap is not supported.
//
// fft_correlate_pow2 (for sync.hip) is the filter's chain with a caller's geometry: rows of any length zero-extended to a power of two as they
// are loaded, the table the transform of a second sequence, and only the first n values of the inverse transform stored, densely.
//
// Scratch slot Slot::FFT: W_N1 | W_N2 | chirp (L) | transform of the chirp filter (M) | T (rows M, four-step) | W (rows M, Bluestein): the
// work buffers are 2 nmodes M complex values at most.  No atomics: a repeated call is bit-identical.  Every launch is bounded by the
// call's arguments alone.
#include "common.h"
#include "fft_lds.h"
#include <cmath>

namespace qh {

constexpr int FFT_LG_MIN = 8, FFT_LG_SINGLE = 13, FFT_LG_MAX = 24;      // power-of-two sizes; one workgroup per row up to 2^13
constexpr int64_t FFT_BLUE_MAX = (int64_t)1 << 23;                      // longest Bluestein length: 2 L - 1 <= 2^24

enum { FH_NONE = 0, FH_BRICK, FH_BAND, FH_TWORAIL, FH_RAMP, FH_REAL, FH_COMPLEX };

// columns (step 1) or rows (step 2) of one workgroup: about 64 KiB of LDS
template <typename R, int N> constexpr int fft_cols()
{
    constexpr int c = (int)(65536 / ((size_t)N * sizeof(Cx<R>)));
    return c >= 8 ? 8 : (c >= 1 ? c : 1);
}

template <typename R> struct FftLoad {
    const Cx<R> *in;
    int64_t stride, valid;         // row stride; samples of a row that exist (zero beyond)
    int conj, bgen;                // conjugate the value; bgen: `in` is the chirp and the value is the chirp filter b[n]
    const Cx<R> *chirp;            // multiply by chirp[n]
    int hkind;                     // FH_*: multiply by H[n] first (the row is a spectrum of `valid` bins in fftfreq order)
    int64_t i0, i1;
    double p0, p1, p2;
    const void *H;
};

template <typename R> struct FftStore {
    Cx<R> *out;
    int64_t stride, valid;         // row stride; bins that are stored
    const Cx<R> *tab;              // multiply by tab[k] (conjugated if tab_conj)
    int tab_conj, conj;
    R scale;
};

// exp(-2 pi i t) in double, the turn reduced first
__device__ __forceinline__ void fft_ramp(double t, double &cs, double &sn)
{
    t -= rint(t);
    sincospi(-2.0 * t, &sn, &cs);
}

template <typename R> __device__ __forceinline__ Cx<R> fft_hmul(const FftLoad<R> &ld, const Cx<R> *x, int64_t n, Cx<R> v)
{
    const int64_t L = ld.valid;
    const int64_t kk = n < (L - 1) / 2 + 1 ? n : n - L;                // numpy's fftfreq numerator
    const Cx<R> zero{(R)0, (R)0};
    switch (ld.hkind) {
    case FH_BRICK: {                                                   // position after fftshift in [i0, i1)
        int64_t j = n + L / 2;
        if (j >= L) j -= L;
        return (j >= ld.i0 && j < ld.i1) ? v : zero;
    }
    case FH_BAND: {
        const double f = (double)kk * ld.p0;
        return fabs(f - ld.p1) < ld.p2 ? v : zero;
    }
    case FH_TWORAIL: {
        const double f = (double)kk * ld.p0;
        double ci, si, cq, sq;
        fft_ramp(ld.p1 * f, ci, si);
        fft_ramp(ld.p2 * f, cq, sq);
        if ((L & 1) == 0 && n == L / 2) { si = 0.0; sq = 0.0; }        // (H[k] + conj H[-k]) / 2 at the Nyquist bin
        const int64_t m = n == 0 ? 0 : L - n;
        const Cx<R> xm = cconj(ldg(x + m));
        const R h = (R)0.5;
        const Cx<R> a{h * (v.re + xm.re), h * (v.im + xm.im)}, b{h * (v.re - xm.re), h * (v.im - xm.im)};
        return cadd(cmul(Cx<R>{(R)ci, (R)si}, a), cmul(Cx<R>{(R)cq, (R)sq}, b));
    }
    case FH_RAMP: {
        double c, s;
        fft_ramp(ld.p1 * ((double)kk * ld.p0), c, s);
        return cmul(Cx<R>{(R)c, (R)s}, v);
    }
    case FH_REAL: {
        const R h = ((const R *)ld.H)[n];
        return Cx<R>{h * v.re, h * v.im};
    }
    default:
        return cmul(ldg((const Cx<R> *)ld.H + n), v);
    }
}

template <typename R> __device__ __forceinline__ Cx<R> fft_load(const FftLoad<R> &ld, int row, int64_t n, int64_t M)
{
    const Cx<R> zero{(R)0, (R)0};
    if (ld.bgen) {                                                     // b[n] = conj(w[n]), n < L; b[M - n] = b[n]; zero between
        const int64_t m = n < ld.valid ? n : (n > M - ld.valid ? M - n : -1);
        return m < 0 ? zero : cconj(ldg(ld.in + m));
    }
    if (n >= ld.valid) return zero;
    const Cx<R> *x = ld.in + (size_t)row * ld.stride;
    Cx<R> v = ldg(x + n);
    if (ld.hkind) v = fft_hmul(ld, x, n, v);
    if (ld.conj) v = cconj(v);
    if (ld.chirp) v = cmul(v, ldg(ld.chirp + n));
    return v;
}

template <typename R> __device__ __forceinline__ void fft_store(const FftStore<R> &st, int row, int64_t k, Cx<R> v)
{
    if (k >= st.valid) return;
    if (st.tab) {
        Cx<R> t = ldg(st.tab + k);
        if (st.tab_conj) t = cconj(t);
        v = cmul(v, t);
    }
    if (st.conj) v = cconj(v);
    stg(st.out + (size_t)row * st.stride + k, Cx<R>{v.re * st.scale, v.im * st.scale});
}

// chirp[n] = exp(-i pi n^2 / L), n = 0 .. L - 1: n^2 mod 2 L in integers, the turn (n^2 mod 2 L) / (2 L) below one
template <typename R> __global__ void __launch_bounds__(256) fft_chirp_kernel(Cx<R> *chirp, int64_t L)
{
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= L) return;
    const uint64_t m = ((uint64_t)n * (uint64_t)n) % (uint64_t)(2 * L);
    double cs, sn;
    fft_ramp((double)m / (double)(2 * L), cs, sn);
    stg(chirp + n, Cx<R>{(R)cs, (R)sn});
}

// one workgroup per row.  grid (rows)
template <typename R, int N>
__global__ void __launch_bounds__(CD_T) fft_row_kernel(FftLoad<R> ld, FftStore<R> st, const Cx<R> *__restrict__ tw)
{
    extern __shared__ __attribute__((aligned(16))) char smem_fft[];
    Cx<R> *buf = reinterpret_cast<Cx<R> *>(smem_fft);
    const int row = blockIdx.x;
    for (int t = threadIdx.x; t < N; t += CD_T) buf[t] = fft_load(ld, row, t, N);
    __syncthreads();
    fft_from<R, N, 1>(buf, tw);
    for (int t = threadIdx.x; t < N; t += CD_T) fft_store(st, row, t, buf[t]);
}

// Step 1 of the four-step transform.  grid (N2 / cols, rows); T (rows, N1, N2)
template <typename R, int N1>
__global__ void __launch_bounds__(CD_T) fft_step1_kernel(FftLoad<R> ld, int N2, const Cx<R> *__restrict__ tw1, Cx<R> *__restrict__ T)
{
    extern __shared__ __attribute__((aligned(16))) char smem_fft[];
    Cx<R> *buf = reinterpret_cast<Cx<R> *>(smem_fft);
    constexpr int C = fft_cols<R, N1>(), LD = N1 + 1;
    const int64_t M = (int64_t)N1 * N2;
    const int row = blockIdx.y, c0 = blockIdx.x * C;
    for (int i = threadIdx.x; i < N1 * C; i += CD_T) {
        const int c = i % C, n1 = i / C;
        buf[c * LD + n1] = fft_load(ld, row, (int64_t)n1 * N2 + c0 + c, M);
    }
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < C; c++) fft_from<R, N1, 1>(buf + c * LD, tw1);
    Cx<R> *t = T + (size_t)row * M;
    for (int i = threadIdx.x; i < N1 * C; i += CD_T) {
        const int c = i % C, k1 = i / C;
        double cs, sn;
        fft_ramp((double)((int64_t)k1 * (c0 + c)) / (double)M, cs, sn);           // exact turn, in [0, 1)
        stg(t + (size_t)k1 * N2 + c0 + c, cmul(buf[c * LD + k1], Cx<R>{(R)cs, (R)sn}));
    }
}

// Step 2.  grid (N1 / cols, rows): rows k1 = c0 .. c0 + cols - 1 of T over n2; bin k1 + N1 k2
template <typename R, int N2>
__global__ void __launch_bounds__(CD_T) fft_step2_kernel(const Cx<R> *__restrict__ T, int N1, const Cx<R> *__restrict__ tw2, FftStore<R> st)
{
    extern __shared__ __attribute__((aligned(16))) char smem_fft[];
    Cx<R> *buf = reinterpret_cast<Cx<R> *>(smem_fft);
    constexpr int C = fft_cols<R, N2>(), LD = N2 + 1;
    const int64_t M = (int64_t)N1 * N2;
    const int row = blockIdx.y, c0 = blockIdx.x * C;
    const Cx<R> *t = T + (size_t)row * M + (size_t)c0 * N2;
    for (int i = threadIdx.x; i < N2 * C; i += CD_T) {
        const int c = i / N2, n2 = i % N2;
        buf[c * LD + n2] = ldg(t + (size_t)c * N2 + n2);
    }
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < C; c++) fft_from<R, N2, 1>(buf + c * LD, tw2);
    for (int i = threadIdx.x; i < N2 * C; i += CD_T) {
        const int c = i % C, k2 = i / C;
        fft_store(st, row, (int64_t)(c0 + c) + (int64_t)N1 * k2, buf[c * LD + k2]);
    }
}

// ------------------------------------------------------------------------------------------------ host side
template <typename R> struct FftPlan {
    int64_t L = 0, M = 0;
    int N1 = 1, N2 = 1;            // N1 = 1: one workgroup per row of M = N2 points
    bool blue = false;
    Cx<R> *tw1 = nullptr, *tw2 = nullptr, *chirp = nullptr, *Bhat = nullptr, *T = nullptr, *W = nullptr;
};

static bool fft_length_ok(int64_t L)
{
    if (L < 2) return false;
    if ((L & (L - 1)) == 0 && L >= ((int64_t)1 << FFT_LG_MIN)) return L <= ((int64_t)1 << FFT_LG_MAX);
    return L <= FFT_BLUE_MAX;
}

template <typename R, int N> static int fft_row_launch(const FftLoad<R> &ld, const FftStore<R> &st, int rows, const Cx<R> *tw)
{
    const size_t lds = (size_t)N * sizeof(Cx<R>);
    int rc = dyn_lds(fft_row_kernel<R, N>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL((fft_row_kernel<R, N>), dim3(rows), dim3(CD_T), lds, g_stream, ld, st, tw);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R, int N1> static int fft_step1_launch(const FftLoad<R> &ld, int rows, int N2, const Cx<R> *tw1, Cx<R> *T)
{
    constexpr int C = fft_cols<R, N1>();
    const size_t lds = (size_t)C * (N1 + 1) * sizeof(Cx<R>);
    int rc = dyn_lds(fft_step1_kernel<R, N1>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL((fft_step1_kernel<R, N1>), dim3(N2 / C, rows), dim3(CD_T), lds, g_stream, ld, N2, tw1, T);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R, int N2> static int fft_step2_launch(const Cx<R> *T, int rows, int N1, const Cx<R> *tw2, const FftStore<R> &st)
{
    constexpr int C = fft_cols<R, N2>();
    const size_t lds = (size_t)C * (N2 + 1) * sizeof(Cx<R>);
    int rc = dyn_lds(fft_step2_kernel<R, N2>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL((fft_step2_kernel<R, N2>), dim3(N1 / C, rows), dim3(CD_T), lds, g_stream, T, N1, tw2, st);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

// one transform of size plan.M on `rows` rows
template <typename R> static int fft_pow2(const FftPlan<R> &p, const FftLoad<R> &ld, const FftStore<R> &st, int rows)
{
    if (p.N1 == 1) {
        switch (p.N2) {
        case 256: return fft_row_launch<R, 256>(ld, st, rows, p.tw2);
        case 512: return fft_row_launch<R, 512>(ld, st, rows, p.tw2);
        case 1024: return fft_row_launch<R, 1024>(ld, st, rows, p.tw2);
        case 2048: return fft_row_launch<R, 2048>(ld, st, rows, p.tw2);
        case 4096: return fft_row_launch<R, 4096>(ld, st, rows, p.tw2);
        default: return fft_row_launch<R, 8192>(ld, st, rows, p.tw2);
        }
    }
    int rc;
    switch (p.N1) {
    case 128: rc = fft_step1_launch<R, 128>(ld, rows, p.N2, p.tw1, p.T); break;
    case 256: rc = fft_step1_launch<R, 256>(ld, rows, p.N2, p.tw1, p.T); break;
    case 512: rc = fft_step1_launch<R, 512>(ld, rows, p.N2, p.tw1, p.T); break;
    case 1024: rc = fft_step1_launch<R, 1024>(ld, rows, p.N2, p.tw1, p.T); break;
    case 2048: rc = fft_step1_launch<R, 2048>(ld, rows, p.N2, p.tw1, p.T); break;
    default: rc = fft_step1_launch<R, 4096>(ld, rows, p.N2, p.tw1, p.T); break;
    }
    if (rc) return rc;
    switch (p.N2) {
    case 128: return fft_step2_launch<R, 128>(p.T, rows, p.N1, p.tw2, st);
    case 256: return fft_step2_launch<R, 256>(p.T, rows, p.N1, p.tw2, st);
    case 512: return fft_step2_launch<R, 512>(p.T, rows, p.N1, p.tw2, st);
    case 1024: return fft_step2_launch<R, 1024>(p.T, rows, p.N1, p.tw2, st);
    case 2048: return fft_step2_launch<R, 2048>(p.T, rows, p.N1, p.tw2, st);
    default: return fft_step2_launch<R, 4096>(p.T, rows, p.N1, p.tw2, st);
    }
}

// sizes, scratch and tables of a call on rows of L samples; a Bluestein length also gets its chirp and the chirp filter's transform
template <typename R> static int fft_plan(int nmodes, int64_t L, FftPlan<R> &p)
{
    p.L = L;
    p.blue = !((L & (L - 1)) == 0 && L >= ((int64_t)1 << FFT_LG_MIN));
    int lg = FFT_LG_MIN;
    const int64_t need = p.blue ? 2 * L - 1 : L;
    while (((int64_t)1 << lg) < need) lg++;
    p.M = (int64_t)1 << lg;
    const int lgN1 = lg > FFT_LG_SINGLE ? lg / 2 : 0;
    p.N1 = 1 << lgN1;
    p.N2 = 1 << (lg - lgN1);
    const size_t cx = sizeof(Cx<R>);
    ScratchLayout lay;
    const size_t o_tw1 = lay.take((size_t)p.N1 * cx), o_tw2 = lay.take((size_t)p.N2 * cx), o_chirp = lay.take(p.blue ? (size_t)L * cx : 0),
                 o_B = lay.take(p.blue ? (size_t)p.M * cx : 0), o_T = lay.take(p.N1 > 1 ? (size_t)nmodes * p.M * cx : 0),
                 o_W = lay.take(p.blue ? (size_t)nmodes * p.M * cx : 0);
    void *base = nullptr;
    int rc = scratch(Slot::FFT, lay.total, &base);
    if (rc) return rc;
    char *sb = (char *)base;
    p.tw1 = (Cx<R> *)(sb + o_tw1); p.tw2 = (Cx<R> *)(sb + o_tw2); p.chirp = (Cx<R> *)(sb + o_chirp); p.Bhat = (Cx<R> *)(sb + o_B);
    p.T = (Cx<R> *)(sb + o_T); p.W = (Cx<R> *)(sb + o_W);
    if (p.N1 > 1) hipLaunchKernelGGL((twiddle_kernel<R>), dim3((p.N1 + 255) / 256), dim3(256), 0, g_stream, p.tw1, p.N1);
    hipLaunchKernelGGL((twiddle_kernel<R>), dim3((p.N2 + 255) / 256), dim3(256), 0, g_stream, p.tw2, p.N2);
    QH_HIP(hipGetLastError());
    if (p.blue) {
        hipLaunchKernelGGL((fft_chirp_kernel<R>), dim3((unsigned)((L + 255) / 256)), dim3(256), 0, g_stream, p.chirp, L);
        QH_HIP(hipGetLastError());
        FftLoad<R> ld{};
        ld.in = p.chirp; ld.stride = 0; ld.valid = L; ld.bgen = 1;
        FftStore<R> st{};
        st.out = p.Bhat; st.stride = p.M; st.valid = p.M; st.scale = (R)1;
        if ((rc = fft_pow2(p, ld, st, 1))) return rc;
    }
    return QH_OK;
}

// out = fft(H . in) or ifft(H . in) of every row (H as `h` describes it: hkind and parameters; FH_NONE for a plain transform)
template <typename R> static int fft_transform(const FftPlan<R> &p, const Cx<R> *in, Cx<R> *out, int nmodes, int inverse, const FftLoad<R> &h)
{
    const int64_t L = p.L;
    FftLoad<R> ld = h;
    ld.in = in; ld.stride = L; ld.valid = L; ld.conj = inverse; ld.bgen = 0; ld.chirp = nullptr;
    FftStore<R> st{};
    st.out = out; st.stride = L; st.valid = L;
    if (!p.blue) {
        st.conj = inverse;
        st.scale = inverse ? (R)(1.0 / (double)L) : (R)1;
        return fft_pow2(p, ld, st, nmodes);
    }
    // Bluestein.  first transform: A = FFT_M(x w, zero-padded); W = conj(A B).  second: FFT_M(W) = conj(M c), c the convolution
    ld.chirp = p.chirp;
    FftStore<R> sa{};
    sa.out = p.W; sa.stride = p.M; sa.valid = p.M; sa.tab = p.Bhat; sa.conj = 1; sa.scale = (R)1;
    int rc = fft_pow2(p, ld, sa, nmodes);
    if (rc) return rc;
    FftLoad<R> lb{};
    lb.in = p.W; lb.stride = p.M; lb.valid = p.M;
    st.tab = p.chirp; st.tab_conj = 1;                                 // forward: conj(F conj(w)) / M = c w; inverse: F conj(w) / (M L) = conj(c w) / L
    st.conj = !inverse;
    st.scale = (R)(inverse ? 1.0 / (double)p.M / (double)L : 1.0 / (double)p.M);
    return fft_pow2(p, lb, st, nmodes);
}

static const char *FFT_RANGE = "fft: L must be a power of two from 2^8 to 2^24, or any other length from 2 to 2^23";

template <typename R> int fft_dev(const void *E, int nmodes, int64_t L, int inverse, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(fft_length_ok(L), FFT_RANGE);
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535, "fft: bad sizes");
    QH_REQUIRE(E && out, "fft: E and out must be given");
    FftPlan<R> p;
    if ((rc = fft_plan<R>(nmodes, L, p))) return rc;
    FftLoad<R> h{};
    return fft_transform<R>(p, (const Cx<R> *)E, (Cx<R> *)out, nmodes, inverse ? 1 : 0, h);
}

template <typename R>
int spectral_filter_dev(const void *E, int nmodes, int64_t L, int kind, double p0, double p1, double p2, int64_t i0, int64_t i1, const void *H, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(fft_length_ok(L), FFT_RANGE);
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535, "spectral_filter: bad sizes");
    QH_REQUIRE(E && out, "spectral_filter: E and out must be given");
    QH_REQUIRE(kind >= FH_BRICK && kind <= FH_COMPLEX, "spectral_filter: kind is 1 (brick wall), 2 (band), 3 (two-rail delay), 4 (delay), 5 / 6 (real / complex table)");
    QH_REQUIRE((kind != FH_REAL && kind != FH_COMPLEX) || H, "spectral_filter: a table kind needs H");
    QH_REQUIRE(std::isfinite(p0) && std::isfinite(p1) && std::isfinite(p2), "spectral_filter: parameters must be finite");
    FftPlan<R> p;
    if ((rc = fft_plan<R>(nmodes, L, p))) return rc;
    FftLoad<R> none{}, h{};
    h.hkind = kind; h.p0 = p0; h.p1 = p1; h.p2 = p2; h.i0 = i0; h.i1 = i1; h.H = H;
    // the spectrum lands in `out`; the inverse transform multiplies by H as it loads it and writes `out` again
    if ((rc = fft_transform<R>(p, (const Cx<R> *)E, (Cx<R> *)out, nmodes, 0, none))) return rc;
    return fft_transform<R>(p, (const Cx<R> *)out, (Cx<R> *)out, nmodes, 1, h);
}

// The padding lives in the load functor (zero beyond `valid`) and the cut to n values in the store functor: three transforms, no pass of
// their own for either.  yrev is transformed in place, the table multiply is the kind-6 load of the inverse transform.
template <typename R> int fft_correlate_pow2(const void *x, int rows, int64_t nx, void *yrev, int64_t ny, int64_t P, void *spec, void *cc, int64_t n)
{
    FftPlan<R> p;
    int rc = fft_plan<R>(rows, P, p);
    if (rc) return rc;
    FftLoad<R> ld{};
    ld.in = (const Cx<R> *)yrev; ld.stride = P; ld.valid = ny;
    FftStore<R> st{};
    st.out = (Cx<R> *)yrev; st.stride = P; st.valid = P; st.scale = (R)1;
    if ((rc = fft_pow2(p, ld, st, 1))) return rc;
    ld.in = (const Cx<R> *)x; ld.stride = nx; ld.valid = nx;
    st.out = (Cx<R> *)spec;
    if ((rc = fft_pow2(p, ld, st, rows))) return rc;
    FftLoad<R> li{};
    li.in = (const Cx<R> *)spec; li.stride = P; li.valid = P; li.conj = 1; li.hkind = FH_COMPLEX; li.H = yrev;
    FftStore<R> so{};
    so.out = (Cx<R> *)cc; so.stride = n; so.valid = n; so.conj = 1; so.scale = (R)(1.0 / (double)P);
    return fft_pow2(p, li, so, rows);
}
template int fft_correlate_pow2<float>(const void *, int, int64_t, void *, int64_t, int64_t, void *, void *, int64_t);
template int fft_correlate_pow2<double>(const void *, int, int64_t, void *, int64_t, int64_t, void *, void *, int64_t);

}  // namespace qh

extern "C" {
int qh_fft_c64_dev(const void *E, int nmodes, int64_t L, int inverse, void *out) { return qh::fft_dev<float>(E, nmodes, L, inverse, out); }
int qh_fft_c128_dev(const void *E, int nmodes, int64_t L, int inverse, void *out) { return qh::fft_dev<double>(E, nmodes, L, inverse, out); }
int qh_spectral_filter_c64_dev(const void *E, int nmodes, int64_t L, int kind, double p0, double p1, double p2, int64_t i0, int64_t i1, const void *H, void *out)
{ return qh::spectral_filter_dev<float>(E, nmodes, L, kind, p0, p1, p2, i0, i1, H, out); }
int qh_spectral_filter_c128_dev(const void *E, int nmodes, int64_t L, int kind, double p0, double p1, double p2, int64_t i0, int64_t i1, const void *H, void *out)
{ return qh::spectral_filter_dev<double>(E, nmodes, L, kind, p0, p1, p2, i0, i1, H, out); }
}
