// Shared device/host helpers of libqampy_hip (gfx950 only; wave64 is hard-coded throughout).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/qampy_hip.h"

namespace qh {

// ---------------------------------------------------------------------------------------------- host-side state
extern thread_local hipStream_t g_stream;     // per host thread (api.hip)
extern int g_device;
void set_error(const std::string &s);
int hip_fail(hipError_t e, const char *what, const char *file, int line);

#define QH_HIP(call)                                                        \
    do {                                                                    \
        hipError_t _e = (call);                                             \
        if (_e != hipSuccess) return qh::hip_fail(_e, #call, __FILE__, __LINE__); \
    } while (0)

#define QH_REQUIRE(cond, msg)                                   \
    do {                                                        \
        if (!(cond)) { qh::set_error(msg); return QH_ERR_ARG; } \
    } while (0)

// First statement of the kernels on a tier-b trainer's critical path (chains, eigen-solver, control kernels): issue priority over the
// waves of a streaming kernel of another stream that shares the SIMD (the phase search of the previous capture, pipeline.py
// run(overlap=True)).  Costs one scalar instruction; without a co-runner it changes nothing.
#define QH_WAVE_FIRST() __builtin_amdgcn_s_setprio(3)

int ensure_init();
hipStream_t side_stream();       // the library stream that is NOT the current one (work overlapped with the current stream)
hipStream_t helper_stream();     // a third stream for small launches beside both (the coarse model of a tier-b sweep)
// Test / measurement hooks (qh_set_form): every switch that forces a kernel form the automatic choice would not take at that size lives in ONE table of
// atomics, set through the C ABI; the launch paths read the table, never the environment.  (The environment variables of rounds 1-5 - QAMPY_HIP_TRAINER,
// QAMPY_HIP_PIT_FORM, ... - are read ONCE, when the library is loaded, as the table's initial values: scripts/ that export them keep working.)
enum FormKey { FORM_TRAINER = 0, FORM_PIT, FORM_SEG_LANES, FORM_PIT_PROBE, FORM_BPS, FORM_PIT_TAIL, FORM_COUNT };
int form(FormKey k);
const char *trainer_force();   // "" (automatic) or "direct" / "lookahead" / "iterative": qh_set_trainer(), else QAMPY_HIP_TRAINER
double gram_budget_gb();         // scratch the Gram tables of one call may take (qh_set_gram_budget_gb; default: QAMPY_HIP_GRAM_BUDGET_GB read once, else 160)
int pit_timing_mode();            // which relaxation passes of a tier-b sweep get HIP events: 0 none, 1 pass 1 (default), 2 all (qh_set_pit_timing)
int default_tier();               // 0: tier a (exact), 1: tier b - what the drop-in host-array trainers run (qh_set_default_tier)
double default_tier_tol();        // tolerance of the default tier b (qh_set_default_tier)
// The scratch slots: grow-only device buffers of the calling host thread (not of a stream).  Every slot has ONE owning source file, so two units
// never meet in a buffer whatever streams they run on; the one exception is GRAM (tests/test_scratch_slots.py holds the sources to this).
enum class Slot : int {
    BPS_ANGLES,          // ring of test-angle tables of the phase search (bps.hip)
    BPS_CHUNKS,          // wrap counts per chunk of the phase search's unwrap, one- and two-stage (bps.hip)
    BPS_ALPHABET,        // ring of alphabet descriptors of the phase search (bps.hip)
    TWOSTAGE,            // ring of fine-angle and rotator tables of the two-stage phase search (bps.hip)
    STEP_SIZES,          // the per-mode step sizes of an adaptive trainer call (train_impl.h)
    GRAM,                // Gram tables of the lookahead (train_la.h) and block-iterative (train_bi.h) trainers: two forms of one trainer in one
                         // translation unit, of which a call runs one - the only slot with two owners
    BI_LEVELS,           // decision levels and their counts of the block-iterative trainer (train_bi.h)
    PIT_WORK,            // tier b: segment taps, estimates and the selection of a sweep (train_pit.h)
    PIT_CTRL,            // tier b: the control block PitCtrl that steers the relaxation passes (train_pit.h)
    PIT_COV,             // tier b: covariance blocks of the basis (train_pit.h)
    PIT_BASIS,           // tier b: the basis and the products of the correction (train_pit.h)
    PIT_ROTATIONS,       // tier b: Jacobi rotations of the eigen-solver's sweeps (train_pit.h)
    PIT_ACQ,             // tier b: acquisition head, and the adaptive form's per-segment state (train_pit.h)
    PIT_MODEL,           // tier b: partials and fits of the coarse model (train_pit.h)
    SER,                 // symbol indices and lag counts of the symbol-error count (ser.hip)
    SYNTH,               // filter taps, PMD parameters and tile phases of the test-capture synthesis (synth.hip)
    METRICS,             // workgroup partials and totals of metrics_dev (metrics.hip)
    SNR_EST,             // per-symbol partials and totals of estimate_snr (metrics.hip)
    AWGN_MC,             // workgroup partials and totals of the Monte-Carlo curves, awgn_mc_dev (metrics.hip)
    CD_TABLE,            // twiddles and H of the dispersion filter (cd.hip)
    RESAMPLE_TABLE,      // phase-major taps of the polyphase resampler (resample.hip)
    ROW_MOMENTS,         // partial sums of the per-row moments (resample.hip)
    FOE,                 // tables, spectrum and intermediates of the frequency-offset estimate (foe.hip)
    IMPAIR,              // tile totals, power partials and sigma of the point-wise impairment pass (impair.hip)
    PMD,                 // twiddles and H of the PMD filter (impair.hip)
    TXRESP,              // tile extrema and the row extrema a call forms for itself (txresp.hip)
    SOS,                 // tile end states / start states of the sections filter (txresp.hip)
    CPR,                 // angles, wrap counts and partial moments of the feed-forward carrier recovery (cpr.hip)
    FFT,                 // tables and work buffers of the whole-row transforms (fft.hip)
    IQ,                  // tile totals of the IQ moments (iq.hip)
    SYNC,                // reversed conjugate of y and its transform, spectra of the rows of x (sync.hip)
    PEAK,                // one partial per tile of the correlation's peak search (sync.hip)
    PILOT,               // pilot phases, knots and wrap counts of the pilot-aided estimates (pilot.hip)
    PRECOMP,             // tile maxima and scales of the pattern table, tile sums of the DAC pre-emphasis (precomp.hip)
    BLIND,               // workgroup partials of the blind moments, distance sums and QPSK sums (blind.hip)
    HYBRID,              // tile sums of the frame classes, workgroup partials of the hybrid metrics (hybrid.hip)
    FIBRE,               // power partials, pscale and the two dispersion tables of the split-step propagation (fibre.hip)
    COUNT
};
int scratch(Slot slot, size_t bytes, void **p);  // grow-only device scratch of the calling thread
unsigned scratch_epoch();        // changes whenever the calling thread's scratch slots are released (contents cached in a slot are gone)

// A table formed on the host and kept in a scratch slot until its key changes: one upload per key.  `key` is an opaque byte string the caller
// fills with everything the contents depend on (sizes, sizeof(R), coefficients or taps); fill(host) writes the `bytes` of the table.  The table is
// formed again when the key differs, the scratch was released (scratch_epoch) or the slot has grown; whatever still reads the old table (a launch
// on another of this thread's streams) or the host copy (the last upload) finishes first.  One instance per slot and host thread.
struct TableCache {
    std::string key;
    std::vector<char> host;          // kept alive for the asynchronous upload
    void *dev = nullptr;
    unsigned epoch = 0;
    template <typename F> int get(Slot slot, const std::string &k, size_t bytes, F fill, const void **tab)
    {
        void *p = nullptr;
        int rc;
        if (dev && key == k && epoch == scratch_epoch()) {
            if ((rc = scratch(slot, bytes, &p))) return rc;
            if (p == dev) { *tab = p; return QH_OK; }
        }
        if (dev) QH_HIP(hipDeviceSynchronize());
        dev = nullptr;
        if ((rc = scratch(slot, bytes, &p))) return rc;
        host.resize(bytes);
        fill(host.data());
        QH_HIP(hipMemcpyAsync(p, host.data(), bytes, hipMemcpyHostToDevice, g_stream));
        key = k; dev = p; epoch = scratch_epoch();
        *tab = p;
        return QH_OK;
    }
};
// appends the bytes of a value to a TableCache key
template <typename T> inline void key_add(std::string &k, const T &v) { k.append(reinterpret_cast<const char *>(&v), sizeof(T)); }

constexpr double QH_PI = 3.14159265358979323846, QH_TWO_PI = 2 * QH_PI;      // (the doubling is exact: QH_TWO_PI is the double nearest 2 pi)

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }
// Layout of one scratch slot as regions aligned to 256 bytes: take() every region in order, pass `total` to scratch(), add the offsets to its base.
struct ScratchLayout {
    size_t total = 0;
    size_t take(size_t bytes) { const size_t o = total; total += up256(bytes); return o; }
};
// a kernel that asks for more than 64 KiB of dynamic LDS has to be opted in before its launch
template <typename K> int dyn_lds(K kernel, size_t bytes)
{
    if (bytes > 64 * 1024) QH_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return QH_OK;
}

// two-stage phase search on device pointers (bps.hip); the C entry points in api.hip check the arguments
int bps_twostage_recover_f32(const void *E, int nm, int64_t L, const void *angles, int A, int B, const void *symbols, int M, int N, int32_t *idx1,
                             int32_t *idx2, void *ph, void *Eout);
int bps_twostage_recover_f64(const void *E, int nm, int64_t L, const void *angles, int A, int B, const void *symbols, int M, int N, int32_t *idx1,
                             int32_t *idx2, void *ph, void *Eout);

// Correlation of `rows` rows of x (nx samples each, dense) with one sequence on power-of-two transforms of size P (fft.hip): yrev (P values, the
// first ny given: the conjugate of y reversed) is replaced by its transform, spec (rows, P) takes the transforms of the zero-extended rows, and
// cc (rows, n), n <= P, the first n values of ifft(spec . yrev) of every row.  The caller checks the sizes; P is a power of two, 2^8 .. 2^24.
template <typename R> int fft_correlate_pow2(const void *x, int rows, int64_t nx, void *yrev, int64_t ny, int64_t P, void *spec, void *cc, int64_t n);

// Staging memory of the host-pointer entry points: power-of-two size classes kept in a small pool (api.hip) instead of a
// hipMalloc / hipFree pair per call - hipFree synchronises the device, and the pilot receiver makes dozens of small calls.
// The entry points synchronise their stream before they return, so a buffer is idle when it goes back to the pool.
int pool_alloc(size_t bytes, void **p, size_t *cap);
void pool_free(void *p, size_t cap);

// RAII device scratch used by the host-pointer entry points
struct DevBuf {
    void *p = nullptr;
    size_t n = 0, cap = 0;
    ~DevBuf() { if (p) pool_free(p, cap); }
    int alloc(size_t bytes) {
        n = bytes;
        return pool_alloc(bytes ? bytes : 1, &p, &cap);
    }
    int from_host(const void *h, size_t bytes) {
        int rc = alloc(bytes);
        if (rc) return rc;
        if (bytes) QH_HIP(hipMemcpyAsync(p, h, bytes, hipMemcpyHostToDevice, g_stream));
        return QH_OK;
    }
    int to_host(void *h, size_t bytes) const {
        if (bytes) QH_HIP(hipMemcpyAsync(h, p, bytes, hipMemcpyDeviceToHost, g_stream));
        return QH_OK;
    }
};

// ---------------------------------------------------------------------------------------------- complex pairs
template <typename R> struct Cx { R re, im; };

template <typename R> struct Cx2T;
template <> struct Cx2T<float> { using type = float2; };
template <> struct Cx2T<double> { using type = double2; };

template <typename R> __device__ __forceinline__ Cx<R> ldg(const Cx<R> *p)
{
    using V = typename Cx2T<R>::type;
    V v = *reinterpret_cast<const V *>(p);
    return Cx<R>{v.x, v.y};
}
template <typename R> __device__ __forceinline__ void stg(Cx<R> *p, Cx<R> v)
{
    using V = typename Cx2T<R>::type;
    V o; o.x = v.re; o.y = v.im;
    *reinterpret_cast<V *>(p) = o;
}

__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float abs_(float a) { return __builtin_fabsf(a); }
__device__ __forceinline__ double abs_(double a) { return __builtin_fabs(a); }
__device__ __forceinline__ float min_(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double min_(double a, double b) { return __builtin_fmin(a, b); }
template <typename R> __device__ __forceinline__ void sincos_(R x, R *s, R *c);
template <> __device__ __forceinline__ void sincos_<float>(float x, float *s, float *c) { sincosf(x, s, c); }
template <> __device__ __forceinline__ void sincos_<double>(double x, double *s, double *c) { sincos(x, s, c); }

template <typename R> __device__ __forceinline__ Cx<R> cadd(Cx<R> a, Cx<R> b) { return Cx<R>{a.re + b.re, a.im + b.im}; }
template <typename R> __device__ __forceinline__ Cx<R> csub(Cx<R> a, Cx<R> b) { return Cx<R>{a.re - b.re, a.im - b.im}; }
template <typename R> __device__ __forceinline__ Cx<R> cmul(Cx<R> a, Cx<R> b) { return Cx<R>{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
template <typename R> __device__ __forceinline__ Cx<R> cconj(Cx<R> a) { return Cx<R>{a.re, -a.im}; }
template <typename R> __device__ __forceinline__ Cx<R> pow4(Cx<R> x)
{
    const Cx<R> s = cmul(x, x);
    return cmul(s, s);
}

// ---------------------------------------------------------------------------------------------- wave64 cross-lane
// DPP controls (gfx9 encoding)
constexpr int DPP_QUAD_1032 = 0xB1;        // quad_perm:[1,0,3,2]
constexpr int DPP_QUAD_2301 = 0x4E;        // quad_perm:[2,3,0,1]
constexpr int DPP_ROW_HALF_MIRROR = 0x141;
constexpr int DPP_ROW_MIRROR = 0x140;
constexpr int DPP_ROW_BCAST15 = 0x142;
constexpr int DPP_ROW_BCAST31 = 0x143;

template <int CTRL, int ROW_MASK = 0xF> __device__ __forceinline__ float dpp_mov(float v)
{
    // lanes whose row is masked off keep `old` (= 0): adding it is a no-op, exactly what the row_bcast steps need
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, false));
}
template <int CTRL, int ROW_MASK = 0xF> __device__ __forceinline__ double dpp_mov(double v)
{
    long long b = __builtin_bit_cast(long long, v);
    int lo = (int)b, hi = (int)(b >> 32);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xF, false);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ float readlane(float v, int lane)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
__device__ __forceinline__ double readlane(double v, int lane)
{
    long long b = __builtin_bit_cast(long long, v);
    int lo = __builtin_amdgcn_readlane((int)b, lane), hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ int readlane(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

// sum over the 64 lanes of a wave; the total is returned wave-uniformly (read back from lane 63)
template <typename R> __device__ __forceinline__ R wave_sum(R v)
{
    v += dpp_mov<DPP_QUAD_1032>(v);
    v += dpp_mov<DPP_QUAD_2301>(v);
    v += dpp_mov<DPP_ROW_HALF_MIRROR>(v);
    v += dpp_mov<DPP_ROW_MIRROR>(v);
    v += dpp_mov<DPP_ROW_BCAST15, 0xA>(v);
    v += dpp_mov<DPP_ROW_BCAST31, 0xC>(v);
    return readlane(v, 63);
}
// two sums with their DPP chains interleaved (re / im of a complex dot product)
template <typename R> __device__ __forceinline__ void wave_sum2(R &a, R &b)
{
    a += dpp_mov<DPP_QUAD_1032>(a);            b += dpp_mov<DPP_QUAD_1032>(b);
    a += dpp_mov<DPP_QUAD_2301>(a);            b += dpp_mov<DPP_QUAD_2301>(b);
    a += dpp_mov<DPP_ROW_HALF_MIRROR>(a);      b += dpp_mov<DPP_ROW_HALF_MIRROR>(b);
    a += dpp_mov<DPP_ROW_MIRROR>(a);           b += dpp_mov<DPP_ROW_MIRROR>(b);
    a += dpp_mov<DPP_ROW_BCAST15, 0xA>(a);     b += dpp_mov<DPP_ROW_BCAST15, 0xA>(b);
    a += dpp_mov<DPP_ROW_BCAST31, 0xC>(a);     b += dpp_mov<DPP_ROW_BCAST31, 0xC>(b);
    a = readlane(a, 63);
    b = readlane(b, 63);
}
// Sum of a double over a workgroup of T threads in a fixed order - wave_sum, then waves 0, 1, 2, ... - to every thread: the same bits in
// every workgroup and every run.  red: T / 64 entries of LDS.  Ends in a barrier: red may be used again.
template <int T> __device__ __forceinline__ double block_sum(double s, double *red)
{
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = 0.;
    for (int w = 0; w < T / 64; w++) t += red[w];
    __syncthreads();
    return t;
}
// two sums at once, the wave sums interleaved
template <int T> __device__ __forceinline__ void block_sum2(double &a, double &b, double (*red)[2])
{
    wave_sum2(a, b);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = a; red[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    a = b = 0.;
    for (int w = 0; w < T / 64; w++) { a += red[w][0]; b += red[w][1]; }
    __syncthreads();
}
// min over the 64 lanes, returned wave-uniformly
template <typename R> __device__ __forceinline__ R wave_min(R v)
{
    // masked-off rows would read `old` = 0, so the bcast steps are written with explicit selects instead
    v = min_(v, dpp_mov<DPP_QUAD_1032>(v));
    v = min_(v, dpp_mov<DPP_QUAD_2301>(v));
    v = min_(v, dpp_mov<DPP_ROW_HALF_MIRROR>(v));
    v = min_(v, dpp_mov<DPP_ROW_MIRROR>(v));
    R r0 = readlane(v, 0), r1 = readlane(v, 16), r2 = readlane(v, 32), r3 = readlane(v, 48);
    return min_(min_(r0, r1), min_(r2, r3));
}

}  // namespace qh
