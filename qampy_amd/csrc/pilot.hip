// Pilot frames on gfx950 without leaving device memory: assemble a frame from pilots and payload, take it apart again, and the pilot-aided
// estimates - unwrapped pilot phase, its moving average, the carrier-phase trace and its removal, the frequency offset from the slope of the
// phase and the constant phase.
//
// Reference behaviour:
//   qampy/signals.py:1494-1545                 SignalWithPilots.__new__ / _cal_pilot_idx: a frame of F symbols is S pilots (the sequence) followed by
//                                              payload with one phase pilot every R symbols, the first of them at position S
//   qampy/signals.py:1753-1804                 get_data / extract_pilots: boolean-mask gathers over whole frames
//   qampy/core/pilotbased_receiver.py:258-327  pilot_based_cpe_new: angle(E[pilots] conj(sent)), np.unwrap, moving average over N pilots, np.interp to
//                                              every symbol, E exp(-1j trace)
//   qampy/core/pilotbased_receiver.py:32-73    pilot_based_foe: np.polyfit(arange(n), unwrapped phase, 1) per mode
//   qampy/phaserec.py:194-218                  find_pilot_const_phase: mean of the unwrapped phase per mode
//
// Geometry by rule, no index tables: position i of a frame is a pilot if i < S, or if R > 0 and (i - S) % R == 0.  Its ordinal among the pilots is
// i (i < S) or S + (i - S) / R; the ordinal of a payload position is ((i - S) / R) (R - 1) + (i - S) % R - 1, or i - S when R == 0.  Assemble and
// split both walk the FRAME positions (one thread per position, the frame side of the copy coalesced, the packed side coalesced but for the gaps
// the pilots leave), so one pass over a frame serves payload and pilots together and neither needs the inverse maps.  Both move every sample once:
// HBM traffic is their floor.
//
// Unwrapped pilot phase, three launches: pilot_theta_kernel (gather, angle in double for both precisions, wrap counts of a chunk of UW_CHUNK pilots and
// their sum; the count of a chunk's first pilot is decided from the chunk's own angle of the pilot in front and stored, so that the last kernel repeats
// exactly this decision), unwrap_scan_kernel (unwrap_scan.h: exact integer prefix sum over the chunk sums), pilot_unwrap_kernel (prefix inside the
// chunk, phase = theta + 2 pi K, in place).  The estimates that follow touch one value per PILOT - a few thousand per frame - and are bound by launch
// latency, not by bandwidth: pilot_knots_kernel (every output a direct sum of its N phases in double, N <= PILOT_NMAX), pilot_fit_kernel (one
// workgroup per mode: mean, then centred sums in double), pilot_fo_kernel.  pilot_interp_kernel (np.interp to every symbol and de-rotation) is the one
// pass over the field: 8 B in, 8 + 4 out per complex64 symbol (complex128: 16, 16 + 8).
#include "common.h"
#include "unwrap_scan.h"

namespace qh {
namespace {

constexpr int PILOT_NMAX = 1023;                       // longest moving average (odd)
constexpr int PL_THREADS = 256;

struct PilotGeom { int64_t F, S, R, NP, ND; };

// pilot (true) or payload (false) at position i of a frame, and its ordinal among its kind
__device__ __forceinline__ bool pilot_at(const PilotGeom &g, int64_t i, int64_t *ord)
{
    if (i < g.S) { *ord = i; return true; }
    const int64_t b = i - g.S;
    if (g.R == 0) { *ord = b; return false; }
    const int64_t q = b / g.R, r = b - q * g.R;
    if (r == 0) { *ord = g.S + q; return true; }
    *ord = q * (g.R - 1) + r - 1;
    return false;
}

// ------------------------------------------------------------------------------------------------ assemble / split
template <typename R>
__global__ void __launch_bounds__(PL_THREADS) pilot_frame_kernel(const Cx<R> *__restrict__ pilots, const Cx<R> *__restrict__ payload, const int32_t *__restrict__ labels,
                                                                 PilotGeom g, int64_t nframes, int own_payload, double scale, Cx<R> *__restrict__ frame,
                                                                 int32_t *__restrict__ idx_frame)
{
    const int64_t total = nframes * g.F;
    const int64_t p = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x;
    if (p >= total) return;
    const int64_t mode = blockIdx.y;
    const int64_t f = p / g.F, i = p - f * g.F;
    int64_t ord;
    if (pilot_at(g, i, &ord)) {
        const Cx<R> x = ldg(pilots + mode * g.NP + ord);
        // the product in double, rounded once: what numpy's multiplication by a scalar of either width leaves
        stg(frame + mode * total + p, Cx<R>{(R)((double)x.re * scale), (R)((double)x.im * scale)});
        if (idx_frame) idx_frame[mode * total + p] = -1;
    } else {
        const int64_t row = own_payload ? nframes * g.ND : g.ND, at = own_payload ? f * g.ND + ord : ord;
        stg(frame + mode * total + p, ldg(payload + mode * row + at));
        if (idx_frame) idx_frame[mode * total + p] = labels[mode * row + at];
    }
}

template <typename R>
__global__ void __launch_bounds__(PL_THREADS) pilot_split_kernel(const Cx<R> *__restrict__ E, int64_t L, PilotGeom g, const int32_t *__restrict__ frames, int64_t nfr,
                                                                 Cx<R> *__restrict__ payload, Cx<R> *__restrict__ pilots)
{
    const int64_t p = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x;
    if (p >= nfr * g.F) return;
    const int64_t mode = blockIdx.y;
    const int64_t q = p / g.F, i = p - q * g.F;
    const int64_t f = frames[q];
    if (f < 0 || (f + 1) * g.F > L) return;             // (the host layer refuses such a list; nothing outside the rows is ever read)
    int64_t ord;
    const bool pil = pilot_at(g, i, &ord);
    if (pil ? pilots == nullptr : payload == nullptr) return;
    const Cx<R> x = ldg(E + mode * L + f * g.F + i);
    if (pil) stg(pilots + (mode * nfr + q) * g.NP + ord, x);
    else stg(payload + (mode * nfr + q) * g.ND + ord, x);
}

// ------------------------------------------------------------------------------------------------ unwrapped pilot phase
template <typename R> struct PhaseArgs {
    const Cx<R> *E;          // (nmodes, L)
    const Cx<R> *sent;       // (nmodes, nref)
    const int64_t *where;    // (npf) positions inside a frame; nullptr: pilot j sits at sample j
    int64_t L, npf, F, span, n, nref, nchunk;
};

__device__ __forceinline__ int64_t pilot_pos(const int64_t *where, int64_t npf, int64_t F, int64_t j)
{
    if (!where) return j;
    const int64_t f = j / npf;
    return where[j - f * npf] + f * F;
}

// angle of pilot j of a mode against its reference, in double; a position outside the span counts as a zero sample (angle 0)
template <typename R> __device__ __forceinline__ double pilot_angle(const PhaseArgs<R> &a, int64_t mode, int64_t j)
{
    const int64_t pos = pilot_pos(a.where, a.npf, a.F, j);
    if (pos < 0 || pos >= a.span) return 0.;
    const Cx<R> x = ldg(a.E + mode * a.L + pos), s = ldg(a.sent + mode * a.nref + j % a.nref);
    const double xr = (double)x.re, xi = (double)x.im, sr = (double)s.re, si = (double)s.im;
    return atan2(xi * sr - xr * si, xr * sr + xi * si);
}

template <typename R>
__global__ void __launch_bounds__(UW_THREADS) pilot_theta_kernel(PhaseArgs<R> a, double *__restrict__ theta, int *__restrict__ chunk_sum, int *__restrict__ first_jump)
{
    __shared__ double th[UW_CHUNK + 1];                // th[li]: angle of pilot base - 1 + li
    __shared__ int red[UW_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t mode = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * UW_CHUNK;
#pragma unroll
    for (int r = 0; r < UW_PER_THREAD; r++) {
        const int el = r * UW_THREADS + tid;
        const int64_t k = base + el;
        double t = 0.;
        if (k < a.n) {
            t = pilot_angle<R>(a, mode, k);
            theta[mode * a.n + k] = t;
        }
        th[1 + el] = t;
    }
    if (tid == 0) th[0] = base >= 1 ? pilot_angle<R>(a, mode, base - 1) : 0.;
    __syncthreads();
    const int s = block_sum_int(strided_wrap_counts(th, base, a.n, first_jump + mode * a.nchunk + blockIdx.x), red);
    if (tid == 0) chunk_sum[mode * a.nchunk + blockIdx.x] = s;
}

// theta -> theta + 2 pi K in place: a workgroup reads and writes its own chunk only (the step into the chunk was decided by pilot_theta_kernel)
__global__ void __launch_bounds__(UW_THREADS) pilot_unwrap_kernel(double *__restrict__ phase, int64_t n, int64_t nchunk, const int *__restrict__ chunk_off,
                                                                  const int *__restrict__ first_jump)
{
    __shared__ double th[UW_CHUNK];
    __shared__ int corr[UW_CHUNK];
    __shared__ int wsum[UW_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t mode = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * UW_CHUNK;
#pragma unroll
    for (int r = 0; r < UW_PER_THREAD; r++) {
        const int el = r * UW_THREADS + tid;
        const int64_t k = base + el;
        th[el] = k < n ? phase[mode * n + k] : 0.;
    }
    __syncthreads();
    int jmp[UW_PER_THREAD];
    owned_wrap_counts(th, base, n, first_jump + mode * nchunk + blockIdx.x, jmp);
    chunk_prefix(jmp, chunk_off[mode * nchunk + blockIdx.x], corr, wsum);
#pragma unroll
    for (int r = 0; r < UW_PER_THREAD; r++) {
        const int el = r * UW_THREADS + tid;
        const int64_t k = base + el;
        if (k < n) phase[mode * n + k] = th[el] + 2 * QH_PI * (double)corr[el];
    }
}

template <typename R> void launch_phase(PhaseArgs<R> a, int nmodes, double *phase, const UnwrapScratch &s)
{
    const dim3 grid((unsigned)a.nchunk, nmodes);
    hipLaunchKernelGGL((pilot_theta_kernel<R>), grid, dim3(UW_THREADS), 0, g_stream, a, phase, s.csum, s.first);
    hipLaunchKernelGGL(unwrap_scan_kernel, dim3(nmodes), dim3(1024), 0, g_stream, s.csum, a.nchunk);
    hipLaunchKernelGGL(pilot_unwrap_kernel, grid, dim3(UW_THREADS), 0, g_stream, phase, a.n, a.nchunk, (const int *)s.csum, (const int *)s.first);
}

// ------------------------------------------------------------------------------------------------ knots, trace, fit
__global__ void __launch_bounds__(PL_THREADS) pilot_knots_kernel(const double *__restrict__ phase, int64_t n, int N, const int64_t *__restrict__ where, int64_t npf,
                                                                 int64_t F, double *__restrict__ knot_phase, int64_t *__restrict__ knot_pos)
{
    const int64_t nk = n - N + 1;
    const int64_t k = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x;
    if (k >= nk) return;
    const double *p = phase + (int64_t)blockIdx.y * n + k;
    double s = 0.;
    for (int t = 0; t < N; t++) s += p[t];
    knot_phase[(int64_t)blockIdx.y * nk + k] = s / (double)N;
    if (blockIdx.y == 0 && knot_pos) knot_pos[k] = pilot_pos(where, npf, F, k + N / 2);
}

// np.interp of the knot phases to every symbol of [0, span) - constant before the first and after the last knot - and its removal.  The trace is
// rounded once to the signal's real type; the rotation takes the phase reduced to (-pi, pi] in double first, so that a long trace keeps its digits.
template <typename R>
__global__ void __launch_bounds__(PL_THREADS) pilot_interp_kernel(const Cx<R> *__restrict__ E, int64_t L, int64_t span, const int64_t *__restrict__ knots,
                                                                  const double *__restrict__ kph, int64_t nk, Cx<R> *__restrict__ Eout, R *__restrict__ trace)
{
    const int64_t i = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x;
    if (i >= span) return;
    const int64_t mode = blockIdx.y;
    const double *p = kph + mode * nk;
    double ph;
    if (i <= knots[0]) ph = p[0];
    else if (i >= knots[nk - 1]) ph = p[nk - 1];
    else {
        int64_t lo = 0, hi = nk - 1;                   // knots[lo] <= i < knots[hi]
        while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (knots[mid] <= i) lo = mid; else hi = mid; }
        const double slope = (p[hi] - p[lo]) / (double)(knots[hi] - knots[lo]);
        ph = slope * (double)(i - knots[lo]) + p[lo];
    }
    trace[mode * span + i] = (R)ph;
    const R t = (R)(ph - 2 * QH_PI * rint(ph / (2 * QH_PI)));
    R sn, cs;
    if constexpr (sizeof(R) == 4) sincosf(t, &sn, &cs); else sincos(t, &sn, &cs);
    const Cx<R> x = ldg(E + mode * L + i);
    stg(Eout + mode * span + i, Cx<R>{fma_(x.re, cs, x.im * sn), fma_(x.im, cs, -(x.re * sn))});
}

// One workgroup per mode over the n unwrapped phases y_k: the mean, and (fit != nullptr) the least-squares line through (k, y_k) from sums centred on
// both means: slope = sum (k - kbar)(y - ybar) / sum (k - kbar)^2, intercept = ybar - slope kbar.  fit[mode] = [slope / (2 pi), intercept].
__global__ void __launch_bounds__(PL_THREADS) pilot_fit_kernel(const double *__restrict__ phase, int64_t n, double *__restrict__ fit, double *__restrict__ mean)
{
    __shared__ double red[PL_THREADS / 64];
    const double *y = phase + (int64_t)blockIdx.x * n;
    double s = 0.;
    for (int64_t k = threadIdx.x; k < n; k += PL_THREADS) s += y[k];
    const double ybar = block_sum<PL_THREADS>(s, red) / (double)n;
    if (mean && threadIdx.x == 0) mean[blockIdx.x] = ybar;
    if (!fit) return;                                  // (uniform)
    const double kbar = 0.5 * (double)(n - 1);
    double sxy = 0., sxx = 0.;
    for (int64_t k = threadIdx.x; k < n; k += PL_THREADS) {
        const double dk = (double)k - kbar;
        sxy += dk * (y[k] - ybar);
        sxx += dk * dk;
    }
    sxy = block_sum<PL_THREADS>(sxy, red);
    sxx = block_sum<PL_THREADS>(sxx, red);
    if (threadIdx.x == 0) {
        const double slope = sxy / sxx;
        fit[2 * blockIdx.x] = slope / (2 * QH_PI);
        fit[2 * blockIdx.x + 1] = ybar - slope * kbar;
    }
}

// fo[mode]: the mode's own slope / (2 pi), or the mean over the modes (summed in mode order) in every entry
__global__ void __launch_bounds__(64) pilot_fo_kernel(const double *__restrict__ fit, int nmodes, int average, double *__restrict__ fo)
{
    double avg = 0.;
    if (average) {
        for (int m = 0; m < nmodes; m++) avg += fit[2 * m];
        avg /= (double)nmodes;
    }
    for (int m = threadIdx.x; m < nmodes; m += 64) fo[m] = average ? avg : fit[2 * m];
}

template <typename R>
__global__ void __launch_bounds__(PL_THREADS) rotate_rows_kernel(const Cx<R> *E, int64_t L, const double *__restrict__ phi, Cx<R> *out)      // (out may be E)
{
    const int64_t i = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x;
    if (i >= L) return;
    const int64_t mode = blockIdx.y;
    double sn, cs;
    sincos(phi[mode], &sn, &cs);
    const Cx<R> x = ldg(E + mode * L + i);
    const double xr = (double)x.re, xi = (double)x.im;
    stg(out + mode * L + i, Cx<R>{(R)(xr * cs + xi * sn), (R)(xi * cs - xr * sn)});
}

// ------------------------------------------------------------------------------------------------ host side
int pilot_geom(int64_t F, int64_t S, int64_t R, PilotGeom *g, const char *who)
{
    if (!(F >= 1 && S >= 0 && S <= F && R >= 0 && R != 1) || (R > 0 && (F - S) % R != 0)) {
        set_error(std::string(who) + ": a frame of F symbols needs 0 <= S <= F and R == 0 or R >= 2 with (F - S) % R == 0");
        return QH_ERR_ARG;
    }
    g->F = F; g->S = S; g->R = R;
    g->NP = S + (R > 0 ? (F - S) / R : 0);
    g->ND = F - g->NP;
    return QH_OK;
}

inline bool grid_ok(int64_t n, int per) { return (n + per - 1) / per <= 0x7fffffffLL; }

template <typename R>
int pilot_frame_dev(const void *pilots, const void *payload, const int32_t *labels, int nmodes, int64_t F, int64_t S, int64_t Rr, int64_t nframes, int own_payload,
                    double scale, void *frame, int32_t *idx_frame)
{
    int rc = ensure_init();
    if (rc) return rc;
    PilotGeom g;
    if ((rc = pilot_geom(F, S, Rr, &g, "pilot_frame"))) return rc;
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && nframes >= 1 && nframes <= ((int64_t)1 << 40) / F && grid_ok(nframes * F, PL_THREADS), "pilot_frame: bad sizes");
    QH_REQUIRE(frame && (pilots || g.NP == 0) && (payload || g.ND == 0), "pilot_frame: pilots, payload and frame must be given");
    QH_REQUIRE(!idx_frame || labels || g.ND == 0, "pilot_frame: idx_frame needs the payload labels");
    hipLaunchKernelGGL((pilot_frame_kernel<R>), dim3((unsigned)((nframes * F + PL_THREADS - 1) / PL_THREADS), nmodes), dim3(PL_THREADS), 0, g_stream, (const Cx<R> *)pilots,
                       (const Cx<R> *)payload, labels, g, nframes, own_payload ? 1 : 0, scale, (Cx<R> *)frame, idx_frame);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R>
int pilot_split_dev(const void *E, int nmodes, int64_t L, int64_t F, int64_t S, int64_t Rr, const int32_t *frames, int64_t nfr, void *payload, void *pilots)
{
    int rc = ensure_init();
    if (rc) return rc;
    PilotGeom g;
    if ((rc = pilot_geom(F, S, Rr, &g, "pilot_split"))) return rc;
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= F && nfr >= 1 && nfr <= ((int64_t)1 << 40) / F && grid_ok(nfr * F, PL_THREADS), "pilot_split: bad sizes");
    QH_REQUIRE(E && frames && (payload || pilots), "pilot_split: E, frames and one of payload and pilots must be given");
    hipLaunchKernelGGL((pilot_split_kernel<R>), dim3((unsigned)((nfr * F + PL_THREADS - 1) / PL_THREADS), nmodes), dim3(PL_THREADS), 0, g_stream, (const Cx<R> *)E, L, g,
                       frames, nfr, (Cx<R> *)payload, (Cx<R> *)pilots);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R>
int phase_args(PhaseArgs<R> *a, const char *who, const void *E, int nmodes, int64_t L, const int64_t *where, int64_t npf, int64_t nframes, int64_t F, int64_t span, int64_t n,
               const void *sent, int64_t nref)
{
    const bool ok = nmodes >= 1 && nmodes <= 65535 && L >= 1 && F >= 1 && npf >= 1 && npf <= F && nframes >= 1 && nframes <= ((int64_t)1 << 40) / F && span >= 1 && span <= L &&
                    span <= nframes * F && n >= 1 && n <= npf * nframes && n <= span && nref >= 1 && E && where && sent;
    if (!ok) {
        set_error(std::string(who) + ": bad sizes (1 <= npf <= F, 1 <= span <= min(L, nframes F), 1 <= n <= min(npf nframes, span), nref >= 1; E, where and sent given)");
        return QH_ERR_ARG;
    }
    a->E = (const Cx<R> *)E; a->sent = (const Cx<R> *)sent; a->where = where;
    a->L = L; a->npf = npf; a->F = F; a->span = span; a->n = n; a->nref = nref;
    a->nchunk = (n + UW_CHUNK - 1) / UW_CHUNK;
    return QH_OK;
}

template <typename R>
int pilot_phase_dev(const void *E, int nmodes, int64_t L, const int64_t *where, int64_t npf, int64_t nframes, int64_t F, int64_t span, int64_t n, const void *sent,
                    int64_t nref, double *phase)
{
    int rc = ensure_init();
    if (rc) return rc;
    PhaseArgs<R> a;
    if ((rc = phase_args<R>(&a, "pilot_phase", E, nmodes, L, where, npf, nframes, F, span, n, sent, nref))) return rc;
    QH_REQUIRE(phase, "pilot_phase: phase must be given");
    UnwrapScratch s;
    if ((rc = unwrap_scratch(Slot::PILOT, nmodes, a.nchunk, 0, &s))) return rc;
    launch_phase<R>(a, nmodes, phase, s);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

int pilot_knots_dev(const double *phase, int nmodes, int64_t n, int N, const int64_t *where, int64_t npf, int64_t F, double *knot_phase, int64_t *knot_pos)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && n >= 1 && grid_ok(n, PL_THREADS), "pilot_knots: bad sizes");
    QH_REQUIRE(N >= 3 && N <= PILOT_NMAX && (N & 1) && N <= n, "pilot_knots: N must be odd, between 3 and min(n, 1023)");
    QH_REQUIRE(phase && knot_phase, "pilot_knots: phase and knot_phase must be given");
    QH_REQUIRE(!knot_pos || !where || (npf >= 1 && F >= npf), "pilot_knots: bad position table");
    const int64_t nk = n - N + 1;
    hipLaunchKernelGGL(pilot_knots_kernel, dim3((unsigned)((nk + PL_THREADS - 1) / PL_THREADS), nmodes), dim3(PL_THREADS), 0, g_stream, phase, n, N, where, npf, F, knot_phase,
                       knot_pos);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R>
int pilot_cpe_dev(const void *E, int nmodes, int64_t L, const int64_t *where, int64_t npf, int64_t nframes, int64_t F, int64_t span, int64_t n, const void *sent, int64_t nref,
                  int N, void *Eout, void *trace)
{
    int rc = ensure_init();
    if (rc) return rc;
    PhaseArgs<R> a;
    if ((rc = phase_args<R>(&a, "pilot_cpe", E, nmodes, L, where, npf, nframes, F, span, n, sent, nref))) return rc;
    QH_REQUIRE(N >= 3 && N <= PILOT_NMAX && (N & 1) && N <= n, "pilot_cpe: N must be odd, between 3 and min(n, 1023)");
    QH_REQUIRE(Eout && trace && grid_ok(span, PL_THREADS), "pilot_cpe: Eout and trace must be given");
    const int64_t nk = n - N + 1;
    // scratch: phase | knot phases | knot positions | (chunk sums | first counts)
    ScratchLayout head;
    const size_t o_phase = head.take((size_t)nmodes * n * sizeof(double)), o_kph = head.take((size_t)nmodes * nk * sizeof(double)), o_pos = head.take((size_t)nk * sizeof(int64_t));
    UnwrapScratch s;
    if ((rc = unwrap_scratch(Slot::PILOT, nmodes, a.nchunk, head.total, &s))) return rc;
    double *phase = (double *)(s.base + o_phase), *kph = (double *)(s.base + o_kph);
    int64_t *kpos = (int64_t *)(s.base + o_pos);
    launch_phase<R>(a, nmodes, phase, s);
    hipLaunchKernelGGL(pilot_knots_kernel, dim3((unsigned)((nk + PL_THREADS - 1) / PL_THREADS), nmodes), dim3(PL_THREADS), 0, g_stream, (const double *)phase, n, N, where, npf, F,
                       kph, kpos);
    hipLaunchKernelGGL((pilot_interp_kernel<R>), dim3((unsigned)((span + PL_THREADS - 1) / PL_THREADS), nmodes), dim3(PL_THREADS), 0, g_stream, (const Cx<R> *)E, L, span,
                       (const int64_t *)kpos, (const double *)kph, nk, (Cx<R> *)Eout, (R *)trace);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

// unwrapped phase of rec against ref (both (nmodes, n), pilot j at sample j) into scratch
template <typename R> int pair_phase(const char *who, const void *rec, const void *ref, int nmodes, int64_t n, int64_t nmin, double **phase)
{
    if (!(nmodes >= 1 && nmodes <= 65535 && n >= nmin && n <= ((int64_t)1 << 40) && rec && ref)) {
        set_error(std::string(who) + ": bad sizes, or rec / ref not given");
        return QH_ERR_ARG;
    }
    PhaseArgs<R> a;
    a.E = (const Cx<R> *)rec; a.sent = (const Cx<R> *)ref; a.where = nullptr;
    a.L = n; a.npf = 1; a.F = 1; a.span = n; a.n = n; a.nref = n;
    a.nchunk = (n + UW_CHUNK - 1) / UW_CHUNK;
    UnwrapScratch s;
    int rc = unwrap_scratch(Slot::PILOT, nmodes, a.nchunk, (size_t)nmodes * n * sizeof(double), &s);
    if (rc) return rc;
    *phase = (double *)s.base;
    launch_phase<R>(a, nmodes, *phase, s);
    return QH_OK;
}

template <typename R> int pilot_foe_dev(const void *rec, const void *ref, int nmodes, int64_t n, int average, double *fit, double *fo)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(fit && fo, "pilot_foe: fit and fo must be given");
    double *phase = nullptr;
    if ((rc = pair_phase<R>("pilot_foe", rec, ref, nmodes, n, 2, &phase))) return rc;
    hipLaunchKernelGGL(pilot_fit_kernel, dim3(nmodes), dim3(PL_THREADS), 0, g_stream, (const double *)phase, n, fit, (double *)nullptr);
    hipLaunchKernelGGL(pilot_fo_kernel, dim3(1), dim3(64), 0, g_stream, (const double *)fit, nmodes, average ? 1 : 0, fo);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R> int pilot_const_phase_dev(const void *rec, const void *ref, int nmodes, int64_t n, double *mean)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(mean, "pilot_const_phase: the output must be given");
    double *phase = nullptr;
    if ((rc = pair_phase<R>("pilot_const_phase", rec, ref, nmodes, n, 1, &phase))) return rc;
    hipLaunchKernelGGL(pilot_fit_kernel, dim3(nmodes), dim3(PL_THREADS), 0, g_stream, (const double *)phase, n, (double *)nullptr, mean);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R> int rotate_rows_dev(const void *E, int nmodes, int64_t L, const double *phi, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 1 && grid_ok(L, PL_THREADS), "rotate_rows: bad sizes");
    QH_REQUIRE(E && phi && out, "rotate_rows: E, phi and out must be given");
    hipLaunchKernelGGL((rotate_rows_kernel<R>), dim3((unsigned)((L + PL_THREADS - 1) / PL_THREADS), nmodes), dim3(PL_THREADS), 0, g_stream, (const Cx<R> *)E, L, phi, (Cx<R> *)out);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

}  // namespace
}  // namespace qh

extern "C" {
int qh_pilot_frame_c64_dev(const void *pilots, const void *payload, const int32_t *labels, int nmodes, int64_t F, int64_t S, int64_t R, int64_t nframes, int own_payload,
                           double pilot_scale, void *frame, int32_t *idx_frame)
{ return qh::pilot_frame_dev<float>(pilots, payload, labels, nmodes, F, S, R, nframes, own_payload, pilot_scale, frame, idx_frame); }
int qh_pilot_frame_c128_dev(const void *pilots, const void *payload, const int32_t *labels, int nmodes, int64_t F, int64_t S, int64_t R, int64_t nframes, int own_payload,
                            double pilot_scale, void *frame, int32_t *idx_frame)
{ return qh::pilot_frame_dev<double>(pilots, payload, labels, nmodes, F, S, R, nframes, own_payload, pilot_scale, frame, idx_frame); }
int qh_pilot_split_c64_dev(const void *E, int nmodes, int64_t L, int64_t F, int64_t S, int64_t R, const int32_t *frames, int64_t nfr, void *payload, void *pilots)
{ return qh::pilot_split_dev<float>(E, nmodes, L, F, S, R, frames, nfr, payload, pilots); }
int qh_pilot_split_c128_dev(const void *E, int nmodes, int64_t L, int64_t F, int64_t S, int64_t R, const int32_t *frames, int64_t nfr, void *payload, void *pilots)
{ return qh::pilot_split_dev<double>(E, nmodes, L, F, S, R, frames, nfr, payload, pilots); }
int qh_pilot_phase_c64_dev(const void *E, int nmodes, int64_t L, const int64_t *where, int64_t npf, int64_t nframes, int64_t F, int64_t span, int64_t n, const void *sent,
                           int64_t nref, double *phase)
{ return qh::pilot_phase_dev<float>(E, nmodes, L, where, npf, nframes, F, span, n, sent, nref, phase); }
int qh_pilot_phase_c128_dev(const void *E, int nmodes, int64_t L, const int64_t *where, int64_t npf, int64_t nframes, int64_t F, int64_t span, int64_t n, const void *sent,
                            int64_t nref, double *phase)
{ return qh::pilot_phase_dev<double>(E, nmodes, L, where, npf, nframes, F, span, n, sent, nref, phase); }
int qh_pilot_knots_dev(const double *phase, int nmodes, int64_t n, int N, const int64_t *where, int64_t npf, int64_t F, double *knot_phase, int64_t *knot_pos)
{ return qh::pilot_knots_dev(phase, nmodes, n, N, where, npf, F, knot_phase, knot_pos); }
int qh_pilot_cpe_c64_dev(const void *E, int nmodes, int64_t L, const int64_t *where, int64_t npf, int64_t nframes, int64_t F, int64_t span, int64_t n, const void *sent,
                         int64_t nref, int N, void *Eout, void *trace)
{ return qh::pilot_cpe_dev<float>(E, nmodes, L, where, npf, nframes, F, span, n, sent, nref, N, Eout, trace); }
int qh_pilot_cpe_c128_dev(const void *E, int nmodes, int64_t L, const int64_t *where, int64_t npf, int64_t nframes, int64_t F, int64_t span, int64_t n, const void *sent,
                          int64_t nref, int N, void *Eout, void *trace)
{ return qh::pilot_cpe_dev<double>(E, nmodes, L, where, npf, nframes, F, span, n, sent, nref, N, Eout, trace); }
int qh_pilot_foe_c64_dev(const void *rec, const void *ref, int nmodes, int64_t n, int average, double *fit, double *fo)
{ return qh::pilot_foe_dev<float>(rec, ref, nmodes, n, average, fit, fo); }
int qh_pilot_foe_c128_dev(const void *rec, const void *ref, int nmodes, int64_t n, int average, double *fit, double *fo)
{ return qh::pilot_foe_dev<double>(rec, ref, nmodes, n, average, fit, fo); }
int qh_pilot_const_phase_c64_dev(const void *rec, const void *ref, int nmodes, int64_t n, double *phase)
{ return qh::pilot_const_phase_dev<float>(rec, ref, nmodes, n, phase); }
int qh_pilot_const_phase_c128_dev(const void *rec, const void *ref, int nmodes, int64_t n, double *phase)
{ return qh::pilot_const_phase_dev<double>(rec, ref, nmodes, n, phase); }
int qh_rotate_rows_c64_dev(const void *E, int nmodes, int64_t L, const double *phi, void *out)
{ return qh::rotate_rows_dev<float>(E, nmodes, L, phi, out); }
int qh_rotate_rows_c128_dev(const void *E, int nmodes, int64_t L, const double *phi, void *out)
{ return qh::rotate_rows_dev<double>(E, nmodes, L, phi, out); }
}
