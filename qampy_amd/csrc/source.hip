// The bit source and the Gray mapper in HBM: what qampy.core.prbs (make_prbs_extXOR / make_prbs_intXOR), PRBSBits and
// SignalQAMGrayCoded._modulate / _demodulate (qampy/signals.py:89-137, :678-731) do on the host.  Everything here is integer or a table
// look-up: the results are the reference's bit for bit.
//
//   source    PRBS -> bits / labels / symbols of one row in ONE launch.  A thread owns `wpt` 32-bit words of the sequence; it jumps to its
//             first bit (prbs_core.h: <= 31 multiplications of 31-bit polynomials, none of them depending on the call's start), runs the
//             recurrence 14 .. 28 bits per step (external form) and leaves its words in LDS.  Then the workgroup writes what the caller asked
//             for from LDS, coalesced: the bits as one byte each, 16 per store on the 16-byte grid of the destination (whatever its
//             alignment; the ragged ends byte by byte), and - fused form - labels (MSB first per symbol) and alphabet[label].
//             Bits only: wpt = 8, SRC_W = 65536 bits per workgroup.  Fused: wpt = nb, so every thread's stretch is 32 whole symbols and a
//             workgroup SRC_SYMS = 8192 symbols, whatever nb: no symbol straddles a thread or a workgroup.
//   map       bits (bytes, any non-zero value is a one) -> labels and / or alphabet[label], one thread per symbol; a label outside [0, M) -> 0.
//   unmap     labels -> bits, one thread per symbol; the low nb bits of a label.
//   shaped    probabilistically shaped symbols: two counter-based uniform draws per sample pick the I and the Q level (see ps_symbols_kernel).
//
// No atomics, no scratch: a repeated call is bit-identical.  Every launch is bounded by the call's arguments alone.
#include "common.h"
#include "prbs_core.h"
#include "philox.h"

namespace qh {

constexpr int SRC_T = 256;                          // threads of every kernel here
constexpr int SRC_WPT_BITS = 8;                     // words per thread of the bits-only form
constexpr int SRC_WPT_MAX = 10;                     // = the largest nb
constexpr int64_t SRC_W = (int64_t)SRC_T * SRC_WPT_BITS * 32;      // bits per workgroup, bits-only form
constexpr int SRC_SPT = 32;                         // symbols per thread of the fused form
constexpr int SRC_SYMS = SRC_T * SRC_SPT;           // symbols per workgroup of the fused form
constexpr int64_t SRC_NMAX = (int64_t)1 << 31;      // most bits of a row, most symbols of a mapping call
constexpr int64_t SRC_START_MAX = (int64_t)1 << 62;

// 32 bits of the LDS bit array from bit `off` on (the array has one zero word behind its last)
__device__ __forceinline__ uint32_t src_bits_at(const uint32_t *lds, int off)
{
    const int w = off >> 5, s = off & 31;
    return (uint32_t)((((uint64_t)lds[w + 1] << 32) | lds[w]) >> s);
}
// four bits -> four bytes of 0 / 1, the lowest bit in the lowest byte
__device__ __forceinline__ uint32_t src_spread4(uint32_t x) { return ((x & 0xFu) * 0x00204081u) & 0x01010101u; }

// grid (workgroups of the row).  nbits: bits of the row; wpt: words per thread; bits / labels / symbols: each written if given.
// SYMS: nb = wpt, nsym symbols of nb bits, alphabet of 2^nb points.
template <typename R, bool SYMS>
__global__ void __launch_bounds__(SRC_T) source_kernel(const PrbsParams p, int wpt, int64_t nbits, uint8_t *__restrict__ bits, int64_t nsym,
                                                        int32_t *__restrict__ labels, const Cx<R> *__restrict__ alphabet, Cx<R> *__restrict__ symbols)
{
    __shared__ uint32_t lds[SRC_T * SRC_WPT_MAX + 1];
    const int tid = threadIdx.x;
    const int64_t wg_bits = (int64_t)SRC_T * wpt * 32;
    const int64_t g0 = (int64_t)blockIdx.x * wg_bits;                      // first bit of this workgroup, < nbits <= 2^31
    const int64_t mine = g0 + (int64_t)tid * wpt * 32;                     // first bit of this thread
    if (mine < nbits) {
        uint64_t v;
        int known;
        prbs_seek(p, (uint32_t)mine, v, known);
        for (int w = 0; w < wpt; w++) lds[tid * wpt + w] = prbs_next(v, known, p.o, p.m) ^ p.flip;
    } else {
        for (int w = 0; w < wpt; w++) lds[tid * wpt + w] = 0;
    }
    if (tid == 0) lds[SRC_T * wpt] = 0;
    __syncthreads();

    const int len = (int)(nbits - g0 < wg_bits ? nbits - g0 : wg_bits);      // bits of this workgroup that exist
    if (bits) {
        uint8_t *dst = bits + g0;
        const int mis = (int)((uintptr_t)dst & 15);
        const int nvec = (len + mis + 15) >> 4;
        for (int v = tid; v < nvec; v += SRC_T) {
            const int rel = 16 * v - mis;                                    // bit of this workgroup in the vector's first byte; < 0 only for v = 0
            const uint32_t x = rel >= 0 ? src_bits_at(lds, rel) : src_bits_at(lds, 0) << (-rel);
            if (rel >= 0 && rel + 16 <= len) {
                uint4 o;
                o.x = src_spread4(x); o.y = src_spread4(x >> 4); o.z = src_spread4(x >> 8); o.w = src_spread4(x >> 12);
                *reinterpret_cast<uint4 *>(dst + rel) = o;
            } else {
                for (int b = 0; b < 16; b++)
                    if (rel + b >= 0 && rel + b < len) dst[rel + b] = (uint8_t)((x >> b) & 1u);
            }
        }
    }
    if constexpr (SYMS) {
        const int nb = wpt;
        const int64_t s0 = (int64_t)blockIdx.x * SRC_SYMS;
#pragma unroll 4
        for (int i = 0; i < SRC_SPT; i++) {
            const int s = i * SRC_T + tid;
            if (s0 + s >= nsym) break;
            const int32_t label = (int32_t)(__brev(src_bits_at(lds, s * nb)) >> (32 - nb));      // the first bit is the label's MSB
            if (labels) labels[s0 + s] = label;
            if (symbols) stg(symbols + s0 + s, ldg(alphabet + label));
        }
    }
}

// one thread per symbol: label from nb bytes, MSB first
template <typename R>
__global__ void __launch_bounds__(SRC_T) source_map_kernel(const uint8_t *__restrict__ bits, int64_t nsym, int nb, int32_t *__restrict__ labels,
                                                            const Cx<R> *__restrict__ alphabet, int M, Cx<R> *__restrict__ symbols)
{
    const int64_t s = (int64_t)blockIdx.x * SRC_T + threadIdx.x;
    if (s >= nsym) return;
    const uint8_t *b = bits + s * nb;
    int32_t label = 0;
    for (int j = 0; j < nb; j++) label = (label << 1) | (b[j] != 0);
    if (labels) labels[s] = label;
    if (symbols) stg(symbols + s, label < M ? ldg(alphabet + label) : Cx<R>{(R)0, (R)0});
}

__global__ void __launch_bounds__(SRC_T) source_unmap_kernel(const int32_t *__restrict__ labels, int64_t nsym, int nb, uint8_t *__restrict__ bits)
{
    const int64_t s = (int64_t)blockIdx.x * SRC_T + threadIdx.x;
    if (s >= nsym) return;
    const uint32_t label = (uint32_t)labels[s];
    uint8_t *b = bits + s * nb;
    for (int j = 0; j < nb; j++) b[j] = (uint8_t)((label >> (nb - 1 - j)) & 1u);
}

// The shaped source (theory.generate_ps_symbols): rail I and rail Q of sample n of mode m each pick one of L levels with the probabilities px.
// The Philox words x (I) and y (Q) of counter (n low, n high, m, IMP_STREAM_SHAPE) become u = word 2^-32 in double, and the level's index is the
// number of entries of the cumulative table that are <= u (np.searchsorted(cdf, u, side="right")).  The table comes by value, padded to PS_LMAX
// entries with 2 (never <= u), its last real entry 1 (never <= u either): the search is six fixed steps and its answer lies in [0, L).
constexpr int PS_LMAX = 64;                         // most levels of a rail
constexpr int PS_T = 256, PS_PER = 4, PS_TILE = PS_T * PS_PER;      // samples of one mode per workgroup
struct PsTables { double cdf[PS_LMAX], level[PS_LMAX]; };

template <typename R>
__global__ void __launch_bounds__(PS_T) ps_symbols_kernel(const PsTables tab, int L, int64_t N, unsigned k0, unsigned k1, const int32_t *__restrict__ label_table,
                                                           Cx<R> *__restrict__ out, int32_t *__restrict__ labels)
{
    __shared__ double cdf[PS_LMAX];
    __shared__ R level[PS_LMAX];
    if (threadIdx.x < PS_LMAX) { cdf[threadIdx.x] = tab.cdf[threadIdx.x]; level[threadIdx.x] = (R)tab.level[threadIdx.x]; }
    __syncthreads();
    const int m = blockIdx.y;
#pragma unroll
    for (int j = 0; j < PS_PER; j++) {
        const int64_t n = (int64_t)blockIdx.x * PS_TILE + j * PS_T + threadIdx.x;
        if (n >= N) break;
        const Philox w = philox4x32_10((unsigned)n, (unsigned)((uint64_t)n >> 32), (unsigned)m, IMP_STREAM_SHAPE, k0, k1);
        const double ui = (double)w.x * 0x1p-32, uq = (double)w.y * 0x1p-32;
        int i = 0, q = 0;
#pragma unroll
        for (int step = PS_LMAX / 2; step >= 1; step >>= 1) {
            if (cdf[i + step - 1] <= ui) i += step;
            if (cdf[q + step - 1] <= uq) q += step;
        }
        stg(out + (size_t)m * N + n, Cx<R>{level[i], level[q]});
        if (labels) labels[(size_t)m * N + n] = label_table[i * L + q];
    }
}

// ------------------------------------------------------------------------------------------------ host side
// cdf, level: HOST tables of L entries; label_table (L, L) int32 in device memory, needed when labels is given
template <typename R>
static int ps_symbols_dev(void *out, int nmodes, int64_t N, const double *level, const double *cdf, int L, uint64_t seed, int32_t *labels,
                          const int32_t *label_table)
{
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && N >= 1 && N <= SRC_NMAX, "ps_symbols: 1 .. 65535 modes of 1 .. 2^31 samples");      // one workgroup per tile: 2^21 at the most
    QH_REQUIRE(L >= 1 && L <= PS_LMAX, "ps_symbols: between 1 and 64 levels");
    QH_REQUIRE(out && level && cdf, "ps_symbols: out, the levels and the cumulative table must be given");
    QH_REQUIRE(!labels || label_table, "ps_symbols: labels need the label table");
    PsTables tab;
    for (int i = 0; i < PS_LMAX; i++) { tab.cdf[i] = 2.0; tab.level[i] = 0.0; }
    for (int i = 0; i < L; i++) {
        QH_REQUIRE(cdf[i] >= 0 && cdf[i] <= 1 && (i == 0 || cdf[i] >= cdf[i - 1]), "ps_symbols: the cumulative table must rise from >= 0 to 1");
        tab.cdf[i] = cdf[i]; tab.level[i] = level[i];
    }
    QH_REQUIRE(cdf[L - 1] == 1.0, "ps_symbols: the last entry of the cumulative table must be 1");
    int rc = ensure_init();
    if (rc) return rc;
    hipLaunchKernelGGL((ps_symbols_kernel<R>), dim3((unsigned)((N + PS_TILE - 1) / PS_TILE), nmodes), dim3(PS_T), 0, g_stream, tab, L, N, (unsigned)seed,
                       (unsigned)(seed >> 32), label_table, (Cx<R> *)out, labels);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

static int src_check_prbs(int order, int kind, int64_t seed, int64_t start)
{
    QH_REQUIRE(order == 7 || order == 15 || order == 23 || order == 31, "prbs: the order must be one of 7, 15, 23, 31");
    QH_REQUIRE(kind == PRBS_EXT || kind == PRBS_INT, "prbs: kind must be 0 (external XOR) or 1 (internal XOR)");
    QH_REQUIRE(seed >= 0 && seed < ((int64_t)1 << order), "prbs: the seed must lie in [0, 2^order)");
    QH_REQUIRE(start >= 0 && start <= SRC_START_MAX, "prbs: start must lie in [0, 2^62]");
    return QH_OK;
}

static int prbs_bits_dev(int order, int kind, int64_t seed, int64_t start, int invert, int64_t n, uint8_t *bits)
{
    int rc = src_check_prbs(order, kind, seed, start);
    if (rc) return rc;
    QH_REQUIRE(n >= 1 && n <= SRC_NMAX, "prbs_bits: n must lie in [1, 2^31]");
    QH_REQUIRE(bits, "prbs_bits: bits must be given");
    if ((rc = ensure_init())) return rc;
    const PrbsParams p = prbs_setup(order, kind, (uint32_t)seed, start, invert);
    hipLaunchKernelGGL((source_kernel<float, false>), dim3((unsigned)((n + SRC_W - 1) / SRC_W)), dim3(SRC_T), 0, g_stream, p, SRC_WPT_BITS, n, bits,
                       (int64_t)0, (int32_t *)nullptr, (const Cx<float> *)nullptr, (Cx<float> *)nullptr);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

static int src_check_map(int64_t nsym, int nb)
{
    QH_REQUIRE(nb >= 2 && nb <= SRC_WPT_MAX, "source: bits per symbol must lie in [2, 10]");
    QH_REQUIRE(nsym >= 1 && nsym <= SRC_NMAX, "source: the number of symbols must lie in [1, 2^31]");
    return QH_OK;
}

template <typename R>
static int prbs_symbols_dev(int order, int kind, int64_t seed, int64_t start, int64_t nsym, int nb, const void *alphabet, int M, void *symbols,
                            int32_t *labels, uint8_t *bits)
{
    int rc = src_check_prbs(order, kind, seed, start);
    if (rc) return rc;
    if ((rc = src_check_map(nsym, nb))) return rc;
    QH_REQUIRE(nsym * nb <= SRC_NMAX, "prbs_symbols: at most 2^31 bits per row");
    QH_REQUIRE(M == (1 << nb), "prbs_symbols: the alphabet must have 2^nb points");
    QH_REQUIRE(alphabet && symbols, "prbs_symbols: alphabet and symbols must be given");
    if ((rc = ensure_init())) return rc;
    const PrbsParams p = prbs_setup(order, kind, (uint32_t)seed, start, 0);
    hipLaunchKernelGGL((source_kernel<R, true>), dim3((unsigned)((nsym + SRC_SYMS - 1) / SRC_SYMS)), dim3(SRC_T), 0, g_stream, p, nb, nsym * nb, bits, nsym,
                       labels, (const Cx<R> *)alphabet, (Cx<R> *)symbols);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

template <typename R>
static int map_bits_dev(const uint8_t *bits, int64_t nsym, int nb, const void *alphabet, int M, void *symbols, int32_t *labels, bool want_symbols)
{
    int rc = src_check_map(nsym, nb);
    if (rc) return rc;
    QH_REQUIRE(bits, "source: bits must be given");
    if (want_symbols) QH_REQUIRE(alphabet && symbols && M >= 1, "modulate_bits: alphabet (at least one point) and symbols must be given");
    else QH_REQUIRE(labels, "bits_to_labels: labels must be given");
    if ((rc = ensure_init())) return rc;
    hipLaunchKernelGGL((source_map_kernel<R>), dim3((unsigned)((nsym + SRC_T - 1) / SRC_T)), dim3(SRC_T), 0, g_stream, bits, nsym, nb, labels,
                       (const Cx<R> *)alphabet, M, (Cx<R> *)symbols);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

static int labels_to_bits_dev(const int32_t *labels, int64_t nsym, int nb, uint8_t *bits)
{
    int rc = src_check_map(nsym, nb);
    if (rc) return rc;
    QH_REQUIRE(labels && bits, "labels_to_bits: labels and bits must be given");
    if ((rc = ensure_init())) return rc;
    hipLaunchKernelGGL(source_unmap_kernel, dim3((unsigned)((nsym + SRC_T - 1) / SRC_T)), dim3(SRC_T), 0, g_stream, labels, nsym, nb, bits);
    QH_HIP(hipGetLastError());
    return QH_OK;
}

}  // namespace qh

extern "C" {
int qh_ps_symbols_c64_dev(void *out, int nmodes, int64_t N, const double *level, const double *cdf, int L, uint64_t seed, int32_t *labels,
                          const int32_t *label_table)
{ return qh::ps_symbols_dev<float>(out, nmodes, N, level, cdf, L, seed, labels, label_table); }
int qh_ps_symbols_c128_dev(void *out, int nmodes, int64_t N, const double *level, const double *cdf, int L, uint64_t seed, int32_t *labels,
                           const int32_t *label_table)
{ return qh::ps_symbols_dev<double>(out, nmodes, N, level, cdf, L, seed, labels, label_table); }
int qh_prbs_bits_dev(int order, int kind, int64_t seed, int64_t start, int invert, int64_t n, uint8_t *bits)
{ return qh::prbs_bits_dev(order, kind, seed, start, invert, n, bits); }
int qh_bits_to_labels_dev(const uint8_t *bits, int64_t nsym, int nb, int32_t *labels)
{ return qh::map_bits_dev<float>(bits, nsym, nb, nullptr, 0, nullptr, labels, false); }
int qh_labels_to_bits_dev(const int32_t *labels, int64_t nsym, int nb, uint8_t *bits) { return qh::labels_to_bits_dev(labels, nsym, nb, bits); }
int qh_modulate_bits_c64_dev(const uint8_t *bits, int64_t nsym, int nb, const void *alphabet, int M, void *symbols, int32_t *labels)
{ return qh::map_bits_dev<float>(bits, nsym, nb, alphabet, M, symbols, labels, true); }
int qh_modulate_bits_c128_dev(const uint8_t *bits, int64_t nsym, int nb, const void *alphabet, int M, void *symbols, int32_t *labels)
{ return qh::map_bits_dev<double>(bits, nsym, nb, alphabet, M, symbols, labels, true); }
int qh_prbs_symbols_c64_dev(int order, int kind, int64_t seed, int64_t start, int64_t nsym, int nb, const void *alphabet, int M, void *symbols,
                            int32_t *labels, uint8_t *bits)
{ return qh::prbs_symbols_dev<float>(order, kind, seed, start, nsym, nb, alphabet, M, symbols, labels, bits); }
int qh_prbs_symbols_c128_dev(int order, int kind, int64_t seed, int64_t start, int64_t nsym, int nb, const void *alphabet, int M, void *symbols,
                             int32_t *labels, uint8_t *bits)
{ return qh::prbs_symbols_dev<double>(order, kind, seed, start, nsym, nb, alphabet, M, symbols, labels, bits); }
}
