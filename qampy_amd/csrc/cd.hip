// Static all-pass filtering of every row of an (nmodes, L) array: chromatic-dispersion compensation and emulation
// (qampy/core/equalisation/equalisation.py:596-669 CDcomp, qampy/core/impairments.py:673-703 add_dispersion).
//
//   H(w) = exp(j (c2 w^2 + c1 w + c0)) / N,   w = 2 pi k / N on numpy's fftfreq grid of the block size N (rad / sample, [-pi, pi))
//
// One workgroup transforms one block of one row (block_filter.h): load (with its halo) -> forward FFT -> * H -> inverse FFT -> store.  The FFT is a
// Stockham autosort in LDS: every pass reads its butterflies' inputs from LDS into registers, runs radix-8/4 butterflies there
// and writes the results back in place (a barrier between the reads and the writes, so one N-point buffer suffices).  The
// inverse transform is conj(FFT(conj(.))), with the conjugations folded into the multiply by H and the store.
//
// Sizes: N = 256 .. 8192, a power of two, for both precisions.  One buffer of N complex values: 64 KiB (complex64) or 128 KiB
// (complex128) at N = 8192; complex128 at 16384 would need 256 KiB against 160 KiB of LDS per CU.
//
// Twiddles W_N^m and H (1/N of the inverse folded in) come from tables formed on the host in double precision - the phase of
// H reduced modulo 2 pi in double before its sine and cosine - cast to the signal's precision and uploaded once per
// (N, c2, c1, c0, dtype) into scratch slot Slot::CD_TABLE.
//
// Boundary modes:
//   circular (0)  overlap-save.  Block j keeps output samples [j n, (j + 1) n), n = N / 2, of a transform over input positions
//                 j n - N/4 .. j n + n + N/4 - 1, taken modulo L (any L >= 1; the last block may be partial).  N == L: one
//                 transform per row, no overlap.
//   linear (1)    the reference's zero-padded overlap-add: block j holds input [j n, (j + 1) n) at offset N/4 of N zeros, its N
//                 outputs land at j n - N/4 ..; output length n (L // n).  Every output sample is the sum of two blocks' outputs.
//                 Even blocks are written first (their outputs tile the row without overlap), then the odd blocks add theirs
//                 in a second launch on the same stream: no atomics and no scratch; the sum of two terms is exact in either
//                 order, so the result is that of the reference's accumulation.
#include "block_filter.h"

namespace qh {

constexpr int CD_NMIN = 256, CD_NMAX = 8192;

// ------------------------------------------------------------------------------------------------ host side
static thread_local TableCache g_cd;

template <typename R> static int cd_table(int N, double c2, double c1, double c0, const Cx<R> **tab)
{
    std::string key;
    key_add(key, c2); key_add(key, c1); key_add(key, c0);
    return filter_table<R>(g_cd, Slot::CD_TABLE, N, key, [=](int k) {
        const double w = QH_TWO_PI * (double)k / (double)N;
        return c2 * w * w + c1 * w + c0;
    }, tab);
}

static bool cd_size_ok(int N) { return N >= CD_NMIN && N <= CD_NMAX && (N & (N - 1)) == 0; }

template <typename R>
int cd_filter_dev(const void *E, int nmodes, int64_t L, int N, double c2, double c1, double c0, int mode, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(cd_size_ok(N), "cd_filter: N must be a power of two from 256 to 8192");
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 0, "cd_filter: bad sizes");
    QH_REQUIRE(mode == 0 || mode == 1, "cd_filter: mode is 0 (circular) or 1 (linear)");
    QH_REQUIRE(std::isfinite(c2) && std::isfinite(c1) && std::isfinite(c0), "cd_filter: coefficients must be finite");
    QH_REQUIRE(E && out && E != out, "cd_filter: out must be a buffer other than E");
    const int64_t Lout = mode == 0 ? L : (L / (N / 2)) * (N / 2);
    if (Lout == 0) return QH_OK;
    QH_REQUIRE(mode == 1 || (L + N / 2 - 1) / (N / 2) <= 0x7fffffffLL, "cd_filter: L too long");
    const Cx<R> *tab;
    if ((rc = cd_table<R>(N, c2, c1, c0, &tab))) return rc;
    return block_filter<R>(N, (const Cx<R> *)E, (Cx<R> *)out, nmodes, L, Lout, tab, PlainRow<R>{}, mode);
}

template <typename R>
int cd_filter_host(const void *E, int nmodes, int64_t L, int N, double c2, double c1, double c0, int mode, void *out)
{
    int rc = ensure_init();
    if (rc) return rc;
    QH_REQUIRE(cd_size_ok(N), "cd_filter: N must be a power of two from 256 to 8192");
    QH_REQUIRE(nmodes >= 1 && nmodes <= 65535 && L >= 0, "cd_filter: bad sizes");
    QH_REQUIRE(mode == 0 || mode == 1, "cd_filter: mode is 0 (circular) or 1 (linear)");
    const int64_t Lout = mode == 0 ? L : (L / (N / 2)) * (N / 2);
    if (Lout == 0) return QH_OK;
    DevBuf dE, dout;
    if ((rc = dE.from_host(E, (size_t)nmodes * L * sizeof(Cx<R>)))) return rc;
    if ((rc = dout.alloc((size_t)nmodes * Lout * sizeof(Cx<R>)))) return rc;
    if ((rc = cd_filter_dev<R>(dE.p, nmodes, L, N, c2, c1, c0, mode, dout.p))) return rc;
    if ((rc = dout.to_host(out, dout.n))) return rc;
    QH_HIP(hipStreamSynchronize(g_stream));
    return QH_OK;
}

}  // namespace qh

extern "C" {
int qh_cd_filter_c64(const void *E, int nmodes, int64_t L, int N, double c2, double c1, double c0, int mode, void *out)
{ return qh::cd_filter_host<float>(E, nmodes, L, N, c2, c1, c0, mode, out); }
int qh_cd_filter_c128(const void *E, int nmodes, int64_t L, int N, double c2, double c1, double c0, int mode, void *out)
{ return qh::cd_filter_host<double>(E, nmodes, L, N, c2, c1, c0, mode, out); }
int qh_cd_filter_c64_dev(const void *E, int nmodes, int64_t L, int N, double c2, double c1, double c0, int mode, void *out)
{ return qh::cd_filter_dev<float>(E, nmodes, L, N, c2, c1, c0, mode, out); }
int qh_cd_filter_c128_dev(const void *E, int nmodes, int64_t L, int N, double c2, double c1, double c0, int mode, void *out)
{ return qh::cd_filter_dev<double>(E, nmodes, L, N, c2, c1, c0, mode, out); }
}
