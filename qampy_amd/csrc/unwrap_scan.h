// The device form of np.unwrap's bookkeeping, shared by the blind phase search (bps.hip), the feed-forward estimators (cpr.hip) and the
// pilot-aided estimates (pilot.hip).
// np.unwrap's running correction is an integer prefix sum K of wrap counts c_k = -1 where theta_k - theta_(k-1) > pi, +1 where it is < -pi,
// else 0 - exact - taken in three launches: every chunk of UW_CHUNK elements of a row sums its counts, ONE workgroup per row turns the chunk
// sums into chunk offsets (unwrap_scan_kernel), and every chunk adds its offset to its own prefix.  No workgroup waits on another.
// Here: the count, the two ways a workgroup of UW_THREADS threads walks its chunk's counts (strided for the sum, in owned runs for the
// prefix), the sum and the prefix over the workgroup, the middle launch and the scratch the three launches share.  (bps.hip uses the middle
// launch only: its in-chunk scan is another.)
#pragma once
#include "common.h"

namespace qh {

constexpr int UW_THREADS = 256;
constexpr int UW_PER_THREAD = 4;
constexpr int UW_CHUNK = UW_THREADS * UW_PER_THREAD;

// np.unwrap's correction for the step prev -> cur of a sequence of angles, in units of 2 pi (+-pi itself: 0, as numpy)
__device__ __forceinline__ int wrap_count(double prev, double cur)
{
    const double d = cur - prev;
    return d > QH_PI ? -1 : (d < -QH_PI ? 1 : 0);
}

// sum of an int over the workgroup, to thread 0
__device__ __forceinline__ int block_sum_int(int s, int *red)
{
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    int t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < UW_THREADS / 64; w++) t += red[w];
    return t;
}

// First launch, the chunk of the elements base .. base + UW_CHUNK - 1 of a row of n: this thread's sum of the wrap counts of its UW_PER_THREAD
// strided elements (block_sum_int makes it the chunk's sum).  th is the chunk's UW_CHUNK + 1 angles in LDS, th[0] the element in front of
// the chunk; the count of the chunk's first element, decided from it, goes to *first_jump so that the last launch repeats exactly this decision.
__device__ __forceinline__ int strided_wrap_counts(const double *th, int64_t base, int64_t n, int *first_jump)
{
    int s = 0;
#pragma unroll
    for (int r = 0; r < UW_PER_THREAD; r++) {
        const int el = r * UW_THREADS + threadIdx.x;
        const int64_t k = base + el;
        int j = 0;
        if (k >= 1 && k < n) j = wrap_count(th[el], th[el + 1]);
        if (el == 0) *first_jump = j;
        s += j;
    }
    return s;
}

// Last launch: thread t owns the UW_PER_THREAD consecutive elements from t * UW_PER_THREAD on; jmp[r] receives the inclusive sum of their
// wrap counts inside the thread.  th is the chunk's UW_CHUNK angles in LDS; the chunk's first element takes its count from *first_jump.
__device__ __forceinline__ void owned_wrap_counts(const double *th, int64_t base, int64_t n, const int *first_jump, int (&jmp)[UW_PER_THREAD])
{
    int local = 0;
#pragma unroll
    for (int r = 0; r < UW_PER_THREAD; r++) {
        const int el = threadIdx.x * UW_PER_THREAD + r;
        const int64_t k = base + el;
        int j = 0;
        if (k >= 1 && k < n) j = el == 0 ? *first_jump : wrap_count(th[el - 1], th[el]);
        local += j;
        jmp[r] = local;
    }
}

// Inclusive prefix of the wrap counts over one chunk, plus the chunk's offset: jmp as owned_wrap_counts leaves it; corr[e] receives K of
// element e of the chunk.  wsum: UW_THREADS / 64 entries of LDS.  Ends in a barrier.
__device__ __forceinline__ void chunk_prefix(const int (&jmp)[UW_PER_THREAD], int chunk_off, int *corr, int *wsum)
{
    const int local = jmp[UW_PER_THREAD - 1];
    int incl = local;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if ((int)(threadIdx.x & 63) >= o) incl += t;
    }
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    int off = chunk_off + incl - local;
    for (int w = 0; w < (int)(threadIdx.x >> 6); w++) off += wsum[w];
#pragma unroll
    for (int r = 0; r < UW_PER_THREAD; r++) corr[threadIdx.x * UW_PER_THREAD + r] = off + jmp[r];
    __syncthreads();
}

// (The kernel is `static`: three translation units include this header.)
static __global__ void __launch_bounds__(1024) unwrap_scan_kernel(int *chunk_sum, int64_t nchunk)
{
    // exclusive scan of the chunk sums of one mode by one workgroup: a run of consecutive chunks per thread (loaded together), wave
    // scans of the run totals, the 16 wave totals through LDS.  (A single wave walking the array 64 entries at a time was a chain of
    // 64 dependent global round trips: 32 us for 4096 chunks.)
    __shared__ int wtot[16];
    int *cs = chunk_sum + (int64_t)blockIdx.x * nchunk;
    const int64_t len = (nchunk + 1023) / 1024;
    const int64_t i0 = (int64_t)threadIdx.x * len, i1 = i0 + len < nchunk ? i0 + len : nchunk;
    int tot = 0;
    for (int64_t i = i0; i < i1; i++) tot += cs[i];
    int incl = tot;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if ((int)(threadIdx.x & 63) >= o) incl += t;
    }
    if ((threadIdx.x & 63) == 63) wtot[threadIdx.x >> 6] = incl;
    __syncthreads();
    int run = incl - tot;
    for (int w = 0; w < (int)(threadIdx.x >> 6); w++) run += wtot[w];
    for (int64_t i = i0; i < i1; i++) { const int v = cs[i]; cs[i] = run; run += v; }
}

// Scratch of the three launches in a caller's slot, behind `head` bytes the caller keeps for itself (at base): chunk sums | wrap count of
// every chunk's first element
struct UnwrapScratch { char *base; int *csum, *first; };
inline int unwrap_scratch(Slot slot, int nmodes, int64_t nchunk, size_t head, UnwrapScratch *s)
{
    ScratchLayout lay;
    lay.take(head);
    const size_t o_sum = lay.take((size_t)nmodes * nchunk * sizeof(int)), o_first = lay.take((size_t)nmodes * nchunk * sizeof(int));
    void *sb = nullptr;
    int rc = scratch(slot, lay.total, &sb);
    if (rc) return rc;
    s->base = (char *)sb;
    s->csum = (int *)(s->base + o_sum);
    s->first = (int *)(s->base + o_first);
    return QH_OK;
}

}  // namespace qh
