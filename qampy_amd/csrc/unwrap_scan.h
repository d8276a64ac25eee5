// The middle phase of the device form of np.unwrap, shared by the blind phase search (bps.hip) and the feed-forward estimators (cpr.hip).
// np.unwrap's running correction is an integer prefix sum of wrap counts - exact - taken in three launches: every chunk of UW_CHUNK
// elements of a row sums its counts, ONE workgroup per row turns the chunk sums into chunk offsets (the kernel below), and every chunk
// adds its offset to its own prefix.  No workgroup waits on another.
// (The kernel is `static`: two translation units include this header.)
#pragma once
#include "common.h"

namespace qh {

constexpr int UW_THREADS = 256;
constexpr int UW_PER_THREAD = 4;
constexpr int UW_CHUNK = UW_THREADS * UW_PER_THREAD;

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

}  // namespace qh
