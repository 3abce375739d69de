// Block-wide counting, the one place for it: the two primitives every ordered compaction is built from (tn_pointcloud.hip,
// tn_mesh.hip, tn_knn.hip: count per tile, scan the tile counts, emit), and the one-block scan of the tile counts itself.
//
//   block_rank<THREADS>(keep, total)       this thread's rank among the block's threads with `keep`, lower threads first
//   block_exclusive<THREADS>(own, total)   the sum of `own` over the block's lower threads
// Both also give every thread the block's `total`; what becomes of it is the caller's business (thread 0 of a count kernel
// writes it to tiles[blockIdx.x]).  The results are integer sums: exact in any order.  THREADS = the block's thread count, a
// multiple of the wave.  The contract, which the call sites depend on:
//   * EVERY thread of the block calls the primitive — it contains the one __syncthreads().  A thread with nothing to add
//     passes false / 0; early returns (i >= n, !keep, own == 0) come AFTER the call.
//   * The LDS array inside is one per instantiation: a second call of the same instantiation in one kernel needs a barrier
//     between the first call's reads and the second call's writes (scan_tiles' loop ends with it).
//   * That one barrier also orders whatever the block wrote to LDS before the call (the emit kernels' colour table).
#pragma once
#include "tn_device.h"

namespace tn {

namespace detail {
// after the waves' totals are in LDS: the barrier, the sum of the waves before mine, the sum of all
template <int THREADS>
__device__ __forceinline__ uint32_t waves_before(const uint32_t *wave_total, uint32_t &total) {
    const int wave = threadIdx.x / TN_WAVE;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < THREADS / TN_WAVE; ++w) {
        const uint32_t v = wave_total[w];
        before += w < wave ? v : 0u;
        total += v;
    }
    return before;
}
}  // namespace detail

template <int THREADS>
__device__ __forceinline__ uint32_t block_rank(bool keep, uint32_t &total) {
    __shared__ uint32_t wave_total[THREADS / TN_WAVE];
    const unsigned long long mask = __ballot(keep);
    if (threadIdx.x % TN_WAVE == 0) wave_total[threadIdx.x / TN_WAVE] = (uint32_t)__popcll(mask);
    const uint32_t in_wave = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    return detail::waves_before<THREADS>(wave_total, total) + in_wave;
}

template <int THREADS>
__device__ __forceinline__ uint32_t block_exclusive(uint32_t own, uint32_t &total) {
    __shared__ uint32_t wave_total[THREADS / TN_WAVE];
    const int lane = threadIdx.x % TN_WAVE;
    uint32_t incl = own;  // the in-wave inclusive prefix
#pragma unroll
    for (int o = 1; o < TN_WAVE; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, TN_WAVE);
        if (lane >= o) incl += up;
    }
    if (lane == TN_WAVE - 1) wave_total[threadIdx.x / TN_WAVE] = incl;
    return detail::waves_before<THREADS>(wave_total, total) + (incl - own);
}

constexpr int kScan = 1024;   // tile counts the scan block takes per pass = its threads

// ONE block of kScan threads: tiles[b] <- base + (exclusive prefix of the tile counts), kScan tile counts per pass with a running
// carry; count[0] <- base + the sum of all counts.  base = count[0] as the block finds it (APPEND: a counter that several calls
// advance) or 0 (the counter is overwritten).  One block: nothing ever waits for another block.  A pass sums at most kScan tile
// counts in 32 bits: the callers' per-tile counts stay below 2^22.
template <bool APPEND>
__device__ __forceinline__ void scan_tiles(long long *__restrict__ tiles, long long num_tiles, long long *__restrict__ count) {
    __shared__ long long count_in;
    if (threadIdx.x == 0) count_in = APPEND ? count[0] : 0;  // (the one thread that writes it back reads it)
    __syncthreads();
    long long carry = count_in;
    for (long long first = 0; first < num_tiles; first += kScan) {
        const long long b = first + threadIdx.x;
        uint32_t total;
        const uint32_t before = block_exclusive<kScan>(b < num_tiles ? (uint32_t)tiles[b] : 0u, total);
        if (b < num_tiles) tiles[b] = carry + (long long)before;
        carry += (long long)total;
        __syncthreads();  // block_exclusive's LDS is rewritten by the next pass
    }
    if (threadIdx.x == 0) count[0] = carry;
}

}  // namespace tn
