// The one-block exclusive scan of per-tile counts that the ordered compactions share (tn_pointcloud.hip, tn_mesh.hip): count per
// tile, THIS scan, emit.  tiles[b] <- base + (exclusive prefix of the tile counts), kScan tile counts per pass with a running
// carry; count[0] <- base + the sum of all counts.  base = count[0] as the block finds it (APPEND: a counter that several calls
// advance) or 0 (the counter is overwritten).  One block: nothing ever waits for another block.
#pragma once
#include "tn_device.h"

namespace tn {

constexpr int kScan = 1024;   // tile counts the scan block takes per pass = its threads
constexpr int kScanWaves = kScan / TN_WAVE;

// a pass sums at most kScan tile counts in 32 bits: the callers' per-tile counts stay below 2^22
template <bool APPEND>
__device__ __forceinline__ void scan_tiles(long long *__restrict__ tiles, long long num_tiles, long long *__restrict__ count) {
    __shared__ uint32_t wave_total[kScanWaves];
    __shared__ long long count_in;
    const int lane = threadIdx.x % TN_WAVE, wave = threadIdx.x / TN_WAVE;
    if (threadIdx.x == 0) count_in = APPEND ? count[0] : 0;  // (the one thread that writes it back reads it)
    __syncthreads();
    long long carry = count_in;
    for (long long first = 0; first < num_tiles; first += kScan) {
        const long long b = first + threadIdx.x;
        const uint32_t own = b < num_tiles ? (uint32_t)tiles[b] : 0u;
        uint32_t incl = own;
#pragma unroll
        for (int o = 1; o < TN_WAVE; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o, TN_WAVE);
            if (lane >= o) incl += up;
        }
        if (lane == TN_WAVE - 1) wave_total[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kScanWaves; ++w) {
            const uint32_t v = wave_total[w];
            before += w < wave ? v : 0u;
            total += v;
        }
        if (b < num_tiles) tiles[b] = carry + (long long)(before + incl - own);
        carry += (long long)total;
        __syncthreads();  // wave_total is rewritten by the next pass
    }
    if (threadIdx.x == 0) count[0] = carry;
}

}  // namespace tn
