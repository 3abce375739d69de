// A stable least-significant-digit radix sort of (uint64 key, int32 value) pairs (DESIGN.md "Point-cloud export": the device sort).
// The output is defined to the bit (include/thermonerf_hip.h): the pairs in ascending order of the key's low 8 * ceil(key_bits / 8)
// bits, pairs that are equal there in their input order.  One pass per 8-bit digit, lowest digit first; a pass is three plain launches:
//   1. histogram  one block per tile of kTileKeys keys counts its 256 digits (integer LDS atomics: a count is exact in any order)
//                 and writes them DIGIT-MAJOR, counts[digit * tiles + tile]
//   2. scan       scan_tiles<false> of tn_scan.h, one block, over all 256 * tiles entries: an entry becomes the number of keys with a
//                 lower digit anywhere plus the keys with its digit in earlier tiles — the global base of (digit, tile)
//   3. scatter    the block recomputes its digits and ranks its keys among the tile's equal digits, in input order; destination =
//                 base of (digit, tile) + that rank
// A stable pass per digit, lowest first, is a sort that is stable as a whole.  The passes ping-pong between the caller's output
// buffers and a partner pair in the workspace, started so that the LAST pass writes the outputs; the first pass reads the inputs
// (and makes up the values 0 .. n-1 when values_in is NULL), so the inputs are never written.
// No allocation, no host synchronisation, and NO block ever waits for another block: no decoupled look-back, no grid barrier, no
// cooperative launch; what one pass knows about the others' keys it learns from the kernel boundary.
//
// THE IN-TILE RANK.  A tile is kItems rounds of kBlock consecutive keys; in round r thread t holds key tile_first + r * kBlock + t, so
// the input order inside a tile is (round, wave, lane).  Per round:
//   * peers = the lanes of my wave that hold my digit: eight 64-bit __ballot masks, one per digit bit, each ANDed in as it is or
//     complemented, on top of the ballot of the lanes that hold a key at all.  My rank in the wave = the peers below my lane; the
//     lowest peer writes the group's size to wave_count[wave][digit].
//   * barrier; my rank in the round = the wave_count[w][digit] of the waves before mine + my rank in the wave; the destination adds
//     digit_base[digit], which starts at the global base of (digit, tile) and has advanced by the earlier rounds' counts.
//   * barrier; thread d (kBlock = 256 = the digits) adds the round's wave counts of digit d to digit_base[d] and zeroes them; barrier.
// Every thread of the block reaches every barrier and every ballot, the lanes beyond n in the last tile included (they hold no key,
// write nothing and are in nobody's peers).  The keys of a tile sit in kItems registers named at compile time (the round loop is
// unrolled); the rank never indexes a register array with a run-time value, so nothing lands in scratch.
#include "tn_device.h"
#include "tn_scan.h"

using namespace tn;

namespace {

constexpr int kBlock = 256;                  // threads per block of the histogram and scatter kernels = the digits of a pass
constexpr int kItems = 8;                    // keys per thread
constexpr int kTileKeys = kBlock * kItems;   // keys per tile (tn_sort_tile()); a (digit, tile) count is at most this, far below 2^22
constexpr int kWaves = kBlock / TN_WAVE;
constexpr int kDigits = 256;

static_assert(kBlock == kDigits, "thread d of a block owns digit d");

__device__ __forceinline__ uint32_t digit_of(unsigned long long key, int shift) { return (uint32_t)(key >> shift) & 255u; }

__global__ void __launch_bounds__(kBlock)
histogram_kernel(const unsigned long long *__restrict__ keys, long long n, int shift, long long tiles, long long *__restrict__ counts) {
    __shared__ uint32_t hist[kDigits];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const long long first = (long long)blockIdx.x * kTileKeys + threadIdx.x;
#pragma unroll
    for (int r = 0; r < kItems; ++r) {
        const long long i = first + (long long)r * kBlock;
        if (i < n) atomicAdd(&hist[digit_of(keys[i], shift)], 1u);
    }
    __syncthreads();
    counts[(long long)threadIdx.x * tiles + blockIdx.x] = (long long)hist[threadIdx.x];
}

__global__ void __launch_bounds__(kScan)
scan_kernel(long long *__restrict__ counts, long long entries, long long *__restrict__ total) {
    scan_tiles<false>(counts, entries, total);  // a pass sums at most kScan * kTileKeys = 2^21
}

// IOTA: the values are the keys' input positions (the first pass with values_in == NULL)
template <bool IOTA>
__global__ void __launch_bounds__(kBlock)
scatter_kernel(const unsigned long long *__restrict__ keys_in, const int *__restrict__ values_in, long long n, int shift,
               long long tiles, const long long *__restrict__ bases, unsigned long long *__restrict__ keys_out,
               int *__restrict__ values_out) {
    __shared__ uint32_t wave_count[kWaves][kDigits];
    __shared__ uint32_t digit_base[kDigits];  // destinations are below n <= 2^31 - 1
    const int wave = threadIdx.x / TN_WAVE, lane = threadIdx.x % TN_WAVE;
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    const long long first = (long long)blockIdx.x * kTileKeys + threadIdx.x;
    digit_base[threadIdx.x] = (uint32_t)bases[(long long)threadIdx.x * tiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < kWaves; ++w) wave_count[w][threadIdx.x] = 0;
    unsigned long long key[kItems];
#pragma unroll
    for (int r = 0; r < kItems; ++r) {
        const long long i = first + (long long)r * kBlock;
        key[r] = i < n ? keys_in[i] : 0ull;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kItems; ++r) {
        const long long i = first + (long long)r * kBlock;
        const bool valid = i < n;
        const uint32_t digit = digit_of(key[r], shift);
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long with_bit = __ballot(bit);
            peers &= bit ? with_bit : ~with_bit;
        }
        const uint32_t in_wave = (uint32_t)__popcll(peers & lanes_below);
        if (valid && in_wave == 0) wave_count[wave][digit] = (uint32_t)__popcll(peers);
        __syncthreads();
        uint32_t before = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const uint32_t c = wave_count[w][digit];
            before += w < wave ? c : 0u;
        }
        const long long dst = (long long)(digit_base[digit] + before + in_wave);
        if (valid && dst < n) {  // (dst < n always holds for bases that are this pass's scan; it keeps a store inside the buffers whatever they are)
            keys_out[dst] = key[r];
            values_out[dst] = IOTA ? (int)i : values_in[i];
        }
        __syncthreads();
        uint32_t round_total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            round_total += wave_count[w][threadIdx.x];
            wave_count[w][threadIdx.x] = 0;
        }
        digit_base[threadIdx.x] += round_total;
        __syncthreads();
    }
}

inline bool bad_count(int64_t n) { return n < 0 || n > 0x7fffffffLL; }

inline long long tiles_of(long long n) { return ceil_div(n, kTileKeys); }

inline size_t keys_bytes(long long n) { return (size_t)n * sizeof(unsigned long long); }

inline size_t values_bytes(long long n) { return ((size_t)n * sizeof(int) + 7) / 8 * 8; }

}  // namespace

extern "C" {

int32_t tn_sort_tile(void) { return kTileKeys; }

// the partner keys, the partner values, 256 counts per tile, the scan's total
size_t tn_sort_pairs_workspace_bytes(int64_t n) {
    if (bad_count(n)) return 0;
    return keys_bytes(n) + values_bytes(n) + ((size_t)tiles_of(n) * kDigits + 1) * sizeof(long long);
}

int tn_sort_pairs(const uint64_t *keys_in, const int32_t *values_in, int64_t n, int key_bits, uint64_t *keys_out,
                  int32_t *values_out, void *workspace, size_t workspace_bytes, void *stream) {
    if (key_bits < 1 || key_bits > 64) return TN_ERR_UNSUPPORTED;
    if (bad_count(n)) return TN_ERR_SHAPE;
    if (n == 0) return TN_OK;
    if (!keys_in || !keys_out || !values_out || !workspace) return TN_ERR_NULL;
    if (misaligned(keys_in, 8) || misaligned(values_in, 4) || misaligned(keys_out, 8) || misaligned(values_out, 4) ||
        misaligned(workspace, 8))
        return TN_ERR_SHAPE;
    if (workspace_bytes < tn_sort_pairs_workspace_bytes(n)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long long count = (long long)n, tiles = tiles_of(count), entries = tiles * kDigits;
    char *ws = reinterpret_cast<char *>(workspace);
    unsigned long long *keys_partner = reinterpret_cast<unsigned long long *>(ws);
    int *values_partner = reinterpret_cast<int *>(ws + keys_bytes(count));
    long long *counts = reinterpret_cast<long long *>(ws + keys_bytes(count) + values_bytes(count));
    long long *total = counts + entries;
    unsigned long long *keys_user = reinterpret_cast<unsigned long long *>(keys_out);
    const int passes = (key_bits + 7) / 8;
    const unsigned long long *src_keys = reinterpret_cast<const unsigned long long *>(keys_in);
    const int *src_values = values_in;
    for (int p = 0; p < passes; ++p) {
        const bool to_user = (passes - 1 - p) % 2 == 0;  // the last pass writes the caller's buffers
        unsigned long long *dst_keys = to_user ? keys_user : keys_partner;
        int *dst_values = to_user ? values_out : values_partner;
        const int shift = 8 * p;
        hipLaunchKernelGGL(histogram_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, s, src_keys, count, shift, tiles, counts);
        TN_LAUNCH_CHECK();
        hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kScan), 0, s, counts, entries, total);
        TN_LAUNCH_CHECK();
        if (src_values)
            hipLaunchKernelGGL(scatter_kernel<false>, dim3((unsigned)tiles), dim3(kBlock), 0, s, src_keys, src_values, count, shift,
                               tiles, counts, dst_keys, dst_values);
        else
            hipLaunchKernelGGL(scatter_kernel<true>, dim3((unsigned)tiles), dim3(kBlock), 0, s, src_keys, src_values, count, shift,
                               tiles, counts, dst_keys, dst_values);
        TN_LAUNCH_CHECK();
        src_keys = dst_keys;
        src_values = dst_values;
    }
    return TN_OK;
}

}  // extern "C"
