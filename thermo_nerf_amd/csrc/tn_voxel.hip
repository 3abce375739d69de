// Voxel down-sampling of a thermal point cloud: one averaged point per occupied voxel (DESIGN.md "Point-cloud export": voxel
// down-sampling; include/thermonerf_hip.h defines every output to the bit).  A voxel's members are averaged in ASCENDING POINT INDEX,
// which is the order the stable sort of (voxel key, point index) leaves them in — so the fp64 sums, and with them every output, are
// the same on every run.  Launches on the caller's stream:
//   1. keys    one thread per point: the voxel key, or `total` (behind every voxel) for a point that is dropped
//   2. sort    tn_sort_pairs (tn_sort.hip) of (key, 0 .. n-1) over bit_length(total) key bits: three launches per 8 bits
//   3. heads   j is a head iff key[j] < total and (j == 0 or key[j] != key[j-1]); the heads are compacted in order by the count /
//              one-block scan / emit of tn_scan.h: heads[v] = the position of voxel v's first member in the sorted list
//   4. average one thread per voxel (below the capacity) walks its run of the sorted index list and writes its point
// No atomics at all, no allocation, no host synchronisation, and no block ever waits for another.  The walk of step 4 is sequential
// per voxel because the sums are ordered by definition: a voxel of 10^5 members is 10^5 steps of one thread (a sensible voxel holds
// tens to hundreds).
#include "tn_device.h"
#include "tn_scan.h"
#include "tn_voxel_grid.h"

using namespace tn;

namespace {

constexpr int kTile = 256;  // points / sorted positions / voxels per block of every kernel but the scan

__global__ void __launch_bounds__(kTile)
keys_kernel(const float *__restrict__ positions, long long n, VoxelGrid g, unsigned long long *__restrict__ keys) {
    const long long i = (long long)blockIdx.x * kTile + threadIdx.x;
    if (i >= n) return;
    keys[i] = voxel_key(positions, i, g);
}

__global__ void __launch_bounds__(kTile)
count_heads_kernel(const unsigned long long *__restrict__ keys, long long n, unsigned long long total, long long *__restrict__ tiles) {
    const long long j = (long long)blockIdx.x * kTile + threadIdx.x;
    uint32_t heads;
    block_rank<kTile>(voxel_head(keys, j, n, total), heads);
    if (threadIdx.x == 0) tiles[blockIdx.x] = (long long)heads;
}

__global__ void __launch_bounds__(kScan)
scan_kernel(long long *__restrict__ tiles, long long num_tiles, long long *__restrict__ count) {
    scan_tiles<false>(tiles, num_tiles, count);  // a pass sums at most kScan * kTile = 2^18
}

__global__ void __launch_bounds__(kTile)
emit_heads_kernel(const unsigned long long *__restrict__ keys, long long n, unsigned long long total, const long long *__restrict__ tiles,
                  int *__restrict__ heads) {
    const long long j = (long long)blockIdx.x * kTile + threadIdx.x;
    const bool head = voxel_head(keys, j, n, total);
    uint32_t unused;
    const uint32_t rank = block_rank<kTile>(head, unused);
    if (!head) return;
    const long long v = tiles[blockIdx.x] + (long long)rank;  // <= j < n: inside heads[n]
    if (v < n) heads[v] = (int)j;
}

__global__ void __launch_bounds__(kTile)
average_kernel(const unsigned long long *__restrict__ keys, const int *__restrict__ order, long long n, const int *__restrict__ heads,
               const long long *__restrict__ count, long long capacity, VoxelInputs in, VoxelOutputs out,
               const long long *__restrict__ source, long long *__restrict__ source_out) {  // both may be NULL
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    if (v >= capacity || v >= count[0]) return;
    const long long start = heads[v];
    voxel_average(keys, order, n, start, in, out, v);
    if (source_out) source_out[v] = source[order[start]];
}

inline bool bad_count(int64_t n) { return n < 0 || n > 0x7fffffffLL; }

inline long long tiles_of(long long n) { return ceil_div(n, kTile); }

inline size_t keys_bytes(long long n) { return (size_t)n * sizeof(unsigned long long); }

}  // namespace

extern "C" {

// the keys, the sorted keys, the sorted point indices, the heads, the tile counts of the heads, the sort's own workspace
size_t tn_voxel_downsample_workspace_bytes(int64_t num_points) {
    if (bad_count(num_points)) return 0;
    return 2 * keys_bytes(num_points) + 2 * ints_bytes(num_points) + (size_t)tiles_of(num_points) * sizeof(long long) +
           tn_sort_pairs_workspace_bytes(num_points);
}

int tn_voxel_downsample(const float *positions, const uint8_t *colors, const float *temperature, const uint8_t *thermal_colors,
                        const int64_t *source, int64_t num_points, const tn_voxel_params *params, float *positions_out,
                        uint8_t *colors_out, float *temperature_out, uint8_t *thermal_colors_out, int64_t *source_out,
                        int32_t *voxel_count, int64_t capacity, int64_t *count, void *workspace, size_t workspace_bytes, void *stream) {
    if (!params || !count) return TN_ERR_NULL;
    if (bad_count(num_points) || capacity < 0) return TN_ERR_SHAPE;
    if (voxel_params_unsupported(params)) return TN_ERR_UNSUPPORTED;
    if (num_points > 0 && (!positions || !colors || !temperature || !workspace)) return TN_ERR_NULL;
    if (capacity > 0 && (!positions_out || !colors_out || !temperature_out || !voxel_count)) return TN_ERR_NULL;
    if (num_points > 0 && ((thermal_colors_out && !thermal_colors) || (source_out && !source))) return TN_ERR_NULL;
    if (misaligned(positions, 4) || misaligned(temperature, 4) || misaligned(source, 8) || misaligned(positions_out, 4) ||
        misaligned(temperature_out, 4) || misaligned(source_out, 8) || misaligned(voxel_count, 4) || misaligned(count, 8) ||
        misaligned(workspace, 8))
        return TN_ERR_SHAPE;
    if (workspace_bytes < tn_voxel_downsample_workspace_bytes(num_points)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (num_points == 0) return hipMemsetAsync(count, 0, sizeof(int64_t), s) == hipSuccess ? TN_OK : TN_ERR_LAUNCH;
    const long long n = (long long)num_points;
    const VoxelGrid g = voxel_grid_of(params);
    char *ws = reinterpret_cast<char *>(workspace);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws);
    unsigned long long *sorted_keys = reinterpret_cast<unsigned long long *>(ws + keys_bytes(n));
    int *order = reinterpret_cast<int *>(ws + 2 * keys_bytes(n));
    int *heads = reinterpret_cast<int *>(ws + 2 * keys_bytes(n) + ints_bytes(n));
    long long *tiles = reinterpret_cast<long long *>(ws + 2 * keys_bytes(n) + 2 * ints_bytes(n));
    void *sort_ws = tiles + tiles_of(n);
    const unsigned blocks = (unsigned)tiles_of(n);
    hipLaunchKernelGGL(keys_kernel, dim3(blocks), dim3(kTile), 0, s, positions, n, g, keys);
    TN_LAUNCH_CHECK();
    const int code = tn_sort_pairs(reinterpret_cast<const uint64_t *>(keys), nullptr, num_points, bit_length(g.total),
                                   reinterpret_cast<uint64_t *>(sorted_keys), order, sort_ws, tn_sort_pairs_workspace_bytes(num_points),
                                   stream);
    if (code != TN_OK) return code;
    long long *cnt = reinterpret_cast<long long *>(count);
    hipLaunchKernelGGL(count_heads_kernel, dim3(blocks), dim3(kTile), 0, s, sorted_keys, n, g.total, tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kScan), 0, s, tiles, tiles_of(n), cnt);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(emit_heads_kernel, dim3(blocks), dim3(kTile), 0, s, sorted_keys, n, g.total, tiles, heads);
    TN_LAUNCH_CHECK();
    const long long walkers = capacity < n ? (long long)capacity : n;  // there are at most n voxels
    if (walkers > 0) {
        const VoxelInputs in = {positions, temperature, colors, thermal_colors};
        const VoxelOutputs out = {positions_out, temperature_out, colors_out, thermal_colors_out, voxel_count};
        hipLaunchKernelGGL(average_kernel, dim3((unsigned)tiles_of(walkers)), dim3(kTile), 0, s, sorted_keys, order, n, heads, cnt,
                           (long long)capacity, in, out, reinterpret_cast<const long long *>(source),
                           reinterpret_cast<long long *>(source_out));
        TN_LAUNCH_CHECK();
    }
    return TN_OK;
}

}  // extern "C"
