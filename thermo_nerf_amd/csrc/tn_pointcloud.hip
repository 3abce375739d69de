// Point-cloud export: the rendered outputs of one pose -> the surviving points, appended IN RAY ORDER behind a device-resident
// counter (DESIGN.md "Point-cloud export").  Nerfstudio's exporter back-projects the rendered depth, drops transparent and
// out-of-box rays and keeps positions and colours; here a point also carries its temperature in degrees.  Every step is ONE
// correctly rounded fp32 operation (explicit *_rn intrinsics), so a cloud is defined bit for bit (include/thermonerf_hip.h).
//
// Three plain launches per call, no host synchronisation, no allocation:
//   1. count   one block per tile of kTile rays: the predicate, the block's number of kept rays (block_rank, tn_scan.h) -> tile[b]
//   2. scan    ONE block: count_in = count[0]; tile[b] <- count_in + (exclusive prefix of the tile counts), kScan tiles per
//              pass with a running carry; count[0] <- count_in + kept (the full number, also beyond the capacity)
//   3. emit    the predicate again (the same device function on the same inputs: the same bits), the ray's rank among the
//              block's kept rays (block_rank again), destination = tile[b] + rank; nothing is written at an index >= capacity
// The order of the output is a prefix sum, never the arrival order of atomics, and NO block ever waits for another block: no
// decoupled look-back, no grid barrier, no cooperative launch — a block that spins on a tile which is not resident is how a
// shared card gets hung.  One block per tile, uncapped (no grid-stride, hence no cap boundary).
//
// A lane owns one ray; every access is a 4-byte (8-byte for the int64 arrays) element access, so inputs may start at any ray of
// a larger allocation.  Traffic: 36 B per ray in the count pass, 48 B per ray in the emit pass, <= 30 B per survivor; measured
// 0.07 ms per 1080p pose with half of the rays kept, beside a 31 ms render (tools/export_bench.py,
// profiles/micro/export_pointcloud.txt).  Like tn_frame.hip the kernels are launch- and latency-bound and not a tuning target.
#include "tn_device.h"
#include "tn_scan.h"

using namespace tn;

namespace {

constexpr int kTile = 256;    // rays per tile = threads per block of the count and emit kernels

struct Ray {  // what the predicate leaves behind for the emit
    float p[3];
    float thermal;
};

// the filter of ray i (i < n); every comparison is strict and false for a NaN
__device__ __forceinline__ bool keep_ray(const float *__restrict__ origins, const float *__restrict__ directions,
                                         const float *__restrict__ depth, const float *__restrict__ accumulation,
                                         const float *__restrict__ thermal, const tn_pointcloud_params &q, long long i, Ray &r) {
    const float t = depth[i];
    bool keep = accumulation[i] > q.min_accumulation;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        r.p[c] = add_rn(origins[3 * i + c], mul_rn(directions[3 * i + c], t));
        keep = keep && r.p[c] > q.box_min[c] && r.p[c] < q.box_max[c];
    }
    r.thermal = thermal[i];
    return keep && r.thermal > q.thermal_lo && r.thermal < q.thermal_hi;
}

__global__ void __launch_bounds__(kTile)
count_kernel(const float *__restrict__ origins, const float *__restrict__ directions, const float *__restrict__ depth,
             const float *__restrict__ accumulation, const float *__restrict__ thermal, tn_pointcloud_params q, long long n,
             long long *__restrict__ tiles) {
    const long long i = (long long)blockIdx.x * kTile + threadIdx.x;
    Ray r;
    uint32_t total;
    block_rank<kTile>(i < n && keep_ray(origins, directions, depth, accumulation, thermal, q, i, r), total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = (long long)total;
}

__global__ void __launch_bounds__(kScan)
scan_kernel(long long *__restrict__ tiles, long long num_tiles, long long *__restrict__ count) {
    scan_tiles<true>(tiles, num_tiles, count);  // a pass sums at most kScan * kTile = 2^18
}

__global__ void __launch_bounds__(kTile)
emit_kernel(const float *__restrict__ origins, const float *__restrict__ directions, const float *__restrict__ depth,
            const float *__restrict__ accumulation, const float *__restrict__ rgb, const float *__restrict__ thermal,
            tn_pointcloud_params q, long long n, long long source_base, const uint8_t *__restrict__ table,
            const long long *__restrict__ tiles, float *__restrict__ positions, uint8_t *__restrict__ colors,
            float *__restrict__ temperature, uint8_t *__restrict__ thermal_colors, long long *__restrict__ source,
            long long capacity) {
    __shared__ uint32_t lut[256];
    if (thermal_colors) load_lut<kTile>(lut, table);
    const long long i = (long long)blockIdx.x * kTile + threadIdx.x;
    Ray r;
    const bool keep = i < n && keep_ray(origins, directions, depth, accumulation, thermal, q, i, r);
    uint32_t total;
    const uint32_t rank = block_rank<kTile>(keep, total);  // its barrier is also the one between the table's fill and its reads
    if (!keep) return;
    const long long dst = tiles[blockIdx.x] + (long long)rank;
    if (dst >= capacity) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        positions[3 * dst + c] = affine_row(q.to_world + 4 * c, r.p);
        colors[3 * dst + c] = (uint8_t)quantise(mul_rn(rgb[3 * i + c], 255.0f));
    }
    temperature[dst] = add_rn(mul_rn(r.thermal, q.temperature_span), q.temperature_min);
    // (a kept thermal is never NaN: it passed two comparisons)
    if (thermal_colors) store_rgb8(thermal_colors + 3 * dst, lut_entry(lut, r.thermal));
    if (source) source[dst] = source_base + i;
}

inline long long tiles_of(long long num_rays) { return ceil_div(num_rays, kTile); }

}  // namespace

extern "C" {

int32_t tn_pointcloud_tile_rays(void) { return kTile; }

int32_t tn_pointcloud_scan_width(void) { return kScan; }

size_t tn_pointcloud_workspace_bytes(int64_t num_rays) {
    return num_rays > 0 ? (size_t)tiles_of(num_rays) * sizeof(long long) : 0;
}

int tn_pointcloud_append(const float *origins, const float *directions, const float *depth, const float *accumulation,
                         const float *rgb, const float *thermal, int64_t num_rays, int64_t source_base,
                         const tn_pointcloud_params *params, const uint8_t *thermal_table, float *positions, uint8_t *colors,
                         float *temperature, uint8_t *thermal_colors, int64_t *source, int64_t capacity, int64_t *count,
                         void *workspace, size_t workspace_bytes, void *stream) {
    if (!origins || !directions || !depth || !accumulation || !rgb || !thermal || !params || !count) return TN_ERR_NULL;
    if (capacity > 0 && (!positions || !colors || !temperature)) return TN_ERR_NULL;
    if (thermal_colors && !thermal_table) return TN_ERR_NULL;
    if (num_rays < 0 || capacity < 0) return TN_ERR_SHAPE;
    if (tiles_of(num_rays) > 0x7fffffffLL) return TN_ERR_SHAPE;  // one block per tile: the grid's x extent
    if (misaligned(origins, 4) || misaligned(directions, 4) || misaligned(depth, 4) || misaligned(accumulation, 4) ||
        misaligned(rgb, 4) || misaligned(thermal, 4) || misaligned(positions, 4) || misaligned(temperature, 4) ||
        misaligned(source, 8) || misaligned(count, 8) || misaligned(workspace, 8))
        return TN_ERR_SHAPE;
    if (num_rays == 0) return TN_OK;
    if (!workspace) return TN_ERR_NULL;
    if (workspace_bytes < tn_pointcloud_workspace_bytes(num_rays)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long long n = num_rays, num_tiles = tiles_of(n);
    long long *tiles = reinterpret_cast<long long *>(workspace);
    long long *cnt = reinterpret_cast<long long *>(count);
    hipLaunchKernelGGL(count_kernel, dim3((unsigned)num_tiles), dim3(kTile), 0, s, origins, directions, depth, accumulation, thermal,
                       *params, n, tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kScan), 0, s, tiles, num_tiles, cnt);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(emit_kernel, dim3((unsigned)num_tiles), dim3(kTile), 0, s, origins, directions, depth, accumulation, rgb,
                       thermal, *params, n, (long long)source_base, thermal_table, tiles, positions, colors, temperature,
                       thermal_colors, reinterpret_cast<long long *>(source), (long long)capacity);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

}  // extern "C"
