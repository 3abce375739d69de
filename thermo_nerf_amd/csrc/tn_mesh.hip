// Thermal mesh export: rendered poses -> a TSDF volume -> an indexed triangle list by SURFACE NETS (DESIGN.md "Mesh export").
// nerfstudio's TSDF exporter fuses rendered depth into a voxel volume and extracts a surface; here a vertex also carries its
// temperature in degrees.  Every step is ONE correctly rounded fp32 operation (explicit *_rn intrinsics; quotients and roots are
// formed in fp64 and rounded once, which for fp32 operands IS the correctly rounded fp32 result: 53 >= 2 * 24 + 2), so a volume
// and a mesh are defined bit for bit (include/thermonerf_hip.h).
//
// tn_tsdf_integrate: one plain launch per pose, one thread per voxel, x fastest: the seven planes are coalesced streams, a voxel
// is read, updated and written by its own thread only (no atomics), a skipped voxel writes nothing.
// tn_mesh_extract: six plain launches, the ordered count / scan / emit of tn_pointcloud.hip twice, on the block-wide primitives
// of tn_scan.h:
//   1. count   active cells per tile of kTile cells (block_rank's total)                        -> cell_tiles[b]
//   2. scan    ONE block: exclusive prefix of the tile counts, counts[0] <- the number of vertices
//   3. emit    the predicate again, block_rank: cell_index[cell] <- vertex index or -1 for EVERY cell, vertex data only below
//              capacity_vertices
//   4. count   triangles per tile of kTile grid points (0, 2, 4 or 6 per point: a quad per crossing edge p -> p + e_a whose four
//              cells are active; block_exclusive's total)                                       -> point_tiles[b]
//   5. scan    counts[1] <- the number of triangles
//   6. emit    the predicate again, block_exclusive of the per-point counts; nothing at or beyond capacity_triangles
// No atomics, no allocation, no host synchronisation, and NO block ever waits for another block (no look-back, no grid barrier,
// no cooperative launch).  One block per tile, uncapped.
//
// Traffic: a pose reads and writes at most 7 planes = 56 B per voxel; the extraction reads 2 planes 8 times per cell, twice, which
// the caches mostly absorb.  Measured at 256^3 (tools/mesh_bench.py, profiles/micro/export_mesh.txt): 0.23 ms per 1080p pose beside
// 30.9 ms of rendering, 1.07 ms for the extraction.
#include "tn_device.h"
#include "tn_scan.h"

using namespace tn;

namespace {

constexpr int kTile = 256;  // cells / grid points per tile = threads per block of every kernel but the scan

struct Dims {
    int nx, ny, nz;
    long long points;  // nx * ny * nz <= 2^31 - 1
    long long cells;   // (nx - 1)(ny - 1)(nz - 1)
};

inline Dims dims_of(const tn_mesh_params &q) {
    Dims d;
    d.nx = q.dims[0], d.ny = q.dims[1], d.nz = q.dims[2];
    d.points = (long long)d.nx * d.ny * d.nz;
    d.cells = (long long)(d.nx - 1) * (d.ny - 1) * (d.nz - 1);
    return d;
}

__device__ __forceinline__ float grid_coord(const tn_mesh_params &q, int c, float idx) {
    return add_rn(q.lo[c], mul_rn(idx, q.step[c]));
}

// ---- fusion --------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kTile)
integrate_kernel(const float *__restrict__ depth, const float *__restrict__ accumulation, const float *__restrict__ thermal,
                 const float *__restrict__ rgb, int height, int width, tn_mesh_params q, Dims d, float *__restrict__ volume) {
    const long long vox = (long long)blockIdx.x * kTile + threadIdx.x;
    if (vox >= d.points) return;
    const int i = (int)(vox % d.nx), j = (int)(vox / d.nx % d.ny), k = (int)(vox / ((long long)d.nx * d.ny));
    const float p[3] = {grid_coord(q, 0, (float)i), grid_coord(q, 1, (float)j), grid_coord(q, 2, (float)k)};
    const float c[3] = {affine_row(q.w2c, p), affine_row(q.w2c + 4, p), affine_row(q.w2c + 8, p)};
    const float zc = -c[2];  // the camera looks along -z
    if (!(zc > 0.0f)) return;
    const float u = add_rn(div_rn(mul_rn(q.fx, c[0]), zc), q.cx);
    const float v = add_rn(div_rn(mul_rn(q.fy, -c[1]), zc), q.cy);
    if (!(u >= 0.0f && u < (float)width && v >= 0.0f && v < (float)height)) return;  // (a NaN fails)
    const int pix = (int)v * width + (int)u;  // the nearest pixel: centres sit at +0.5
    if (!(accumulation[pix] > q.min_accumulation)) return;
    const float dist = sqrt_rn(add_rn(add_rn(mul_rn(c[0], c[0]), mul_rn(c[1], c[1])), mul_rn(c[2], c[2])));
    const float sdf = sub_rn(depth[pix], dist);  // the engine's depth is a distance along a unit direction
    if (!(sdf >= -q.truncation && sdf < INFINITY)) return;
    float *plane = volume + vox;
    plane[0] = add_rn(plane[0], fminf(1.0f, mul_rn(sdf, q.inv_truncation)));
    plane[d.points] = add_rn(plane[d.points], 1.0f);
    if (sdf <= q.truncation) {  // near the surface: free space far in front of it must not take the colour of what lies behind
        plane[2 * d.points] = add_rn(plane[2 * d.points], thermal[pix]);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) plane[(3 + ch) * d.points] = add_rn(plane[(3 + ch) * d.points], rgb[3 * (long long)pix + ch]);
        plane[6 * d.points] = add_rn(plane[6 * d.points], 1.0f);
    }
}

// ---- extraction ----------------------------------------------------------------------------------------------------------------

// grid point g: observed iff weight > 0; its value f = tsdf_sum / weight; inside iff observed and f < 0
__device__ __forceinline__ bool point_state(const float *__restrict__ volume, const Dims &d, long long g, float &f) {
    const float w = volume[d.points + g];
    const bool observed = w > 0.0f;
    f = observed ? div_rn(volume[g], w) : 0.0f;
    return observed;
}

struct Cell {
    int i, j, k;
    long long corner;  // grid point (i, j, k)
    float f[8];        // corner values, x fastest
};

// cell `cell` (< d.cells): active iff all 8 corners are observed and they are neither all inside nor all outside
__device__ __forceinline__ bool cell_active(const float *__restrict__ volume, const Dims &d, long long cell, Cell &c) {
    const int cx = d.nx - 1, cy = d.ny - 1;
    c.i = (int)(cell % cx), c.j = (int)(cell / cx % cy), c.k = (int)(cell / ((long long)cx * cy));
    c.corner = ((long long)c.k * d.ny + c.j) * d.nx + c.i;
    bool all = true;
    int inside = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const long long g = c.corner + (e & 1) + (long long)(e >> 1 & 1) * d.nx + (long long)(e >> 2) * d.nx * d.ny;
        all = point_state(volume, d, g, c.f[e]) && all;
        inside += c.f[e] < 0.0f ? 1 : 0;
    }
    return all && inside > 0 && inside < 8;
}

__global__ void __launch_bounds__(kTile)
count_cells_kernel(const float *__restrict__ volume, Dims d, long long *__restrict__ tiles) {
    const long long cell = (long long)blockIdx.x * kTile + threadIdx.x;
    Cell c;
    uint32_t total;
    block_rank<kTile>(cell < d.cells && cell_active(volume, d, cell, c), total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = (long long)total;
}

template <bool APPEND>
__global__ void __launch_bounds__(kScan)
scan_kernel(long long *__restrict__ tiles, long long num_tiles, long long *__restrict__ count) {
    scan_tiles<APPEND>(tiles, num_tiles, count);  // a pass sums at most kScan * 6 * kTile < 2^21
}

__global__ void __launch_bounds__(kTile)
emit_vertices_kernel(const float *__restrict__ volume, tn_mesh_params q, Dims d, const uint8_t *__restrict__ table,
                     const long long *__restrict__ tiles, int *__restrict__ cell_index, float *__restrict__ positions,
                     uint8_t *__restrict__ colors, float *__restrict__ temperature, uint8_t *__restrict__ thermal_colors,
                     long long capacity) {
    __shared__ uint32_t lut[256];
    if (thermal_colors) load_lut<kTile>(lut, table);
    const long long cell = (long long)blockIdx.x * kTile + threadIdx.x;
    Cell c;
    const bool keep = cell < d.cells && cell_active(volume, d, cell, c);
    uint32_t total;
    const uint32_t rank = block_rank<kTile>(keep, total);  // its barrier is also the one between the table's fill and its reads
    if (cell >= d.cells) return;
    if (!keep) {
        cell_index[cell] = -1;
        return;
    }
    const long long dst = tiles[blockIdx.x] + (long long)rank;  // < the number of cells <= 2^31 - 1
    cell_index[cell] = (int)dst;
    if (dst >= capacity) return;
    // the vertex: the mean of the crossings of the cell's 12 edges, axis 0, 1, 2; within an axis the two other offsets run
    // (0,0) (1,0) (0,1) (1,1), the lower-numbered axis first
    float s[3] = {0.0f, 0.0f, 0.0f}, n = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int b = a == 0 ? 1 : 0, cc = a == 2 ? 1 : 2;  // the other two axes, ascending
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ob = e & 1, oc = e >> 1;
            const int ca = ob << b | oc << cc;
            const float fa = c.f[ca], fb = c.f[ca | 1 << a];
            if ((fa < 0.0f) != (fb < 0.0f)) {
                s[a] = add_rn(s[a], div_rn(fa, sub_rn(fa, fb)));
                s[b] = add_rn(s[b], (float)ob);
                s[cc] = add_rn(s[cc], (float)oc);
                n = add_rn(n, 1.0f);
            }
        }
    }
    const int idx[3] = {c.i, c.j, c.k};
    float p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = add_rn(q.lo[a], mul_rn(add_rn((float)idx[a], div_rn(s[a], n)), q.step[a]));
    // attributes: the pooled near-surface observations of the 8 corners, x-fastest corner order
    float sum[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const long long g = c.corner + (e & 1) + (long long)(e >> 1 & 1) * d.nx + (long long)(e >> 2) * d.nx * d.ny;
#pragma unroll
        for (int pl = 0; pl < 5; ++pl) sum[pl] = add_rn(sum[pl], volume[(2 + pl) * d.points + g]);
    }
    const float mean_thermal = div_rn(sum[0], sum[4]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        positions[3 * dst + a] = affine_row(q.to_world + 4 * a, p);
        colors[3 * dst + a] = (uint8_t)quantise(mul_rn(div_rn(sum[1 + a], sum[4]), 255.0f));
    }
    temperature[dst] = add_rn(mul_rn(mean_thermal, q.temperature_span), q.temperature_min);
    if (thermal_colors) store_rgb8(thermal_colors + 3 * dst, lut_entry_nan(lut, mean_thermal));  // NaN -> (0, 0, 0)
}

struct Quads {
    int v[3][4];   // per axis: the four cells' vertex indices, already in emission order
    bool on[3];
};

// the quads of grid point g (< d.points): one per axis a whose edge g -> g + e_a is crossing and whose four cells, at offsets
// (-1,-1) (0,-1) (0,0) (-1,0) in (b, c) = ((a+1)%3, (a+2)%3), all exist and are active; returns their number
__device__ __forceinline__ int point_quads(const float *__restrict__ volume, const Dims &d, const int *__restrict__ cell_index,
                                           long long g, Quads &out) {
    const int n[3] = {d.nx, d.ny, d.nz};
    const int idx[3] = {(int)(g % d.nx), (int)(g / d.nx % d.ny), (int)(g / ((long long)d.nx * d.ny))};
    const long long pstride[3] = {1, d.nx, (long long)d.nx * d.ny};
    const long long cstride[3] = {1, d.nx - 1, (long long)(d.nx - 1) * (d.ny - 1)};
    float f0;
    const bool seen = point_state(volume, d, g, f0);
    int count = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        out.on[a] = false;
        if (!seen || idx[a] > n[a] - 2 || idx[b] < 1 || idx[b] > n[b] - 2 || idx[c] < 1 || idx[c] > n[c] - 2) continue;
        float f1;
        if (!point_state(volume, d, g + pstride[a], f1) || (f0 < 0.0f) == (f1 < 0.0f)) continue;
        const long long cell = idx[0] * cstride[0] + idx[1] * cstride[1] + idx[2] * cstride[2];
        const int v0 = cell_index[cell - cstride[b] - cstride[c]], v1 = cell_index[cell - cstride[c]];
        const int v2 = cell_index[cell], v3 = cell_index[cell - cstride[b]];
        if (v0 < 0 || v1 < 0 || v2 < 0 || v3 < 0) continue;
        const bool flip = f1 < 0.0f;  // g + e_a is the inside end: reversed, so that normals point from inside to outside
        out.v[a][0] = v0, out.v[a][1] = flip ? v3 : v1, out.v[a][2] = v2, out.v[a][3] = flip ? v1 : v3;
        out.on[a] = true;
        ++count;
    }
    return count;
}

__global__ void __launch_bounds__(kTile)
count_triangles_kernel(const float *__restrict__ volume, Dims d, const int *__restrict__ cell_index, long long *__restrict__ tiles) {
    const long long g = (long long)blockIdx.x * kTile + threadIdx.x;
    Quads qd;
    uint32_t total;
    block_exclusive<kTile>(g < d.points ? 2u * (uint32_t)point_quads(volume, d, cell_index, g, qd) : 0u, total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = (long long)total;
}

__global__ void __launch_bounds__(kTile)
emit_triangles_kernel(const float *__restrict__ volume, Dims d, const int *__restrict__ cell_index,
                      const long long *__restrict__ tiles, int *__restrict__ triangles, long long capacity) {
    const long long g = (long long)blockIdx.x * kTile + threadIdx.x;
    Quads qd;
    const uint32_t own = g < d.points ? 2u * (uint32_t)point_quads(volume, d, cell_index, g, qd) : 0u;
    uint32_t total;
    const uint32_t before = block_exclusive<kTile>(own, total);
    if (own == 0u) return;
    long long dst = tiles[blockIdx.x] + (long long)before;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!qd.on[a]) continue;
        const int *v = qd.v[a];
        if (dst < capacity) {
            triangles[3 * dst] = v[0];
            triangles[3 * dst + 1] = v[1];
            triangles[3 * dst + 2] = v[2];
        }
        if (dst + 1 < capacity) {
            triangles[3 * dst + 3] = v[0];
            triangles[3 * dst + 4] = v[2];
            triangles[3 * dst + 5] = v[3];
        }
        dst += 2;
    }
}

inline long long tiles_of(long long items) { return ceil_div(items, kTile); }

inline size_t index_bytes(long long cells) { return ((size_t)cells * sizeof(int) + 7) / 8 * 8; }

// TN_OK, or the error of a grid the kernels do not take
inline int check_dims(const tn_mesh_params &q) {
    long long points = 1;
    for (int c = 0; c < 3; ++c) {
        if (q.dims[c] < 2) return TN_ERR_SHAPE;
        points *= q.dims[c];
        if (points > 0x7fffffffLL) return TN_ERR_UNSUPPORTED;  // vertex indices are int32
    }
    return TN_OK;
}

}  // namespace

extern "C" {

int32_t tn_mesh_tile(void) { return kTile; }

int32_t tn_mesh_scan_width(void) { return kScan; }

size_t tn_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
    tn_mesh_params q;
    q.dims[0] = nx, q.dims[1] = ny, q.dims[2] = nz;
    if (check_dims(q) != TN_OK) return 0;
    const Dims d = dims_of(q);
    return index_bytes(d.cells) + (size_t)(tiles_of(d.cells) + tiles_of(d.points)) * sizeof(long long);
}

int tn_tsdf_integrate(const float *depth, const float *accumulation, const float *thermal, const float *rgb, int32_t height,
                      int32_t width, const tn_mesh_params *params, float *volume, void *stream) {
    if (!depth || !accumulation || !thermal || !rgb || !params || !volume) return TN_ERR_NULL;
    if (height < 1 || width < 1 || (long long)height * width > 0x7fffffffLL) return TN_ERR_SHAPE;
    if (const int bad = check_dims(*params)) return bad;
    if (misaligned(depth, 4) || misaligned(accumulation, 4) || misaligned(thermal, 4) || misaligned(rgb, 4) || misaligned(volume, 4))
        return TN_ERR_SHAPE;
    const Dims d = dims_of(*params);
    hipLaunchKernelGGL(integrate_kernel, dim3((unsigned)tiles_of(d.points)), dim3(kTile), 0, (hipStream_t)stream, depth, accumulation,
                       thermal, rgb, (int)height, (int)width, *params, d, volume);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

int tn_mesh_extract(const float *volume, const tn_mesh_params *params, const uint8_t *thermal_table, float *positions,
                    uint8_t *colors, float *temperature, uint8_t *thermal_colors, int64_t capacity_vertices, int32_t *triangles,
                    int64_t capacity_triangles, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream) {
    if (!volume || !params || !counts || !workspace) return TN_ERR_NULL;
    if (capacity_vertices > 0 && (!positions || !colors || !temperature)) return TN_ERR_NULL;
    if (capacity_triangles > 0 && !triangles) return TN_ERR_NULL;
    if (thermal_colors && !thermal_table) return TN_ERR_NULL;
    if (capacity_vertices < 0 || capacity_triangles < 0) return TN_ERR_SHAPE;
    if (const int bad = check_dims(*params)) return bad;
    if (misaligned(volume, 4) || misaligned(positions, 4) || misaligned(temperature, 4) || misaligned(triangles, 4) ||
        misaligned(counts, 8) || misaligned(workspace, 8))
        return TN_ERR_SHAPE;
    if (workspace_bytes < tn_mesh_workspace_bytes(params->dims[0], params->dims[1], params->dims[2])) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const Dims d = dims_of(*params);
    const long long cell_tiles_n = tiles_of(d.cells), point_tiles_n = tiles_of(d.points);
    int *cell_index = reinterpret_cast<int *>(workspace);
    long long *cell_tiles = reinterpret_cast<long long *>(reinterpret_cast<char *>(workspace) + index_bytes(d.cells));
    long long *point_tiles = cell_tiles + cell_tiles_n;
    long long *cnt = reinterpret_cast<long long *>(counts);
    hipLaunchKernelGGL(count_cells_kernel, dim3((unsigned)cell_tiles_n), dim3(kTile), 0, s, volume, d, cell_tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_kernel<false>, dim3(1), dim3(kScan), 0, s, cell_tiles, cell_tiles_n, cnt);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(emit_vertices_kernel, dim3((unsigned)cell_tiles_n), dim3(kTile), 0, s, volume, *params, d, thermal_table,
                       cell_tiles, cell_index, positions, colors, temperature, thermal_colors, (long long)capacity_vertices);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(count_triangles_kernel, dim3((unsigned)point_tiles_n), dim3(kTile), 0, s, volume, d, cell_index, point_tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_kernel<false>, dim3(1), dim3(kScan), 0, s, point_tiles, point_tiles_n, cnt + 1);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(emit_triangles_kernel, dim3((unsigned)point_tiles_n), dim3(kTile), 0, s, volume, d, cell_index, point_tiles,
                       triangles, (long long)capacity_triangles);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

}  // extern "C"
