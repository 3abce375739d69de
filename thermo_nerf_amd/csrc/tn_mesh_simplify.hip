// Vertex-clustering simplification of an indexed triangle list (DESIGN.md "Mesh simplification"; include/thermonerf_hip.h defines
// every output to the bit).  The vertices are clustered by the cell of tn_voxel_params' grid they fall in, exactly as
// tn_voxel_downsample clusters points (tn_voxel_grid.h); a triangle survives iff its three corners fall in three different clusters
// and no earlier triangle has the same cluster triple up to rotation; a cluster becomes a vertex iff a surviving triangle names it.
// Launches on the caller's stream:
//   1. vertex keys   one thread per vertex: the cell key, or `total` for a non-member
//   2. sort          tn_sort_pairs of (key, 0 .. V-1) over bit_length(total) bits
//   3. clusters      the heads of the runs of equal keys compacted in order (count, one-block scan, emit): heads[c] = where cluster
//                    c's run starts; the emit also writes every vertex's cluster rank (-1 for a non-member)
//   4. triples       one thread per triangle: validity, the three ranks, the canonical rotation (smallest rank first), the sort
//                    key(s); a block adds its dropped triangles to counts[2] (one integer atomic per block)
//   5. sort          with b = bit_length(V): if 3 b + 1 <= 64, ONE sort of the key (first << 2b | second << b | third), dropped
//                    triangles behind with bit 3b; otherwise TWO stable sorts, by the third rank, then by (first << b | second)
//                    with bit 2b for the dropped ones.  Either way equal triples end up adjacent in ascending triangle index.
//   6. flags         the head of every run of equal triples is the KEPT triangle: kept[t] = 1 and used[cluster] = 1 for its three
//                    clusters (plain stores of the same value), kept[t] = 0 for every other triangle
//   7. compaction    of kept[] in triangle order and of used[] in cluster order (count, one-block scan, emit, each); the cluster
//                    emit gives cluster_out[c] (the output vertex or -1) and walks the cluster's run for its means
//   8. emit          the kept triangles re-indexed through rank and cluster_out; vertex_map
// No allocation, no host synchronisation, no float atomics, and no block ever waits for another.  The walk of step 7 is sequential
// per cluster because the sums are ordered by definition: a cluster of 10^5 members is 10^5 steps of one thread (a sensible cell
// holds a handful of surface-nets vertices).
#include "tn_device.h"
#include "tn_scan.h"
#include "tn_voxel_grid.h"

using namespace tn;

namespace {

constexpr int kTile = 256;  // vertices / triangles / sorted positions / clusters per block of every kernel but the scan

__global__ void __launch_bounds__(kTile)
vertex_keys_kernel(const float *__restrict__ positions, long long n, VoxelGrid g, unsigned long long *__restrict__ keys) {
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

// the scan of the kept triangles also closes the books: counts[3] = T - kept - dropped
__global__ void __launch_bounds__(kScan)
scan_kept_kernel(long long *__restrict__ tiles, long long num_tiles, long long num_triangles, long long *__restrict__ counts) {
    scan_tiles<false>(tiles, num_tiles, counts + 1);
    if (threadIdx.x == 0) counts[3] = num_triangles - counts[1] - counts[2];  // (this thread wrote counts[1])
}

// heads[c] = the sorted position where cluster c starts; rank[i] = the cluster of vertex i = the heads at or before its position,
// less one
__global__ void __launch_bounds__(kTile)
emit_heads_kernel(const unsigned long long *__restrict__ keys, const int *__restrict__ order, long long n, unsigned long long total,
                  const long long *__restrict__ tiles, int *__restrict__ heads, int *__restrict__ rank) {
    const long long j = (long long)blockIdx.x * kTile + threadIdx.x;
    const bool head = voxel_head(keys, j, n, total);
    uint32_t unused;
    const uint32_t before = block_rank<kTile>(head, unused);
    if (j >= n) return;
    const long long c = tiles[blockIdx.x] + (long long)before + (head ? 1 : 0) - 1;  // < n
    if (head && c < n) heads[c] = (int)j;
    const long long i = order[j];
    if (i >= 0 && i < n) rank[i] = keys[j] < total && c >= 0 ? (int)c : -1;  // (a member always has a head at or before it)
}

struct Triples {
    int bits;                       // b = bit_length(V): a rank is below 2^b
    unsigned long long *keys;       // one sort: the whole triple; two sorts: (first, second)
    unsigned long long *third;      // two sorts only
    unsigned long long dropped;     // the key of an invalid or degenerate triangle: behind every triple
};

template <bool TWO>
__global__ void __launch_bounds__(kTile)
triples_kernel(const int *__restrict__ triangles, long long num_triangles, long long num_vertices, const int *__restrict__ rank, Triples out,
               unsigned long long *__restrict__ dropped_count) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    bool good = t < num_triangles;
    unsigned long long c[3] = {0, 0, 0};
    if (good) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const long long i = triangles[3 * t + a];
            const int r = i >= 0 && i < num_vertices ? rank[i] : -1;
            good = good && r >= 0;
            c[a] = (unsigned long long)(r >= 0 ? r : 0);
        }
        good = good && c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
    }
    uint32_t dropped;
    block_rank<kTile>(t < num_triangles && !good, dropped);
    if (threadIdx.x == 0 && dropped) atomicAdd(dropped_count, (unsigned long long)dropped);
    if (t >= num_triangles) return;
    unsigned long long first = c[0], second = c[1], third = c[2];  // the rotation with the smallest first: the three differ
    if (c[1] < c[0] && c[1] < c[2]) {
        first = c[1], second = c[2], third = c[0];
    } else if (c[2] < c[0] && c[2] < c[1]) {
        first = c[2], second = c[0], third = c[1];
    }
    if (TWO) {
        out.keys[t] = good ? (first << out.bits) | second : out.dropped;
        out.third[t] = good ? third : 0ull;
    } else {
        out.keys[t] = good ? (((first << out.bits) | second) << out.bits) | third : out.dropped;
    }
}

__global__ void __launch_bounds__(kTile)
gather_kernel(const unsigned long long *__restrict__ keys, const int *__restrict__ order, long long n, unsigned long long *__restrict__ out) {
    const long long j = (long long)blockIdx.x * kTile + threadIdx.x;
    if (j >= n) return;
    const long long t = order[j];
    out[j] = t >= 0 && t < n ? keys[t] : ~0ull;
}

// sorted position j: its triangle, kept iff it starts a run of equal triples.  `third` (per triangle, two sorts only) completes
// the comparison of the sorted (first, second) keys.
__global__ void __launch_bounds__(kTile)
flags_kernel(const unsigned long long *__restrict__ sorted, const int *__restrict__ order, const unsigned long long *__restrict__ third,
             long long num_triangles, unsigned long long dropped, const int *__restrict__ triangles, long long num_vertices,
             const int *__restrict__ rank, int *__restrict__ kept, int *__restrict__ used) {
    const long long j = (long long)blockIdx.x * kTile + threadIdx.x;
    if (j >= num_triangles) return;
    const long long t = order[j];
    if (t < 0 || t >= num_triangles) return;
    const unsigned long long key = sorted[j];
    bool head = key < dropped;
    if (head && j > 0 && key == sorted[j - 1]) {
        const long long before = order[j - 1];
        head = third != nullptr && before >= 0 && before < num_triangles && third[t] != third[before];
    }
    kept[t] = head ? 1 : 0;
    if (!head) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const long long i = triangles[3 * t + a];  // in [0, V) and a member: the key says so
        if (i >= 0 && i < num_vertices && rank[i] >= 0) used[rank[i]] = 1;
    }
}

// `limit`: a device count that bounds n further (the clusters among V slots), or NULL
__device__ __forceinline__ bool flagged(const int *__restrict__ flags, long long i, long long n, const long long *__restrict__ limit) {
    return i < n && (limit == nullptr || i < limit[0]) && flags[i] != 0;
}

__global__ void __launch_bounds__(kTile)
count_flags_kernel(const int *__restrict__ flags, long long n, const long long *__restrict__ limit, long long *__restrict__ tiles) {
    const long long i = (long long)blockIdx.x * kTile + threadIdx.x;
    uint32_t total;
    block_rank<kTile>(flagged(flags, i, n, limit), total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = (long long)total;
}

__global__ void __launch_bounds__(kTile)
emit_clusters_kernel(const int *__restrict__ used, long long num_vertices, const long long *__restrict__ clusters,
                     const long long *__restrict__ tiles, const unsigned long long *__restrict__ keys, const int *__restrict__ order,
                     const int *__restrict__ heads, long long capacity, VoxelInputs in, VoxelOutputs out, int *__restrict__ cluster_out) {
    const long long c = (long long)blockIdx.x * kTile + threadIdx.x;
    const bool keep = flagged(used, c, num_vertices, clusters);
    uint32_t unused;
    const uint32_t before = block_rank<kTile>(keep, unused);
    if (c >= num_vertices || c >= clusters[0]) return;
    const long long v = tiles[blockIdx.x] + (long long)before;  // <= c
    cluster_out[c] = keep ? (int)v : -1;
    if (keep && v < capacity) voxel_average(keys, order, num_vertices, heads[c], in, out, v);
}

__global__ void __launch_bounds__(kTile)
emit_triangles_kernel(const int *__restrict__ kept, const int *__restrict__ triangles, long long num_triangles, long long num_vertices,
                      const long long *__restrict__ tiles, const int *__restrict__ rank, const int *__restrict__ cluster_out,
                      long long capacity, int *__restrict__ triangles_out, int *__restrict__ triangle_source) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    const bool keep = flagged(kept, t, num_triangles, nullptr);
    uint32_t unused;
    const uint32_t before = block_rank<kTile>(keep, unused);
    if (!keep) return;
    const long long o = tiles[blockIdx.x] + (long long)before;  // <= t
    if (o >= capacity) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const long long i = triangles[3 * t + a];
        const int r = i >= 0 && i < num_vertices ? rank[i] : -1;
        triangles_out[3 * o + a] = r >= 0 ? cluster_out[r] : -1;  // (a kept triangle's clusters are all used)
    }
    if (triangle_source) triangle_source[o] = (int)t;
}

__global__ void __launch_bounds__(kTile)
vertex_map_kernel(const int *__restrict__ rank, const int *__restrict__ cluster_out, long long num_vertices, int *__restrict__ vertex_map) {
    const long long i = (long long)blockIdx.x * kTile + threadIdx.x;
    if (i >= num_vertices) return;
    const int r = rank[i];
    vertex_map[i] = r >= 0 ? cluster_out[r] : -1;
}

inline long long tiles_of(long long n) { return ceil_div(n, kTile); }

inline size_t keys_bytes(long long n) { return (size_t)n * sizeof(unsigned long long); }

inline bool two_sorts(long long num_vertices) { return 3 * bit_length((unsigned long long)num_vertices) + 1 > 64; }

// the workspace, in order: per vertex the keys, the sorted keys, five int arrays (order, heads, rank, used, cluster_out) and the tile
// counts; the cluster count; per triangle two key arrays (four with two sorts), the order (two with two sorts), kept and the tile
// counts; the sort's own workspace for the longer of the two lists
struct Layout {
    unsigned long long *vertex_keys, *vertex_sorted, *triangle_keys[4];
    int *vertex_order, *heads, *rank, *used, *cluster_out, *triangle_order[2], *kept;
    long long *vertex_tiles, *clusters, *triangle_tiles;
    void *sort;
    size_t sort_bytes, bytes;
};

inline Layout layout_of(char *ws, long long v, long long t) {
    Layout l;
    size_t at = 0;
    auto take = [&](size_t bytes) {  // (ws == NULL: the sizes alone)
        char *p = ws ? ws + at : nullptr;
        at += bytes;
        return p;
    };
    const bool two = two_sorts(v);
    l.vertex_keys = reinterpret_cast<unsigned long long *>(take(keys_bytes(v)));
    l.vertex_sorted = reinterpret_cast<unsigned long long *>(take(keys_bytes(v)));
    int **per_vertex[5] = {&l.vertex_order, &l.heads, &l.rank, &l.used, &l.cluster_out};
    for (int k = 0; k < 5; ++k) *per_vertex[k] = reinterpret_cast<int *>(take(ints_bytes(v)));
    l.vertex_tiles = reinterpret_cast<long long *>(take((size_t)tiles_of(v) * sizeof(long long)));
    l.clusters = reinterpret_cast<long long *>(take(sizeof(long long)));
    for (int k = 0; k < 4; ++k) l.triangle_keys[k] = k < (two ? 4 : 2) ? reinterpret_cast<unsigned long long *>(take(keys_bytes(t))) : nullptr;
    for (int k = 0; k < 2; ++k) l.triangle_order[k] = k < (two ? 2 : 1) ? reinterpret_cast<int *>(take(ints_bytes(t))) : nullptr;
    l.kept = reinterpret_cast<int *>(take(ints_bytes(t)));
    l.triangle_tiles = reinterpret_cast<long long *>(take((size_t)tiles_of(t) * sizeof(long long)));
    l.sort_bytes = tn_sort_pairs_workspace_bytes(v > t ? v : t);
    l.sort = take(l.sort_bytes);
    l.bytes = at;
    return l;
}

}  // namespace

extern "C" {

size_t tn_mesh_simplify_workspace_bytes(int64_t num_vertices, int64_t num_triangles) {
    if (bad_counts(num_vertices, num_triangles)) return 0;
    return layout_of(nullptr, (long long)num_vertices, (long long)num_triangles).bytes;
}

int tn_mesh_simplify(const float *positions, const uint8_t *colors, const float *temperature, const uint8_t *thermal_colors,
                     const int32_t *triangles, int64_t num_vertices, int64_t num_triangles, const tn_voxel_params *params,
                     float *positions_out, uint8_t *colors_out, float *temperature_out, uint8_t *thermal_colors_out,
                     int32_t *cluster_count, int64_t capacity_vertices, int32_t *triangles_out, int32_t *triangle_source,
                     int64_t capacity_triangles, int32_t *vertex_map, int64_t *counts, void *workspace, size_t workspace_bytes,
                     void *stream) {
    if (!params || !counts) return TN_ERR_NULL;
    if (bad_counts(num_vertices, num_triangles) || capacity_vertices < 0 || capacity_triangles < 0) return TN_ERR_SHAPE;
    if (voxel_params_unsupported(params)) return TN_ERR_UNSUPPORTED;
    if (num_vertices > 0 && (!positions || !colors || !temperature || !workspace)) return TN_ERR_NULL;
    if (num_triangles > 0 && !triangles) return TN_ERR_NULL;
    if (capacity_vertices > 0 && (!positions_out || !colors_out || !temperature_out || !cluster_count)) return TN_ERR_NULL;
    if (capacity_triangles > 0 && !triangles_out) return TN_ERR_NULL;
    if (thermal_colors_out && !thermal_colors) return TN_ERR_NULL;
    if (misaligned(positions, 4) || misaligned(temperature, 4) || misaligned(triangles, 4) || misaligned(positions_out, 4) ||
        misaligned(temperature_out, 4) || misaligned(cluster_count, 4) || misaligned(triangles_out, 4) ||
        misaligned(triangle_source, 4) || misaligned(vertex_map, 4) || misaligned(counts, 8) || misaligned(workspace, 8))
        return TN_ERR_SHAPE;
    if (workspace_bytes < tn_mesh_simplify_workspace_bytes(num_vertices, num_triangles)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long long nv = (long long)num_vertices, nt = (long long)num_triangles;
    if (hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s) != hipSuccess) return TN_ERR_LAUNCH;
    if (nv == 0) return TN_OK;
    if (nt == 0)  // no triangle, no used cluster: every vertex maps to -1 (all bits set)
        return !vertex_map || hipMemsetAsync(vertex_map, 0xff, (size_t)nv * sizeof(int32_t), s) == hipSuccess ? TN_OK : TN_ERR_LAUNCH;
    const VoxelGrid g = voxel_grid_of(params);
    const Layout l = layout_of(reinterpret_cast<char *>(workspace), nv, nt);
    long long *cnt = reinterpret_cast<long long *>(counts);
    const unsigned vertex_blocks = (unsigned)tiles_of(nv), triangle_blocks = (unsigned)tiles_of(nt);
    int code;

    // 1 - 3: the clusters
    hipLaunchKernelGGL(vertex_keys_kernel, dim3(vertex_blocks), dim3(kTile), 0, s, positions, nv, g, l.vertex_keys);
    TN_LAUNCH_CHECK();
    code = tn_sort_pairs(reinterpret_cast<const uint64_t *>(l.vertex_keys), nullptr, num_vertices, bit_length(g.total),
                         reinterpret_cast<uint64_t *>(l.vertex_sorted), l.vertex_order, l.sort, l.sort_bytes, stream);
    if (code != TN_OK) return code;
    hipLaunchKernelGGL(count_heads_kernel, dim3(vertex_blocks), dim3(kTile), 0, s, l.vertex_sorted, nv, g.total, l.vertex_tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kScan), 0, s, l.vertex_tiles, tiles_of(nv), l.clusters);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(emit_heads_kernel, dim3(vertex_blocks), dim3(kTile), 0, s, l.vertex_sorted, l.vertex_order, nv, g.total,
                       l.vertex_tiles, l.heads, l.rank);
    TN_LAUNCH_CHECK();

    // 4 - 5: the canonical triples, equal ones adjacent in ascending triangle index
    const bool two = two_sorts(nv);
    const int bits = bit_length((unsigned long long)nv);
    const Triples triples = {bits, l.triangle_keys[0], two ? l.triangle_keys[1] : nullptr, 1ull << ((two ? 2 : 3) * bits)};
    unsigned long long *dropped_count = reinterpret_cast<unsigned long long *>(cnt + 2);
    const unsigned long long *sorted;
    const int *order;
    if (two) {
        hipLaunchKernelGGL(triples_kernel<true>, dim3(triangle_blocks), dim3(kTile), 0, s, triangles, nt, nv, l.rank, triples, dropped_count);
        TN_LAUNCH_CHECK();
        code = tn_sort_pairs(reinterpret_cast<const uint64_t *>(triples.third), nullptr, num_triangles, bits,
                             reinterpret_cast<uint64_t *>(l.triangle_keys[2]), l.triangle_order[1], l.sort, l.sort_bytes, stream);
        if (code != TN_OK) return code;
        hipLaunchKernelGGL(gather_kernel, dim3(triangle_blocks), dim3(kTile), 0, s, triples.keys, l.triangle_order[1], nt, l.triangle_keys[3]);
        TN_LAUNCH_CHECK();
        code = tn_sort_pairs(reinterpret_cast<const uint64_t *>(l.triangle_keys[3]), l.triangle_order[1], num_triangles, 2 * bits + 1,
                             reinterpret_cast<uint64_t *>(l.triangle_keys[2]), l.triangle_order[0], l.sort, l.sort_bytes, stream);
        if (code != TN_OK) return code;
        sorted = l.triangle_keys[2];
    } else {
        hipLaunchKernelGGL(triples_kernel<false>, dim3(triangle_blocks), dim3(kTile), 0, s, triangles, nt, nv, l.rank, triples, dropped_count);
        TN_LAUNCH_CHECK();
        code = tn_sort_pairs(reinterpret_cast<const uint64_t *>(triples.keys), nullptr, num_triangles, 3 * bits + 1,
                             reinterpret_cast<uint64_t *>(l.triangle_keys[1]), l.triangle_order[0], l.sort, l.sort_bytes, stream);
        if (code != TN_OK) return code;
        sorted = l.triangle_keys[1];
    }
    order = l.triangle_order[0];

    // 6: kept triangles, used clusters
    if (hipMemsetAsync(l.used, 0, (size_t)nv * sizeof(int), s) != hipSuccess) return TN_ERR_LAUNCH;
    hipLaunchKernelGGL(flags_kernel, dim3(triangle_blocks), dim3(kTile), 0, s, sorted, order, triples.third, nt, triples.dropped, triangles,
                       nv, l.rank, l.kept, l.used);
    TN_LAUNCH_CHECK();

    // 7: the two compactions; the clusters' emit writes the vertices
    hipLaunchKernelGGL(count_flags_kernel, dim3(triangle_blocks), dim3(kTile), 0, s, l.kept, nt, nullptr, l.triangle_tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_kept_kernel, dim3(1), dim3(kScan), 0, s, l.triangle_tiles, tiles_of(nt), nt, cnt);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(count_flags_kernel, dim3(vertex_blocks), dim3(kTile), 0, s, l.used, nv, l.clusters, l.vertex_tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kScan), 0, s, l.vertex_tiles, tiles_of(nv), cnt);
    TN_LAUNCH_CHECK();
    const VoxelInputs in = {positions, temperature, colors, thermal_colors};
    const VoxelOutputs out = {positions_out, temperature_out, colors_out, thermal_colors_out, cluster_count};
    hipLaunchKernelGGL(emit_clusters_kernel, dim3(vertex_blocks), dim3(kTile), 0, s, l.used, nv, l.clusters, l.vertex_tiles, l.vertex_sorted,
                       l.vertex_order, l.heads, (long long)capacity_vertices, in, out, l.cluster_out);
    TN_LAUNCH_CHECK();

    // 8: the triangles and the map
    if (capacity_triangles > 0) {
        hipLaunchKernelGGL(emit_triangles_kernel, dim3(triangle_blocks), dim3(kTile), 0, s, l.kept, triangles, nt, nv, l.triangle_tiles, l.rank,
                           l.cluster_out, (long long)capacity_triangles, triangles_out, triangle_source);
        TN_LAUNCH_CHECK();
    }
    if (vertex_map) {
        hipLaunchKernelGGL(vertex_map_kernel, dim3(vertex_blocks), dim3(kTile), 0, s, l.rank, l.cluster_out, nv, vertex_map);
        TN_LAUNCH_CHECK();
    }
    return TN_OK;
}

}  // extern "C"
