// Connected components of an indexed triangle list, and the removal of small ones (DESIGN.md "Mesh export": components).  The
// labels, the per-component triangle counts, the summary and the filtered mesh are integers defined to the bit
// (include/thermonerf_hip.h): a label is the SMALLEST vertex index of its component, kept vertices and triangles keep their input
// order.  Connectivity is VERTEX connectivity — two triangles that share one vertex are one component — which is what makes a
// floater that touches the wall part of the wall, and what an indexed list gives for nothing: a triangle unites its three indices.
//
// tn_mesh_components, at most six plain launches:
//   1. init       parent[v] <- v (parent IS `labels`), component_triangles[v] <- 0, summary <- 0
//   2. hook       one thread per valid triangle unites (v0, v1) and (v1, v2) in a lock-free union-find
//   3. flatten    labels[v] <- the root of v
//   4. count      one thread per valid triangle: component_triangles[labels[v0]] += 1 (integer atomicAdd, one per wave and label
//                 where the lanes agree with the wave's first valid lane)
//   5. summarise  one thread per vertex: roots are counted (block_rank's total, one integer atomicAdd per block) and bid
//                 (count << 32) | (0x7fffffff - label) in ONE 64-bit atomicMax per wave: the largest count, the lowest label on a tie
//   6. unpack     one thread: the winning bid -> summary[1], summary[2]
// (2 - 4 are skipped when there is no triangle.)  tn_mesh_filter_components, six plain launches: the ordered count / scan / emit
// of tn_mesh.hip twice, on tn_scan.h — vertices (which also leaves vertex_map[v] = new index or -1 in the workspace), then
// triangles.  Integer atomics only; no allocation, no host synchronisation, and NO block ever waits for another block (no
// spinning on another thread's progress, no grid barrier, no cooperative launch).  Nothing in any output depends on the order in
// which threads arrive: the union-find's TREE does, its roots do not, and sums and maxima of integers are exact in any order.
//
// THE UNION-FIND (load_parent / find_root / unite, with the proof that every walk ends, that a stale read is harmless and that the
// root is the smallest index of its tree) is tn_union_find.h, shared with tn_mesh_patches.hip.  After the hook kernel every valid
// triangle's vertices share a root, and no two components were ever joined without a triangle.
#include "tn_device.h"
#include "tn_scan.h"
#include "tn_union_find.h"

using namespace tn;

namespace {

constexpr int kTile = 256;  // vertices / triangles per tile = threads per block of every kernel but the scan (tn_mesh_tile())

__device__ __forceinline__ bool valid_triangle(const int *__restrict__ tri, long long t, int num_vertices, int (&v)[3]) {
    v[0] = tri[3 * t], v[1] = tri[3 * t + 1], v[2] = tri[3 * t + 2];
    const unsigned n = (unsigned)num_vertices;
    return (unsigned)v[0] < n && (unsigned)v[1] < n && (unsigned)v[2] < n;
}

__global__ void __launch_bounds__(kTile)
init_kernel(int num_vertices, int *__restrict__ parent, int *__restrict__ component_triangles, long long *__restrict__ summary) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    if (v < 3) summary[v] = 0;
    if (v >= num_vertices) return;
    parent[v] = (int)v;
    component_triangles[v] = 0;
}

__global__ void __launch_bounds__(kTile)
hook_kernel(const int *__restrict__ tri, long long num_triangles, int num_vertices, int *parent) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    int v[3];
    if (t >= num_triangles || !valid_triangle(tri, t, num_vertices, v)) return;
    if (v[0] != v[1]) unite(parent, v[0], v[1]);
    if (v[1] != v[2]) unite(parent, v[1], v[2]);
}

__global__ void __launch_bounds__(kTile)
flatten_kernel(int num_vertices, int *labels) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    if (v >= num_vertices) return;
    int x = (int)v, p = labels[x];
    while (p != x) {
        x = p;
        p = labels[x];
    }
    if (x != (int)v) labels[v] = x;
}

__global__ void __launch_bounds__(kTile)
count_kernel(const int *__restrict__ tri, long long num_triangles, int num_vertices, const int *__restrict__ labels,
             int *__restrict__ component_triangles) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    int v[3];
    const bool valid = t < num_triangles && valid_triangle(tri, t, num_vertices, v);
    const int label = valid ? labels[v[0]] : -1;
    // neighbouring triangles mostly share a label: the lanes that agree with the wave's first valid lane add once, together
    const unsigned long long valid_mask = __ballot(valid);
    if (valid_mask == 0ull) return;
    const int leader = __ffsll((long long)valid_mask) - 1;
    const int leader_label = __shfl(label, leader, TN_WAVE);
    const bool same = valid && label == leader_label;
    const unsigned long long same_mask = __ballot(same);
    if ((int)(threadIdx.x % TN_WAVE) == leader) atomicAdd(component_triangles + label, (int)__popcll(same_mask));
    else if (valid && !same) atomicAdd(component_triangles + label, 1);
}

__global__ void __launch_bounds__(kTile)
summarise_kernel(int num_vertices, const int *__restrict__ labels, const int *__restrict__ component_triangles,
                 unsigned long long *__restrict__ summary) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    const bool root = v < num_vertices && labels[v] == (int)v;
    uint32_t roots;
    block_rank<kTile>(root, roots);
    if (threadIdx.x == 0 && roots) atomicAdd(summary, (unsigned long long)roots);
    unsigned long long bid = root ? (unsigned long long)(uint32_t)component_triangles[v] << 32 | (uint32_t)(0x7fffffff - (int)v) : 0ull;
#pragma unroll
    for (int o = TN_WAVE / 2; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(bid, o, TN_WAVE);
        bid = other > bid ? other : bid;
    }
    if (threadIdx.x % TN_WAVE == 0 && bid) atomicMax(summary + 1, bid);
}

__global__ void unpack_kernel(long long *__restrict__ summary) {
    const unsigned long long bid = (unsigned long long)summary[1];  // 0 only when V == 0, which launches nothing
    summary[1] = (long long)(bid >> 32);
    summary[2] = (long long)(0x7fffffff - (int)(uint32_t)bid);
}

// ---- the filter ----------------------------------------------------------------------------------------------------------------

struct Keep {
    const int *component_triangles;
    const long long *summary;  // NULL: largest_only is off
    long long min_triangles;   // already max(min_triangles, 1)
    __device__ __forceinline__ bool operator()(int label) const {
        return (long long)component_triangles[label] >= min_triangles && (!summary || (long long)label == summary[2]);
    }
};

__global__ void __launch_bounds__(kTile)
count_vertices_kernel(int num_vertices, const int *__restrict__ labels, Keep keep, long long *__restrict__ tiles) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    uint32_t total;
    block_rank<kTile>(v < num_vertices && keep(labels[v]), total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = (long long)total;
}

__global__ void __launch_bounds__(kScan)
scan_kernel(long long *__restrict__ tiles, long long num_tiles, long long *__restrict__ count) {
    scan_tiles<false>(tiles, num_tiles, count);  // a pass sums at most kScan * kTile = 2^18
}

__global__ void __launch_bounds__(kTile)
emit_vertices_kernel(int num_vertices, const int *__restrict__ labels, Keep keep, const long long *__restrict__ tiles,
                     int *__restrict__ vertex_map, int *__restrict__ vertex_source, long long capacity) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    const bool kept = v < num_vertices && keep(labels[v]);
    uint32_t total;
    const uint32_t rank = block_rank<kTile>(kept, total);
    if (v >= num_vertices) return;
    if (!kept) {
        vertex_map[v] = -1;
        return;
    }
    const long long dst = tiles[blockIdx.x] + (long long)rank;  // < V <= 2^31 - 1
    vertex_map[v] = (int)dst;
    if (dst < capacity) vertex_source[dst] = (int)v;
}

__global__ void __launch_bounds__(kTile)
count_triangles_kernel(const int *__restrict__ tri, long long num_triangles, int num_vertices, const int *__restrict__ labels,
                       Keep keep, long long *__restrict__ tiles) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    int v[3];
    uint32_t total;
    block_rank<kTile>(t < num_triangles && valid_triangle(tri, t, num_vertices, v) && keep(labels[v[0]]), total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = (long long)total;
}

__global__ void __launch_bounds__(kTile)
emit_triangles_kernel(const int *__restrict__ tri, long long num_triangles, int num_vertices, const int *__restrict__ labels,
                      Keep keep, const long long *__restrict__ tiles, const int *__restrict__ vertex_map,
                      int *__restrict__ triangles_out, long long capacity) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    int v[3];
    const bool kept = t < num_triangles && valid_triangle(tri, t, num_vertices, v) && keep(labels[v[0]]);
    uint32_t total;
    const uint32_t rank = block_rank<kTile>(kept, total);
    if (!kept) return;
    const long long dst = tiles[blockIdx.x] + (long long)rank;
    if (dst >= capacity) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) triangles_out[3 * dst + c] = vertex_map[v[c]];  // the three share a label: all kept
}

inline long long tiles_of(long long items) { return ceil_div(items, kTile); }

inline size_t map_bytes(long long num_vertices) { return ((size_t)num_vertices * sizeof(int) + 7) / 8 * 8; }

inline bool bad_count(int64_t n) { return n < 0 || n > 0x7fffffffLL; }

}  // namespace

extern "C" {

size_t tn_mesh_components_workspace_bytes(int64_t num_vertices, int64_t num_triangles) {
    if (bad_count(num_vertices) || bad_count(num_triangles)) return 0;
    return map_bytes(num_vertices) + (size_t)(tiles_of(num_vertices) + tiles_of(num_triangles)) * sizeof(long long);
}

int tn_mesh_components(const int32_t *triangles, int64_t num_triangles, int64_t num_vertices, int32_t *labels,
                       int32_t *component_triangles, int64_t *summary, void *stream) {
    if (!summary) return TN_ERR_NULL;
    if (num_vertices > 0 && (!labels || !component_triangles)) return TN_ERR_NULL;
    if (num_triangles > 0 && !triangles) return TN_ERR_NULL;
    if (bad_count(num_vertices) || bad_count(num_triangles)) return TN_ERR_SHAPE;
    if (misaligned(triangles, 4) || misaligned(labels, 4) || misaligned(component_triangles, 4) || misaligned(summary, 8))
        return TN_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    if (num_vertices == 0) return hipMemsetAsync(summary, 0, 3 * sizeof(int64_t), s) == hipSuccess ? TN_OK : TN_ERR_LAUNCH;
    const int nv = (int)num_vertices;
    const long long nt = (long long)num_triangles;
    const unsigned vertex_tiles = (unsigned)tiles_of(nv), triangle_tiles = (unsigned)tiles_of(nt);
    long long *sum = reinterpret_cast<long long *>(summary);
    hipLaunchKernelGGL(init_kernel, dim3(vertex_tiles), dim3(kTile), 0, s, nv, labels, component_triangles, sum);
    TN_LAUNCH_CHECK();
    if (nt > 0) {
        hipLaunchKernelGGL(hook_kernel, dim3(triangle_tiles), dim3(kTile), 0, s, triangles, nt, nv, labels);
        TN_LAUNCH_CHECK();
        hipLaunchKernelGGL(flatten_kernel, dim3(vertex_tiles), dim3(kTile), 0, s, nv, labels);
        TN_LAUNCH_CHECK();
        hipLaunchKernelGGL(count_kernel, dim3(triangle_tiles), dim3(kTile), 0, s, triangles, nt, nv, labels, component_triangles);
        TN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(summarise_kernel, dim3(vertex_tiles), dim3(kTile), 0, s, nv, labels, component_triangles,
                       reinterpret_cast<unsigned long long *>(summary));
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(unpack_kernel, dim3(1), dim3(1), 0, s, sum);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

int tn_mesh_filter_components(const int32_t *triangles, int64_t num_triangles, int64_t num_vertices, const int32_t *labels,
                              const int32_t *component_triangles, const int64_t *summary, int64_t min_triangles,
                              int32_t largest_only, int32_t *vertex_source, int64_t capacity_vertices, int32_t *triangles_out,
                              int64_t capacity_triangles, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream) {
    if (!counts) return TN_ERR_NULL;
    if (num_vertices > 0 && (!labels || !component_triangles || !workspace)) return TN_ERR_NULL;
    if (num_triangles > 0 && !triangles) return TN_ERR_NULL;
    if (capacity_vertices > 0 && !vertex_source) return TN_ERR_NULL;
    if (capacity_triangles > 0 && !triangles_out) return TN_ERR_NULL;
    if (largest_only && !summary) return TN_ERR_NULL;
    if (capacity_vertices < 0 || capacity_triangles < 0 || min_triangles < 0) return TN_ERR_SHAPE;
    if (bad_count(num_vertices) || bad_count(num_triangles)) return TN_ERR_SHAPE;
    if (misaligned(triangles, 4) || misaligned(labels, 4) || misaligned(component_triangles, 4) || misaligned(summary, 8) ||
        misaligned(vertex_source, 4) || misaligned(triangles_out, 4) || misaligned(counts, 8) || misaligned(workspace, 8))
        return TN_ERR_SHAPE;
    if (workspace_bytes < tn_mesh_components_workspace_bytes(num_vertices, num_triangles)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (num_vertices == 0) return hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s) == hipSuccess ? TN_OK : TN_ERR_LAUNCH;
    const int nv = (int)num_vertices;
    const long long nt = (long long)num_triangles;
    const long long vertex_tiles_n = tiles_of(nv), triangle_tiles_n = tiles_of(nt);
    int *vertex_map = reinterpret_cast<int *>(workspace);
    long long *vertex_tiles = reinterpret_cast<long long *>(reinterpret_cast<char *>(workspace) + map_bytes(nv));
    long long *triangle_tiles = vertex_tiles + vertex_tiles_n;
    long long *cnt = reinterpret_cast<long long *>(counts);
    const Keep keep = {component_triangles, largest_only ? reinterpret_cast<const long long *>(summary) : nullptr,
                       min_triangles > 1 ? (long long)min_triangles : 1LL};
    hipLaunchKernelGGL(count_vertices_kernel, dim3((unsigned)vertex_tiles_n), dim3(kTile), 0, s, nv, labels, keep, vertex_tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kScan), 0, s, vertex_tiles, vertex_tiles_n, cnt);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(emit_vertices_kernel, dim3((unsigned)vertex_tiles_n), dim3(kTile), 0, s, nv, labels, keep, vertex_tiles,
                       vertex_map, vertex_source, (long long)capacity_vertices);
    TN_LAUNCH_CHECK();
    if (nt > 0) {
        hipLaunchKernelGGL(count_triangles_kernel, dim3((unsigned)triangle_tiles_n), dim3(kTile), 0, s, triangles, nt, nv, labels,
                           keep, triangle_tiles);
        TN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kScan), 0, s, triangle_tiles, triangle_tiles_n, cnt + 1);
    TN_LAUNCH_CHECK();
    if (nt > 0) {
        hipLaunchKernelGGL(emit_triangles_kernel, dim3((unsigned)triangle_tiles_n), dim3(kTile), 0, s, triangles, nt, nv, labels,
                           keep, triangle_tiles, vertex_map, triangles_out, (long long)capacity_triangles);
        TN_LAUNCH_CHECK();
    }
    return TN_OK;
}

}  // extern "C"
