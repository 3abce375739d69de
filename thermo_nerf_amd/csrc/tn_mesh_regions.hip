// Thermal regions of an indexed triangle list (DESIGN.md "Thermal regions"; include/thermonerf_hip.h defines every output to the
// bit): the faces whose temperature lies in a window, joined into regions through shared vertices, and per region the area, the
// area-weighted mean temperature and centroid, the extremes, the bounds and the hottest / coldest vertex.  Launches on the caller's
// stream (the steps marked * are tn_group_sum.h's, shared with tn_mesh_patches.hip):
//   1. faces        one thread per face: USABLE / SELECTED, the face record (area, area x temperature, area x centroid, the face's
//                   temperature, its box, its hottest and coldest corner), the masked triangle list (a face outside the window gets
//                   -1 indices), face_area; the tile counts of the usable and of the selected faces
//   2. lists *      the two scans -> counts[2], counts[1]; the usable and the selected faces compacted in face order
//   3. components   tn_mesh_components of the masked list: labels[v] = the smallest vertex of v's region
//   4. keys, sort   tn_sort_pairs of (label, 0 .. T-1), V for a face outside the window: a region's faces adjacent, in ascending face
//                   index, the regions in ascending label
//   5. heads *      count / scan / emit over the sorted positions: the region number r, counts[0] = R.  A region's faces are the
//                   distance to the next head, the last region's up to counts[1]
//   6. blocks *     count / scan / emit over the regions: where every region's 256-blocks start
//   7. assign       one thread per face: face_region; one thread per sorted position *: the head of every 256-block
//   8. block sums * ONE THREAD PER 256-BLOCK walks its faces' records through the sorted order into one partial record
//   9. regions      one thread per region walks its blocks' partials in block order * and writes the row
//  10. totals *     the same two levels over the two lists of step 2, areas only
// (6, 8 and 9 are skipped for the sizing call.)  No allocation, no host synchronisation, no float atomics, and no block ever waits for
// another.  A thread's sequential walk is 256 records, then n / 256 partials: a region of 10^6 faces is 3906 walks of 256 side by side,
// then one of 3906.
// The face record is 96 bytes, 16-byte aligned: six 16-byte loads per face of the walk, nothing else is gathered there (the corners'
// positions and temperatures were read once, in face order, by step 1).
#include "tn_device.h"
#include "tn_group_sum.h"

using namespace tn;

namespace {

constexpr int kTile = kFaceTile;  // faces / sorted positions / regions per thread block of every kernel but the scan

// the corner (index, temperature) joins the running hottest / coldest: compared as numbers, the lowest index on a tie
__device__ __forceinline__ void hotter(int &best, float &tbest, int i, float t) {
    if (best < 0 || t > tbest || (t == tbest && i < best)) best = i, tbest = t;
}
__device__ __forceinline__ void colder(int &best, float &tbest, int i, float t) {
    if (best < 0 || t < tbest || (t == tbest && i < best)) best = i, tbest = t;
}

// a face's record, a block's partial and a region's accumulator are one thing: five ordered sums and the order-free extremes
struct alignas(16) Acc {
    double s[5];           // area, area x temperature, area x centroid x / y / z
    float tmin, tmax;      // of the face temperatures
    float lo[3], hi[3];    // of the corners' positions
    int hot, cold;         // the hottest / coldest corner; -1: none yet
    float thot, tcold;     // their temperatures
    int pad[2];
    // a walk holds one record beside its accumulator (22 registers each): a second one in flight no longer fits the 64 registers of
    // 8 waves per SIMD, which both walking kernels have
    static constexpr int kAhead = 1;
    static __device__ __forceinline__ Acc empty() {
        Acc a;
#pragma unroll
        for (int k = 0; k < 5; ++k) a.s[k] = 0.0;
        a.tmin = INFINITY, a.tmax = -INFINITY;
#pragma unroll
        for (int k = 0; k < 3; ++k) a.lo[k] = INFINITY, a.hi[k] = -INFINITY;
        a.hot = a.cold = -1;
        a.thot = a.tcold = 0.0f;
        a.pad[0] = a.pad[1] = 0;
        return a;
    }
    // this joined by r, r behind everything this holds: the five sums take one rounded addition each
    __device__ __forceinline__ void join(const Acc &r) {
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] = __dadd_rn(s[k], r.s[k]);
        tmin = min_ord(tmin, r.tmin);
        tmax = max_ord(tmax, r.tmax);
#pragma unroll
        for (int k = 0; k < 3; ++k) lo[k] = min_ord(lo[k], r.lo[k]), hi[k] = max_ord(hi[k], r.hi[k]);
        if (r.hot >= 0) hotter(hot, thot, r.hot, r.thot);
        if (r.cold >= 0) colder(cold, tcold, r.cold, r.tcold);
    }
};
static_assert(sizeof(Acc) == 96, "six 16-byte loads");

constexpr int kUsable = 1, kSelected = 2;

__global__ void __launch_bounds__(kTile)
faces_kernel(const float *__restrict__ positions, const float *__restrict__ temperature, const int *__restrict__ triangles,
             long long num_vertices, long long num_triangles, float window_lo, float window_hi, Acc *__restrict__ records,
             int *__restrict__ masked, int *__restrict__ flags, double *__restrict__ face_area, FaceLists lists) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    bool usable = false, selected = false;
    if (t < num_triangles) {
        const Face f = load_face(positions, temperature, triangles, num_vertices, t);
        usable = f.placed && f.warm;
        if (usable) {
            selected = window_lo <= f.tf && f.tf <= window_hi;
            Acc r = Acc::empty();
            r.s[0] = f.area;
            r.s[1] = __dmul_rn(f.area, (double)f.tf);
            r.tmin = r.tmax = f.tf;
#pragma unroll
            for (int k = 0; k < 3; ++k) r.s[2 + k] = f.moment[k], r.lo[k] = f.lo[k], r.hi[k] = f.hi[k];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                hotter(r.hot, r.thot, (int)f.i[a], f.c[a]);
                colder(r.cold, r.tcold, (int)f.i[a], f.c[a]);
            }
            records[t] = r;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) masked[3 * t + a] = selected ? (int)f.i[a] : -1;
        flags[t] = (usable ? kUsable : 0) | (selected ? kSelected : 0);
        if (face_area) face_area[t] = usable ? f.area : 0.0;
    }
    count_lists(lists, (usable ? kUsable : 0) | (selected ? kSelected : 0));
}

// the label of a selected face is that of its first vertex; V is the key of every other face
__global__ void __launch_bounds__(kTile)
keys_kernel(const int *__restrict__ masked, const int *__restrict__ flags, long long num_triangles, long long num_vertices,
            const int *__restrict__ labels, unsigned long long *__restrict__ keys) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    if (t >= num_triangles) return;
    long long label = -1;
    if (flags[t] & kSelected) {
        const long long i0 = masked[3 * t];
        if (i0 >= 0 && i0 < num_vertices) label = labels[i0];
    }
    keys[t] = label >= 0 && label < num_vertices ? (unsigned long long)label : (unsigned long long)num_vertices;
}

// face t: face_region.  Sorted position t (with_blocks, once the blocks are placed): the head of a 256-block records where it starts
__global__ void __launch_bounds__(kTile)
assign_kernel(const unsigned long long *__restrict__ keys, Groups g, bool with_blocks, int *__restrict__ face_region) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    if (t >= g.num_triangles) return;
    const long long num_regions = groups_of(g);
    const unsigned long long key = keys[t];
    face_region[t] = key < (unsigned long long)g.labels ? group_of(g, (long long)key, num_regions) : -1;
    if (with_blocks) block_head(g, t, num_regions);
}

__global__ void __launch_bounds__(kTile)
regions_kernel(Groups g, const Acc *__restrict__ records, const Acc *__restrict__ partials, long long capacity,
               tn_mesh_region *__restrict__ regions) {
    const long long r = (long long)blockIdx.x * kTile + threadIdx.x;
    const long long num_regions = groups_of(g);
    if (r >= capacity || r >= num_regions) return;
    const long long faces = faces_of(g, r, num_regions);
    const Acc a = group_sum(g, r, faces, records, partials);
    tn_mesh_region out;
    out.area = a.s[0];
    out.label = (int32_t)g.label[r];
    out.faces = (int32_t)faces;
    const bool flat = a.s[0] == 0.0;
    out.mean_temperature = flat ? quiet_nan() : (float)__ddiv_rn(a.s[1], a.s[0]);
    out.min_temperature = a.tmin;
    out.max_temperature = a.tmax;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out.centroid[k] = flat ? quiet_nan() : (float)__ddiv_rn(a.s[2 + k], a.s[0]);
        out.bounds[k] = a.lo[k];
        out.bounds[3 + k] = a.hi[k];
    }
    out.coldest_vertex = a.cold;
    out.hottest_vertex = a.hot;
    regions[r] = out;
}

inline long long tiles_of(long long n) { return ceil_div(n, kTile); }

// the workspace, in order: the face records (16-byte aligned: up to 8 bytes of slack in front), the block partials, the totals'
// partials, the sort keys and the sorted keys, the number of blocks, tn_mesh_components' summary, two arrays of tile counts, then
// the int arrays per face (masked indices x 3, flags, two lists, order), per vertex (labels, component_triangles, of_label), per region
// (label, first_face, first_block) and per block (block_first), and the sort's own workspace
struct Layout {
    Acc *records, *partials;
    double *total_partials;
    unsigned long long *keys, *sorted;
    long long *num_blocks, *summary, *head_tiles, *block_tiles;
    int *masked, *flags, *order, *labels, *component_triangles;
    FaceLists lists;  // 0: the usable faces, counts[2] of them; 1: the selected faces, counts[1] of them
    Groups regions;   // the labels are vertices: L = V; a region has a face, and three vertices of its own: capacity = min(V / 3, T)
    void *sort;
    size_t sort_bytes, bytes;
};

inline Layout layout_of(char *ws, long long v, long long t, long long *counts) {
    Layout l;
    size_t at = ws ? (size_t)(reinterpret_cast<uintptr_t>(ws) % 16) : 8;  // ws is 8-byte aligned: 0 or 8; sized for 8
    const size_t skip = at;
    auto take = [&](size_t bytes) {  // (ws == NULL: the sizes alone)
        char *p = ws ? ws + at : nullptr;
        at += bytes;
        return p;
    };
    Groups &g = l.regions;
    g.num_triangles = t, g.labels = v;
    g.capacity = v / 3 < t ? v / 3 : t;
    g.direct = 0;                             // every region has its partials: the rows wait for no walk of 256 records
    g.max_blocks = tiles_of(t) + g.capacity;  // sum of ceil(faces / 256) <= T / 256 + R
    l.records = reinterpret_cast<Acc *>(take((size_t)t * sizeof(Acc)));
    l.partials = reinterpret_cast<Acc *>(take((size_t)g.max_blocks * sizeof(Acc)));
    l.total_partials = reinterpret_cast<double *>(take((size_t)(2 * ceil_div(t, kSumBlock)) * sizeof(double)));
    l.keys = reinterpret_cast<unsigned long long *>(take((size_t)t * sizeof(unsigned long long)));
    l.sorted = reinterpret_cast<unsigned long long *>(take((size_t)t * sizeof(unsigned long long)));
    l.num_blocks = reinterpret_cast<long long *>(take(sizeof(long long)));
    l.summary = reinterpret_cast<long long *>(take(3 * sizeof(long long)));
    for (auto &p : l.lists.tiles) p = reinterpret_cast<long long *>(take((size_t)tiles_of(t) * sizeof(long long)));
    // the lists are emitted before the regions are numbered, and the totals read the lists and their lengths alone: the two arrays
    // serve again for the heads (tiles of T) and the blocks (tiles of capacity <= T).  Two arrays of their own would make the workspace
    // of a mesh of many more faces than vertices larger than it was with the counts over the vertices (V = 8, T = 2^20: by 64 KiB)
    l.head_tiles = l.lists.tiles[0], l.block_tiles = l.lists.tiles[1];
    l.masked = reinterpret_cast<int *>(take(ints_bytes(3 * t)));
    int **per_face[4] = {&l.flags, &l.lists.faces[0], &l.lists.faces[1], &l.order};
    for (auto p : per_face) *p = reinterpret_cast<int *>(take(ints_bytes(t)));
    int **per_vertex[3] = {&l.labels, &l.component_triangles, &g.of_label};
    for (auto p : per_vertex) *p = reinterpret_cast<int *>(take(ints_bytes(v)));
    int **per_region[3] = {&g.label, &g.first_face, &g.first_block};
    for (auto p : per_region) *p = reinterpret_cast<int *>(take(ints_bytes(g.capacity)));
    g.block_first = reinterpret_cast<int *>(take(ints_bytes(g.max_blocks)));
    l.sort_bytes = tn_sort_pairs_workspace_bytes(t);
    l.sort = take(l.sort_bytes);
    l.bytes = at - skip + 8;
    l.lists.bit[0] = kUsable, l.lists.bit[1] = kSelected;
    l.lists.length[0] = counts ? counts + 2 : nullptr, l.lists.length[1] = counts ? counts + 1 : nullptr;
    g.sorted = l.sorted, g.order = l.order, g.counts = counts, g.num_blocks = l.num_blocks;
    return l;
}

}  // namespace

extern "C" {

size_t tn_mesh_regions_workspace_bytes(int64_t num_vertices, int64_t num_triangles) {
    if (bad_counts(num_vertices, num_triangles)) return 0;
    return layout_of(nullptr, (long long)num_vertices, (long long)num_triangles, nullptr).bytes;
}

int tn_mesh_regions(const float *positions, const float *temperature, const int32_t *triangles, int64_t num_vertices,
                    int64_t num_triangles, float min_temperature, float max_temperature, tn_mesh_region *regions,
                    int64_t capacity_regions, int32_t *face_region, double *face_area, int64_t *counts, double *totals,
                    void *workspace, size_t workspace_bytes, void *stream) {
    if (!counts || !totals) return TN_ERR_NULL;
    if (bad_counts(num_vertices, num_triangles) || capacity_regions < 0) return TN_ERR_SHAPE;
    if (min_temperature != min_temperature || max_temperature != max_temperature) return TN_ERR_UNSUPPORTED;
    const bool work = num_vertices > 0 && num_triangles > 0;
    if (work && (!positions || !temperature || !workspace)) return TN_ERR_NULL;
    if (num_triangles > 0 && (!triangles || !face_region)) return TN_ERR_NULL;
    if (capacity_regions > 0 && !regions) return TN_ERR_NULL;
    if (misaligned(positions, 4) || misaligned(temperature, 4) || misaligned(triangles, 4) || misaligned(face_region, 4) ||
        misaligned(regions, 8) || misaligned(face_area, 8) || misaligned(counts, 8) || misaligned(totals, 8) || misaligned(workspace, 8))
        return TN_ERR_SHAPE;
    if (work && workspace_bytes < tn_mesh_regions_workspace_bytes(num_vertices, num_triangles)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long long nv = (long long)num_vertices, nt = (long long)num_triangles;
    if (!work) {
        if (hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), s) != hipSuccess) return TN_ERR_LAUNCH;
        if (hipMemsetAsync(totals, 0, 2 * sizeof(double), s) != hipSuccess) return TN_ERR_LAUNCH;
        if (nt > 0 && hipMemsetAsync(face_region, 0xff, (size_t)nt * sizeof(int32_t), s) != hipSuccess) return TN_ERR_LAUNCH;
        if (nt > 0 && face_area && hipMemsetAsync(face_area, 0, (size_t)nt * sizeof(double), s) != hipSuccess) return TN_ERR_LAUNCH;
        return TN_OK;
    }
    const Layout l = layout_of(reinterpret_cast<char *>(workspace), nv, nt, reinterpret_cast<long long *>(counts));
    const Groups &g = l.regions;
    const unsigned face_blocks = (unsigned)tiles_of(nt);
    const bool rows = capacity_regions > 0 && g.capacity > 0;  // (fewer than three vertices: no region, and no launch of no block)
    const long long cap = (long long)capacity_regions;
    int code;

    // 1 - 2: the faces, the two counts, the two lists
    hipLaunchKernelGGL(faces_kernel, dim3(face_blocks), dim3(kTile), 0, s, positions, temperature, triangles, nv, nt, min_temperature,
                       max_temperature, l.records, l.masked, l.flags, face_area, l.lists);
    TN_LAUNCH_CHECK();
    if ((code = list_faces(l.lists, l.flags, nt, s)) != TN_OK) return code;

    // 3 - 5: the labels of the selected faces; a region's faces adjacent in ascending face index; the regions numbered in ascending label
    code = tn_mesh_components(l.masked, num_triangles, num_vertices, l.labels, l.component_triangles,
                              reinterpret_cast<int64_t *>(l.summary), stream);
    if (code != TN_OK) return code;
    hipLaunchKernelGGL(keys_kernel, dim3(face_blocks), dim3(kTile), 0, s, l.masked, l.flags, nt, nv, l.labels, l.keys);
    TN_LAUNCH_CHECK();
    code = tn_sort_pairs(reinterpret_cast<const uint64_t *>(l.keys), nullptr, num_triangles, key_bits((unsigned long long)nv),  // 0 .. V
                         reinterpret_cast<uint64_t *>(l.sorted), l.order, l.sort, l.sort_bytes, stream);
    if (code != TN_OK) return code;
    if ((code = number_groups(g, l.head_tiles, s)) != TN_OK) return code;

    // 6 - 7: where the blocks start; face_region
    if (rows && (code = place_blocks(g, l.block_tiles, s)) != TN_OK) return code;
    hipLaunchKernelGGL(assign_kernel, dim3(face_blocks), dim3(kTile), 0, s, l.keys, g, rows, face_region);
    TN_LAUNCH_CHECK();

    // 8 - 9: the block partials, the regions' rows
    if (rows) {
        if ((code = sum_blocks(g, cap, l.records, l.partials, s)) != TN_OK) return code;
        hipLaunchKernelGGL(regions_kernel, dim3((unsigned)tiles_of(cap < g.capacity ? cap : g.capacity)), dim3(kTile), 0, s, g, l.records,
                           l.partials, cap, regions);
        TN_LAUNCH_CHECK();
    }

    // 10: the mesh's area and the selected area
    return list_totals(l.lists, nt, l.records, l.total_partials, totals, s);
}

}  // extern "C"
