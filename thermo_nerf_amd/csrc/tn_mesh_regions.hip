// Thermal regions of an indexed triangle list (DESIGN.md "Thermal regions"; include/thermonerf_hip.h defines every output to the
// bit): the faces whose temperature lies in a window, joined into regions through shared vertices, and per region the area, the
// area-weighted mean temperature and centroid, the extremes, the bounds and the hottest / coldest vertex.  Launches on the caller's
// stream:
//   1. faces        one thread per face: USABLE / SELECTED, the face record (area, area x temperature, area x centroid, the face's
//                   temperature, its box, its hottest and coldest corner), the masked triangle list (a face outside the window gets
//                   -1 indices), face_area; the tile counts of the usable and of the selected faces
//   2. scan         one block: the two exclusive scans -> counts[2], counts[1]
//   3. lists        the usable and the selected faces compacted in face order (the two lists of `totals`)
//   4. components   tn_mesh_components of the masked list: labels[v] = the smallest vertex of v's region, component_triangles[root] =
//                   the region's faces
//   5. roots        count / scan / emit over the vertices of the roots that own a face: the region number r, where the region's
//                   faces start in the sorted order (the exclusive sum of the faces) and where its 256-blocks start (the exclusive
//                   sum of ceil(faces / 256)); counts[0] = R
//   6. keys         one thread per face: face_region, and the sort key (the label; V for a face outside the window)
//   7. sort         tn_sort_pairs of (key, 0 .. T-1): a region's faces adjacent, in ascending face index
//   8. blocks       one thread per sorted position: the head of every 256-block records where it starts
//   9. block sums   ONE THREAD PER 256-BLOCK walks its faces' records through the sorted order into one partial record
//  10. regions      one thread per region walks its blocks' partials in block order and writes the row
//  11. totals       the same two levels over the two lists of step 3, areas only
// No allocation, no host synchronisation, no float atomics, and no block ever waits for another.  A thread's sequential walk is 256
// records, then n / 256 partials: a region of 10^6 faces is 3906 walks of 256 side by side, then one of 3906.
// The face record is 96 bytes, 16-byte aligned: six 16-byte loads per face of the walk, nothing else is gathered there (the corners'
// positions and temperatures were read once, in face order, by step 1).
#include "tn_device.h"
#include "tn_scan.h"

using namespace tn;

namespace {

constexpr int kTile = 256;   // faces / vertices / sorted positions / blocks / regions per thread block of every kernel but the scan
constexpr int kBlock = 256;  // entries per block of SUM2

// a face's record, a block's partial and a region's accumulator are one thing: five ordered sums and the order-free extremes
struct alignas(16) Acc {
    double s[5];           // area, area x temperature, area x centroid x / y / z
    float tmin, tmax;      // of the face temperatures
    float lo[3], hi[3];    // of the corners' positions
    int hot, cold;         // the hottest / coldest corner; -1: none yet
    float thot, tcold;     // their temperatures
    int pad[2];
};
static_assert(sizeof(Acc) == 96, "six 16-byte loads");

__device__ __forceinline__ Acc acc_empty() {
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

// the total order of the extremes: the numbers' order with -0.0 below +0.0 (so that a minimum does not depend on who came first)
__device__ __forceinline__ float lower_of(float a, float b) { return f2key(b) < f2key(a) ? b : a; }
__device__ __forceinline__ float higher_of(float a, float b) { return f2key(b) > f2key(a) ? b : a; }

// the corner (index, temperature) joins the running hottest / coldest: compared as numbers, the lowest index on a tie
__device__ __forceinline__ void hotter(int &best, float &tbest, int i, float t) {
    if (best < 0 || t > tbest || (t == tbest && i < best)) best = i, tbest = t;
}
__device__ __forceinline__ void colder(int &best, float &tbest, int i, float t) {
    if (best < 0 || t < tbest || (t == tbest && i < best)) best = i, tbest = t;
}

// a <- a joined by r, r behind everything a holds: the five sums take one rounded addition each
__device__ __forceinline__ void acc_join(Acc &a, const Acc &r) {
#pragma unroll
    for (int k = 0; k < 5; ++k) a.s[k] = __dadd_rn(a.s[k], r.s[k]);
    a.tmin = lower_of(a.tmin, r.tmin);
    a.tmax = higher_of(a.tmax, r.tmax);
#pragma unroll
    for (int k = 0; k < 3; ++k) a.lo[k] = lower_of(a.lo[k], r.lo[k]), a.hi[k] = higher_of(a.hi[k], r.hi[k]);
    if (r.hot >= 0) hotter(a.hot, a.thot, r.hot, r.thot);
    if (r.cold >= 0) colder(a.cold, a.tcold, r.cold, r.tcold);
}

constexpr int kUsable = 1, kSelected = 2;

__global__ void __launch_bounds__(kTile)
faces_kernel(const float *__restrict__ positions, const float *__restrict__ temperature, const int *__restrict__ triangles,
             long long num_vertices, long long num_triangles, float window_lo, float window_hi, Acc *__restrict__ records,
             int *__restrict__ masked, int *__restrict__ flags, double *__restrict__ face_area, long long *__restrict__ usable_tiles,
             long long *__restrict__ selected_tiles) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    bool usable = false, selected = false;
    if (t < num_triangles) {
        const long long i[3] = {triangles[3 * t], triangles[3 * t + 1], triangles[3 * t + 2]};
        bool ok = i[0] >= 0 && i[0] < num_vertices && i[1] >= 0 && i[1] < num_vertices && i[2] >= 0 && i[2] < num_vertices;
        ok = ok && i[0] != i[1] && i[1] != i[2] && i[0] != i[2];
        float p[3][3], c[3];
        if (ok) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                c[a] = temperature[i[a]];
                ok = ok && finite(c[a]);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    p[a][k] = positions[3 * i[a] + k];
                    ok = ok && finite(p[a][k]);
                }
            }
        }
        usable = ok;
        double area = 0.0;
        if (usable) {
            const float tf = (float)__ddiv_rn(__dadd_rn(__dadd_rn((double)c[0], (double)c[1]), (double)c[2]), 3.0);
            selected = window_lo <= tf && tf <= window_hi;
            double e1[3], e2[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                e1[k] = __dsub_rn((double)p[1][k], (double)p[0][k]);
                e2[k] = __dsub_rn((double)p[2][k], (double)p[0][k]);
            }
            const double cx = __dsub_rn(__dmul_rn(e1[1], e2[2]), __dmul_rn(e1[2], e2[1]));
            const double cy = __dsub_rn(__dmul_rn(e1[2], e2[0]), __dmul_rn(e1[0], e2[2]));
            const double cz = __dsub_rn(__dmul_rn(e1[0], e2[1]), __dmul_rn(e1[1], e2[0]));
            const double n2 = __dadd_rn(__dadd_rn(__dmul_rn(cx, cx), __dmul_rn(cy, cy)), __dmul_rn(cz, cz));
            area = __dmul_rn(0.5, __dsqrt_rn(n2));
            Acc r = acc_empty();
            r.s[0] = area;
            r.s[1] = __dmul_rn(area, (double)tf);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double centre = __ddiv_rn(__dadd_rn(__dadd_rn((double)p[0][k], (double)p[1][k]), (double)p[2][k]), 3.0);
                r.s[2 + k] = __dmul_rn(area, centre);
            }
            r.tmin = r.tmax = tf;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int k = 0; k < 3; ++k) r.lo[k] = lower_of(r.lo[k], p[a][k]), r.hi[k] = higher_of(r.hi[k], p[a][k]);
                hotter(r.hot, r.thot, (int)i[a], c[a]);
                colder(r.cold, r.tcold, (int)i[a], c[a]);
            }
            records[t] = r;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) masked[3 * t + a] = selected ? (int)i[a] : -1;
        flags[t] = (usable ? kUsable : 0) | (selected ? kSelected : 0);
        if (face_area) face_area[t] = area;
    }
    uint32_t total;
    block_rank<kTile>(usable, total);
    if (threadIdx.x == 0) usable_tiles[blockIdx.x] = (long long)total;
    __syncthreads();  // block_rank's LDS is rewritten by the second call
    block_rank<kTile>(selected, total);
    if (threadIdx.x == 0) selected_tiles[blockIdx.x] = (long long)total;
}

__global__ void __launch_bounds__(kScan)
scan_faces_kernel(long long *__restrict__ usable_tiles, long long *__restrict__ selected_tiles, long long num_tiles,
                  long long *__restrict__ counts) {
    scan_tiles<false>(usable_tiles, num_tiles, counts + 2);
    __syncthreads();
    scan_tiles<false>(selected_tiles, num_tiles, counts + 1);
}

__global__ void __launch_bounds__(kTile)
lists_kernel(const int *__restrict__ flags, long long num_triangles, const long long *__restrict__ usable_tiles,
             const long long *__restrict__ selected_tiles, int *__restrict__ usable_list, int *__restrict__ selected_list) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    const int f = t < num_triangles ? flags[t] : 0;
    uint32_t unused;
    const uint32_t before_usable = block_rank<kTile>((f & kUsable) != 0, unused);
    __syncthreads();
    const uint32_t before_selected = block_rank<kTile>((f & kSelected) != 0, unused);
    if (f & kUsable) {
        const long long o = usable_tiles[blockIdx.x] + (long long)before_usable;  // <= t
        if (o >= 0 && o < num_triangles) usable_list[o] = (int)t;
    }
    if (f & kSelected) {
        const long long o = selected_tiles[blockIdx.x] + (long long)before_selected;
        if (o >= 0 && o < num_triangles) selected_list[o] = (int)t;
    }
}

// a vertex is the ROOT of a region iff it is its own label and owns a face
__device__ __forceinline__ int root_faces(const int *__restrict__ labels, const int *__restrict__ component_triangles, long long v,
                                          long long num_vertices) {
    if (v >= num_vertices || labels[v] != (int)v) return 0;
    const int n = component_triangles[v];
    return n > 0 ? n : 0;
}

__device__ __forceinline__ uint32_t blocks_of(int faces) { return ((uint32_t)faces + kBlock - 1) / kBlock; }

__global__ void __launch_bounds__(kTile)
count_roots_kernel(const int *__restrict__ labels, const int *__restrict__ component_triangles, long long num_vertices,
                   long long *__restrict__ region_tiles, long long *__restrict__ face_tiles, long long *__restrict__ block_tiles) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    const int n = root_faces(labels, component_triangles, v, num_vertices);
    uint32_t regions, faces, blocks;
    block_rank<kTile>(n > 0, regions);
    block_exclusive<kTile>((uint32_t)n, faces);
    __syncthreads();  // block_exclusive's LDS is rewritten by the second call
    block_exclusive<kTile>(blocks_of(n), blocks);
    if (threadIdx.x == 0) {
        region_tiles[blockIdx.x] = (long long)regions;
        face_tiles[blockIdx.x] = (long long)faces;
        block_tiles[blockIdx.x] = (long long)blocks;
    }
}

// the three sums stay below 2^32 in every pass: R <= T, the faces <= T, the blocks <= T / 256 + R
__global__ void __launch_bounds__(kScan)
scan_roots_kernel(long long *__restrict__ region_tiles, long long *__restrict__ face_tiles, long long *__restrict__ block_tiles,
                  long long num_tiles, long long *__restrict__ counts, long long *__restrict__ sums) {
    scan_tiles<false>(region_tiles, num_tiles, counts);
    __syncthreads();
    scan_tiles<false>(face_tiles, num_tiles, sums);
    __syncthreads();
    scan_tiles<false>(block_tiles, num_tiles, sums + 1);
}

struct Regions {  // per root vertex: its region; per region: its label, where its faces and its blocks start
    int *of_root, *label, *first_face, *first_block;
    long long capacity;  // rows of the three per-region arrays
};

__global__ void __launch_bounds__(kTile)
emit_roots_kernel(const int *__restrict__ labels, const int *__restrict__ component_triangles, long long num_vertices,
                  const long long *__restrict__ region_tiles, const long long *__restrict__ face_tiles,
                  const long long *__restrict__ block_tiles, Regions out) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    const int n = root_faces(labels, component_triangles, v, num_vertices);
    uint32_t unused;
    const uint32_t regions_before = block_rank<kTile>(n > 0, unused);
    const uint32_t faces_before = block_exclusive<kTile>((uint32_t)n, unused);
    __syncthreads();
    const uint32_t blocks_before = block_exclusive<kTile>(blocks_of(n), unused);
    if (v >= num_vertices) return;
    const long long r = region_tiles[blockIdx.x] + (long long)regions_before;
    const bool root = n > 0 && r >= 0 && r < out.capacity;
    out.of_root[v] = root ? (int)r : -1;
    if (!root) return;
    out.label[r] = (int)v;
    out.first_face[r] = (int)(face_tiles[blockIdx.x] + (long long)faces_before);
    out.first_block[r] = (int)(block_tiles[blockIdx.x] + (long long)blocks_before);
}

// the region of a label, or -1; checks what it reads
__device__ __forceinline__ int region_of(const Regions &g, long long label, long long num_vertices) {
    if (label < 0 || label >= num_vertices) return -1;
    const int r = g.of_root[label];
    return r >= 0 && r < g.capacity ? r : -1;
}

__global__ void __launch_bounds__(kTile)
keys_kernel(const int *__restrict__ masked, const int *__restrict__ flags, long long num_triangles, long long num_vertices,
            const int *__restrict__ labels, Regions g, int *__restrict__ face_region, unsigned long long *__restrict__ keys) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    if (t >= num_triangles) return;
    long long label = -1;
    int r = -1;
    if (flags[t] & kSelected) {
        const long long i0 = masked[3 * t];
        if (i0 >= 0 && i0 < num_vertices) label = labels[i0];
        r = region_of(g, label, num_vertices);
    }
    face_region[t] = r;
    keys[t] = r >= 0 ? (unsigned long long)label : (unsigned long long)num_vertices;
}

// sorted position j starts block (j - first face) / 256 of its region iff that is a whole number
__global__ void __launch_bounds__(kTile)
block_heads_kernel(const unsigned long long *__restrict__ sorted, long long num_triangles, long long num_vertices, Regions g,
                   long long max_blocks, int *__restrict__ block_first) {
    const long long j = (long long)blockIdx.x * kTile + threadIdx.x;
    if (j >= num_triangles) return;
    const unsigned long long key = sorted[j];
    if (key >= (unsigned long long)num_vertices) return;
    const int r = region_of(g, (long long)key, num_vertices);
    if (r < 0) return;
    const long long d = j - (long long)g.first_face[r];
    if (d < 0 || d % kBlock != 0) return;
    const long long b = (long long)g.first_block[r] + d / kBlock;
    if (b >= 0 && b < max_blocks) block_first[b] = (int)j;
}

__global__ void __launch_bounds__(kTile)
block_sums_kernel(const unsigned long long *__restrict__ sorted, const int *__restrict__ order, long long num_triangles,
                  long long num_vertices, Regions g, const int *__restrict__ component_triangles, const Acc *__restrict__ records,
                  const int *__restrict__ block_first, const long long *__restrict__ num_blocks, long long max_blocks,
                  Acc *__restrict__ partials) {
    const long long b = (long long)blockIdx.x * kTile + threadIdx.x;
    if (b >= max_blocks || b >= num_blocks[0]) return;
    Acc a = acc_empty();
    const long long j0 = block_first[b];
    if (j0 >= 0 && j0 < num_triangles) {
        const unsigned long long key = sorted[j0];
        const int r = key < (unsigned long long)num_vertices ? region_of(g, (long long)key, num_vertices) : -1;
        if (r >= 0) {
            long long end = (long long)g.first_face[r] + (long long)component_triangles[key];  // where the region's faces end
            end = end < num_triangles ? end : num_triangles;
            end = end < j0 + kBlock ? end : j0 + kBlock;
            for (long long j = j0; j < end; ++j) {
                const long long t = order[j];
                if (t >= 0 && t < num_triangles) acc_join(a, records[t]);
            }
        }
    }
    partials[b] = a;
}

__global__ void __launch_bounds__(kTile)
regions_kernel(Regions g, long long num_vertices, const int *__restrict__ component_triangles, const long long *__restrict__ counts,
               const long long *__restrict__ num_blocks, long long max_blocks, const Acc *__restrict__ partials,
               long long capacity, tn_mesh_region *__restrict__ regions) {
    const long long r = (long long)blockIdx.x * kTile + threadIdx.x;
    if (r >= capacity || r >= g.capacity || r >= counts[0]) return;
    const long long label = g.label[r];
    if (label < 0 || label >= num_vertices) return;
    const int faces = component_triangles[label];
    long long b = g.first_block[r], end = b + (long long)blocks_of(faces > 0 ? faces : 0);
    end = end < max_blocks ? end : max_blocks;
    end = end < num_blocks[0] ? end : num_blocks[0];
    Acc a = acc_empty();
    for (b = b < 0 ? 0 : b; b < end; ++b) acc_join(a, partials[b]);
    tn_mesh_region out;
    out.area = a.s[0];
    out.label = (int32_t)label;
    out.faces = faces;
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

// the two lists of `totals`: y = 0 the usable faces (their number is counts[2]), y = 1 the selected ones (counts[1])
__global__ void __launch_bounds__(kTile)
total_blocks_kernel(const int *__restrict__ usable_list, const int *__restrict__ selected_list, const long long *__restrict__ counts,
                    long long num_triangles, const Acc *__restrict__ records, long long blocks_per_list, double *__restrict__ partials) {
    const long long b = (long long)blockIdx.x * kTile + threadIdx.x;
    const int y = blockIdx.y;
    long long n = counts[2 - y];
    n = n < num_triangles ? n : num_triangles;
    if (b >= blocks_per_list || b * kBlock >= n) return;
    const int *list = y ? selected_list : usable_list;
    const long long end = (b + 1) * kBlock < n ? (b + 1) * kBlock : n;
    double s = 0.0;
    for (long long k = b * kBlock; k < end; ++k) {
        const long long t = list[k];
        if (t >= 0 && t < num_triangles) s = __dadd_rn(s, records[t].s[0]);
    }
    partials[y * blocks_per_list + b] = s;
}

__global__ void totals_kernel(const long long *__restrict__ counts, long long num_triangles, long long blocks_per_list,
                              const double *__restrict__ partials, double *__restrict__ totals) {
    if (threadIdx.x != 0) return;
    const int y = blockIdx.x;
    long long n = counts[2 - y];
    n = n < num_triangles ? n : num_triangles;
    long long blocks = (n + kBlock - 1) / kBlock;
    blocks = blocks < blocks_per_list ? blocks : blocks_per_list;
    double s = 0.0;
    for (long long b = 0; b < blocks; ++b) s = __dadd_rn(s, partials[y * blocks_per_list + b]);
    totals[y] = s;
}

inline long long tiles_of(long long n) { return ceil_div(n, kTile); }

inline size_t ints_bytes(long long n) { return ((size_t)n * sizeof(int) + 7) / 8 * 8; }

inline int key_bits(long long num_vertices) {  // the keys are 0 .. V
    int bits = 1;
    while (bits < 63 && (1LL << bits) <= num_vertices) ++bits;
    return bits;
}

// the workspace, in order: the face records (16-byte aligned: up to 8 bytes of slack in front), the block partials, the totals'
// partials, the sort keys and the sorted keys, the device sums (faces, blocks), tn_mesh_components' summary, six arrays of tile
// counts, then the int arrays per face (masked indices x 3, flags, two lists, order), per vertex (labels, component_triangles,
// of_root), per region (label, first_face, first_block) and per block (block_first), and the sort's own workspace
struct Layout {
    Acc *records, *partials;
    double *total_partials;
    unsigned long long *keys, *sorted;
    long long *sums, *summary, *usable_tiles, *selected_tiles, *region_tiles, *face_tiles, *block_tiles;
    int *masked, *flags, *usable_list, *selected_list, *order, *labels, *component_triangles, *block_first;
    Regions regions;
    long long max_blocks, blocks_per_list;
    void *sort;
    size_t sort_bytes, bytes;
};

inline Layout layout_of(char *ws, long long v, long long t) {
    Layout l;
    size_t at = ws ? (size_t)(reinterpret_cast<uintptr_t>(ws) % 16) : 8;  // ws is 8-byte aligned: 0 or 8; sized for 8
    const size_t skip = at;
    auto take = [&](size_t bytes) {  // (ws == NULL: the sizes alone)
        char *p = ws ? ws + at : nullptr;
        at += bytes;
        return p;
    };
    const long long max_regions = v / 3 < t ? v / 3 : t;  // a region has a face, and three vertices of its own
    l.max_blocks = tiles_of(t) + max_regions;             // kBlock == kTile: sum of ceil(faces / 256) <= T / 256 + R
    l.blocks_per_list = ceil_div(t, kBlock);
    l.records = reinterpret_cast<Acc *>(take((size_t)t * sizeof(Acc)));
    l.partials = reinterpret_cast<Acc *>(take((size_t)l.max_blocks * sizeof(Acc)));
    l.total_partials = reinterpret_cast<double *>(take((size_t)(2 * l.blocks_per_list) * sizeof(double)));
    l.keys = reinterpret_cast<unsigned long long *>(take((size_t)t * sizeof(unsigned long long)));
    l.sorted = reinterpret_cast<unsigned long long *>(take((size_t)t * sizeof(unsigned long long)));
    l.sums = reinterpret_cast<long long *>(take(2 * sizeof(long long)));
    l.summary = reinterpret_cast<long long *>(take(3 * sizeof(long long)));
    long long **face_tiles[2] = {&l.usable_tiles, &l.selected_tiles};
    for (auto p : face_tiles) *p = reinterpret_cast<long long *>(take((size_t)tiles_of(t) * sizeof(long long)));
    long long **vertex_tiles[3] = {&l.region_tiles, &l.face_tiles, &l.block_tiles};
    for (auto p : vertex_tiles) *p = reinterpret_cast<long long *>(take((size_t)tiles_of(v) * sizeof(long long)));
    l.masked = reinterpret_cast<int *>(take(ints_bytes(3 * t)));
    int **per_face[4] = {&l.flags, &l.usable_list, &l.selected_list, &l.order};
    for (auto p : per_face) *p = reinterpret_cast<int *>(take(ints_bytes(t)));
    int **per_vertex[3] = {&l.labels, &l.component_triangles, &l.regions.of_root};
    for (auto p : per_vertex) *p = reinterpret_cast<int *>(take(ints_bytes(v)));
    int **per_region[3] = {&l.regions.label, &l.regions.first_face, &l.regions.first_block};
    for (auto p : per_region) *p = reinterpret_cast<int *>(take(ints_bytes(max_regions)));
    l.regions.capacity = max_regions;
    l.block_first = reinterpret_cast<int *>(take(ints_bytes(l.max_blocks)));
    l.sort_bytes = tn_sort_pairs_workspace_bytes(t);
    l.sort = take(l.sort_bytes);
    l.bytes = at - skip + 8;
    return l;
}

}  // namespace

extern "C" {

size_t tn_mesh_regions_workspace_bytes(int64_t num_vertices, int64_t num_triangles) {
    if (bad_counts(num_vertices, num_triangles)) return 0;
    return layout_of(nullptr, (long long)num_vertices, (long long)num_triangles).bytes;
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
    const Layout l = layout_of(reinterpret_cast<char *>(workspace), nv, nt);
    long long *cnt = reinterpret_cast<long long *>(counts);
    const unsigned vertex_blocks = (unsigned)tiles_of(nv), face_blocks = (unsigned)tiles_of(nt);
    int code;

    // 1 - 3: the faces, the two counts, the two lists
    hipLaunchKernelGGL(faces_kernel, dim3(face_blocks), dim3(kTile), 0, s, positions, temperature, triangles, nv, nt, min_temperature,
                       max_temperature, l.records, l.masked, l.flags, face_area, l.usable_tiles, l.selected_tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_faces_kernel, dim3(1), dim3(kScan), 0, s, l.usable_tiles, l.selected_tiles, tiles_of(nt), cnt);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(lists_kernel, dim3(face_blocks), dim3(kTile), 0, s, l.flags, nt, l.usable_tiles, l.selected_tiles, l.usable_list,
                       l.selected_list);
    TN_LAUNCH_CHECK();

    // 4 - 5: the regions of the selected faces, numbered in ascending label
    code = tn_mesh_components(l.masked, num_triangles, num_vertices, l.labels, l.component_triangles,
                              reinterpret_cast<int64_t *>(l.summary), stream);
    if (code != TN_OK) return code;
    hipLaunchKernelGGL(count_roots_kernel, dim3(vertex_blocks), dim3(kTile), 0, s, l.labels, l.component_triangles, nv, l.region_tiles,
                       l.face_tiles, l.block_tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_roots_kernel, dim3(1), dim3(kScan), 0, s, l.region_tiles, l.face_tiles, l.block_tiles, tiles_of(nv), cnt, l.sums);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(emit_roots_kernel, dim3(vertex_blocks), dim3(kTile), 0, s, l.labels, l.component_triangles, nv, l.region_tiles,
                       l.face_tiles, l.block_tiles, l.regions);
    TN_LAUNCH_CHECK();

    // 6 - 8: face_region; a region's faces adjacent in ascending face index; where every 256-block starts
    hipLaunchKernelGGL(keys_kernel, dim3(face_blocks), dim3(kTile), 0, s, l.masked, l.flags, nt, nv, l.labels, l.regions, face_region, l.keys);
    TN_LAUNCH_CHECK();
    code = tn_sort_pairs(reinterpret_cast<const uint64_t *>(l.keys), nullptr, num_triangles, key_bits(nv),
                         reinterpret_cast<uint64_t *>(l.sorted), l.order, l.sort, l.sort_bytes, stream);
    if (code != TN_OK) return code;
    hipLaunchKernelGGL(block_heads_kernel, dim3(face_blocks), dim3(kTile), 0, s, l.sorted, nt, nv, l.regions, l.max_blocks, l.block_first);
    TN_LAUNCH_CHECK();

    // 9 - 10: the block partials, the regions' rows
    hipLaunchKernelGGL(block_sums_kernel, dim3((unsigned)tiles_of(l.max_blocks)), dim3(kTile), 0, s, l.sorted, l.order, nt, nv, l.regions,
                       l.component_triangles, l.records, l.block_first, l.sums + 1, l.max_blocks, l.partials);
    TN_LAUNCH_CHECK();
    if (capacity_regions > 0 && l.regions.capacity > 0) {
        const long long rows = capacity_regions < l.regions.capacity ? (long long)capacity_regions : l.regions.capacity;
        hipLaunchKernelGGL(regions_kernel, dim3((unsigned)tiles_of(rows)), dim3(kTile), 0, s, l.regions, nv, l.component_triangles, cnt,
                           l.sums + 1, l.max_blocks, l.partials, (long long)capacity_regions, regions);
        TN_LAUNCH_CHECK();
    }

    // 11: the mesh's area and the selected area
    hipLaunchKernelGGL(total_blocks_kernel, dim3((unsigned)tiles_of(l.blocks_per_list), 2), dim3(kTile), 0, s, l.usable_list, l.selected_list,
                       cnt, nt, l.records, l.blocks_per_list, l.total_partials);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(totals_kernel, dim3(2), dim3(TN_WAVE), 0, s, cnt, nt, l.blocks_per_list, l.total_partials, totals);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

}  // extern "C"
