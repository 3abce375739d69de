// Thermal hot spots of an indexed triangle list (DESIGN.md "Thermal hot spots"; include/thermonerf_hip.h defines every output to the
// bit): the local maxima of the per-vertex temperature, their basins of steepest ascent, the saddles between adjacent basins, and —
// once the host has merged the basin graph (tn_persistence.h) — the extent and the row of every spot that stands out.
//
// tn_mesh_peaks, on the caller's stream:
//   1. keys, sort   a 32-bit order-preserving key per vertex (reversed for HOT: the top comes first; 0xffffffff without a finite
//                   temperature), tn_sort_pairs of (key, 0 .. V-1): the vertex at every rank; one thread per rank writes rank[v]
//   2. ascent       one thread per vertex walks its corner list: up[v] = the neighbour of the smallest rank if that is below its own
//   3. jumps        ceil(log2(max(2, V))) launches over two arrays, each reading one and writing the other: peak[v]
//   4. basins       count / scan / emit over the peak flags: the basins in ascending peak vertex, basin_peak, vertex_basin
//   5. edge keys    one thread per half-edge: (min(a, b), max(a, b)) of the two basins it joins, or the key of no pair
//   6. sort         tn_sort_pairs of (key, 0 .. 3T-1): a pair's half-edges side by side, the pairs in ascending (a, b)
//   7. saddles      count / scan / emit over the heads of the runs; the head's thread walks its run for the smallest pass
// tn_mesh_spots, on the caller's stream (the steps marked * are tn_group_sum.h's, shared with tn_mesh_regions.hip):
//   1. vertices     one thread per vertex: vertex_spot from its basin's spot, the spot's limit and bound; the spot's vertex count
//   2. faces        one thread per face: load_face *, USABLE, face_spot, the face record, the sort key; the tile counts
//   3. lists *      the two scans -> counts[2], counts[1]
//   4. sort, heads *, blocks *, assign, block sums *   as tn_mesh_regions does it, the label being the spot
//   5. rows         one thread per spot: its group's sum *, or the empty row
// No allocation, no host synchronisation, no float atomics (the integer ones: the finite vertices, one per block, the vertices of a
// spot, one per wave and spot, and the sort's), every error code before any launch, and no block ever waits for another.  The kernels check
// what they dereference: a list is clipped to [0, 3T], a corner outside it or of an invalid triangle is skipped, a rank, a basin, a
// spot and a sorted position are used only inside their arrays — foreign inputs give other numbers, never an access outside.
#include <cmath>

#include "tn_device.h"
#include "tn_group_sum.h"
#include "tn_mesh_lists.h"
#include "tn_persistence.h"

using namespace tn;

namespace {

constexpr int kTile = kFaceTile;  // vertices / half-edges / faces / spots per thread block of every kernel but the scan
constexpr unsigned long long kNoValue = 0xffffffffull;  // the rank key of a vertex without a finite temperature

inline long long tiles_of(long long n) { return ceil_div(n, kTile); }

// ---- tn_mesh_peaks ----------------------------------------------------------------------------------------------------------------------

// finite temperatures have f2key in [0x00800000, 0xff7fffff]: so has its complement, and 0xffffffff lies behind both
__global__ void __launch_bounds__(kTile)
rank_keys_kernel(const float *__restrict__ temperature, long long num_vertices, bool coldest, unsigned long long *__restrict__ keys) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    if (v >= num_vertices) return;
    const float t = temperature[v];
    unsigned long long key = kNoValue;
    if (finite(t)) {
        const unsigned k = f2key((__float_as_uint(t) << 1) == 0u ? 0.0f : t);  // -0.0 is +0.0
        key = coldest ? k : ~k;
    }
    keys[v] = key;
}

__global__ void __launch_bounds__(kTile)
ranks_kernel(const int *__restrict__ by_rank, long long num_vertices, int *__restrict__ rank) {
    const long long r = (long long)blockIdx.x * kTile + threadIdx.x;
    if (r >= num_vertices) return;
    const long long v = by_rank[r];
    if (v >= 0 && v < num_vertices) rank[v] = (int)r;
}

// up[v]: -1 without a finite temperature.  A vertex without one has a rank behind every finite vertex's: it never wins
__global__ void __launch_bounds__(kTile)
ascent_kernel(const float *__restrict__ temperature, const int *__restrict__ tri, long long num_corners, int num_vertices,
              const int *__restrict__ offsets, const int *__restrict__ corners, const int *__restrict__ rank, int *__restrict__ up) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    if (v >= num_vertices) return;
    if (!finite(temperature[v])) {
        up[v] = -1;
        return;
    }
    long long begin, end;
    list_of(offsets, v, num_corners, begin, end);
    int best = (int)v, best_rank = rank[v];
    for (long long i = begin; i < end; ++i) {
        const long long c = corners[i];
        if (c < 0 || c >= num_corners) continue;
        const long long t = c / 3;
        const int j = (int)(c - 3 * t);
        const Tri tr = load_triangle(tri, t);
        if (!valid_triangle(tr, num_vertices)) continue;
        const int q = j == 0 ? tr.v[1] : (j == 1 ? tr.v[2] : tr.v[0]);  // index (j + 1) % 3
        const int r = j == 0 ? tr.v[2] : (j == 1 ? tr.v[0] : tr.v[1]);  // index (j + 2) % 3
        const int rq = rank[q], rr = rank[r];
        if (rq < best_rank) best = q, best_rank = rq;
        if (rr < best_rank) best = r, best_rank = rr;
    }
    up[v] = best;
}

__global__ void __launch_bounds__(kTile) jump_kernel(const int *__restrict__ src, long long num_vertices, int *__restrict__ dst) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    if (v >= num_vertices) return;
    const long long p = src[v];
    long long q = p;
    if (p >= 0 && p < num_vertices) {
        q = src[p];
        if (q < 0 || q >= num_vertices) q = p;
    }
    dst[v] = (int)q;
}

__device__ __forceinline__ bool is_peak(const int *__restrict__ peak, long long v, long long num_vertices) {
    return v < num_vertices && peak[v] == (int)v;
}

__global__ void __launch_bounds__(kTile)
count_peaks_kernel(const int *__restrict__ peak, long long num_vertices, long long *__restrict__ tiles, long long *__restrict__ finite_vertices) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    uint32_t total, with_value;
    block_rank<kTile>(is_peak(peak, v, num_vertices), total);
    __syncthreads();  // block_rank's LDS is rewritten by the second call
    block_rank<kTile>(v < num_vertices && peak[v] >= 0, with_value);
    if (threadIdx.x != 0) return;
    tiles[blockIdx.x] = (long long)total;
    if (with_value) atomicAdd(reinterpret_cast<unsigned long long *>(finite_vertices), (unsigned long long)with_value);
}

__global__ void __launch_bounds__(kTile)
emit_peaks_kernel(const int *__restrict__ peak, long long num_vertices, const long long *__restrict__ tiles, long long capacity,
                  int *__restrict__ basin_of_peak, int *__restrict__ basin_peak) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    const bool keep = is_peak(peak, v, num_vertices);
    uint32_t unused;
    const uint32_t before = block_rank<kTile>(keep, unused);
    if (!keep) return;
    const long long b = tiles[blockIdx.x] + (long long)before;  // <= v
    basin_of_peak[v] = (int)b;
    if (b >= 0 && b < capacity) basin_peak[b] = (int)v;
}

__global__ void __launch_bounds__(kTile)
basins_kernel(const int *__restrict__ peak, const int *__restrict__ basin_of_peak, long long num_vertices, int *__restrict__ vertex_basin) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    if (v >= num_vertices) return;
    const long long p = peak[v];
    vertex_basin[v] = p >= 0 && p < num_vertices && peak[p] == (int)p ? basin_of_peak[p] : -1;
}

// what the half-edge sort orders by: `bits` bits for each basin of the pair, the lower basin on top; none = (V, V)
struct EdgeKeys {
    int bits;
    unsigned long long none;
};

// half-edge h = 3 t + j runs from index j to index (j + 1) % 3 of triangle t; false: outside the list or of an invalid triangle
__device__ __forceinline__ bool half_edge(const int *__restrict__ tri, long long h, long long num_corners, int num_vertices, int &u, int &w) {
    if (h < 0 || h >= num_corners) return false;
    const long long t = h / 3;
    const int j = (int)(h - 3 * t);
    const Tri tr = load_triangle(tri, t);
    if (!valid_triangle(tr, num_vertices)) return false;
    u = tr.v[j];
    w = j == 0 ? tr.v[1] : (j == 1 ? tr.v[2] : tr.v[0]);
    return true;
}

__global__ void __launch_bounds__(kTile)
edge_keys_kernel(const int *__restrict__ tri, long long num_corners, int num_vertices, const int *__restrict__ vertex_basin, EdgeKeys e,
                 unsigned long long *__restrict__ keys) {
    const long long h = (long long)blockIdx.x * kTile + threadIdx.x;
    if (h >= num_corners) return;
    unsigned long long key = e.none;
    int u, w;
    if (half_edge(tri, h, num_corners, num_vertices, u, w)) {
        const int a = vertex_basin[u], b = vertex_basin[w];  // -1 without a finite temperature
        if (a >= 0 && b >= 0 && a != b && a < num_vertices && b < num_vertices)
            key = ((unsigned long long)(a < b ? a : b) << e.bits) | (unsigned long long)(a < b ? b : a);
    }
    keys[h] = key;
}

__device__ __forceinline__ bool is_pair_head(const unsigned long long *__restrict__ sorted, long long j, long long n, unsigned long long none) {
    if (j >= n) return false;
    const unsigned long long key = sorted[j];
    return key < none && (j == 0 || sorted[j - 1] != key);
}

__global__ void __launch_bounds__(kTile)
count_pairs_kernel(const unsigned long long *__restrict__ sorted, long long num_corners, EdgeKeys e, long long *__restrict__ tiles) {
    const long long j = (long long)blockIdx.x * kTile + threadIdx.x;
    uint32_t total;
    block_rank<kTile>(is_pair_head(sorted, j, num_corners, e.none), total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = (long long)total;
}

// the head of a run writes its pair's row: the smallest pass over the run's half-edges (a minimum over integers: order-free)
__global__ void __launch_bounds__(kTile)
emit_saddles_kernel(const unsigned long long *__restrict__ sorted, const int *__restrict__ order, const int *__restrict__ tri,
                    long long num_corners, int num_vertices, const int *__restrict__ rank, const int *__restrict__ by_rank, EdgeKeys e,
                    const long long *__restrict__ tiles, long long capacity, tn_mesh_saddle *__restrict__ saddles) {
    const long long j = (long long)blockIdx.x * kTile + threadIdx.x;
    const bool head = is_pair_head(sorted, j, num_corners, e.none);
    uint32_t unused;
    const uint32_t before = block_rank<kTile>(head, unused);
    if (!head) return;
    const long long s = tiles[blockIdx.x] + (long long)before;  // <= j
    if (s < 0 || s >= capacity) return;
    const unsigned long long key = sorted[j];
    int pass = num_vertices;  // above every rank
    for (long long k = j; k < num_corners && sorted[k] == key; ++k) {
        int u, w;
        if (!half_edge(tri, order[k], num_corners, num_vertices, u, w)) continue;
        const int ru = rank[u], rw = rank[w];
        const int lower = ru > rw ? ru : rw;
        pass = lower < pass ? lower : pass;
    }
    tn_mesh_saddle row;
    row.a = (int32_t)(key >> e.bits);
    row.b = (int32_t)(key & ((1ull << e.bits) - 1ull));
    row.pass_vertex = pass >= 0 && pass < num_vertices ? by_rank[pass] : -1;
    row.pass_rank = pass;
    saddles[s] = row;
}

// the workspace of tn_mesh_peaks, in order: the sort keys and the sorted keys (n = max(V, 3T) of each), the tile counts, then the int
// arrays: the half-edges in sorted order (3T), per vertex the vertex at every rank, the two arrays of the jumps and the basin of a peak,
// and the sort's own workspace
struct PeaksLayout {
    unsigned long long *keys, *sorted;
    long long *tiles;
    int *order, *by_rank, *hop[2], *basin_of_peak;
    void *sort;
    size_t sort_bytes, bytes;
};

inline PeaksLayout peaks_layout(char *ws, long long v, long long t) {
    PeaksLayout l;
    size_t at = 0;
    auto take = [&](size_t bytes) {  // (ws == NULL: the sizes alone)
        char *p = ws ? ws + at : nullptr;
        at += bytes;
        return p;
    };
    const long long n = v > 3 * t ? v : 3 * t;
    l.keys = reinterpret_cast<unsigned long long *>(take((size_t)n * sizeof(unsigned long long)));
    l.sorted = reinterpret_cast<unsigned long long *>(take((size_t)n * sizeof(unsigned long long)));
    l.tiles = reinterpret_cast<long long *>(take((size_t)tiles_of(n) * sizeof(long long)));
    l.order = reinterpret_cast<int *>(take(ints_bytes(3 * t)));
    int **per_vertex[4] = {&l.by_rank, &l.hop[0], &l.hop[1], &l.basin_of_peak};
    for (auto p : per_vertex) *p = reinterpret_cast<int *>(take(ints_bytes(v)));
    l.sort_bytes = tn_sort_pairs_workspace_bytes(n);
    l.sort = take(l.sort_bytes);
    l.bytes = at + 8;
    return l;
}

inline int jump_rounds(long long v) {
    int rounds = 1;
    while ((1ll << rounds) < v) ++rounds;  // ceil(log2(max(2, V)))
    return rounds;
}

// ---- tn_mesh_spots ----------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ void hotter(int &best, float &tbest, int i, float t) {
    if (best < 0 || t > tbest || (t == tbest && i < best)) best = i, tbest = t;
}
__device__ __forceinline__ void colder(int &best, float &tbest, int i, float t) {
    if (best < 0 || t < tbest || (t == tbest && i < best)) best = i, tbest = t;
}

// a face's record, a block's partial and a spot's accumulator, the fields of a thermal region's: five ordered sums, order-free extremes
struct alignas(16) Acc {
    double s[5];           // area, area x temperature, area x centroid x / y / z
    float tmin, tmax;      // of the face temperatures
    float lo[3], hi[3];    // of the corners' positions
    int hot, cold;         // the hottest / coldest corner; -1: none yet
    float thot, tcold;     // their temperatures
    int pad[2];
    static constexpr int kAhead = 1;  // 22 registers a record, as the regions' walk holds them
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

constexpr int kUsable = 1, kInSpot = 2;

// what the Python layer uploads after the merge: per basin its spot, per spot its peak, its limit and its bound
struct Spots {
    const int *rank, *vertex_basin;  // [V]
    const int *basin_spot;           // [B] the spot of every basin, -1 of a basin in none
    const int *peak, *limit;         // [K] the spot's peak vertex; the pass rank its vertices stay below
    const float *bound;              // [K] the temperature its vertices reach (HOT: at least; COLD: at most)
    long long basins, spots;
    bool coldest;
};

__global__ void __launch_bounds__(kTile)
spot_vertices_kernel(const float *__restrict__ temperature, long long num_vertices, Spots sp, int *__restrict__ vertex_spot,
                     int *__restrict__ spot_vertices) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    int spot = -1;
    if (v < num_vertices) {
        const long long b = sp.vertex_basin[v];
        const float t = temperature[v];
        if (b >= 0 && b < sp.basins && finite(t)) {
            const long long k = sp.basin_spot[b];
            if (k >= 0 && k < sp.spots && sp.rank[v] < sp.limit[k] && (sp.coldest ? t <= sp.bound[k] : t >= sp.bound[k])) spot = (int)k;
        }
        vertex_spot[v] = spot;
    }
    // one atomic per wave and spot, not per vertex: neighbouring vertices share a spot, and a million additions to a dozen counters
    // took 7.8 ms (profiles/micro/mesh_hotspots.txt).  Every lane of the wave runs the loop; `left` is the same in all of them
    const int lane = threadIdx.x % TN_WAVE;
    unsigned long long left = __ballot(spot >= 0);
    while (left) {
        const int leader = __ffsll((long long)left) - 1;
        const int s = __shfl(spot, leader, TN_WAVE);
        const unsigned long long same = __ballot(spot == s);
        if (lane == leader) atomicAdd(spot_vertices + s, (int)__popcll(same));
        left &= ~same;
    }
}

__global__ void __launch_bounds__(kTile)
spot_faces_kernel(const float *__restrict__ positions, const float *__restrict__ temperature, const int *__restrict__ triangles,
                  long long num_vertices, long long num_triangles, const int *__restrict__ vertex_spot, long long num_spots,
                  Acc *__restrict__ records, int *__restrict__ flags, unsigned long long *__restrict__ keys, int *__restrict__ face_spot,
                  FaceLists lists) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    bool usable = false;
    int spot = -1;
    if (t < num_triangles) {
        const Face f = load_face(positions, temperature, triangles, num_vertices, t);
        usable = f.placed && f.warm;
        if (usable) {
            const int k0 = vertex_spot[f.i[0]], k1 = vertex_spot[f.i[1]], k2 = vertex_spot[f.i[2]];
            if (k0 >= 0 && k0 < num_spots && k0 == k1 && k0 == k2) spot = k0;
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
        flags[t] = (usable ? kUsable : 0) | (spot >= 0 ? kInSpot : 0);
        keys[t] = spot >= 0 ? (unsigned long long)spot : (unsigned long long)num_spots;
        face_spot[t] = spot;
    }
    count_lists(lists, (usable ? kUsable : 0) | (spot >= 0 ? kInSpot : 0));
}

__global__ void __launch_bounds__(kTile) spot_assign_kernel(Groups g) {
    const long long j = (long long)blockIdx.x * kTile + threadIdx.x;
    if (j >= g.num_triangles) return;
    block_head(g, j, groups_of(g));
}

// one thread per spot; with_faces: the groups exist (a spot without a whole face has no group: the empty row)
__global__ void __launch_bounds__(kTile)
spot_rows_kernel(Groups g, bool with_faces, const Acc *__restrict__ records, const Acc *__restrict__ partials, Spots sp,
                 const int *__restrict__ spot_vertices, tn_mesh_spot *__restrict__ spots) {
    const long long k = (long long)blockIdx.x * kTile + threadIdx.x;
    if (k >= sp.spots) return;
    Acc a = Acc::empty();
    long long faces = 0;
    if (with_faces) {
        const long long n = groups_of(g);
        const int q = group_of(g, k, n);
        if (q >= 0) {
            faces = faces_of(g, q, n);
            a = group_sum(g, q, faces, records, partials);
        }
    }
    tn_mesh_spot out;
    out.area = a.s[0];
    out.label = sp.peak[k];
    out.faces = (int32_t)faces;
    const bool flat = a.s[0] == 0.0, none = faces == 0;
    out.mean_temperature = flat ? quiet_nan() : (float)__ddiv_rn(a.s[1], a.s[0]);
    out.min_temperature = none ? quiet_nan() : a.tmin;
    out.max_temperature = none ? quiet_nan() : a.tmax;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out.centroid[c] = flat ? quiet_nan() : (float)__ddiv_rn(a.s[2 + c], a.s[0]);
        out.bounds[c] = none ? quiet_nan() : a.lo[c];
        out.bounds[3 + c] = none ? quiet_nan() : a.hi[c];
    }
    out.coldest_vertex = a.cold;
    out.hottest_vertex = a.hot;
    out.vertices = spot_vertices[k];
    out.reserved = 0;
    spots[k] = out;
}

// the workspace of tn_mesh_spots, in order: the face records (16-byte aligned: up to 8 bytes of slack in front), the block partials, the
// sort keys and the sorted keys, the number of blocks, two arrays of tile counts, then the int arrays per face (flags, two lists, order),
// per spot (vertices, of_label), per group (label, first_face, first_block) and per block (block_first), and the sort's own workspace
struct SpotsLayout {
    Acc *records, *partials;
    unsigned long long *keys, *sorted;
    long long *num_blocks, *head_tiles, *block_tiles;
    int *flags, *order, *spot_vertices;
    FaceLists lists;  // 0: the usable faces, counts[2] of them; 1: the faces of a spot, counts[1] of them
    Groups groups;    // the labels are spots: L = K; a group has a face: capacity = min(K, T)
    void *sort;
    size_t sort_bytes, bytes;
};

inline SpotsLayout spots_layout(char *ws, long long t, long long k, long long *counts) {
    SpotsLayout l;
    size_t at = ws ? (size_t)(reinterpret_cast<uintptr_t>(ws) % 16) : 8;  // ws is 8-byte aligned: 0 or 8; sized for 8
    const size_t skip = at;
    auto take = [&](size_t bytes) {
        char *p = ws ? ws + at : nullptr;
        at += bytes;
        return p;
    };
    Groups &g = l.groups;
    g.num_triangles = t, g.labels = k;
    g.capacity = k < t ? k : t;
    g.direct = 0;
    g.max_blocks = tiles_of(t) + g.capacity;  // sum of ceil(faces / 256) <= T / 256 + groups
    l.records = reinterpret_cast<Acc *>(take((size_t)t * sizeof(Acc)));
    l.partials = reinterpret_cast<Acc *>(take((size_t)g.max_blocks * sizeof(Acc)));
    l.keys = reinterpret_cast<unsigned long long *>(take((size_t)t * sizeof(unsigned long long)));
    l.sorted = reinterpret_cast<unsigned long long *>(take((size_t)t * sizeof(unsigned long long)));
    l.num_blocks = reinterpret_cast<long long *>(take(sizeof(long long)));
    for (auto &p : l.lists.tiles) p = reinterpret_cast<long long *>(take((size_t)tiles_of(t) * sizeof(long long)));
    l.head_tiles = l.lists.tiles[0], l.block_tiles = l.lists.tiles[1];  // the lists' lengths are out before the groups are numbered
    int **per_face[4] = {&l.flags, &l.lists.faces[0], &l.lists.faces[1], &l.order};
    for (auto p : per_face) *p = reinterpret_cast<int *>(take(ints_bytes(t)));
    int **per_spot[2] = {&l.spot_vertices, &g.of_label};
    for (auto p : per_spot) *p = reinterpret_cast<int *>(take(ints_bytes(k)));
    int **per_group[3] = {&g.label, &g.first_face, &g.first_block};
    for (auto p : per_group) *p = reinterpret_cast<int *>(take(ints_bytes(g.capacity)));
    g.block_first = reinterpret_cast<int *>(take(ints_bytes(g.max_blocks)));
    l.sort_bytes = tn_sort_pairs_workspace_bytes(t);
    l.sort = take(l.sort_bytes);
    l.bytes = at - skip + 8;
    l.lists.bit[0] = kUsable, l.lists.bit[1] = kInSpot;
    l.lists.length[0] = counts ? counts + 2 : nullptr, l.lists.length[1] = counts ? counts + 1 : nullptr;
    g.sorted = l.sorted, g.order = l.order, g.counts = counts, g.num_blocks = l.num_blocks;
    return l;
}

inline bool bad_spot_counts(int64_t v, int64_t b, int64_t k) { return b < 0 || b > v || k < 0 || k > b; }

}  // namespace

extern "C" {

size_t tn_mesh_peaks_workspace_bytes(int64_t num_vertices, int64_t num_triangles) {
    if (bad_counts(num_vertices, num_triangles)) return 0;
    return peaks_layout(nullptr, (long long)num_vertices, (long long)num_triangles).bytes;
}

int tn_mesh_peaks(const float *temperature, const int32_t *triangles, int64_t num_triangles, int64_t num_vertices,
                  const int32_t *offsets, const int32_t *corners, int32_t coldest, int32_t *rank, int32_t *vertex_basin,
                  int32_t *basin_peak, int64_t capacity_basins, tn_mesh_saddle *saddles, int64_t capacity_saddles, int64_t *counts,
                  void *workspace, size_t workspace_bytes, void *stream) {
    if (!counts) return TN_ERR_NULL;
    if (bad_counts(num_vertices, num_triangles) || capacity_basins < 0 || capacity_saddles < 0) return TN_ERR_SHAPE;
    if (num_vertices > 0 && (!temperature || !offsets || !rank || !vertex_basin || !workspace)) return TN_ERR_NULL;
    if (num_vertices > 0 && num_triangles > 0 && (!triangles || !corners)) return TN_ERR_NULL;
    if ((capacity_basins > 0 && !basin_peak) || (capacity_saddles > 0 && !saddles)) return TN_ERR_NULL;
    if (misaligned(temperature, 4) || misaligned(triangles, 4) || misaligned(offsets, 4) || misaligned(corners, 4) || misaligned(rank, 4) ||
        misaligned(vertex_basin, 4) || misaligned(basin_peak, 4) || misaligned(saddles, 4) || misaligned(counts, 8) ||
        misaligned(workspace, 8))
        return TN_ERR_SHAPE;
    if (num_vertices > 0 && workspace_bytes < tn_mesh_peaks_workspace_bytes(num_vertices, num_triangles)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), s) != hipSuccess) return TN_ERR_LAUNCH;
    if (num_vertices == 0) return TN_OK;
    const long long nv = (long long)num_vertices, nt = (long long)num_triangles, nc = 3 * nt;
    const PeaksLayout l = peaks_layout(reinterpret_cast<char *>(workspace), nv, nt);
    long long *n = reinterpret_cast<long long *>(counts);
    const unsigned vertex_blocks = (unsigned)tiles_of(nv);
    int code;

    // 1: the vertex at every rank, the rank of every vertex
    hipLaunchKernelGGL(rank_keys_kernel, dim3(vertex_blocks), dim3(kTile), 0, s, temperature, nv, coldest != 0, l.keys);
    TN_LAUNCH_CHECK();
    code = tn_sort_pairs(reinterpret_cast<const uint64_t *>(l.keys), nullptr, num_vertices, 32, reinterpret_cast<uint64_t *>(l.sorted),
                         l.by_rank, l.sort, l.sort_bytes, stream);
    if (code != TN_OK) return code;
    hipLaunchKernelGGL(ranks_kernel, dim3(vertex_blocks), dim3(kTile), 0, s, l.by_rank, nv, rank);
    TN_LAUNCH_CHECK();

    // 2 - 3: the ascent, the jumps
    hipLaunchKernelGGL(ascent_kernel, dim3(vertex_blocks), dim3(kTile), 0, s, temperature, triangles, nc, (int)nv, offsets, corners, rank,
                       l.hop[0]);
    TN_LAUNCH_CHECK();
    const int rounds = jump_rounds(nv);
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(jump_kernel, dim3(vertex_blocks), dim3(kTile), 0, s, l.hop[r % 2], nv, l.hop[(r + 1) % 2]);
        TN_LAUNCH_CHECK();
    }
    const int *peak = l.hop[rounds % 2];

    // 4: the basins in ascending peak vertex
    hipLaunchKernelGGL(count_peaks_kernel, dim3(vertex_blocks), dim3(kTile), 0, s, peak, nv, l.tiles, n + 2);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_counts_kernel, dim3(1), dim3(kScan), 0, s, l.tiles, (long long)vertex_blocks, n);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(emit_peaks_kernel, dim3(vertex_blocks), dim3(kTile), 0, s, peak, nv, l.tiles, (long long)capacity_basins,
                       l.basin_of_peak, basin_peak);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(basins_kernel, dim3(vertex_blocks), dim3(kTile), 0, s, peak, l.basin_of_peak, nv, vertex_basin);
    TN_LAUNCH_CHECK();
    if (nt == 0) return TN_OK;

    // 5 - 7: the half-edges between two basins, a pair's side by side, the smallest pass of every pair
    EdgeKeys e;
    e.bits = key_bits((unsigned long long)nv);
    e.none = ((unsigned long long)nv << e.bits) | (unsigned long long)nv;
    const unsigned corner_blocks = (unsigned)tiles_of(nc);
    hipLaunchKernelGGL(edge_keys_kernel, dim3(corner_blocks), dim3(kTile), 0, s, triangles, nc, (int)nv, vertex_basin, e, l.keys);
    TN_LAUNCH_CHECK();
    code = tn_sort_pairs(reinterpret_cast<const uint64_t *>(l.keys), nullptr, nc, 2 * e.bits, reinterpret_cast<uint64_t *>(l.sorted),
                         l.order, l.sort, l.sort_bytes, stream);
    if (code != TN_OK) return code;
    hipLaunchKernelGGL(count_pairs_kernel, dim3(corner_blocks), dim3(kTile), 0, s, l.sorted, nc, e, l.tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_counts_kernel, dim3(1), dim3(kScan), 0, s, l.tiles, (long long)corner_blocks, n + 1);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(emit_saddles_kernel, dim3(corner_blocks), dim3(kTile), 0, s, l.sorted, l.order, triangles, nc, (int)nv, rank,
                       l.by_rank, e, l.tiles, (long long)capacity_saddles, saddles);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

int tn_basin_persistence(const int32_t *basin_rank, int64_t num_basins, const tn_mesh_saddle *saddles, int64_t num_saddles,
                         int32_t *death_saddle, int32_t *parent) {
    if (num_basins < 0 || num_basins > 0x7fffffffLL || num_saddles < 0 || num_saddles > 0x7fffffffLL) return TN_ERR_SHAPE;
    if (num_basins > 0 && (!basin_rank || !death_saddle || !parent)) return TN_ERR_NULL;
    if (num_saddles > 0 && !saddles) return TN_ERR_NULL;
    if (misaligned(basin_rank, 4) || misaligned(saddles, 4) || misaligned(death_saddle, 4) || misaligned(parent, 4)) return TN_ERR_SHAPE;
    static_assert(sizeof(tn_mesh_saddle) == 4 * sizeof(int32_t), "a row is four ints");
    const int code = merge(basin_rank, num_basins, reinterpret_cast<const int32_t *>(saddles), num_saddles, death_saddle, parent);
    return code == kPersistenceOk ? TN_OK : (code == kPersistenceBadRow ? TN_ERR_UNSUPPORTED : TN_ERR_WORKSPACE);
}

size_t tn_mesh_spots_workspace_bytes(int64_t num_vertices, int64_t num_triangles, int64_t num_spots) {
    if (bad_counts(num_vertices, num_triangles) || num_spots < 0 || num_spots > num_vertices) return 0;
    return spots_layout(nullptr, (long long)num_triangles, (long long)num_spots, nullptr).bytes;
}

int tn_mesh_spots(const float *positions, const float *temperature, const int32_t *triangles, int64_t num_vertices,
                  int64_t num_triangles, const int32_t *rank, const int32_t *vertex_basin, const int32_t *basin_spot, int64_t num_basins,
                  const int32_t *spot_peak, const int32_t *spot_limit, const float *spot_bound, int64_t num_spots, int32_t coldest,
                  int32_t *vertex_spot, int32_t *face_spot, tn_mesh_spot *spots, int64_t *counts, void *workspace,
                  size_t workspace_bytes, void *stream) {
    if (!counts) return TN_ERR_NULL;
    if (bad_counts(num_vertices, num_triangles) || bad_spot_counts(num_vertices, num_basins, num_spots)) return TN_ERR_SHAPE;
    if (num_vertices > 0 && (!positions || !temperature || !rank || !vertex_basin || !vertex_spot || !workspace)) return TN_ERR_NULL;
    if (num_triangles > 0 && (!triangles || !face_spot)) return TN_ERR_NULL;
    if (num_basins > 0 && !basin_spot) return TN_ERR_NULL;
    if (num_spots > 0 && (!spot_peak || !spot_limit || !spot_bound || !spots)) return TN_ERR_NULL;
    if (misaligned(positions, 4) || misaligned(temperature, 4) || misaligned(triangles, 4) || misaligned(rank, 4) ||
        misaligned(vertex_basin, 4) || misaligned(basin_spot, 4) || misaligned(spot_peak, 4) || misaligned(spot_limit, 4) ||
        misaligned(spot_bound, 4) || misaligned(vertex_spot, 4) || misaligned(face_spot, 4) || misaligned(spots, 8) ||
        misaligned(counts, 8) || misaligned(workspace, 8))
        return TN_ERR_SHAPE;
    if (num_vertices > 0 && workspace_bytes < tn_mesh_spots_workspace_bytes(num_vertices, num_triangles, num_spots)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long long nv = (long long)num_vertices, nt = (long long)num_triangles, nk = (long long)num_spots;
    if (hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), s) != hipSuccess) return TN_ERR_LAUNCH;
    if (nv == 0) {  // no vertex, no basin, no spot
        if (nt > 0 && hipMemsetAsync(face_spot, 0xff, (size_t)nt * sizeof(int32_t), s) != hipSuccess) return TN_ERR_LAUNCH;
        return TN_OK;
    }
    const SpotsLayout l = spots_layout(reinterpret_cast<char *>(workspace), nt, nk, reinterpret_cast<long long *>(counts));
    const Groups &g = l.groups;
    Spots sp;
    sp.rank = rank, sp.vertex_basin = vertex_basin, sp.basin_spot = basin_spot, sp.peak = spot_peak, sp.limit = spot_limit;
    sp.bound = spot_bound, sp.basins = (long long)num_basins, sp.spots = nk, sp.coldest = coldest != 0;
    int code;

    // 1: the extents
    if (nk > 0 && hipMemsetAsync(l.spot_vertices, 0, (size_t)nk * sizeof(int), s) != hipSuccess) return TN_ERR_LAUNCH;
    hipLaunchKernelGGL(spot_vertices_kernel, dim3((unsigned)tiles_of(nv)), dim3(kTile), 0, s, temperature, nv, sp, vertex_spot,
                       l.spot_vertices);
    TN_LAUNCH_CHECK();
    const bool with_faces = nt > 0 && nk > 0;
    if (nt > 0) {
        // 2 - 3: the faces, the two counts
        const unsigned face_blocks = (unsigned)tiles_of(nt);
        hipLaunchKernelGGL(spot_faces_kernel, dim3(face_blocks), dim3(kTile), 0, s, positions, temperature, triangles, nv, nt, vertex_spot, nk,
                           l.records, l.flags, l.keys, face_spot, l.lists);
        TN_LAUNCH_CHECK();
        if ((code = list_faces(l.lists, l.flags, nt, s)) != TN_OK) return code;
    }
    if (with_faces) {
        // 4: a spot's faces side by side in ascending face index, the groups, their blocks and the blocks' partials
        code = tn_sort_pairs(reinterpret_cast<const uint64_t *>(l.keys), nullptr, num_triangles, key_bits((unsigned long long)nk),
                             reinterpret_cast<uint64_t *>(l.sorted), l.order, l.sort, l.sort_bytes, stream);
        if (code != TN_OK) return code;
        if ((code = number_groups(g, l.head_tiles, s)) != TN_OK) return code;
        if ((code = place_blocks(g, l.block_tiles, s)) != TN_OK) return code;
        hipLaunchKernelGGL(spot_assign_kernel, dim3((unsigned)tiles_of(nt)), dim3(kTile), 0, s, g);
        TN_LAUNCH_CHECK();
        if ((code = sum_blocks(g, g.capacity, l.records, l.partials, s)) != TN_OK) return code;
    }
    // 5: the rows
    if (nk > 0) {
        hipLaunchKernelGGL(spot_rows_kernel, dim3((unsigned)tiles_of(nk)), dim3(kTile), 0, s, g, with_faces, l.records, l.partials, sp,
                           l.spot_vertices, spots);
        TN_LAUNCH_CHECK();
    }
    return TN_OK;
}

}  // extern "C"
