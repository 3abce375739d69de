// Geodesic distance on an indexed triangle list (DESIGN.md "Geodesic distance"; include/thermonerf_hip.h defines every output to the
// bit): a Jacobi fixed point of the eikonal equation on the triangles with the virtual-source update, over the corner lists of
// tn_mesh_incidence, and the decay profile — area and temperature per band of distance.
//
// tn_mesh_geodesic, on the caller's stream:
//   restart  fill (+inf, -1), the seeds (two integer atomic minima: the offset's bits, then the seed's number), spread (the second
//            array of every pair equals the first)
//   rounds   launch r reads the arrays r % 2 and writes the others; it returns at once unless launch r - 1 changed a vertex (launch 0:
//            unless a round has changed nothing before).  One thread per vertex, every vertex in every round
//   tally    one block counts the launches that changed something: counts[0] += n, counts[1] = 1 if one ran and changed nothing
//   settle   with n odd the latest iterate lies in the workspace: copied to distance / nearest_seed, so every call starts at parity 0
// tn_mesh_distance_bands (the steps marked * are tn_group_sum.h's, shared with tn_mesh_regions.hip):
//   1. faces   one thread per face: load_face *, the band, the record, the sort key; the tile counts
//   2. counts * the two scans of the tile counts -> counts[2], counts[1] (the lengths alone: nothing here reads a compacted list)
//   3. sort, heads *, blocks *, assign, block sums *   as tn_mesh_regions does it, the label being the band
//   4. rows    one thread per band: its group's sum *, or the empty row
// No allocation, no host synchronisation, no float atomics, every error code before any launch, and no block ever waits for another.
// The kernels check what they dereference: a list is clipped to [0, 3T], a corner outside it, of an invalid triangle or of a triangle
// that does not hold the vertex there is skipped, a seed outside [0, V) is ignored.
#include <cmath>

#include "tn_device.h"
#include "tn_group_sum.h"
#include "tn_mesh_lists.h"

using namespace tn;

namespace {

constexpr int kTile = kFaceTile;
constexpr int kMaxRounds = 4096;  // launches of one call: the flags in the workspace
constexpr int kTally = 256;

inline long long tiles_of(long long n) { return ceil_div(n, kTile); }

__device__ __forceinline__ bool finite64(double x) { return fabs(x) < (double)INFINITY; }  // (a NaN fails)

// ---- tn_mesh_geodesic -------------------------------------------------------------------------------------------------------------------

struct State {
    double *d[2];          // [V] the distances of either parity; d[0] is the caller's
    int *label[2];         // [V] the nearest seed likewise
    int *flags;            // [kMaxRounds + 1] flags[r + 1]: launch r changed a vertex
    long long *odd;        // the tally's word for settle: 1 if the latest iterate has parity 1
};

__global__ void __launch_bounds__(kTile) fill_kernel(State s, long long num_vertices) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    if (v >= num_vertices) return;
    s.d[0][v] = (double)INFINITY;
    s.label[0][v] = -1;
}

// the offset of seed i as the integer that orders it, or false: a vertex outside [0, V), an offset that is not finite or below zero
__device__ __forceinline__ bool seed_of(const int *__restrict__ seed_vertex, const double *__restrict__ seed_offset, long long i,
                                        long long num_vertices, long long &v, unsigned long long &bits) {
    v = seed_vertex[i];
    const double o = seed_offset[i];
    if (v < 0 || v >= num_vertices || !finite64(o) || o < 0.0) return false;
    bits = (unsigned long long)__double_as_longlong(__dadd_rn(o, 0.0));  // -0.0 is +0.0; monotone for offsets >= 0, below +inf's
    return true;
}

__global__ void __launch_bounds__(kTile)
seed_offsets_kernel(const int *__restrict__ seed_vertex, const double *__restrict__ seed_offset, long long num_seeds, long long num_vertices,
                    double *__restrict__ d) {
    const long long i = (long long)blockIdx.x * kTile + threadIdx.x;
    if (i >= num_seeds) return;
    long long v;
    unsigned long long bits;
    if (seed_of(seed_vertex, seed_offset, i, num_vertices, v, bits)) atomicMin(reinterpret_cast<unsigned long long *>(d + v), bits);
}

__global__ void __launch_bounds__(kTile)
seed_labels_kernel(const int *__restrict__ seed_vertex, const double *__restrict__ seed_offset, long long num_seeds, long long num_vertices,
                   const double *__restrict__ d, int *__restrict__ label) {
    const long long i = (long long)blockIdx.x * kTile + threadIdx.x;
    if (i >= num_seeds) return;
    long long v;
    unsigned long long bits;
    if (!seed_of(seed_vertex, seed_offset, i, num_vertices, v, bits)) return;
    if ((unsigned long long)__double_as_longlong(d[v]) == bits) atomicMin(reinterpret_cast<unsigned *>(label + v), (unsigned)i);  // -1 is the largest
}

struct Lists {
    const int *tri, *offsets, *corners;
    long long num_corners;
    int num_vertices;
};

// the corner i of c's list: false if it is outside the corners, its triangle invalid or not holding c there; a, b: the other two in
// the triangle's cyclic order after c
__device__ __forceinline__ bool corner_of(const Lists &m, long long i, int c, int &a, int &b) {
    const long long k = m.corners[i];
    if (k < 0 || k >= m.num_corners) return false;
    const long long t = k / 3;
    const int j = (int)(k - 3 * t);
    const Tri tr = load_triangle(m.tri, t);
    if (!valid_triangle(tr, m.num_vertices)) return false;
    const int self = j == 0 ? tr.v[0] : (j == 1 ? tr.v[1] : tr.v[2]);
    a = j == 0 ? tr.v[1] : (j == 1 ? tr.v[2] : tr.v[0]);
    b = j == 0 ? tr.v[2] : (j == 1 ? tr.v[0] : tr.v[1]);
    return self == c;
}

__global__ void __launch_bounds__(kTile) spread_kernel(State s, Lists m) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    if (v >= m.num_vertices) return;
    s.d[1][v] = s.d[0][v];
    s.label[1][v] = s.label[0][v];
}

__device__ __forceinline__ bool load_point(const float *__restrict__ positions, long long v, double p[3]) {
    const float x = positions[3 * v], y = positions[3 * v + 1], z = positions[3 * v + 2];
    p[0] = (double)x, p[1] = (double)y, p[2] = (double)z;
    return finite(x) && finite(y) && finite(z);
}

__device__ __forceinline__ double dot3(const double x[3], const double y[3]) {
    return __dadd_rn(__dadd_rn(__dmul_rn(x[0], y[0]), __dmul_rn(x[1], y[1])), __dmul_rn(x[2], y[2]));
}

__device__ __forceinline__ void take(double cand, int from, double limit, double &best, int &label) {
    if (cand < best && cand <= limit) best = cand, label = from;  // (a NaN fails both)
}

// the three candidates of triangle (c, a, b) in the header's order of operations
__device__ __forceinline__ void triangle_update(const double pc[3], const double pa[3], const double pb[3], double da, double db, int la,
                                                int lb, double limit, double &best, int &label) {
    double ac[3], bc[3], ab[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ac[k] = __dsub_rn(pc[k], pa[k]);
        bc[k] = __dsub_rn(pc[k], pb[k]);
        ab[k] = __dsub_rn(pb[k], pa[k]);
    }
    take(__dadd_rn(da, __dsqrt_rn(dot3(ac, ac))), la, limit, best, label);
    take(__dadd_rn(db, __dsqrt_rn(dot3(bc, bc))), lb, limit, best, label);
    if (!finite64(da) || !finite64(db)) return;
    const double u = __dsqrt_rn(dot3(ab, ab));
    if (!(u > 0.0)) return;
    double cr[3];
    cr[0] = __dsub_rn(__dmul_rn(ab[1], ac[2]), __dmul_rn(ab[2], ac[1]));
    cr[1] = __dsub_rn(__dmul_rn(ab[2], ac[0]), __dmul_rn(ab[0], ac[2]));
    cr[2] = __dsub_rn(__dmul_rn(ab[0], ac[1]), __dmul_rn(ab[1], ac[0]));
    const double cx = __ddiv_rn(dot3(ab, ac), u);
    const double cy = __ddiv_rn(__dsqrt_rn(dot3(cr, cr)), u);
    if (!(cy > 0.0)) return;
    const double da2 = __dmul_rn(da, da);
    const double sx = __ddiv_rn(__dsub_rn(__dadd_rn(__dmul_rn(u, u), da2), __dmul_rn(db, db)), __dmul_rn(2.0, u));
    const double sy2 = __dsub_rn(da2, __dmul_rn(sx, sx));
    if (!(sy2 >= 0.0)) return;
    const double sy = __dsqrt_rn(sy2);
    const double dx = __dsub_rn(cx, sx), h = __dadd_rn(cy, sy);
    const double xs = __dadd_rn(sx, __ddiv_rn(__dmul_rn(dx, sy), h));
    if (!(xs > 0.0 && xs < u)) return;
    take(__dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(h, h))), da <= db ? la : lb, limit, best, label);
}

// launch r of a call: every vertex is evaluated
__global__ void __launch_bounds__(kTile)
round_kernel(State s, Lists m, const float *__restrict__ positions, double limit, int r, const long long *__restrict__ counts) {
    if (r == 0 ? counts[1] != 0 : s.flags[r] == 0) return;  // converged, or the launch before changed nothing
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    if (v >= m.num_vertices) return;
    const int in = r & 1, out = in ^ 1;
    const int c = (int)v;
    const double *__restrict__ d = s.d[in];
    const int *__restrict__ lab = s.label[in];
    const double old = d[c];
    double best = old;
    int label = lab[c];
    double pc[3];
    if (load_point(positions, c, pc)) {
        long long begin, end;
        list_of(m.offsets, c, m.num_corners, begin, end);
        for (long long i = begin; i < end; ++i) {
            int a, b;
            if (!corner_of(m, i, c, a, b) || a == b || a == c || b == c) continue;
            double pa[3], pb[3];
            const bool fa = load_point(positions, a, pa), fb = load_point(positions, b, pb);
            if (!fa || !fb) continue;
            triangle_update(pc, pa, pb, d[a], d[b], lab[a], lab[b], limit, best, label);
        }
    }
    s.d[out][c] = best;
    s.label[out][c] = label;
    if (best < old) s.flags[r + 1] = 1;
}

__global__ void __launch_bounds__(kTally) tally_kernel(State s, int rounds, long long *__restrict__ counts) {
    __shared__ int changed;
    if (threadIdx.x == 0) changed = 0;
    __syncthreads();
    int mine = 0;
    for (int r = threadIdx.x; r < rounds; r += kTally) mine += s.flags[r + 1] != 0;
    if (mine) atomicAdd(&changed, mine);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int n = changed;  // the launches 0 .. n - 1 changed something; launch n, if there is one, ran and changed nothing
    const bool ran = counts[1] == 0;
    counts[0] += n;
    if (ran && n < rounds) counts[1] = 1;
    s.odd[0] = n & 1;
}

__global__ void __launch_bounds__(kTile) settle_kernel(State s, long long num_vertices) {
    if (s.odd[0] == 0) return;
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    if (v >= num_vertices) return;
    s.d[0][v] = s.d[1][v];
    s.label[0][v] = s.label[1][v];
}

// the workspace of tn_mesh_geodesic, in order: the distances of parity 1, the tally's word, the flags, the labels of parity 1
inline size_t geodesic_layout(char *ws, long long v, State &s) {
    size_t at = 0;
    auto take = [&](size_t bytes) {
        char *p = ws ? ws + at : nullptr;
        at += (bytes + 7) / 8 * 8;
        return p;
    };
    s.d[1] = reinterpret_cast<double *>(take((size_t)v * sizeof(double)));
    s.odd = reinterpret_cast<long long *>(take(sizeof(long long)));
    s.flags = reinterpret_cast<int *>(take((size_t)(kMaxRounds + 1) * sizeof(int)));
    s.label[1] = reinterpret_cast<int *>(take((size_t)v * sizeof(int)));
    return at + 8;
}

// ---- tn_mesh_distance_bands -------------------------------------------------------------------------------------------------------------

// a face's record, a block's partial and a band's accumulator: three ordered sums, order-free extremes and a count
struct alignas(16) Band {
    double s[3];       // area, the area of the faces with a temperature, area x temperature of those
    float tmin, tmax;  // of the face temperatures
    int warm;          // the faces with a temperature
    int pad[3];
    static constexpr int kAhead = 2;
    static __device__ __forceinline__ Band empty() {
        Band a;
        a.s[0] = a.s[1] = a.s[2] = 0.0;
        a.tmin = INFINITY, a.tmax = -INFINITY;
        a.warm = 0;
        a.pad[0] = a.pad[1] = a.pad[2] = 0;
        return a;
    }
    __device__ __forceinline__ void join(const Band &r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = __dadd_rn(s[k], r.s[k]);
        tmin = min_ord(tmin, r.tmin);
        tmax = max_ord(tmax, r.tmax);
        warm += r.warm;
    }
};
static_assert(sizeof(Band) == 48, "three 16-byte loads");

constexpr int kMeasured = 1, kInBand = 2;

__global__ void __launch_bounds__(kTile)
band_faces_kernel(const float *__restrict__ positions, const float *__restrict__ temperature, const int *__restrict__ triangles,
                  long long num_vertices, long long num_triangles, const double *__restrict__ distance, const int *__restrict__ nearest_seed,
                  double width, long long bands, int cell, Band *__restrict__ records, unsigned long long *__restrict__ keys,
                  FaceLists lists) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    int flag = 0;
    if (t < num_triangles) {
        const Face f = load_face(positions, temperature, triangles, num_vertices, t);
        long long band = bands;
        if (f.placed) {
            const double d0 = distance[f.i[0]], d1 = distance[f.i[1]], d2 = distance[f.i[2]];
            bool in = finite64(d0) && finite64(d1) && finite64(d2);
            if (in && cell >= 0) in = nearest_seed[f.i[0]] == cell && nearest_seed[f.i[1]] == cell && nearest_seed[f.i[2]] == cell;
            if (in) {
                flag = kMeasured;
                const double q = __ddiv_rn(__ddiv_rn(__dadd_rn(__dadd_rn(d0, d1), d2), 3.0), width);
                if (q >= 0.0 && q < (double)bands) band = (long long)floor(q), flag |= kInBand;
                Band r = Band::empty();
                r.s[0] = f.area;
                if (f.warm) {
                    r.s[1] = f.area;
                    r.s[2] = __dmul_rn(f.area, (double)f.tf);
                    r.tmin = r.tmax = f.tf;
                    r.warm = 1;
                }
                records[t] = r;  // the only store: a face that is not measured keeps whatever was there, and nothing reads it —
                                 // its key is K, which heads no group, so no walk reaches its record
            }
        }
        keys[t] = (unsigned long long)band;
    }
    count_lists(lists, flag);
}

__global__ void __launch_bounds__(kTile) band_assign_kernel(Groups g) {
    const long long j = (long long)blockIdx.x * kTile + threadIdx.x;
    if (j >= g.num_triangles) return;
    block_head(g, j, groups_of(g));
}

__global__ void __launch_bounds__(kTile)
band_rows_kernel(Groups g, bool with_faces, const Band *__restrict__ records, const Band *__restrict__ partials, long long bands,
                 tn_mesh_band *__restrict__ rows) {
    const long long k = (long long)blockIdx.x * kTile + threadIdx.x;
    if (k >= bands) return;
    Band a = Band::empty();
    long long faces = 0;
    if (with_faces) {
        const long long n = groups_of(g);
        const int q = group_of(g, k, n);
        if (q >= 0) {
            faces = faces_of(g, q, n);
            a = group_sum(g, q, faces, records, partials);
        }
    }
    tn_mesh_band out;
    out.area = a.s[0];
    out.warm_area = a.s[1];
    out.mean_temperature = a.s[1] > 0.0 ? (float)__ddiv_rn(a.s[2], a.s[1]) : quiet_nan();
    out.min_temperature = a.warm > 0 ? a.tmin : quiet_nan();
    out.max_temperature = a.warm > 0 ? a.tmax : quiet_nan();
    out.faces = (int32_t)faces;
    out.warm_faces = a.warm;
    out.reserved = 0;
    rows[k] = out;
}

// the workspace of tn_mesh_distance_bands, in order: the face records (16-byte aligned: up to 8 bytes of slack in front), the block
// partials, the sort keys and the sorted keys, the number of blocks, two arrays of tile counts, then the int arrays per face (order),
// per band (of_label), per group (label, first_face, first_block) and per block (block_first), and the sort's own
struct BandsLayout {
    Band *records, *partials;
    unsigned long long *keys, *sorted;
    long long *num_blocks, *head_tiles, *block_tiles;
    int *order;
    FaceLists lists;  // the counts alone — 0: the faces with three distances (of the cell), counts[2]; 1: those of a band, counts[1]
    Groups groups;    // the labels are bands: L = K; a group has a face: capacity = min(K, T)
    void *sort;
    size_t sort_bytes, bytes;
};

inline BandsLayout bands_layout(char *ws, long long t, long long k, long long *counts) {
    BandsLayout l;
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
    g.max_blocks = tiles_of(t) + g.capacity;
    l.records = reinterpret_cast<Band *>(take((size_t)t * sizeof(Band)));
    l.partials = reinterpret_cast<Band *>(take((size_t)g.max_blocks * sizeof(Band)));
    l.keys = reinterpret_cast<unsigned long long *>(take((size_t)t * sizeof(unsigned long long)));
    l.sorted = reinterpret_cast<unsigned long long *>(take((size_t)t * sizeof(unsigned long long)));
    l.num_blocks = reinterpret_cast<long long *>(take(sizeof(long long)));
    for (auto &p : l.lists.tiles) p = reinterpret_cast<long long *>(take((size_t)tiles_of(t) * sizeof(long long)));
    l.head_tiles = l.lists.tiles[0], l.block_tiles = l.lists.tiles[1];  // the lists' lengths are out before the groups are numbered
    l.order = reinterpret_cast<int *>(take(ints_bytes(t)));
    l.lists.faces[0] = l.lists.faces[1] = nullptr;
    g.of_label = reinterpret_cast<int *>(take(ints_bytes(k)));
    int **per_group[3] = {&g.label, &g.first_face, &g.first_block};
    for (auto p : per_group) *p = reinterpret_cast<int *>(take(ints_bytes(g.capacity)));
    g.block_first = reinterpret_cast<int *>(take(ints_bytes(g.max_blocks)));
    l.sort_bytes = tn_sort_pairs_workspace_bytes(t);
    l.sort = take(l.sort_bytes);
    l.bytes = at - skip + 8;
    l.lists.bit[0] = kMeasured, l.lists.bit[1] = kInBand;
    l.lists.length[0] = counts ? counts + 2 : nullptr, l.lists.length[1] = counts ? counts + 1 : nullptr;
    g.sorted = l.sorted, g.order = l.order, g.counts = counts, g.num_blocks = l.num_blocks;
    return l;
}

constexpr long long kMaxBands = 4096;

}  // namespace

extern "C" {

size_t tn_mesh_geodesic_workspace_bytes(int64_t num_vertices, int64_t num_triangles) {
    if (bad_counts(num_vertices, num_triangles)) return 0;
    State s;
    return geodesic_layout(nullptr, (long long)num_vertices, s);
}

int tn_mesh_geodesic(const float *positions, const int32_t *triangles, int64_t num_triangles, int64_t num_vertices,
                     const int32_t *offsets, const int32_t *corners, const int32_t *seed_vertex, const double *seed_offset,
                     int64_t num_seeds, double max_distance, int32_t restart, int32_t rounds, double *distance,
                     int32_t *nearest_seed, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream) {
    int code = check_indexed_mesh(positions, triangles, num_triangles, num_vertices, offsets, corners, reinterpret_cast<const float *>(distance));
    if (code != TN_OK) return code;
    if (num_vertices > 0 && (!nearest_seed || !counts || !workspace)) return TN_ERR_NULL;
    if (num_vertices > 0 && restart != 0 && num_seeds > 0 && (!seed_vertex || !seed_offset)) return TN_ERR_NULL;
    if (num_seeds < 0 || num_seeds > 0x7fffffffLL || !(max_distance >= 0.0) || rounds < 0 || rounds > kMaxRounds) return TN_ERR_SHAPE;
    if (misaligned(distance, 8) || misaligned(nearest_seed, 4) || misaligned(seed_vertex, 4) || misaligned(seed_offset, 8) ||
        misaligned(counts, 8) || misaligned(workspace, 8))
        return TN_ERR_SHAPE;
    if (num_vertices == 0) return TN_OK;
    if (workspace_bytes < tn_mesh_geodesic_workspace_bytes(num_vertices, num_triangles)) return TN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const long long nv = (long long)num_vertices, ns = (long long)num_seeds;
    State s;
    geodesic_layout(reinterpret_cast<char *>(workspace), nv, s);
    s.d[0] = distance, s.label[0] = nearest_seed;
    Lists m;
    m.tri = triangles, m.offsets = offsets, m.corners = corners, m.num_corners = 3 * (long long)num_triangles, m.num_vertices = (int)nv;
    long long *n = reinterpret_cast<long long *>(counts);
    const unsigned vertex_blocks = (unsigned)tiles_of(nv);

    if (restart != 0) {
        if (hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st) != hipSuccess) return TN_ERR_LAUNCH;
        hipLaunchKernelGGL(fill_kernel, dim3(vertex_blocks), dim3(kTile), 0, st, s, nv);
        TN_LAUNCH_CHECK();
        if (ns > 0) {
            hipLaunchKernelGGL(seed_offsets_kernel, dim3((unsigned)tiles_of(ns)), dim3(kTile), 0, st, seed_vertex, seed_offset, ns, nv, s.d[0]);
            TN_LAUNCH_CHECK();
            hipLaunchKernelGGL(seed_labels_kernel, dim3((unsigned)tiles_of(ns)), dim3(kTile), 0, st, seed_vertex, seed_offset, ns, nv, s.d[0],
                               s.label[0]);
            TN_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(spread_kernel, dim3(vertex_blocks), dim3(kTile), 0, st, s, m);
        TN_LAUNCH_CHECK();
    }
    if (rounds == 0) return TN_OK;
    if (hipMemsetAsync(s.flags, 0, (size_t)(rounds + 1) * sizeof(int), st) != hipSuccess) return TN_ERR_LAUNCH;
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(round_kernel, dim3(vertex_blocks), dim3(kTile), 0, st, s, m, positions, max_distance, r, n);
        TN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(tally_kernel, dim3(1), dim3(kTally), 0, st, s, (int)rounds, n);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(settle_kernel, dim3(vertex_blocks), dim3(kTile), 0, st, s, nv);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

size_t tn_mesh_distance_bands_workspace_bytes(int64_t num_vertices, int64_t num_triangles, int64_t bands) {
    if (bad_counts(num_vertices, num_triangles) || bands < 1 || bands > kMaxBands) return 0;
    return bands_layout(nullptr, (long long)num_triangles, (long long)bands, nullptr).bytes;
}

int tn_mesh_distance_bands(const float *positions, const float *temperature, const int32_t *triangles, int64_t num_vertices,
                           int64_t num_triangles, const double *distance, const int32_t *nearest_seed, double width, int64_t bands,
                           int32_t cell, tn_mesh_band *rows, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream) {
    if (!counts || !rows || !workspace) return TN_ERR_NULL;
    if (bad_counts(num_vertices, num_triangles) || bands < 1 || bands > kMaxBands || !(width > 0.0) || !std::isfinite(width) || cell < -1)
        return TN_ERR_SHAPE;
    if (num_vertices > 0 && (!positions || !temperature || !distance || !nearest_seed)) return TN_ERR_NULL;
    if (num_triangles > 0 && !triangles) return TN_ERR_NULL;
    if (misaligned(positions, 4) || misaligned(temperature, 4) || misaligned(triangles, 4) || misaligned(distance, 8) ||
        misaligned(nearest_seed, 4) || misaligned(rows, 8) || misaligned(counts, 8) || misaligned(workspace, 8))
        return TN_ERR_SHAPE;
    if (workspace_bytes < tn_mesh_distance_bands_workspace_bytes(num_vertices, num_triangles, bands)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long long nv = (long long)num_vertices, nt = (long long)num_triangles, nk = (long long)bands;
    if (hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), s) != hipSuccess) return TN_ERR_LAUNCH;
    const BandsLayout l = bands_layout(reinterpret_cast<char *>(workspace), nt, nk, reinterpret_cast<long long *>(counts));
    const Groups &g = l.groups;
    const bool with_faces = nt > 0 && nv > 0;
    int code;
    if (with_faces) {
        hipLaunchKernelGGL(band_faces_kernel, dim3((unsigned)tiles_of(nt)), dim3(kTile), 0, s, positions, temperature, triangles, nv, nt,
                           distance, nearest_seed, width, nk, (int)cell, l.records, l.keys, l.lists);
        TN_LAUNCH_CHECK();
        hipLaunchKernelGGL(scan_faces_kernel, dim3(1), dim3(kScan), 0, s, l.lists, tiles_of(nt));
        TN_LAUNCH_CHECK();
        code = tn_sort_pairs(reinterpret_cast<const uint64_t *>(l.keys), nullptr, num_triangles, key_bits((unsigned long long)nk),
                             reinterpret_cast<uint64_t *>(l.sorted), l.order, l.sort, l.sort_bytes, stream);
        if (code != TN_OK) return code;
        if ((code = number_groups(g, l.head_tiles, s)) != TN_OK) return code;
        if ((code = place_blocks(g, l.block_tiles, s)) != TN_OK) return code;
        hipLaunchKernelGGL(band_assign_kernel, dim3((unsigned)tiles_of(nt)), dim3(kTile), 0, s, g);
        TN_LAUNCH_CHECK();
        if ((code = sum_blocks(g, g.capacity, l.records, l.partials, s)) != TN_OK) return code;
    }
    hipLaunchKernelGGL(band_rows_kernel, dim3((unsigned)tiles_of(nk)), dim3(kTile), 0, s, g, with_faces, l.records, l.partials, nk, rows);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

}  // extern "C"
