// Planar patches of an indexed triangle list (DESIGN.md "Planar patches"; include/thermonerf_hip.h defines every output to the bit):
// the geometric faces joined ACROSS EDGES (the half-edge twins of tn_mesh_half_edges) while the angle between their normals stays
// under a limit, and per patch the fitted plane, area, flatness, deviation from the plane and the area-weighted mean / min / max
// temperature.  With the limit at 180 degrees (min_cos = -1) the patches are the edge-connected components.  Launches on the caller's
// stream (the steps marked * are tn_group_sum.h's, shared with tn_mesh_regions.hip):
//   1. faces        one thread per face: GEOMETRIC / THERMAL, the face record (area, thermal area, area x temperature, area x centroid,
//                   the vector area, the face's temperature and box), its unit normal, parent[f] <- f; the tile counts of both kinds
//   2. scan *       one block: the two exclusive scans -> counts[1], the thermal faces
//   3. lists *      the geometric and the thermal faces compacted in face order (the two lists of `totals`)
//   4. hook         one thread per half-edge: where the join predicate holds the two faces are united in the lock-free union-find
//                   of tn_union_find.h over the T faces; the half-edges at which it holds are counted (one integer atomic per block)
//   5. flatten      parent[f] <- the root of f: the smallest face of its patch, the LABEL
//   6. keys, sort   tn_sort_pairs of (label, 0 .. T-1), T for a face that is not geometric: a patch's faces adjacent, in ascending
//                   face index, the patches in ascending label
//   7. heads *      count / scan / emit over the sorted positions: the first position of every run IS the patch's first face, its
//                   rank the patch number q; counts[0] = Q.  A patch's faces are the distance to the next head: no atomics
//   8. blocks *     count / scan / emit over the patches: where the 256-blocks of a patch of MORE than 256 faces start
//   9. assign       one thread per face: face_patch; one thread per sorted position *: the head of every 256-block records where it starts
//  10. block sums * ONE THREAD PER 256-BLOCK walks its faces' records through the sorted order into one partial record
//  11. rows         one thread per patch walks its faces (up to 256: the one block of SUM2) or its blocks' partials in block order and
//                   writes the row: centroid, plane, flatness, temperatures; both deviations NaN
//  12. deviations   one thread per face of a written row: the three corners against the row's plane -> (term, largest |e|)
//  13. block sums, rows   the same two levels over the deviations; the row's rms_deviation and max_deviation
//  14. totals *     the same two levels over the two lists of step 3, areas only
// (8 - 13 are skipped for the sizing call.)  No allocation, no host synchronisation, no float atomics, and no block ever waits for
// another.  A thread's sequential walk is 256 records, then n / 256 partials.  A patch of up to 256 faces has no partial: a mesh of T
// single faces would otherwise need T of them.  The face record is 112 bytes, 16-byte aligned: seven 16-byte loads per face of the
// walk; the unit normal is 32 bytes of its own, which is all the hook kernel gathers from the face across the edge.
#include "tn_device.h"
#include "tn_group_sum.h"
#include "tn_union_find.h"

using namespace tn;

namespace {

constexpr int kTile = kFaceTile;  // faces / half-edges / sorted positions / blocks / patches per thread block of every kernel but the scan

// a face's record, a block's partial and a patch's accumulator are one thing: nine ordered sums, a count and the order-free extremes
struct alignas(16) Acc {
    double s[9];         // area, thermal area, area x temperature, area x centroid x / y / z, vector area x / y / z
    float tmin, tmax;    // of the thermal faces' temperatures
    float lo[3], hi[3];  // of the corners' positions
    int thermal;         // thermal faces
    int pad;
    static constexpr int kAhead = 4;  // records a walk loads ahead of its joins
    static __device__ __forceinline__ Acc empty() {
        Acc a;
#pragma unroll
        for (int k = 0; k < 9; ++k) a.s[k] = 0.0;
        a.tmin = INFINITY, a.tmax = -INFINITY;
#pragma unroll
        for (int k = 0; k < 3; ++k) a.lo[k] = INFINITY, a.hi[k] = -INFINITY;
        a.thermal = 0, a.pad = 0;
        return a;
    }
    // this joined by r, r behind everything this holds: the nine sums take one rounded addition each
    __device__ __forceinline__ void join(const Acc &r) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] = __dadd_rn(s[k], r.s[k]);
        tmin = min_ord(tmin, r.tmin);
        tmax = max_ord(tmax, r.tmax);
#pragma unroll
        for (int k = 0; k < 3; ++k) lo[k] = min_ord(lo[k], r.lo[k]), hi[k] = max_ord(hi[k], r.hi[k]);
        thermal += r.thermal;
    }
};
static_assert(sizeof(Acc) == 112, "seven 16-byte loads");

// the second pass: the ordered sum of the faces' terms and the largest |e| (no NaN gets here: a maximum of numbers is order-free)
struct alignas(16) Dev {
    double term, emax;
    static constexpr int kAhead = 8;
    static __device__ __forceinline__ Dev empty() { return Dev{0.0, 0.0}; }
    __device__ __forceinline__ void join(const Dev &r) {
        term = __dadd_rn(term, r.term);
        emax = r.emax > emax ? r.emax : emax;
    }
};

struct alignas(16) Normal {  // the unit normal of a geometric face; geometric = 0 of every other face
    double u[3];
    long long geometric;
};
static_assert(sizeof(Normal) == 32, "two 16-byte loads");

constexpr int kGeometric = 1, kThermal = 2;

__global__ void __launch_bounds__(kTile)
faces_kernel(const float *__restrict__ positions, const float *__restrict__ temperature, const int *__restrict__ triangles,
             long long num_vertices, long long num_triangles, Acc *__restrict__ records, Normal *__restrict__ normals,
             int *__restrict__ parent, int *__restrict__ flags, FaceLists lists, long long *__restrict__ counts) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    if (t == 0) counts[2] = 0;  // the hook kernel adds to it
    bool geometric = false, thermal = false;
    if (t < num_triangles) {
        const Face f = load_face(positions, temperature, triangles, num_vertices, t);
        Normal n = {{0.0, 0.0, 0.0}, 0};
        if (f.placed && f.n2 > 0.0) {
            geometric = true;
            thermal = f.warm;
            Acc r = Acc::empty();
            r.s[0] = f.area;
            if (thermal) {
                r.s[1] = f.area;
                r.s[2] = __dmul_rn(f.area, (double)f.tf);
                r.tmin = r.tmax = f.tf;
                r.thermal = 1;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                r.s[3 + k] = f.moment[k];
                r.s[6 + k] = __dmul_rn(0.5, f.cr[k]);
                n.u[k] = __ddiv_rn(f.cr[k], f.len);
                r.lo[k] = f.lo[k], r.hi[k] = f.hi[k];
            }
            n.geometric = 1;
            records[t] = r;
        }
        normals[t] = n;
        parent[t] = (int)t;
        flags[t] = (geometric ? kGeometric : 0) | (thermal ? kThermal : 0);
    }
    count_lists(lists, (geometric ? kGeometric : 0) | (thermal ? kThermal : 0));
}

// half-edge h of face f: JOINED with the face of twin[h] iff that is another geometric face and the normals' dot reaches min_cos.
// twin is foreign: its value is used as an index only inside [0, 3T).
__global__ void __launch_bounds__(kTile)
hook_kernel(const int *__restrict__ twin, long long num_triangles, const Normal *__restrict__ normals, double min_cos, int *parent,
            unsigned long long *__restrict__ joined_half_edges) {
    const long long h = (long long)blockIdx.x * kTile + threadIdx.x;
    bool joined = false;
    if (h < 3 * num_triangles) {
        const long long f = h / 3, other = twin[h];
        const long long g = other >= 0 && other < 3 * num_triangles ? other / 3 : f;
        if (g != f) {
            const Normal a = normals[f], b = normals[g];
            if (a.geometric == 1 && b.geometric == 1) {
                const double dot = __dadd_rn(__dadd_rn(__dmul_rn(a.u[0], b.u[0]), __dmul_rn(a.u[1], b.u[1])), __dmul_rn(a.u[2], b.u[2]));
                joined = dot >= min_cos;
            }
            if (joined) unite(parent, (int)f, (int)g);
        }
    }
    uint32_t total;
    block_rank<kTile>(joined, total);
    if (threadIdx.x == 0 && total) atomicAdd(joined_half_edges, (unsigned long long)total);
}

__global__ void __launch_bounds__(kTile)
flatten_kernel(long long num_triangles, int *parent) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    if (t >= num_triangles) return;
    int x = (int)t, p = parent[x];
    while (p != x && p >= 0 && p < x) {  // (parent[x] < x for a non-root: the walk ends)
        x = p;
        p = parent[x];
    }
    if (x != (int)t) parent[t] = x;
}

__global__ void __launch_bounds__(kTile)
keys_kernel(const int *__restrict__ flags, const int *__restrict__ parent, long long num_triangles,
            unsigned long long *__restrict__ keys) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    if (t >= num_triangles) return;
    const long long label = parent[t];
    const bool in = (flags[t] & kGeometric) && label >= 0 && label < num_triangles;
    keys[t] = in ? (unsigned long long)label : (unsigned long long)num_triangles;
}

// face t: face_patch.  Sorted position t (with_blocks, once the blocks are placed): the head of a 256-block records where it starts
__global__ void __launch_bounds__(kTile)
assign_kernel(const int *__restrict__ flags, const int *__restrict__ parent, Groups g, bool with_blocks, int *__restrict__ face_patch) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    if (t >= g.num_triangles) return;
    const long long num_patches = groups_of(g);
    face_patch[t] = (flags[t] & kGeometric) ? group_of(g, parent[t], num_patches) : -1;
    if (with_blocks) block_head(g, t, num_patches);
}

__global__ void __launch_bounds__(kTile)
rows_kernel(Groups g, const Acc *__restrict__ records, const Acc *__restrict__ partials, long long capacity,
            tn_mesh_patch *__restrict__ patches) {
    const long long q = (long long)blockIdx.x * kTile + threadIdx.x;
    const long long num_patches = groups_of(g);
    if (q >= capacity || q >= num_patches) return;
    const long long faces = faces_of(g, q, num_patches);
    const Acc a = group_sum(g, q, faces, records, partials);
    tn_mesh_patch out;
    out.area = a.s[0];
    out.thermal_area = a.s[1];
#pragma unroll
    for (int k = 0; k < 3; ++k) out.centroid[k] = __ddiv_rn(a.s[3 + k], a.s[0]);
    const double nn = __dadd_rn(__dadd_rn(__dmul_rn(a.s[6], a.s[6]), __dmul_rn(a.s[7], a.s[7])), __dmul_rn(a.s[8], a.s[8]));
    if (nn > 0.0) {
        const double len = __dsqrt_rn(nn);
#pragma unroll
        for (int k = 0; k < 3; ++k) out.plane[k] = __ddiv_rn(a.s[6 + k], len);
        out.plane[3] = __dadd_rn(__dadd_rn(__dmul_rn(out.plane[0], out.centroid[0]), __dmul_rn(out.plane[1], out.centroid[1])),
                                 __dmul_rn(out.plane[2], out.centroid[2]));
        out.flatness = (float)__ddiv_rn(len, a.s[0]);
    } else {
        out.plane[0] = out.plane[1] = out.plane[2] = out.plane[3] = 0.0;
        out.flatness = 0.0f;
    }
    out.rms_deviation = out.max_deviation = quiet_nan();  // (with a plane the second pass overwrites both)
    const bool cold = a.s[1] == 0.0;
    out.mean_temperature = cold ? quiet_nan() : (float)__ddiv_rn(a.s[2], a.s[1]);
    out.min_temperature = cold ? quiet_nan() : a.tmin;
    out.max_temperature = cold ? quiet_nan() : a.tmax;
#pragma unroll
    for (int k = 0; k < 3; ++k) out.bounds[k] = a.lo[k], out.bounds[3 + k] = a.hi[k];
    out.label = g.label[q];
    out.faces = (int32_t)faces;
    out.thermal_faces = a.thermal;
    out.reserved = 0;
    patches[q] = out;
}

// a row has a plane iff its normal is not all zero (a unit vector's largest component is at least sqrt(1/3))
__device__ __forceinline__ bool has_plane(const tn_mesh_patch &row) { return row.plane[0] != 0.0 || row.plane[1] != 0.0 || row.plane[2] != 0.0; }

__global__ void __launch_bounds__(kTile)
deviations_kernel(const float *__restrict__ positions, const int *__restrict__ triangles, long long num_vertices, Groups g,
                  const int *__restrict__ face_patch, long long capacity, const tn_mesh_patch *__restrict__ patches,
                  const Acc *__restrict__ records, Dev *__restrict__ deviations) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    if (t >= g.num_triangles) return;
    const long long q = face_patch[t];
    if (q < 0 || q >= capacity || q >= groups_of(g)) return;
    Dev d = Dev::empty();
    const long long i[3] = {triangles[3 * t], triangles[3 * t + 1], triangles[3 * t + 2]};
    const bool ok = i[0] >= 0 && i[0] < num_vertices && i[1] >= 0 && i[1] < num_vertices && i[2] >= 0 && i[2] < num_vertices;
    const double *plane = patches[q].plane, *centre = patches[q].centroid;
    const double n[3] = {plane[0], plane[1], plane[2]}, c[3] = {centre[0], centre[1], centre[2]};
    if (ok && (n[0] != 0.0 || n[1] != 0.0 || n[2] != 0.0)) {
        double e[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float *p = positions + 3 * i[a];
            e[a] = __dadd_rn(__dadd_rn(__dmul_rn(n[0], __dsub_rn((double)p[0], c[0])), __dmul_rn(n[1], __dsub_rn((double)p[1], c[1]))),
                             __dmul_rn(n[2], __dsub_rn((double)p[2], c[2])));
            const double m = fabs(e[a]);
            d.emax = m > d.emax ? m : d.emax;
        }
        const double s = __dadd_rn(__dadd_rn(e[0], e[1]), e[2]);
        const double squares = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(e[0], e[0]), __dmul_rn(e[1], e[1])), __dmul_rn(e[2], e[2])),
                                         __dmul_rn(s, s));
        d.term = __dmul_rn(__ddiv_rn(records[t].s[0], 12.0), squares);
    }
    deviations[t] = d;
}

__global__ void __launch_bounds__(kTile)
finish_rows_kernel(Groups g, const Dev *__restrict__ deviations, const Dev *__restrict__ partials, long long capacity,
                   tn_mesh_patch *__restrict__ patches) {
    const long long q = (long long)blockIdx.x * kTile + threadIdx.x;
    const long long num_patches = groups_of(g);
    if (q >= capacity || q >= num_patches || !has_plane(patches[q])) return;
    const Dev d = group_sum(g, q, faces_of(g, q, num_patches), deviations, partials);
    patches[q].rms_deviation = (float)__dsqrt_rn(__ddiv_rn(d.term, patches[q].area));
    patches[q].max_deviation = (float)d.emax;
}

inline long long tiles_of(long long n) { return ceil_div(n, kTile); }

// the workspace, in order: the face records (16-byte aligned: up to 8 bytes of slack in front), their block partials, the unit
// normals, the deviations and their block partials, the totals' partials, the sort keys and the sorted keys, the device sums (thermal
// faces, blocks), four arrays of tile counts, then the int arrays per face (parent, flags, two lists, order, of_label), per patch
// (label, first_face, first_block) and per block (block_first), and the sort's own workspace
struct Layout {
    Acc *records, *partials;
    Normal *normals;
    Dev *deviations, *deviation_partials;
    double *total_partials;
    unsigned long long *keys, *sorted;
    long long *sums, *head_tiles, *block_tiles;
    int *parent, *flags, *order;
    FaceLists lists;  // 0: the geometric faces, counts[1] of them; 1: the thermal faces, sums[0] of them
    Groups patches;   // the labels are faces: L = T, and a patch may be one face: capacity = T
    void *sort;
    size_t sort_bytes, bytes;
};

inline Layout layout_of(char *ws, long long t, long long *counts) {
    Layout l;
    size_t at = ws ? (size_t)(reinterpret_cast<uintptr_t>(ws) % 16) : 8;  // ws is 8-byte aligned: 0 or 8; sized for 8
    const size_t skip = at;
    auto take = [&](size_t bytes) {  // (ws == NULL: the sizes alone)
        char *p = ws ? ws + at : nullptr;
        at += bytes;
        return p;
    };
    Groups &g = l.patches;
    g.num_triangles = g.labels = g.capacity = t;
    g.direct = kSumBlock;            // a mesh of T single faces would otherwise need T partials
    g.max_blocks = 2 * tiles_of(t);  // only patches of more than 256 faces have blocks: sum of ceil(n / 256) < T / 256 + T / 256
    l.records = reinterpret_cast<Acc *>(take((size_t)t * sizeof(Acc)));
    l.partials = reinterpret_cast<Acc *>(take((size_t)g.max_blocks * sizeof(Acc)));
    l.normals = reinterpret_cast<Normal *>(take((size_t)t * sizeof(Normal)));
    l.deviations = reinterpret_cast<Dev *>(take((size_t)t * sizeof(Dev)));
    l.deviation_partials = reinterpret_cast<Dev *>(take((size_t)g.max_blocks * sizeof(Dev)));
    l.total_partials = reinterpret_cast<double *>(take((size_t)(2 * ceil_div(t, kSumBlock)) * sizeof(double)));
    l.keys = reinterpret_cast<unsigned long long *>(take((size_t)t * sizeof(unsigned long long)));
    l.sorted = reinterpret_cast<unsigned long long *>(take((size_t)t * sizeof(unsigned long long)));
    l.sums = reinterpret_cast<long long *>(take(2 * sizeof(long long)));
    long long **tiles[4] = {&l.lists.tiles[0], &l.lists.tiles[1], &l.head_tiles, &l.block_tiles};
    for (auto p : tiles) *p = reinterpret_cast<long long *>(take((size_t)tiles_of(t) * sizeof(long long)));
    int **per_face[9] = {&l.parent, &l.flags, &l.lists.faces[0], &l.lists.faces[1], &l.order, &g.of_label, &g.label, &g.first_face,
                         &g.first_block};
    for (auto p : per_face) *p = reinterpret_cast<int *>(take(ints_bytes(t)));
    g.block_first = reinterpret_cast<int *>(take(ints_bytes(g.max_blocks)));
    l.sort_bytes = tn_sort_pairs_workspace_bytes(t);
    l.sort = take(l.sort_bytes);
    l.bytes = at - skip + 8;
    l.lists.bit[0] = kGeometric, l.lists.bit[1] = kThermal;
    l.lists.length[0] = counts ? counts + 1 : nullptr, l.lists.length[1] = l.sums;
    g.sorted = l.sorted, g.order = l.order, g.counts = counts, g.num_blocks = l.sums + 1;
    return l;
}

}  // namespace

extern "C" {

size_t tn_mesh_patches_workspace_bytes(int64_t num_vertices, int64_t num_triangles) {
    if (bad_counts(num_vertices, num_triangles)) return 0;
    return layout_of(nullptr, (long long)num_triangles, nullptr).bytes;
}

int tn_mesh_patches(const float *positions, const float *temperature, const int32_t *triangles, int64_t num_vertices,
                    int64_t num_triangles, const int32_t *twin, double min_cos, tn_mesh_patch *patches, int64_t capacity_patches,
                    int32_t *face_patch, int64_t *counts, double *totals, void *workspace, size_t workspace_bytes, void *stream) {
    if (!counts || !totals) return TN_ERR_NULL;
    if (bad_counts(num_vertices, num_triangles) || capacity_patches < 0) return TN_ERR_SHAPE;
    if (!(min_cos >= -1.0 && min_cos <= 1.0)) return TN_ERR_UNSUPPORTED;  // (a NaN fails both)
    const bool work = num_vertices > 0 && num_triangles > 0;
    if (work && (!positions || !temperature || !twin || !workspace)) return TN_ERR_NULL;
    if (num_triangles > 0 && (!triangles || !face_patch)) return TN_ERR_NULL;
    if (capacity_patches > 0 && !patches) return TN_ERR_NULL;
    if (misaligned(positions, 4) || misaligned(temperature, 4) || misaligned(triangles, 4) || misaligned(twin, 4) ||
        misaligned(face_patch, 4) || misaligned(patches, 8) || misaligned(counts, 8) || misaligned(totals, 8) || misaligned(workspace, 8))
        return TN_ERR_SHAPE;
    if (work && workspace_bytes < tn_mesh_patches_workspace_bytes(num_vertices, num_triangles)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long long nv = (long long)num_vertices, nt = (long long)num_triangles;
    if (!work) {
        if (hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), s) != hipSuccess) return TN_ERR_LAUNCH;
        if (hipMemsetAsync(totals, 0, 2 * sizeof(double), s) != hipSuccess) return TN_ERR_LAUNCH;
        if (nt > 0 && hipMemsetAsync(face_patch, 0xff, (size_t)nt * sizeof(int32_t), s) != hipSuccess) return TN_ERR_LAUNCH;
        return TN_OK;
    }
    long long *cnt = reinterpret_cast<long long *>(counts);
    const Layout l = layout_of(reinterpret_cast<char *>(workspace), nt, cnt);
    const Groups &g = l.patches;
    const unsigned face_blocks = (unsigned)tiles_of(nt);
    const bool rows = capacity_patches > 0;
    const long long cap = (long long)capacity_patches;
    int code;

    // 1 - 3: the faces, the two counts, the two lists
    hipLaunchKernelGGL(faces_kernel, dim3(face_blocks), dim3(kTile), 0, s, positions, temperature, triangles, nv, nt, l.records, l.normals,
                       l.parent, l.flags, l.lists, cnt);
    TN_LAUNCH_CHECK();
    if ((code = list_faces(l.lists, l.flags, nt, s)) != TN_OK) return code;

    // 4 - 5: the patches as trees over the faces, then every face under its label
    hipLaunchKernelGGL(hook_kernel, dim3((unsigned)tiles_of(3 * nt)), dim3(kTile), 0, s, twin, nt, l.normals, min_cos, l.parent,
                       reinterpret_cast<unsigned long long *>(cnt + 2));
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(flatten_kernel, dim3(face_blocks), dim3(kTile), 0, s, nt, l.parent);
    TN_LAUNCH_CHECK();

    // 6 - 7: a patch's faces adjacent in ascending face index; the patches numbered in ascending label
    hipLaunchKernelGGL(keys_kernel, dim3(face_blocks), dim3(kTile), 0, s, l.flags, l.parent, nt, l.keys);
    TN_LAUNCH_CHECK();
    code = tn_sort_pairs(reinterpret_cast<const uint64_t *>(l.keys), nullptr, num_triangles, key_bits((unsigned long long)nt),  // 0 .. T
                         reinterpret_cast<uint64_t *>(l.sorted), l.order, l.sort, l.sort_bytes, stream);
    if (code != TN_OK) return code;
    if ((code = number_groups(g, l.head_tiles, s)) != TN_OK) return code;

    // 8 - 9: where the blocks start; face_patch
    if (rows && (code = place_blocks(g, l.block_tiles, s)) != TN_OK) return code;
    hipLaunchKernelGGL(assign_kernel, dim3(face_blocks), dim3(kTile), 0, s, l.flags, l.parent, g, rows, face_patch);
    TN_LAUNCH_CHECK();

    // 10 - 13: the first pass and the rows, the second pass and the rows' deviations
    if (rows) {
        const unsigned row_blocks = (unsigned)tiles_of(cap < nt ? cap : nt);
        if ((code = sum_blocks(g, nt, l.records, l.partials, s)) != TN_OK) return code;
        hipLaunchKernelGGL(rows_kernel, dim3(row_blocks), dim3(kTile), 0, s, g, l.records, l.partials, cap, patches);
        TN_LAUNCH_CHECK();
        hipLaunchKernelGGL(deviations_kernel, dim3(face_blocks), dim3(kTile), 0, s, positions, triangles, nv, g, face_patch, cap, patches,
                           l.records, l.deviations);
        TN_LAUNCH_CHECK();
        if ((code = sum_blocks(g, cap, l.deviations, l.deviation_partials, s)) != TN_OK) return code;
        hipLaunchKernelGGL(finish_rows_kernel, dim3(row_blocks), dim3(kTile), 0, s, g, l.deviations, l.deviation_partials, cap, patches);
        TN_LAUNCH_CHECK();
    }

    // 14: the mesh's area and the thermal area
    return list_totals(l.lists, nt, l.records, l.total_partials, totals, s);
}

}  // extern "C"
