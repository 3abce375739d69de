// Planar patches of an indexed triangle list (DESIGN.md "Planar patches"; include/thermonerf_hip.h defines every output to the bit):
// the geometric faces joined ACROSS EDGES (the half-edge twins of tn_mesh_half_edges) while the angle between their normals stays
// under a limit, and per patch the fitted plane, area, flatness, deviation from the plane and the area-weighted mean / min / max
// temperature.  With the limit at 180 degrees (min_cos = -1) the patches are the edge-connected components.  Launches on the caller's
// stream:
//   1. faces        one thread per face: GEOMETRIC / THERMAL, the face record (area, thermal area, area x temperature, area x centroid,
//                   the vector area, the face's temperature and box), its unit normal, parent[f] <- f; the tile counts of both kinds
//   2. scan         one block: the two exclusive scans -> counts[1], the thermal faces
//   3. lists        the geometric and the thermal faces compacted in face order (the two lists of `totals`)
//   4. hook         one thread per half-edge: where the join predicate holds the two faces are united in the lock-free union-find
//                   of tn_union_find.h over the T faces; the half-edges at which it holds are counted (one integer atomic per block)
//   5. flatten      parent[f] <- the root of f: the smallest face of its patch, the LABEL
//   6. keys, sort   tn_sort_pairs of (label, 0 .. T-1), T for a face that is not geometric: a patch's faces adjacent, in ascending
//                   face index, the patches in ascending label
//   7. heads        count / scan / emit over the sorted positions: the first position of every run IS the patch's first face, its
//                   rank the patch number q; counts[0] = Q.  A patch's faces are the distance to the next head: no atomics
//   8. blocks       count / scan / emit over the patches: where the 256-blocks of a patch of MORE than 256 faces start
//   9. assign       one thread per face: face_patch; one thread per sorted position: the head of every 256-block records where it starts
//  10. block sums   ONE THREAD PER 256-BLOCK walks its faces' records through the sorted order into one partial record
//  11. rows         one thread per patch walks its faces (up to 256: the one block of SUM2) or its blocks' partials in block order and
//                   writes the row: centroid, plane, flatness, temperatures; both deviations NaN
//  12. deviations   one thread per face of a written row: the three corners against the row's plane -> (term, largest |e|)
//  13. block sums, rows   the same two levels over the deviations; the row's rms_deviation and max_deviation
//  14. totals       the same two levels over the two lists of step 3, areas only
// (8 - 13 are skipped for the sizing call.)  No allocation, no host synchronisation, no float atomics, and no block ever waits for
// another.  A thread's sequential walk is 256 records, then n / 256 partials.  A patch of up to 256 faces has no partial: a mesh of T
// single faces would otherwise need T of them.  The face record is 112 bytes, 16-byte aligned: seven 16-byte loads per face of the
// walk; the unit normal is 32 bytes of its own, which is all the hook kernel gathers from the face across the edge.
#include "tn_device.h"
#include "tn_scan.h"
#include "tn_union_find.h"

using namespace tn;

namespace {

constexpr int kTile = 256;   // faces / half-edges / sorted positions / blocks / patches per thread block of every kernel but the scan
constexpr int kBlock = 256;  // entries per block of SUM2

// a face's record, a block's partial and a patch's accumulator are one thing: nine ordered sums, a count and the order-free extremes
struct alignas(16) Acc {
    double s[9];         // area, thermal area, area x temperature, area x centroid x / y / z, vector area x / y / z
    float tmin, tmax;    // of the thermal faces' temperatures
    float lo[3], hi[3];  // of the corners' positions
    int thermal;         // thermal faces
    int pad;
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
             int *__restrict__ parent, int *__restrict__ flags, long long *__restrict__ geometric_tiles,
             long long *__restrict__ thermal_tiles, long long *__restrict__ counts) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    if (t == 0) counts[2] = 0;  // the hook kernel adds to it
    bool geometric = false, thermal = false;
    if (t < num_triangles) {
        const long long i[3] = {triangles[3 * t], triangles[3 * t + 1], triangles[3 * t + 2]};
        bool ok = i[0] >= 0 && i[0] < num_vertices && i[1] >= 0 && i[1] < num_vertices && i[2] >= 0 && i[2] < num_vertices;
        ok = ok && i[0] != i[1] && i[1] != i[2] && i[0] != i[2];
        float p[3][3], c[3];
        bool warm = ok;
        if (ok) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                c[a] = temperature[i[a]];
                warm = warm && finite(c[a]);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    p[a][k] = positions[3 * i[a] + k];
                    ok = ok && finite(p[a][k]);
                }
            }
        }
        Normal n = {{0.0, 0.0, 0.0}, 0};
        if (ok) {
            double e1[3], e2[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                e1[k] = __dsub_rn((double)p[1][k], (double)p[0][k]);
                e2[k] = __dsub_rn((double)p[2][k], (double)p[0][k]);
            }
            const double cr[3] = {__dsub_rn(__dmul_rn(e1[1], e2[2]), __dmul_rn(e1[2], e2[1])),
                                  __dsub_rn(__dmul_rn(e1[2], e2[0]), __dmul_rn(e1[0], e2[2])),
                                  __dsub_rn(__dmul_rn(e1[0], e2[1]), __dmul_rn(e1[1], e2[0]))};
            const double n2 = __dadd_rn(__dadd_rn(__dmul_rn(cr[0], cr[0]), __dmul_rn(cr[1], cr[1])), __dmul_rn(cr[2], cr[2]));
            if (n2 > 0.0) {
                geometric = true;
                thermal = warm;
                const double len = __dsqrt_rn(n2), area = __dmul_rn(0.5, len);
                Acc r = Acc::empty();
                r.s[0] = area;
                if (thermal) {
                    const float tf = (float)__ddiv_rn(__dadd_rn(__dadd_rn((double)c[0], (double)c[1]), (double)c[2]), 3.0);
                    r.s[1] = area;
                    r.s[2] = __dmul_rn(area, (double)tf);
                    r.tmin = r.tmax = tf;
                    r.thermal = 1;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double centre = __ddiv_rn(__dadd_rn(__dadd_rn((double)p[0][k], (double)p[1][k]), (double)p[2][k]), 3.0);
                    r.s[3 + k] = __dmul_rn(area, centre);
                    r.s[6 + k] = __dmul_rn(0.5, cr[k]);
                    n.u[k] = __ddiv_rn(cr[k], len);
                }
#pragma unroll
                for (int a = 0; a < 3; ++a) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) r.lo[k] = min_ord(r.lo[k], p[a][k]), r.hi[k] = max_ord(r.hi[k], p[a][k]);
                }
                n.geometric = 1;
                records[t] = r;
            }
        }
        normals[t] = n;
        parent[t] = (int)t;
        flags[t] = (geometric ? kGeometric : 0) | (thermal ? kThermal : 0);
    }
    uint32_t total;
    block_rank<kTile>(geometric, total);
    if (threadIdx.x == 0) geometric_tiles[blockIdx.x] = (long long)total;
    __syncthreads();  // block_rank's LDS is rewritten by the second call
    block_rank<kTile>(thermal, total);
    if (threadIdx.x == 0) thermal_tiles[blockIdx.x] = (long long)total;
}

// sums: [0] the thermal faces, [1] the 256-blocks of the patches that have any
__global__ void __launch_bounds__(kScan)
scan_faces_kernel(long long *__restrict__ geometric_tiles, long long *__restrict__ thermal_tiles, long long num_tiles,
                  long long *__restrict__ counts, long long *__restrict__ sums) {
    scan_tiles<false>(geometric_tiles, num_tiles, counts + 1);
    __syncthreads();
    scan_tiles<false>(thermal_tiles, num_tiles, sums);
}

__global__ void __launch_bounds__(kTile)
lists_kernel(const int *__restrict__ flags, long long num_triangles, const long long *__restrict__ geometric_tiles,
             const long long *__restrict__ thermal_tiles, int *__restrict__ geometric_list, int *__restrict__ thermal_list) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    const int f = t < num_triangles ? flags[t] : 0;
    uint32_t unused;
    const uint32_t before_geometric = block_rank<kTile>((f & kGeometric) != 0, unused);
    __syncthreads();
    const uint32_t before_thermal = block_rank<kTile>((f & kThermal) != 0, unused);
    if (f & kGeometric) {
        const long long o = geometric_tiles[blockIdx.x] + (long long)before_geometric;  // <= t
        if (o >= 0 && o < num_triangles) geometric_list[o] = (int)t;
    }
    if (f & kThermal) {
        const long long o = thermal_tiles[blockIdx.x] + (long long)before_thermal;
        if (o >= 0 && o < num_triangles) thermal_list[o] = (int)t;
    }
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

// sorted position j is the HEAD of a patch iff it holds a label and the position before it holds another
__device__ __forceinline__ bool is_head(const unsigned long long *__restrict__ sorted, long long j, long long num_triangles) {
    if (j >= num_triangles) return false;
    const unsigned long long key = sorted[j];
    return key < (unsigned long long)num_triangles && (j == 0 || sorted[j - 1] != key);
}

__global__ void __launch_bounds__(kTile)
count_heads_kernel(const unsigned long long *__restrict__ sorted, long long num_triangles, long long *__restrict__ head_tiles) {
    const long long j = (long long)blockIdx.x * kTile + threadIdx.x;
    uint32_t total;
    block_rank<kTile>(is_head(sorted, j, num_triangles), total);
    if (threadIdx.x == 0) head_tiles[blockIdx.x] = (long long)total;
}

__global__ void __launch_bounds__(kScan)
scan_counts_kernel(long long *__restrict__ tiles, long long num_tiles, long long *__restrict__ count) {
    scan_tiles<false>(tiles, num_tiles, count);
}

struct Patches {  // per label: its patch; per patch: its label, where its faces start in the sorted order, where its blocks start
    int *of_label, *label, *first_face, *first_block;
};

__global__ void __launch_bounds__(kTile)
emit_heads_kernel(const unsigned long long *__restrict__ sorted, long long num_triangles, const long long *__restrict__ head_tiles,
                  Patches out) {
    const long long j = (long long)blockIdx.x * kTile + threadIdx.x;
    const bool head = is_head(sorted, j, num_triangles);
    uint32_t unused;
    const uint32_t before = block_rank<kTile>(head, unused);
    if (!head) return;
    const long long q = head_tiles[blockIdx.x] + (long long)before;  // <= j
    if (q < 0 || q >= num_triangles) return;
    const long long label = (long long)sorted[j];
    out.label[q] = (int)label;
    out.first_face[q] = (int)j;
    out.of_label[label] = (int)q;
}

// the faces of patch q < Q: up to the next patch's first face, the last one up to the geometric faces
__device__ __forceinline__ long long faces_of(const Patches &g, long long q, long long num_patches, long long num_geometric,
                                              long long num_triangles) {
    const long long first = g.first_face[q];
    long long end = q + 1 < num_patches ? (long long)g.first_face[q + 1] : num_geometric;
    end = end < num_triangles ? end : num_triangles;
    return first >= 0 && end > first ? end - first : 0;
}

// a patch of up to 256 faces is walked by its row's thread and has no partial
__device__ __forceinline__ uint32_t blocks_of(long long faces) { return faces > kBlock ? (uint32_t)((faces + kBlock - 1) / kBlock) : 0u; }

__device__ __forceinline__ long long patches_of(const long long *__restrict__ counts, long long num_triangles) {
    const long long q = counts[0];
    return q < 0 ? 0 : (q < num_triangles ? q : num_triangles);
}

__global__ void __launch_bounds__(kTile)
count_blocks_kernel(Patches g, const long long *__restrict__ counts, long long num_triangles, long long *__restrict__ block_tiles) {
    const long long q = (long long)blockIdx.x * kTile + threadIdx.x;
    const long long num_patches = patches_of(counts, num_triangles);
    const uint32_t own = q < num_patches ? blocks_of(faces_of(g, q, num_patches, counts[1], num_triangles)) : 0u;
    uint32_t total;
    block_exclusive<kTile>(own, total);
    if (threadIdx.x == 0) block_tiles[blockIdx.x] = (long long)total;
}

__global__ void __launch_bounds__(kTile)
emit_blocks_kernel(Patches g, const long long *__restrict__ counts, long long num_triangles, const long long *__restrict__ block_tiles) {
    const long long q = (long long)blockIdx.x * kTile + threadIdx.x;
    const long long num_patches = patches_of(counts, num_triangles);
    const uint32_t own = q < num_patches ? blocks_of(faces_of(g, q, num_patches, counts[1], num_triangles)) : 0u;
    uint32_t unused;
    const uint32_t before = block_exclusive<kTile>(own, unused);
    if (q < num_patches) g.first_block[q] = (int)(block_tiles[blockIdx.x] + (long long)before);
}

// the patch of a label, or -1; checks what it reads
__device__ __forceinline__ int patch_of(const Patches &g, long long label, long long num_patches, long long num_triangles) {
    if (label < 0 || label >= num_triangles) return -1;
    const int q = g.of_label[label];
    return q >= 0 && q < num_patches && g.label[q] == (int)label ? q : -1;
}

// face t: face_patch.  Sorted position t: it starts block (t - first face) / 256 of its patch iff that is a whole number and the
// patch has blocks
__global__ void __launch_bounds__(kTile)
assign_kernel(const int *__restrict__ flags, const int *__restrict__ parent, const unsigned long long *__restrict__ sorted,
              long long num_triangles, Patches g, const long long *__restrict__ counts, long long max_blocks,
              int *__restrict__ face_patch, int *__restrict__ block_first) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    if (t >= num_triangles) return;
    const long long num_patches = patches_of(counts, num_triangles);
    face_patch[t] = (flags[t] & kGeometric) ? patch_of(g, parent[t], num_patches, num_triangles) : -1;
    if (!block_first) return;
    const unsigned long long key = sorted[t];
    if (key >= (unsigned long long)num_triangles) return;
    const int q = patch_of(g, (long long)key, num_patches, num_triangles);
    if (q < 0 || blocks_of(faces_of(g, q, num_patches, counts[1], num_triangles)) == 0) return;
    const long long d = t - (long long)g.first_face[q];
    if (d < 0 || d % kBlock != 0) return;
    const long long b = (long long)g.first_block[q] + d / kBlock;
    if (b >= 0 && b < max_blocks) block_first[b] = (int)t;
}

// the records where(first) .. where(end - 1) joined in that order into one.  A lone thread's walk is a chain of memory round trips unless
// the loads go out ahead of the additions: U addresses, then U loads, then U joins — the same joins in the same order (joining an empty
// record changes nothing: a sum that started from +0.0 is never -0.0).
template <typename R, typename Where>
__device__ __forceinline__ R join_run(long long first, long long end, Where where) {
    constexpr int U = sizeof(R) > 64 ? 4 : 8;
    R a = R::empty();
    for (long long j = first; j < end; j += U) {
        const R *p[U];
        R r[U];
#pragma unroll
        for (int k = 0; k < U; ++k) p[k] = j + k < end ? where(j + k) : nullptr;
#pragma unroll
        for (int k = 0; k < U; ++k) r[k] = p[k] ? *p[k] : R::empty();
#pragma unroll
        for (int k = 0; k < U; ++k) a.join(r[k]);
    }
    return a;
}

// the sorted positions first .. end - 1 walked in order into one record
template <typename R>
__device__ __forceinline__ R walk(const int *__restrict__ order, const R *__restrict__ records, long long first, long long end,
                                  long long num_triangles) {
    end = end < num_triangles ? end : num_triangles;
    return join_run<R>(first < 0 ? 0 : first, end, [&](long long j) -> const R * {
        const long long t = order[j];
        return t >= 0 && t < num_triangles ? records + t : nullptr;
    });
}

// rows: the patches whose rows are written (q < min(Q, capacity)); the second pass has records for no other
template <typename R>
__global__ void __launch_bounds__(kTile)
block_sums_kernel(const unsigned long long *__restrict__ sorted, const int *__restrict__ order, long long num_triangles, Patches g,
                  const long long *__restrict__ counts, long long rows, const R *__restrict__ records,
                  const int *__restrict__ block_first, const long long *__restrict__ num_blocks, long long max_blocks,
                  R *__restrict__ partials) {
    const long long b = (long long)blockIdx.x * kTile + threadIdx.x;
    if (b >= max_blocks || b >= num_blocks[0]) return;
    R a = R::empty();
    const long long j0 = block_first[b];
    if (j0 >= 0 && j0 < num_triangles) {
        const long long num_patches = patches_of(counts, num_triangles);
        const unsigned long long key = sorted[j0];
        const int q = key < (unsigned long long)num_triangles ? patch_of(g, (long long)key, num_patches, num_triangles) : -1;
        if (q >= 0 && q < rows) {
            const long long end = (long long)g.first_face[q] + faces_of(g, q, num_patches, counts[1], num_triangles);
            a = walk(order, records, j0, end < j0 + kBlock ? end : j0 + kBlock, num_triangles);
        }
    }
    partials[b] = a;
}

// SUM2 over the faces of patch q: its one block, or its blocks' partials in block order
template <typename R>
__device__ __forceinline__ R patch_sum(const Patches &g, long long q, long long faces, const int *__restrict__ order,
                                       const R *__restrict__ records, const R *__restrict__ partials, long long num_blocks,
                                       long long max_blocks, long long num_triangles) {
    if (blocks_of(faces) == 0) return walk(order, records, g.first_face[q], (long long)g.first_face[q] + faces, num_triangles);
    long long b = g.first_block[q], end = b + (long long)blocks_of(faces);
    end = end < max_blocks ? end : max_blocks;
    end = end < num_blocks ? end : num_blocks;
    return join_run<R>(b < 0 ? 0 : b, end, [&](long long k) -> const R * { return partials + k; });
}

__global__ void __launch_bounds__(kTile)
rows_kernel(Patches g, const long long *__restrict__ counts, long long num_triangles, const int *__restrict__ order,
            const Acc *__restrict__ records, const Acc *__restrict__ partials, const long long *__restrict__ num_blocks,
            long long max_blocks, long long capacity, tn_mesh_patch *__restrict__ patches) {
    const long long q = (long long)blockIdx.x * kTile + threadIdx.x;
    const long long num_patches = patches_of(counts, num_triangles);
    if (q >= capacity || q >= num_patches) return;
    const long long faces = faces_of(g, q, num_patches, counts[1], num_triangles);
    const Acc a = patch_sum(g, q, faces, order, records, partials, num_blocks[0], max_blocks, num_triangles);
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
deviations_kernel(const float *__restrict__ positions, const int *__restrict__ triangles, long long num_vertices,
                  long long num_triangles, const int *__restrict__ face_patch, const long long *__restrict__ counts, long long capacity,
                  const tn_mesh_patch *__restrict__ patches, const Acc *__restrict__ records, Dev *__restrict__ deviations) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    if (t >= num_triangles) return;
    const long long q = face_patch[t];
    if (q < 0 || q >= capacity || q >= patches_of(counts, num_triangles)) return;
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
finish_rows_kernel(Patches g, const long long *__restrict__ counts, long long num_triangles, const int *__restrict__ order,
                   const Dev *__restrict__ deviations, const Dev *__restrict__ partials, const long long *__restrict__ num_blocks,
                   long long max_blocks, long long capacity, tn_mesh_patch *__restrict__ patches) {
    const long long q = (long long)blockIdx.x * kTile + threadIdx.x;
    const long long num_patches = patches_of(counts, num_triangles);
    if (q >= capacity || q >= num_patches || !has_plane(patches[q])) return;
    const long long faces = faces_of(g, q, num_patches, counts[1], num_triangles);
    const Dev d = patch_sum(g, q, faces, order, deviations, partials, num_blocks[0], max_blocks, num_triangles);
    patches[q].rms_deviation = (float)__dsqrt_rn(__ddiv_rn(d.term, patches[q].area));
    patches[q].max_deviation = (float)d.emax;
}

// the two lists of `totals`: y = 0 the geometric faces (their number is counts[1]), y = 1 the thermal ones (sums[0])
__device__ __forceinline__ long long list_length(const long long *__restrict__ counts, const long long *__restrict__ sums, int y,
                                                 long long num_triangles) {
    const long long n = y ? sums[0] : counts[1];
    return n < 0 ? 0 : (n < num_triangles ? n : num_triangles);
}

__global__ void __launch_bounds__(kTile)
total_blocks_kernel(const int *__restrict__ geometric_list, const int *__restrict__ thermal_list, const long long *__restrict__ counts,
                    const long long *__restrict__ sums, long long num_triangles, const Acc *__restrict__ records,
                    long long blocks_per_list, double *__restrict__ partials) {
    const long long b = (long long)blockIdx.x * kTile + threadIdx.x;
    const int y = blockIdx.y;
    const long long n = list_length(counts, sums, y, num_triangles);
    if (b >= blocks_per_list || b * kBlock >= n) return;
    const int *list = y ? thermal_list : geometric_list;
    const long long end = (b + 1) * kBlock < n ? (b + 1) * kBlock : n;
    double s = 0.0;
    for (long long k = b * kBlock; k < end; ++k) {
        const long long t = list[k];
        if (t >= 0 && t < num_triangles) s = __dadd_rn(s, records[t].s[0]);
    }
    partials[y * blocks_per_list + b] = s;
}

__global__ void totals_kernel(const long long *__restrict__ counts, const long long *__restrict__ sums, long long num_triangles,
                              long long blocks_per_list, const double *__restrict__ partials, double *__restrict__ totals) {
    if (threadIdx.x != 0) return;
    const int y = blockIdx.x;
    const long long n = list_length(counts, sums, y, num_triangles);
    long long blocks = (n + kBlock - 1) / kBlock;
    blocks = blocks < blocks_per_list ? blocks : blocks_per_list;
    double s = 0.0;
    for (long long b = 0; b < blocks; ++b) s = __dadd_rn(s, partials[y * blocks_per_list + b]);
    totals[y] = s;
}

inline long long tiles_of(long long n) { return ceil_div(n, kTile); }

inline size_t ints_bytes(long long n) { return ((size_t)n * sizeof(int) + 7) / 8 * 8; }

inline int key_bits(long long num_triangles) {  // the keys are 0 .. T
    int bits = 1;
    while (bits < 63 && (1LL << bits) <= num_triangles) ++bits;
    return bits;
}

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
    long long *sums, *geometric_tiles, *thermal_tiles, *head_tiles, *block_tiles;
    int *parent, *flags, *geometric_list, *thermal_list, *order, *block_first;
    Patches patches;
    long long max_blocks, blocks_per_list;
    void *sort;
    size_t sort_bytes, bytes;
};

inline Layout layout_of(char *ws, long long t) {
    Layout l;
    size_t at = ws ? (size_t)(reinterpret_cast<uintptr_t>(ws) % 16) : 8;  // ws is 8-byte aligned: 0 or 8; sized for 8
    const size_t skip = at;
    auto take = [&](size_t bytes) {  // (ws == NULL: the sizes alone)
        char *p = ws ? ws + at : nullptr;
        at += bytes;
        return p;
    };
    l.max_blocks = 2 * tiles_of(t);  // only patches of more than 256 faces have blocks: sum of ceil(n / 256) < T / 256 + T / 256
    l.blocks_per_list = ceil_div(t, kBlock);
    l.records = reinterpret_cast<Acc *>(take((size_t)t * sizeof(Acc)));
    l.partials = reinterpret_cast<Acc *>(take((size_t)l.max_blocks * sizeof(Acc)));
    l.normals = reinterpret_cast<Normal *>(take((size_t)t * sizeof(Normal)));
    l.deviations = reinterpret_cast<Dev *>(take((size_t)t * sizeof(Dev)));
    l.deviation_partials = reinterpret_cast<Dev *>(take((size_t)l.max_blocks * sizeof(Dev)));
    l.total_partials = reinterpret_cast<double *>(take((size_t)(2 * l.blocks_per_list) * sizeof(double)));
    l.keys = reinterpret_cast<unsigned long long *>(take((size_t)t * sizeof(unsigned long long)));
    l.sorted = reinterpret_cast<unsigned long long *>(take((size_t)t * sizeof(unsigned long long)));
    l.sums = reinterpret_cast<long long *>(take(2 * sizeof(long long)));
    long long **tiles[4] = {&l.geometric_tiles, &l.thermal_tiles, &l.head_tiles, &l.block_tiles};
    for (auto p : tiles) *p = reinterpret_cast<long long *>(take((size_t)tiles_of(t) * sizeof(long long)));
    int **per_face[9] = {&l.parent, &l.flags, &l.geometric_list, &l.thermal_list, &l.order, &l.patches.of_label, &l.patches.label,
                         &l.patches.first_face, &l.patches.first_block};
    for (auto p : per_face) *p = reinterpret_cast<int *>(take(ints_bytes(t)));
    l.block_first = reinterpret_cast<int *>(take(ints_bytes(l.max_blocks)));
    l.sort_bytes = tn_sort_pairs_workspace_bytes(t);
    l.sort = take(l.sort_bytes);
    l.bytes = at - skip + 8;
    return l;
}

}  // namespace

extern "C" {

size_t tn_mesh_patches_workspace_bytes(int64_t num_vertices, int64_t num_triangles) {
    if (bad_counts(num_vertices, num_triangles)) return 0;
    return layout_of(nullptr, (long long)num_triangles).bytes;
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
    const Layout l = layout_of(reinterpret_cast<char *>(workspace), nt);
    long long *cnt = reinterpret_cast<long long *>(counts);
    const unsigned face_blocks = (unsigned)tiles_of(nt), block_blocks = (unsigned)tiles_of(l.max_blocks);
    const bool rows = capacity_patches > 0;
    const long long cap = (long long)capacity_patches;
    int code;

    // 1 - 3: the faces, the two counts, the two lists
    hipLaunchKernelGGL(faces_kernel, dim3(face_blocks), dim3(kTile), 0, s, positions, temperature, triangles, nv, nt, l.records, l.normals,
                       l.parent, l.flags, l.geometric_tiles, l.thermal_tiles, cnt);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_faces_kernel, dim3(1), dim3(kScan), 0, s, l.geometric_tiles, l.thermal_tiles, tiles_of(nt), cnt, l.sums);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(lists_kernel, dim3(face_blocks), dim3(kTile), 0, s, l.flags, nt, l.geometric_tiles, l.thermal_tiles,
                       l.geometric_list, l.thermal_list);
    TN_LAUNCH_CHECK();

    // 4 - 5: the patches as trees over the faces, then every face under its label
    hipLaunchKernelGGL(hook_kernel, dim3((unsigned)tiles_of(3 * nt)), dim3(kTile), 0, s, twin, nt, l.normals, min_cos, l.parent,
                       reinterpret_cast<unsigned long long *>(cnt + 2));
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(flatten_kernel, dim3(face_blocks), dim3(kTile), 0, s, nt, l.parent);
    TN_LAUNCH_CHECK();

    // 6 - 7: a patch's faces adjacent in ascending face index; the patches numbered in ascending label
    hipLaunchKernelGGL(keys_kernel, dim3(face_blocks), dim3(kTile), 0, s, l.flags, l.parent, nt, l.keys);
    TN_LAUNCH_CHECK();
    code = tn_sort_pairs(reinterpret_cast<const uint64_t *>(l.keys), nullptr, num_triangles, key_bits(nt),
                         reinterpret_cast<uint64_t *>(l.sorted), l.order, l.sort, l.sort_bytes, stream);
    if (code != TN_OK) return code;
    hipLaunchKernelGGL(count_heads_kernel, dim3(face_blocks), dim3(kTile), 0, s, l.sorted, nt, l.head_tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_counts_kernel, dim3(1), dim3(kScan), 0, s, l.head_tiles, tiles_of(nt), cnt);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(emit_heads_kernel, dim3(face_blocks), dim3(kTile), 0, s, l.sorted, nt, l.head_tiles, l.patches);
    TN_LAUNCH_CHECK();

    // 8 - 9: where the blocks start; face_patch
    if (rows) {
        hipLaunchKernelGGL(count_blocks_kernel, dim3(face_blocks), dim3(kTile), 0, s, l.patches, cnt, nt, l.block_tiles);
        TN_LAUNCH_CHECK();
        hipLaunchKernelGGL(scan_counts_kernel, dim3(1), dim3(kScan), 0, s, l.block_tiles, tiles_of(nt), l.sums + 1);
        TN_LAUNCH_CHECK();
        hipLaunchKernelGGL(emit_blocks_kernel, dim3(face_blocks), dim3(kTile), 0, s, l.patches, cnt, nt, l.block_tiles);
        TN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(assign_kernel, dim3(face_blocks), dim3(kTile), 0, s, l.flags, l.parent, l.sorted, nt, l.patches, cnt, l.max_blocks,
                       face_patch, rows ? l.block_first : nullptr);
    TN_LAUNCH_CHECK();

    // 10 - 13: the first pass and the rows, the second pass and the rows' deviations
    if (rows) {
        const unsigned row_blocks = (unsigned)tiles_of(cap < nt ? cap : nt);
        hipLaunchKernelGGL(block_sums_kernel<Acc>, dim3(block_blocks), dim3(kTile), 0, s, l.sorted, l.order, nt, l.patches, cnt, nt, l.records,
                           l.block_first, l.sums + 1, l.max_blocks, l.partials);
        TN_LAUNCH_CHECK();
        hipLaunchKernelGGL(rows_kernel, dim3(row_blocks), dim3(kTile), 0, s, l.patches, cnt, nt, l.order, l.records, l.partials, l.sums + 1,
                           l.max_blocks, cap, patches);
        TN_LAUNCH_CHECK();
        hipLaunchKernelGGL(deviations_kernel, dim3(face_blocks), dim3(kTile), 0, s, positions, triangles, nv, nt, face_patch, cnt, cap, patches,
                           l.records, l.deviations);
        TN_LAUNCH_CHECK();
        hipLaunchKernelGGL(block_sums_kernel<Dev>, dim3(block_blocks), dim3(kTile), 0, s, l.sorted, l.order, nt, l.patches, cnt, cap,
                           l.deviations, l.block_first, l.sums + 1, l.max_blocks, l.deviation_partials);
        TN_LAUNCH_CHECK();
        hipLaunchKernelGGL(finish_rows_kernel, dim3(row_blocks), dim3(kTile), 0, s, l.patches, cnt, nt, l.order, l.deviations,
                           l.deviation_partials, l.sums + 1, l.max_blocks, cap, patches);
        TN_LAUNCH_CHECK();
    }

    // 14: the mesh's area and the thermal area
    hipLaunchKernelGGL(total_blocks_kernel, dim3((unsigned)tiles_of(l.blocks_per_list), 2), dim3(kTile), 0, s, l.geometric_list,
                       l.thermal_list, cnt, l.sums, nt, l.records, l.blocks_per_list, l.total_partials);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(totals_kernel, dim3(2), dim3(TN_WAVE), 0, s, cnt, l.sums, nt, l.blocks_per_list, l.total_partials, totals);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

}  // extern "C"
