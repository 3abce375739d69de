// SUM2 over groups of faces, the one place for it (tn_mesh_regions.hip: the thermal regions; tn_mesh_patches.hip: the planar patches,
// twice; tn_mesh_gradient.hip takes load_face and join_run alone, for its sums over all faces): every face carries a record, every
// face of a group the same label, and the group's row is its faces' records joined in ascending face index, 256 at a time and then
// the 256-blocks' partials in block order — the order include/thermonerf_hip.h defines.
//
//   load_face(...)                         one face's indices, corners and temperatures: what is valid, the edges, the cross product, the area,
//                                          area x centroid, the box, the face temperature — in this operation order only
//   R                                      a record: static R empty(), void join(const R &r) with "r behind everything this holds", and
//                                          kAhead, the records a walk loads ahead of its joins.  The ordered sums take one rounded
//                                          addition each and start from +0.0; everything else in a record is order-free
//   FaceLists, count_lists, list_faces,    two compacted lists of the faces that carry a flag bit (list y: bit[y], its length at
//   list_totals<R>                         length[y]) and the two-level sum of records[t].s[0] over each: the mesh's `totals`
//   Groups, number_groups, place_blocks,   after tn_sort_pairs of (label, 0 .. T-1), a face without a label keyed L or more: the groups
//   block_head, sum_blocks<R>,             numbered in ascending label from the heads of the sorted runs, the 256-blocks of the groups
//   group_sum<R>                           that have more than `direct` faces, their partials, and a group's sum for the thread that writes
//                                          its row
// The launch order of a caller: its faces kernel (count_lists at its end), list_faces, its labels and keys, the sort, number_groups,
// place_blocks, its assign kernel (block_head per sorted position), sum_blocks<R>, its rows kernel (group_sum<R>), list_totals<R>.
//
// The contract, which the call sites and their tests depend on:
//   * THE KERNELS CHECK WHAT THEY DEREFERENCE.  Labels, group numbers, positions and block numbers come out of device memory that a
//     foreign input (patches' twin table) has shaped: of_label is read only inside [0, L), the per-group arrays only below the group
//     count and `capacity`, sorted positions and faces only inside [0, T), blocks only below max_blocks and num_blocks[0].
//     group_of(label) = q only where label[q] == label: of_label is written at the heads alone and is otherwise whatever it was.
//   * A group's faces are the distance to the next head, the last group's up to counts[1]: no per-label count, no atomics.
//   * With direct = 256 a group of up to 256 faces has no partial: its row's thread walks the records themselves.  The row is the
//     same record either way (joining into an empty record is exact for the sums — +0.0 + x = x, and a sum started from +0.0 is
//     never -0.0 — and order-free for the rest).  The choice is the caller's, between memory and time: without the partials of the
//     small groups all partials stay below 2 T / 256 however many groups there are (patches: a mesh of T single faces), but the walks
//     of the small groups then come after the block sums instead of beside them, each as long as a block's (regions, whose V / 3
//     bounds the groups, keeps a partial for every group: direct = 0, at most T / 256 + capacity blocks).
//   * No allocation, no host synchronisation, no float atomics, and no block ever waits for another.
#pragma once
#include <cstddef>

#include "tn_device.h"
#include "tn_scan.h"

namespace tn {

constexpr int kFaceTile = 256;  // faces / sorted positions / groups / blocks per thread block of every kernel here but the scans
constexpr int kSumBlock = 256;  // entries per block of SUM2

inline long long face_tiles_of(long long n) { return ceil_div(n, kFaceTile); }

// ---- the face --------------------------------------------------------------------------------------------------------------------------

struct Face {
    long long i[3];      // the indices as the list has them
    float p[3][3], c[3];  // the corners and their temperatures (read only where the indices allow it)
    bool placed;         // the indices distinct and inside [0, V), the nine coordinates finite: everything below `tf` is computed
    bool warm;           // the indices as above, the three temperatures finite: tf is computed
    float tf;            // the face temperature: the mean of the three, rounded once
    double e1[3], e2[3];  // p1 - p0, p2 - p0
    double cr[3], n2;    // e1 x e2, its squared length
    double len, area;    // sqrt(n2), half of it
    double moment[3];    // area x centroid
    float lo[3], hi[3];  // the box of the corners
};

__device__ __forceinline__ Face load_face(const float *__restrict__ positions, const float *__restrict__ temperature,
                                          const int *__restrict__ triangles, long long num_vertices, long long t) {
    Face f;
    f.i[0] = triangles[3 * t], f.i[1] = triangles[3 * t + 1], f.i[2] = triangles[3 * t + 2];
    const long long *i = f.i;
    bool ok = i[0] >= 0 && i[0] < num_vertices && i[1] >= 0 && i[1] < num_vertices && i[2] >= 0 && i[2] < num_vertices;
    ok = ok && i[0] != i[1] && i[1] != i[2] && i[0] != i[2];
    f.placed = f.warm = ok;
    if (!ok) return f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        f.c[a] = temperature[i[a]];
        f.warm = f.warm && finite(f.c[a]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            f.p[a][k] = positions[3 * i[a] + k];
            f.placed = f.placed && finite(f.p[a][k]);
        }
    }
    if (f.warm) f.tf = (float)__ddiv_rn(__dadd_rn(__dadd_rn((double)f.c[0], (double)f.c[1]), (double)f.c[2]), 3.0);
    if (!f.placed) return f;
    double *e1 = f.e1, *e2 = f.e2;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e1[k] = __dsub_rn((double)f.p[1][k], (double)f.p[0][k]);
        e2[k] = __dsub_rn((double)f.p[2][k], (double)f.p[0][k]);
    }
    f.cr[0] = __dsub_rn(__dmul_rn(e1[1], e2[2]), __dmul_rn(e1[2], e2[1]));
    f.cr[1] = __dsub_rn(__dmul_rn(e1[2], e2[0]), __dmul_rn(e1[0], e2[2]));
    f.cr[2] = __dsub_rn(__dmul_rn(e1[0], e2[1]), __dmul_rn(e1[1], e2[0]));
    f.n2 = __dadd_rn(__dadd_rn(__dmul_rn(f.cr[0], f.cr[0]), __dmul_rn(f.cr[1], f.cr[1])), __dmul_rn(f.cr[2], f.cr[2]));
    f.len = __dsqrt_rn(f.n2);
    f.area = __dmul_rn(0.5, f.len);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double centre = __ddiv_rn(__dadd_rn(__dadd_rn((double)f.p[0][k], (double)f.p[1][k]), (double)f.p[2][k]), 3.0);
        f.moment[k] = __dmul_rn(f.area, centre);
        f.lo[k] = INFINITY, f.hi[k] = -INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a) f.lo[k] = min_ord(f.lo[k], f.p[a][k]), f.hi[k] = max_ord(f.hi[k], f.p[a][k]);
    }
    return f;
}

// ---- the two flagged lists and `totals` ---------------------------------------------------------------------------------------------------

struct FaceLists {
    int bit[2];            // the flag bit of the faces of list 0 / list 1
    long long *tiles[2];   // [tiles of T] the tile counts of the faces kernel, then where each tile's faces start in the list
    int *faces[2];         // [T] the lists, in face order
    long long *length[2];  // where list_faces writes each list's length and everything after it reads it
};

// the end of a faces kernel (EVERY thread of the block, a face beyond T with flags = 0): the two tile counts
__device__ __forceinline__ void count_lists(const FaceLists &l, int flags) {
#pragma unroll
    for (int y = 0; y < 2; ++y) {
        if (y) __syncthreads();  // block_rank's LDS is rewritten by the second call
        uint32_t total;
        block_rank<kFaceTile>((flags & l.bit[y]) != 0, total);
        if (threadIdx.x == 0) l.tiles[y][blockIdx.x] = (long long)total;
    }
}

__device__ __forceinline__ long long list_length(const FaceLists &l, int y, long long num_triangles) {
    const long long n = l.length[y][0];
    return n < 0 ? 0 : (n < num_triangles ? n : num_triangles);
}

// ---- the groups ------------------------------------------------------------------------------------------------------------------------

struct Groups {
    const unsigned long long *sorted;  // [T] the sorted keys: a label inside [0, L), or L and more for a face of no group
    const int *order;                  // [T] the face at every sorted position
    int *of_label;                     // [L] per label: its group (written at the heads alone, see group_of)
    int *label, *first_face, *first_block;  // [capacity] per group: its label, where its faces start in the sorted order and its blocks
    int *block_first;                  // [max_blocks] per block: the sorted position where it starts
    long long *counts;                 // [0] the groups (number_groups writes it), [1] the faces that carry a label (the caller's)
    long long *num_blocks;             // the blocks (place_blocks writes it)
    long long num_triangles, labels, capacity, max_blocks;  // T, L, and the rows of the arrays above
    long long direct;                  // 256 or 0: a group of up to this many faces has no partial, its row's thread walks its records
};

// sorted position j is the HEAD of a group iff it holds a label and the position before it holds another
__device__ __forceinline__ bool is_head(const Groups &g, long long j) {
    if (j >= g.num_triangles) return false;
    const unsigned long long key = g.sorted[j];
    return key < (unsigned long long)g.labels && (j == 0 || g.sorted[j - 1] != key);
}

__device__ __forceinline__ long long groups_of(const Groups &g) {
    const long long n = g.counts[0];
    return n < 0 ? 0 : (n < g.capacity ? n : g.capacity);
}

// the faces of group q < n: up to the next group's first face, the last one up to the faces that carry a label
__device__ __forceinline__ long long faces_of(const Groups &g, long long q, long long n) {
    const long long first = g.first_face[q];
    long long end = q + 1 < n ? (long long)g.first_face[q + 1] : g.counts[1];
    end = end < g.num_triangles ? end : g.num_triangles;
    return first >= 0 && end > first ? end - first : 0;
}

// the 256-blocks of a group of `faces` faces; none where its row's thread walks the records themselves
__device__ __forceinline__ uint32_t blocks_of(const Groups &g, long long faces) {
    return faces > g.direct ? (uint32_t)((faces + kSumBlock - 1) / kSumBlock) : 0u;
}

// the group of a label among the n groups, or -1; checks what it reads
__device__ __forceinline__ int group_of(const Groups &g, long long label, long long n) {
    if (label < 0 || label >= g.labels) return -1;
    const int q = g.of_label[label];
    return q >= 0 && q < n && g.label[q] == (int)label ? q : -1;
}

// sorted position j starts block (j - first face) / 256 of its group iff that is a whole number and the group has blocks (one thread
// per sorted position, from the caller's assign kernel, once place_blocks has run)
__device__ __forceinline__ void block_head(const Groups &g, long long j, long long n) {
    const unsigned long long key = g.sorted[j];
    if (key >= (unsigned long long)g.labels) return;
    const int q = group_of(g, (long long)key, n);
    if (q < 0 || blocks_of(g, faces_of(g, q, n)) == 0) return;
    const long long d = j - (long long)g.first_face[q];
    if (d < 0 || d % kSumBlock != 0) return;
    const long long b = (long long)g.first_block[q] + d / kSumBlock;
    if (b >= 0 && b < g.max_blocks) g.block_first[b] = (int)j;
}

// the records where(first) .. where(end - 1) joined in that order into one.  A lone thread's walk is a chain of memory round trips unless
// the loads go out ahead of the additions: U addresses, then U loads, then U joins — the same joins in the same order (joining an empty
// record changes nothing).  U = R::kAhead records are in registers at once: the record's type weighs round trips against occupancy.
template <typename R, typename Where>
__device__ __forceinline__ R join_run(long long first, long long end, Where where) {
    constexpr int U = R::kAhead;
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
__device__ __forceinline__ R walk(const Groups &g, const R *__restrict__ records, long long first, long long end) {
    end = end < g.num_triangles ? end : g.num_triangles;
    return join_run<R>(first < 0 ? 0 : first, end, [&](long long j) -> const R * {
        const long long t = g.order[j];
        return t >= 0 && t < g.num_triangles ? records + t : nullptr;
    });
}

// SUM2 over the `faces` faces of group q: its one block, or its blocks' partials in block order
template <typename R>
__device__ __forceinline__ R group_sum(const Groups &g, long long q, long long faces, const R *__restrict__ records,
                                       const R *__restrict__ partials) {
    if (blocks_of(g, faces) == 0) return walk(g, records, g.first_face[q], (long long)g.first_face[q] + faces);
    const long long num_blocks = g.num_blocks[0];
    long long b = g.first_block[q], end = b + (long long)blocks_of(g, faces);
    end = end < g.max_blocks ? end : g.max_blocks;
    end = end < num_blocks ? end : num_blocks;
    return join_run<R>(b < 0 ? 0 : b, end, [&](long long k) -> const R * { return partials + k; });
}

}  // namespace tn

// ---- the kernels ----------------------------------------------------------------------------------------------------------------------
// in the unnamed namespace of the source that includes this header, beside that source's own kernels: one copy per source, and a trace
// names them as it names those (`block_sums_kernel<Acc>`, `totals_kernel`), which is what the tools that read traces match

namespace {

using namespace tn;

__global__ void __launch_bounds__(kScan) scan_faces_kernel(FaceLists l, long long num_tiles) {
    scan_tiles<false>(l.tiles[0], num_tiles, l.length[0]);
    __syncthreads();
    scan_tiles<false>(l.tiles[1], num_tiles, l.length[1]);
}

__global__ void __launch_bounds__(kFaceTile) lists_kernel(const int *__restrict__ flags, long long num_triangles, FaceLists l) {
    const long long t = (long long)blockIdx.x * kFaceTile + threadIdx.x;
    const int f = t < num_triangles ? flags[t] : 0;
#pragma unroll
    for (int y = 0; y < 2; ++y) {
        if (y) __syncthreads();
        uint32_t unused;
        const uint32_t before = block_rank<kFaceTile>((f & l.bit[y]) != 0, unused);
        if (f & l.bit[y]) {
            const long long o = l.tiles[y][blockIdx.x] + (long long)before;  // <= t
            if (o >= 0 && o < num_triangles) l.faces[y][o] = (int)t;
        }
    }
}

// blockIdx.y = the list; one thread per 256 of its faces.  areas: the first sum of every face's record, `stride` bytes from face to face
__global__ void __launch_bounds__(kFaceTile)
total_blocks_kernel(FaceLists l, long long num_triangles, const char *__restrict__ areas, long long stride, long long blocks_per_list,
                    double *__restrict__ partials) {
    const long long b = (long long)blockIdx.x * kFaceTile + threadIdx.x;
    const int y = blockIdx.y;
    const long long n = list_length(l, y, num_triangles);
    if (b >= blocks_per_list || b * kSumBlock >= n) return;
    const int *list = l.faces[y];
    const long long end = (b + 1) * kSumBlock < n ? (b + 1) * kSumBlock : n;
    double s = 0.0;
    for (long long k = b * kSumBlock; k < end; ++k) {
        const long long t = list[k];
        if (t >= 0 && t < num_triangles) s = __dadd_rn(s, *reinterpret_cast<const double *>(areas + t * stride));
    }
    partials[y * blocks_per_list + b] = s;
}

__global__ void totals_kernel(FaceLists l, long long num_triangles, long long blocks_per_list, const double *__restrict__ partials,
                              double *__restrict__ totals) {
    if (threadIdx.x != 0) return;
    const int y = blockIdx.x;
    long long blocks = (list_length(l, y, num_triangles) + kSumBlock - 1) / kSumBlock;
    blocks = blocks < blocks_per_list ? blocks : blocks_per_list;
    double s = 0.0;
    for (long long b = 0; b < blocks; ++b) s = __dadd_rn(s, partials[y * blocks_per_list + b]);
    totals[y] = s;
}

__global__ void __launch_bounds__(kFaceTile) count_heads_kernel(Groups g, long long *__restrict__ head_tiles) {
    const long long j = (long long)blockIdx.x * kFaceTile + threadIdx.x;
    uint32_t total;
    block_rank<kFaceTile>(is_head(g, j), total);
    if (threadIdx.x == 0) head_tiles[blockIdx.x] = (long long)total;
}

__global__ void __launch_bounds__(kScan)
scan_counts_kernel(long long *__restrict__ tiles, long long num_tiles, long long *__restrict__ count) {
    scan_tiles<false>(tiles, num_tiles, count);
}

__global__ void __launch_bounds__(kFaceTile) emit_heads_kernel(Groups g, const long long *__restrict__ head_tiles) {
    const long long j = (long long)blockIdx.x * kFaceTile + threadIdx.x;
    const bool head = is_head(g, j);
    uint32_t unused;
    const uint32_t before = block_rank<kFaceTile>(head, unused);
    if (!head) return;
    const long long q = head_tiles[blockIdx.x] + (long long)before;  // <= j
    if (q < 0 || q >= g.capacity) return;
    const long long label = (long long)g.sorted[j];
    g.label[q] = (int)label;
    g.first_face[q] = (int)j;
    g.of_label[label] = (int)q;
}

__global__ void __launch_bounds__(kFaceTile) count_blocks_kernel(Groups g, long long *__restrict__ block_tiles) {
    const long long q = (long long)blockIdx.x * kFaceTile + threadIdx.x;
    const long long n = groups_of(g);
    uint32_t total;
    block_exclusive<kFaceTile>(q < n ? blocks_of(g, faces_of(g, q, n)) : 0u, total);
    if (threadIdx.x == 0) block_tiles[blockIdx.x] = (long long)total;
}

__global__ void __launch_bounds__(kFaceTile) emit_blocks_kernel(Groups g, const long long *__restrict__ block_tiles) {
    const long long q = (long long)blockIdx.x * kFaceTile + threadIdx.x;
    const long long n = groups_of(g);
    uint32_t unused;
    const uint32_t before = block_exclusive<kFaceTile>(q < n ? blocks_of(g, faces_of(g, q, n)) : 0u, unused);
    if (q < n) g.first_block[q] = (int)(block_tiles[blockIdx.x] + (long long)before);
}

// ONE THREAD PER 256-BLOCK walks its faces' records through the sorted order into one partial record.  rows: the groups whose rows are
// written (q < rows); the records of a second pass exist for no other
template <typename R>
__global__ void __launch_bounds__(kFaceTile)
block_sums_kernel(Groups g, long long rows, const R *__restrict__ records, R *__restrict__ partials) {
    const long long b = (long long)blockIdx.x * kFaceTile + threadIdx.x;
    if (b >= g.max_blocks || b >= g.num_blocks[0]) return;
    R a = R::empty();
    const long long j0 = g.block_first[b];
    if (j0 >= 0 && j0 < g.num_triangles) {
        const long long n = groups_of(g);
        const unsigned long long key = g.sorted[j0];
        const int q = key < (unsigned long long)g.labels ? group_of(g, (long long)key, n) : -1;
        if (q >= 0 && q < rows) {
            const long long end = (long long)g.first_face[q] + faces_of(g, q, n);
            a = walk(g, records, j0, end < j0 + kSumBlock ? end : j0 + kSumBlock);
        }
    }
    partials[b] = a;
}

}  // namespace

// ---- the launch sequences (static: each source launches its own copy of the kernels) ---------------------------------------------------

namespace tn {

// the two lengths and the two lists, from the flags and the tile counts of the faces kernel
static inline int list_faces(const FaceLists &l, const int *flags, long long num_triangles, hipStream_t s) {
    const long long tiles = face_tiles_of(num_triangles);
    hipLaunchKernelGGL(scan_faces_kernel, dim3(1), dim3(kScan), 0, s, l, tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(lists_kernel, dim3((unsigned)tiles), dim3(kFaceTile), 0, s, flags, num_triangles, l);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

// totals[y] = SUM2 of records[t].s[0] over list y; partials: 2 * blocks_per_list doubles, blocks_per_list = ceil(T / 256)
template <typename R>
static inline int list_totals(const FaceLists &l, long long num_triangles, const R *records, double *partials, double *totals, hipStream_t s) {
    const long long blocks_per_list = ceil_div(num_triangles, kSumBlock);
    static_assert(offsetof(R, s) == 0, "a record begins with its ordered sums, the area first");
    hipLaunchKernelGGL(total_blocks_kernel, dim3((unsigned)face_tiles_of(blocks_per_list), 2), dim3(kFaceTile), 0, s, l, num_triangles,
                       reinterpret_cast<const char *>(records), (long long)sizeof(R), blocks_per_list, partials);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(totals_kernel, dim3(2), dim3(TN_WAVE), 0, s, l, num_triangles, blocks_per_list, partials, totals);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

// count / scan / emit over the sorted positions: counts[0] = the groups; label, first_face and of_label of every group
static inline int number_groups(const Groups &g, long long *head_tiles, hipStream_t s) {
    const long long tiles = face_tiles_of(g.num_triangles);
    hipLaunchKernelGGL(count_heads_kernel, dim3((unsigned)tiles), dim3(kFaceTile), 0, s, g, head_tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_counts_kernel, dim3(1), dim3(kScan), 0, s, head_tiles, tiles, g.counts);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(emit_heads_kernel, dim3((unsigned)tiles), dim3(kFaceTile), 0, s, g, head_tiles);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

// count / scan / emit over the groups: num_blocks[0] = the blocks; first_block of every group.  block_tiles: one per tile of `capacity`
static inline int place_blocks(const Groups &g, long long *block_tiles, hipStream_t s) {
    const long long tiles = face_tiles_of(g.capacity);
    hipLaunchKernelGGL(count_blocks_kernel, dim3((unsigned)tiles), dim3(kFaceTile), 0, s, g, block_tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_counts_kernel, dim3(1), dim3(kScan), 0, s, block_tiles, tiles, g.num_blocks);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(emit_blocks_kernel, dim3((unsigned)tiles), dim3(kFaceTile), 0, s, g, block_tiles);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

template <typename R>
static inline int sum_blocks(const Groups &g, long long rows, const R *records, R *partials, hipStream_t s) {
    hipLaunchKernelGGL(block_sums_kernel<R>, dim3((unsigned)face_tiles_of(g.max_blocks)), dim3(kFaceTile), 0, s, g, rows, records, partials);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

}  // namespace tn
