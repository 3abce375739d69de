// Level-set curves of a per-vertex scalar on an indexed triangle list (DESIGN.md "Level-set curves"; include/thermonerf_hip.h defines
// every output to the bit): the half-edge twins of a mesh, and the isolines of a scalar — the temperature itself for isotherms, the
// signed distance to a plane for sections — chained into ordered polylines with arc length and the temperature along them.
//
// tn_mesh_half_edges, launches on the caller's stream:
//   1. keys       one thread per half-edge: lo * V + hi of a structural face, V * V of every other; twin <- -1
//   2. sort       tn_sort_pairs of (key, h): an edge class adjacent, in ascending half-edge
//   3. classes    one thread per sorted position: the head of a class looks at its next two neighbours, writes the twins of a class of
//                 two opposite members and counts; the block's four counts join counts[] by one integer atomic each
// tn_mesh_isolines:
//   1. faces      one thread per face: USABLE, the range of levels [first, last) that cross it (binary search in LDS); the tile counts
//   2. scan       one block: S = counts[0], the usable faces = counts[4]; counts[1..3] <- 0
//   3. bases      one thread per face: base_f
//   4. segments   one thread per face walks its levels: the two crossing points, face, level, the successor
//   5. preds      one thread per segment: pred[succ[s]] = s (a single writer: the in-degree is at most 1)
//   6. sweep 1    pointer jumping along the predecessors, ceil(log2(max(2, capacity))) launches that read one array and write the
//                 other: (ancestor, lowest segment seen) -> the head of a path, the lowest member of a cycle
//   7. cut        the first segment of every curve, closed or not; a cycle loses the link into its first segment
//   8. sweep 2    the same jumps over the cut links: (ancestor, rank)
//   9. lengths    the last segment of a curve writes the curve's segment count to its first segment
//  10. curves     count / scan / emit over "is a first segment": q, the points before the curve; counts[1..3]
//  11. points     one thread per segment: its end point to first_point + rank + 1 (the first segment its start point too), the faces,
//                 the segment's length into the arc slot of its end point
//  12. walk       ONE WAVE PER CURVE: 64 lengths at a time, added lane by lane in point order -> arc, W; the extremes; the curve's row
// No allocation, no host synchronisation, no float atomics, and no block ever waits for another.  Every index that is read from memory
// is checked before it is used: a foreign `twin` gives other curves, never an access outside the arrays.
#include "tn_device.h"
#include "tn_scan.h"

using namespace tn;

namespace {

constexpr int kTile = 256;       // half-edges / faces / segments per thread block of every kernel but the scans
constexpr int kMaxLevels = 256;  // levels of one call
constexpr long long kMaxCapacity = 1LL << 30;  // segments of one call: 2 * capacity points are int32 rows, ranks stay below 2^31

inline long long tiles_of(long long n) { return ceil_div(n, kTile); }
__device__ __forceinline__ bool finite64(double x) { return fabs(x) <= 1.7976931348623157e308; }  // (a NaN fails)

// ---- half-edges ------------------------------------------------------------------------------------------------------------------------

// the three indices of face f when it is structural
__device__ __forceinline__ bool structural(const int *__restrict__ triangles, long long f, long long num_vertices, long long (&i)[3]) {
    i[0] = triangles[3 * f], i[1] = triangles[3 * f + 1], i[2] = triangles[3 * f + 2];
    const bool inside = i[0] >= 0 && i[0] < num_vertices && i[1] >= 0 && i[1] < num_vertices && i[2] >= 0 && i[2] < num_vertices;
    return inside && i[0] != i[1] && i[1] != i[2] && i[0] != i[2];
}

__global__ void __launch_bounds__(kTile)
edge_keys_kernel(const int *__restrict__ triangles, long long num_triangles, long long num_vertices, unsigned long long *__restrict__ keys,
                 int *__restrict__ twin) {
    const long long h = (long long)blockIdx.x * kTile + threadIdx.x;
    if (h >= 3 * num_triangles) return;
    const long long f = h / 3;
    const int j = (int)(h - 3 * f);
    long long i[3];
    unsigned long long key = (unsigned long long)num_vertices * (unsigned long long)num_vertices;  // above every class
    if (structural(triangles, f, num_vertices, i)) {
        const long long a = j == 0 ? i[0] : (j == 1 ? i[1] : i[2]), b = j == 0 ? i[1] : (j == 1 ? i[2] : i[0]);
        key = (unsigned long long)(a < b ? a : b) * (unsigned long long)num_vertices + (unsigned long long)(a < b ? b : a);
    }
    keys[h] = key;
    twin[h] = -1;
}

// does sorted half-edge `h` run from the lower to the higher vertex of its class?  (h is a half-edge of a structural face)
__device__ __forceinline__ bool ascending(const int *__restrict__ triangles, long long h) {
    const long long f = h / 3;
    const int j = (int)(h - 3 * f);
    return triangles[3 * f + j] < triangles[3 * f + (j + 1) % 3];
}

__global__ void __launch_bounds__(kTile)
edge_classes_kernel(const unsigned long long *__restrict__ sorted, const int *__restrict__ order, const int *__restrict__ triangles,
                    long long num_triangles, long long num_vertices, int *__restrict__ twin, unsigned long long *__restrict__ counts) {
    const long long n = 3 * num_triangles;
    const long long i = (long long)blockIdx.x * kTile + threadIdx.x;
    const unsigned long long none = (unsigned long long)num_vertices * (unsigned long long)num_vertices;
    int members = 0;  // of the class that starts here: 1, 2, or 3 for "three or more"
    bool same = false;
    if (i < n) {
        const unsigned long long key = sorted[i];
        if (key < none && (i == 0 || sorted[i - 1] != key)) {
            members = 1 + (i + 1 < n && sorted[i + 1] == key ? 1 : 0);
            if (members == 2 && i + 2 < n && sorted[i + 2] == key) members = 3;
            if (members == 2) {
                const long long h0 = order[i], h1 = order[i + 1];
                if (h0 >= 0 && h0 < n && h1 >= 0 && h1 < n) {
                    same = ascending(triangles, h0) == ascending(triangles, h1);
                    if (!same) twin[h0] = (int)h1, twin[h1] = (int)h0;
                }
            }
        }
    }
    uint32_t total[4];
    block_rank<kTile>(members > 0, total[0]);
    __syncthreads();  // block_rank's LDS is rewritten by the next call
    block_rank<kTile>(members == 1, total[1]);
    __syncthreads();
    block_rank<kTile>(members == 3, total[2]);
    __syncthreads();
    block_rank<kTile>(members == 2 && same, total[3]);
    if (threadIdx.x < 4 && total[threadIdx.x] > 0) atomicAdd(&counts[threadIdx.x], (unsigned long long)total[threadIdx.x]);
}

// the workspace of tn_mesh_half_edges, in order: the keys, the sorted keys, the sorted half-edges, the sort's own workspace
struct EdgeLayout {
    unsigned long long *keys, *sorted;
    int *order;
    void *sort;
    size_t sort_bytes, bytes;
};

inline EdgeLayout edge_layout_of(char *ws, long long t) {
    EdgeLayout l;
    size_t at = 0;
    auto take = [&](size_t bytes) {  // (ws == NULL: the sizes alone)
        char *p = ws ? ws + at : nullptr;
        at += bytes;
        return p;
    };
    l.keys = reinterpret_cast<unsigned long long *>(take((size_t)(3 * t) * sizeof(unsigned long long)));
    l.sorted = reinterpret_cast<unsigned long long *>(take((size_t)(3 * t) * sizeof(unsigned long long)));
    l.order = reinterpret_cast<int *>(take(ints_bytes(3 * t)));
    l.sort_bytes = tn_sort_pairs_workspace_bytes(3 * t);
    l.sort = take(l.sort_bytes);
    l.bytes = at + 8;
    return l;
}

// ---- isolines ---------------------------------------------------------------------------------------------------------------------------

struct Levels {  // by value to the kernels that need the levels
    double v[kMaxLevels];
    double normal[3];
    int k;
    int plane;  // 1: the scalar is the signed distance along `normal`; 0: the scalar array
};

// the levels into LDS; the caller's next barrier orders the fill before the first read
__device__ __forceinline__ void load_levels(double *lds, const Levels &lv) {
    for (int e = threadIdx.x; e < kMaxLevels; e += kTile) lds[e] = e < lv.k ? lv.v[e] : INFINITY;
}

// #{k : L_k <= x}
__device__ __forceinline__ int levels_at_most(const double *lds, int k, double x) {
    int lo = 0, hi = k;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lds[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct Corner {
    long long i;
    float p[3], t;
    double s;
};

// the three corners of face f when it is USABLE
__device__ __forceinline__ bool usable_face(const float *__restrict__ positions, const float *__restrict__ temperature,
                                            const int *__restrict__ triangles, const float *__restrict__ scalar, const Levels &lv,
                                            long long f, long long num_vertices, Corner (&c)[3]) {
    long long i[3];
    if (!structural(triangles, f, num_vertices, i)) return false;
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c[a].i = i[a];
        c[a].t = temperature[i[a]];
        ok = ok && finite(c[a].t);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c[a].p[k] = positions[3 * i[a] + k];
            ok = ok && finite(c[a].p[k]);
        }
        if (lv.plane)
            c[a].s = __dadd_rn(__dadd_rn(__dmul_rn(lv.normal[0], (double)c[a].p[0]), __dmul_rn(lv.normal[1], (double)c[a].p[1])),
                               __dmul_rn(lv.normal[2], (double)c[a].p[2]));
        else
            c[a].s = (double)scalar[i[a]];
        ok = ok && finite64(c[a].s);
    }
    return ok;
}

// a face's range of levels in one int: first | last << 16 (both 0 .. 256); -1: not usable
__device__ __forceinline__ int pack_range(int first, int last) { return first | last << 16; }

__global__ void __launch_bounds__(kTile)
faces_kernel(const float *__restrict__ positions, const float *__restrict__ temperature, const int *__restrict__ triangles,
             const float *__restrict__ scalar, const Levels lv, long long num_vertices, long long num_triangles,
             int *__restrict__ face_range, long long *__restrict__ segment_tiles, long long *__restrict__ usable_tiles) {
    __shared__ double levels[kMaxLevels];
    load_levels(levels, lv);
    __syncthreads();
    const long long f = (long long)blockIdx.x * kTile + threadIdx.x;
    bool usable = false;
    int segments = 0;
    if (f < num_triangles) {
        Corner c[3];
        usable = usable_face(positions, temperature, triangles, scalar, lv, f, num_vertices, c);
        int range = -1;
        if (usable) {
            const double lo = fmin(fmin(c[0].s, c[1].s), c[2].s), hi = fmax(fmax(c[0].s, c[1].s), c[2].s);
            const int first = levels_at_most(levels, lv.k, lo), last = levels_at_most(levels, lv.k, hi);
            range = pack_range(first, last);
            segments = last - first;
        }
        face_range[f] = range;
    }
    uint32_t total;
    block_exclusive<kTile>((uint32_t)segments, total);
    if (threadIdx.x == 0) segment_tiles[blockIdx.x] = (long long)total;
    block_rank<kTile>(usable, total);
    if (threadIdx.x == 0) usable_tiles[blockIdx.x] = (long long)total;
}

__global__ void __launch_bounds__(kScan)
scan_faces_kernel(long long *__restrict__ segment_tiles, long long *__restrict__ usable_tiles, long long num_tiles,
                  long long *__restrict__ counts) {
    scan_tiles<false>(segment_tiles, num_tiles, counts);
    __syncthreads();
    scan_tiles<false>(usable_tiles, num_tiles, counts + 4);
    if (threadIdx.x >= 1 && threadIdx.x <= 3) counts[threadIdx.x] = 0;
}

// whether the call has room for its segments: decided on the device, by every kernel behind the scan
__device__ __forceinline__ bool fits(const long long *__restrict__ counts, long long capacity) { return counts[0] <= capacity; }

__global__ void __launch_bounds__(kTile)
bases_kernel(const int *__restrict__ face_range, long long num_triangles, const long long *__restrict__ segment_tiles,
             int *__restrict__ face_base) {
    const long long f = (long long)blockIdx.x * kTile + threadIdx.x;
    const int range = f < num_triangles ? face_range[f] : -1;
    const int segments = range >= 0 ? (range >> 16) - (range & 0xffff) : 0;
    uint32_t unused;
    const uint32_t before = block_exclusive<kTile>((uint32_t)segments, unused);
    if (f < num_triangles) face_base[f] = (int)(segment_tiles[blockIdx.x] + (long long)before);  // (only read when S fits an int)
}

struct alignas(8) Ends {  // a segment's two points: x y z and the temperature
    float start[4], end[4];
};

struct Segments {  // per segment, `capacity` rows each
    Ends *ends;
    int *face, *level, *succ, *pred, *first, *length, *first_point;
    int2 *jump[2];
    long long capacity;
};

// x, y or z as j is 0, 1 or 2, field by field
__device__ __forceinline__ Corner pick(int j, const Corner &x, const Corner &y, const Corner &z) {
    Corner r;
    r.i = j == 0 ? x.i : (j == 1 ? y.i : z.i);
    r.t = j == 0 ? x.t : (j == 1 ? y.t : z.t);
    r.s = j == 0 ? x.s : (j == 1 ? y.s : z.s);
#pragma unroll
    for (int k = 0; k < 3; ++k) r.p[k] = j == 0 ? x.p[k] : (j == 1 ? y.p[k] : z.p[k]);
    return r;
}

// the crossing of level L on the edge between corners a and b, one of them HIGH
__device__ __forceinline__ void crossing(const Corner &a, const Corner &b, double level, float (&out)[4]) {
    const bool a_high = a.s >= level;
    const double s_lo = a_high ? b.s : a.s, s_hi = a_high ? a.s : b.s;
    const double w = __ddiv_rn(__dsub_rn(level, s_lo), __dsub_rn(s_hi, s_lo));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double lo = (double)(a_high ? b.p[k] : a.p[k]), hi = (double)(a_high ? a.p[k] : b.p[k]);
        out[k] = (float)__dadd_rn(lo, __dmul_rn(w, __dsub_rn(hi, lo)));
    }
    const double t_lo = (double)(a_high ? b.t : a.t), t_hi = (double)(a_high ? a.t : b.t);
    out[3] = (float)__dadd_rn(t_lo, __dmul_rn(w, __dsub_rn(t_hi, t_lo)));
}

__global__ void __launch_bounds__(kTile)
segments_kernel(const float *__restrict__ positions, const float *__restrict__ temperature, const int *__restrict__ triangles,
                const float *__restrict__ scalar, const Levels lv, long long num_vertices, long long num_triangles,
                const int *__restrict__ twin, const int *__restrict__ face_range, const int *__restrict__ face_base,
                const long long *__restrict__ counts, Segments g) {
    __shared__ double levels[kMaxLevels];
    load_levels(levels, lv);
    __syncthreads();
    if (!fits(counts, g.capacity)) return;
    const long long total = counts[0];
    const long long f = (long long)blockIdx.x * kTile + threadIdx.x;
    if (f >= num_triangles) return;
    const int range = face_range[f];
    if (range < 0) return;
    const int first = range & 0xffff, last = range >> 16;
    if (first >= last) return;
    Corner c[3];
    if (!usable_face(positions, temperature, triangles, scalar, lv, f, num_vertices, c)) return;
    const long long base = face_base[f];
    for (int k = first; k < last; ++k) {
        const long long s = base + (k - first);
        if (s < 0 || s >= total) return;
        const double level = levels[k];
        const bool high[3] = {c[0].s >= level, c[1].s >= level, c[2].s >= level};
        const int j0 = high[0] != high[1] && high[0] != high[2] ? 0 : (high[1] != high[0] && high[1] != high[2] ? 1 : 2);
        const int j2 = (j0 + 2) % 3;
        // the corners rotated (selects, no indexed private array); the crossed half-edges: hA = c0 -> c1 (3 f + j0), hB = c2 -> c0 (3 f + j2)
        const Corner c0 = pick(j0, c[0], c[1], c[2]), c1 = pick(j0, c[1], c[2], c[0]), c2 = pick(j0, c[2], c[0], c[1]);
        Ends e;
        float on_a[4], on_b[4];
        crossing(c0, c1, level, on_a);
        crossing(c2, c0, level, on_b);
        const bool from_a = c0.s >= level;
#pragma unroll
        for (int a = 0; a < 4; ++a) e.start[a] = from_a ? on_a[a] : on_b[a], e.end[a] = from_a ? on_b[a] : on_a[a];
        const long long h_end = 3 * f + (from_a ? j2 : j0);
        long long succ = -1;
        const long long t = twin[h_end];
        if (t >= 0 && t < 3 * num_triangles) {
            const int r = face_range[t / 3];
            if (r >= 0 && k >= (r & 0xffff) && k < (r >> 16)) succ = (long long)face_base[t / 3] + (k - (r & 0xffff));
            if (succ < 0 || succ >= total) succ = -1;
        }
        g.ends[s] = e;
        g.face[s] = (int)f;
        g.level[s] = k;
        g.succ[s] = (int)succ;
        g.pred[s] = -1;
    }
}

__global__ void __launch_bounds__(kTile)
preds_kernel(const long long *__restrict__ counts, Segments g) {
    if (!fits(counts, g.capacity)) return;
    const long long s = (long long)blockIdx.x * kTile + threadIdx.x;
    if (s >= counts[0]) return;
    const int next = g.succ[s];
    if (next >= 0 && next < counts[0]) g.pred[next] = (int)s;
}

// sweep 1 starts: (the predecessor, or the segment itself at a head; the segment)
__global__ void __launch_bounds__(kTile)
sweep1_start_kernel(const long long *__restrict__ counts, Segments g) {
    if (!fits(counts, g.capacity)) return;
    const long long s = (long long)blockIdx.x * kTile + threadIdx.x;
    if (s >= counts[0]) return;
    const int before = g.pred[s];
    g.jump[0][s] = make_int2(before >= 0 && before < counts[0] ? before : (int)s, (int)s);
}

// one round of sweep 1: (ancestor, lowest seen) <- (ancestor's ancestor, the lower of the two)
__global__ void __launch_bounds__(kTile)
sweep1_kernel(const long long *__restrict__ counts, long long capacity, const int2 *__restrict__ in, int2 *__restrict__ out) {
    if (!fits(counts, capacity)) return;
    const long long s = (long long)blockIdx.x * kTile + threadIdx.x;
    if (s >= counts[0]) return;
    const int2 mine = in[s];
    const int2 far = in[mine.x];  // (an ancestor is a segment: 0 .. S-1 by construction)
    out[s] = make_int2(far.x, mine.y < far.y ? mine.y : far.y);
}

// the curve's first segment and whether it is closed; sweep 2 starts: (the predecessor over the cut links or -1, the rank so far)
__global__ void __launch_bounds__(kTile)
cut_kernel(const long long *__restrict__ counts, Segments g, const int2 *__restrict__ swept, int2 *__restrict__ out) {
    if (!fits(counts, g.capacity)) return;
    const long long s = (long long)blockIdx.x * kTile + threadIdx.x;
    if (s >= counts[0]) return;
    const int2 mine = swept[s];
    const bool cycle = g.pred[mine.x] >= 0;  // the walk never reached a head
    const int first = cycle ? mine.y : mine.x;
    g.first[s] = first | (cycle ? (int)0x80000000 : 0);
    const int before = g.pred[s];
    const bool linked = before >= 0 && before < counts[0] && (long long)first != s;
    out[s] = make_int2(linked ? before : -1, linked ? 1 : 0);
}

__global__ void __launch_bounds__(kTile)
sweep2_kernel(const long long *__restrict__ counts, long long capacity, const int2 *__restrict__ in, int2 *__restrict__ out) {
    if (!fits(counts, capacity)) return;
    const long long s = (long long)blockIdx.x * kTile + threadIdx.x;
    if (s >= counts[0]) return;
    int2 mine = in[s];
    if (mine.x >= 0) {
        const int2 far = in[mine.x];
        mine = make_int2(far.x, (int)(((unsigned)mine.y + (unsigned)far.y) & 0x7fffffffu));
    }
    out[s] = mine;
}

// is s the last segment of its curve?  (no successor, or the successor is where the cycle was cut)
__device__ __forceinline__ bool last_of_curve(const Segments &g, long long s, long long total) {
    const int next = g.succ[s], first = g.first[s];
    return next < 0 || next >= total || (first < 0 && next == (first & 0x7fffffff));
}

__global__ void __launch_bounds__(kTile)
lengths_kernel(const long long *__restrict__ counts, Segments g, const int2 *__restrict__ ranked) {
    if (!fits(counts, g.capacity)) return;
    const long long s = (long long)blockIdx.x * kTile + threadIdx.x;
    if (s >= counts[0]) return;
    if (last_of_curve(g, s, counts[0])) g.length[g.first[s] & 0x7fffffff] = ranked[s].y + 1;
}

// what a first segment adds to the three counts: a curve, its segments, a closed curve
__device__ __forceinline__ bool first_segment(const Segments &g, long long s, long long total, uint32_t &length, bool &closed) {
    length = 0, closed = false;
    if (s >= total) return false;
    const int first = g.first[s];
    if ((long long)(first & 0x7fffffff) != s) return false;
    const int n = g.length[s];
    length = n > 0 ? (uint32_t)n : 0u;
    closed = first < 0;
    return true;
}

__global__ void __launch_bounds__(kTile)
count_curves_kernel(const long long *__restrict__ counts, Segments g, long long *__restrict__ curve_tiles,
                    long long *__restrict__ length_tiles, long long *__restrict__ closed_tiles) {
    if (!fits(counts, g.capacity)) return;
    const long long s = (long long)blockIdx.x * kTile + threadIdx.x;
    uint32_t length, curves, lengths, closeds;
    bool closed;
    const bool first = first_segment(g, s, counts[0], length, closed);
    block_rank<kTile>(first, curves);
    block_exclusive<kTile>(length, lengths);
    __syncthreads();  // block_rank's LDS is rewritten by the second call
    block_rank<kTile>(closed, closeds);
    if (threadIdx.x == 0) {
        curve_tiles[blockIdx.x] = (long long)curves;
        length_tiles[blockIdx.x] = (long long)lengths;
        closed_tiles[blockIdx.x] = (long long)closeds;
    }
}

__global__ void __launch_bounds__(kScan)
scan_curves_kernel(long long *__restrict__ curve_tiles, long long *__restrict__ length_tiles, long long *__restrict__ closed_tiles,
                   long long capacity, long long *__restrict__ counts, long long *__restrict__ sums) {
    if (!fits(counts, capacity)) return;
    const long long num_tiles = (counts[0] + kTile - 1) / kTile;
    scan_tiles<false>(curve_tiles, num_tiles, counts + 1);
    __syncthreads();
    scan_tiles<false>(length_tiles, num_tiles, sums);
    __syncthreads();
    scan_tiles<false>(closed_tiles, num_tiles, counts + 3);
    __syncthreads();
    if (threadIdx.x == 0) counts[2] = counts[0] + counts[1];
}

__global__ void __launch_bounds__(kTile)
emit_curves_kernel(const long long *__restrict__ counts, Segments g, const long long *__restrict__ curve_tiles,
                   const long long *__restrict__ length_tiles, int *__restrict__ curve_first) {
    if (!fits(counts, g.capacity)) return;
    const long long s = (long long)blockIdx.x * kTile + threadIdx.x;
    uint32_t length, unused;
    bool closed;
    const bool first = first_segment(g, s, counts[0], length, closed);
    const uint32_t curves_before = block_rank<kTile>(first, unused);
    const uint32_t lengths_before = block_exclusive<kTile>(length, unused);
    if (!first) return;
    const long long q = curve_tiles[blockIdx.x] + (long long)curves_before;
    g.first_point[s] = (int)(length_tiles[blockIdx.x] + (long long)lengths_before + q);
    if (q >= 0 && q < g.capacity) curve_first[q] = (int)s;
}

struct Points {  // the outputs per point, `rows` rows each
    float *positions, *temperature;
    double *arc;
    int *face;
    long long rows;
};

__global__ void __launch_bounds__(kTile)
points_kernel(const long long *__restrict__ counts, Segments g, const int2 *__restrict__ ranked, Points out) {
    if (!fits(counts, g.capacity)) return;
    const long long total = counts[0];
    const long long s = (long long)blockIdx.x * kTile + threadIdx.x;
    if (s >= total) return;
    const long long first = g.first[s] & 0x7fffffff;
    const long long at = (long long)g.first_point[first] + (long long)ranked[s].y;  // the point this segment starts at
    if (at < 0 || at + 1 >= out.rows) return;
    const Ends e = g.ends[s];
    const int face = g.face[s];
    if (first == s) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out.positions[3 * at + k] = e.start[k];
        out.temperature[at] = e.start[3];
        out.arc[at] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) out.positions[3 * (at + 1) + k] = e.end[k];
    out.temperature[at + 1] = e.end[3];
    out.face[at] = face;
    if (last_of_curve(g, s, total)) out.face[at + 1] = face;
    // the segment's length waits in the arc slot of its end point for the walk
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = __dsub_rn((double)e.end[k], (double)e.start[k]);
    out.arc[at + 1] = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(d[0], d[0]), __dmul_rn(d[1], d[1])), __dmul_rn(d[2], d[2])));
}

// one wave per curve: the lengths and the W terms of 64 segments at a time, added in point order by every lane alike
__global__ void __launch_bounds__(kTile)
walk_kernel(const long long *__restrict__ counts, Segments g, const int *__restrict__ curve_first, Points out,
            tn_mesh_curve *__restrict__ curves) {
    if (!fits(counts, g.capacity)) return;
    const int lane = threadIdx.x % TN_WAVE;
    const long long q = ((long long)blockIdx.x * kTile + threadIdx.x) / TN_WAVE;  // the same in every lane of a wave
    if (q >= counts[1] || q >= g.capacity) return;
    const long long s = curve_first[q];
    if (s < 0 || s >= counts[0]) return;
    const long long n = g.length[s], at = g.first_point[s];
    if (n < 1 || at < 0 || at + n >= out.rows) return;
    double arc = 0.0, w = 0.0;
    float lowest = INFINITY, highest = -INFINITY;
    for (long long first = 0; first < n; first += TN_WAVE) {
        const long long j = first + lane;  // segment j of the curve: from point at + j to point at + j + 1
        double length = 0.0, term = 0.0;
        if (j < n) {
            const float t0 = out.temperature[at + j], t1 = out.temperature[at + j + 1];
            length = out.arc[at + j + 1];
            term = __dmul_rn(length, __dmul_rn(0.5, __dadd_rn((double)t0, (double)t1)));
            lowest = min_ord(lowest, t0), highest = max_ord(highest, t0);
            if (j == n - 1) lowest = min_ord(lowest, t1), highest = max_ord(highest, t1);
        }
        const int here = (int)(n - first < TN_WAVE ? n - first : TN_WAVE);
        double mine = 0.0;
        for (int i = 0; i < here; ++i) {
            arc = __dadd_rn(arc, __shfl(length, i, TN_WAVE));
            w = __dadd_rn(w, __shfl(term, i, TN_WAVE));
            if (i == lane) mine = arc;
        }
        if (j < n) out.arc[at + j + 1] = mine;
    }
#pragma unroll
    for (int o = TN_WAVE / 2; o > 0; o >>= 1) {
        lowest = min_ord(lowest, __shfl_xor(lowest, o, TN_WAVE));
        highest = max_ord(highest, __shfl_xor(highest, o, TN_WAVE));
    }
    if (lane != 0) return;
    const int first = g.first[s];
    tn_mesh_curve row;
    row.length = arc;
    row.level = g.level[s];
    row.first_point = (int32_t)at;
    row.points = (int32_t)(n + 1);
    row.closed = first < 0 ? 1 : 0;
    row.mean_temperature = arc == 0.0 ? quiet_nan() : (float)__ddiv_rn(w, arc);
    row.min_temperature = lowest;
    row.max_temperature = highest;
    row.first_face = g.face[s];
    curves[q] = row;
}

inline int jump_rounds(long long capacity) {  // ceil(log2(max(2, capacity)))
    int rounds = 1;
    while ((1LL << rounds) < capacity) ++rounds;
    return rounds;
}

// the workspace of tn_mesh_isolines, in order: the tile counts (segments and usable faces per face tile; curves, lengths and closed
// curves per segment tile), the device sum, the segments' points and jump arrays, then the int arrays per face (range, base) and per
// segment (face, level, succ, pred, first, length, first_point, curve_first)
struct Layout {
    long long *segment_tiles, *usable_tiles, *curve_tiles, *length_tiles, *closed_tiles, *sums;
    int *face_range, *face_base, *curve_first;
    Segments g;
    size_t bytes;
};

inline Layout layout_of(char *ws, long long t, long long capacity) {
    Layout l;
    size_t at = 0;
    auto take = [&](size_t bytes) {  // (ws == NULL: the sizes alone)
        char *p = ws ? ws + at : nullptr;
        at += bytes;
        return p;
    };
    long long **face_tiles[2] = {&l.segment_tiles, &l.usable_tiles};
    for (auto p : face_tiles) *p = reinterpret_cast<long long *>(take((size_t)tiles_of(t) * sizeof(long long)));
    long long **segment_tiles[3] = {&l.curve_tiles, &l.length_tiles, &l.closed_tiles};
    for (auto p : segment_tiles) *p = reinterpret_cast<long long *>(take((size_t)tiles_of(capacity) * sizeof(long long)));
    l.sums = reinterpret_cast<long long *>(take(sizeof(long long)));
    l.g.ends = reinterpret_cast<Ends *>(take((size_t)capacity * sizeof(Ends)));
    for (auto &p : l.g.jump) p = reinterpret_cast<int2 *>(take((size_t)capacity * sizeof(int2)));
    int **per_face[2] = {&l.face_range, &l.face_base};
    for (auto p : per_face) *p = reinterpret_cast<int *>(take(ints_bytes(t)));
    int **per_segment[8] = {&l.g.face, &l.g.level, &l.g.succ, &l.g.pred, &l.g.first, &l.g.length, &l.g.first_point, &l.curve_first};
    for (auto p : per_segment) *p = reinterpret_cast<int *>(take(ints_bytes(capacity)));
    l.g.capacity = capacity;
    l.bytes = at + 8;
    return l;
}

}  // namespace

extern "C" {

size_t tn_mesh_half_edges_workspace_bytes(int64_t num_vertices, int64_t num_triangles) {
    if (bad_counts(num_vertices, num_triangles)) return 0;
    return edge_layout_of(nullptr, (long long)num_triangles).bytes;
}

int tn_mesh_half_edges(const int32_t *triangles, int64_t num_triangles, int64_t num_vertices, int32_t *twin, int64_t *counts,
                       void *workspace, size_t workspace_bytes, void *stream) {
    if (!counts) return TN_ERR_NULL;
    if (bad_counts(num_vertices, num_triangles)) return TN_ERR_SHAPE;
    if (num_triangles > 0 && (!triangles || !twin || !workspace)) return TN_ERR_NULL;
    if (misaligned(triangles, 4) || misaligned(twin, 4) || misaligned(counts, 8) || misaligned(workspace, 8)) return TN_ERR_SHAPE;
    if (num_triangles > 0 && workspace_bytes < tn_mesh_half_edges_workspace_bytes(num_vertices, num_triangles)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long long nv = (long long)num_vertices, nt = (long long)num_triangles;
    if (hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s) != hipSuccess) return TN_ERR_LAUNCH;
    if (nt == 0) return TN_OK;
    const EdgeLayout l = edge_layout_of(reinterpret_cast<char *>(workspace), nt);
    const unsigned blocks = (unsigned)tiles_of(3 * nt);
    hipLaunchKernelGGL(edge_keys_kernel, dim3(blocks), dim3(kTile), 0, s, triangles, nt, nv, l.keys, twin);
    TN_LAUNCH_CHECK();
    const int code = tn_sort_pairs(reinterpret_cast<const uint64_t *>(l.keys), nullptr, 3 * num_triangles,
                                   key_bits((unsigned long long)nv * (unsigned long long)nv),  // the keys are 0 .. V * V
                                   reinterpret_cast<uint64_t *>(l.sorted), l.order, l.sort, l.sort_bytes, stream);
    if (code != TN_OK) return code;
    hipLaunchKernelGGL(edge_classes_kernel, dim3(blocks), dim3(kTile), 0, s, l.sorted, l.order, triangles, nt, nv, twin,
                       reinterpret_cast<unsigned long long *>(counts));
    TN_LAUNCH_CHECK();
    return TN_OK;
}

size_t tn_mesh_isolines_workspace_bytes(int64_t num_vertices, int64_t num_triangles, int64_t capacity_segments) {
    if (bad_counts(num_vertices, num_triangles) || capacity_segments < 0 || capacity_segments > kMaxCapacity) return 0;
    return layout_of(nullptr, (long long)num_triangles, (long long)capacity_segments).bytes;
}

int tn_mesh_isolines(const float *positions, const float *temperature, const int32_t *triangles, int64_t num_vertices,
                     int64_t num_triangles, const int32_t *twin, const float *scalar, const tn_isoline_params *params,
                     float *point_positions, float *point_temperature, double *point_arc, int32_t *point_face, tn_mesh_curve *curves,
                     int64_t capacity_segments, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream) {
    if (!params || !counts) return TN_ERR_NULL;
    if (bad_counts(num_vertices, num_triangles) || capacity_segments < 0 || capacity_segments > kMaxCapacity) return TN_ERR_SHAPE;
    if (params->num_levels < 1 || params->num_levels > kMaxLevels) return TN_ERR_SHAPE;
    if (misaligned(positions, 4) || misaligned(temperature, 4) || misaligned(triangles, 4) || misaligned(twin, 4) ||
        misaligned(scalar, 4) || misaligned(point_positions, 4) || misaligned(point_temperature, 4) || misaligned(point_arc, 8) ||
        misaligned(point_face, 4) || misaligned(curves, 8) || misaligned(counts, 8) || misaligned(workspace, 8))
        return TN_ERR_SHAPE;
    Levels lv;
    lv.k = params->num_levels;
    lv.plane = scalar ? 0 : 1;
    for (int k = 0; k < kMaxLevels; ++k) {
        lv.v[k] = k < lv.k ? params->levels[k] : 0.0;
        if (k < lv.k && (!std::isfinite(lv.v[k]) || (k > 0 && !(lv.v[k - 1] < lv.v[k])))) return TN_ERR_UNSUPPORTED;
    }
    for (int a = 0; a < 3; ++a) {
        lv.normal[a] = lv.plane ? params->normal[a] : 0.0;
        if (!std::isfinite(lv.normal[a])) return TN_ERR_UNSUPPORTED;
    }
    if (lv.plane && lv.normal[0] == 0.0 && lv.normal[1] == 0.0 && lv.normal[2] == 0.0) return TN_ERR_UNSUPPORTED;
    const bool work = num_vertices > 0 && num_triangles > 0;
    if (work && (!positions || !temperature || !triangles || !twin || !workspace)) return TN_ERR_NULL;
    if (work && capacity_segments > 0 && (!point_positions || !point_temperature || !point_arc || !point_face || !curves))
        return TN_ERR_NULL;
    if (work && workspace_bytes < tn_mesh_isolines_workspace_bytes(num_vertices, num_triangles, capacity_segments))
        return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (!work) return hipMemsetAsync(counts, 0, 5 * sizeof(int64_t), s) == hipSuccess ? TN_OK : TN_ERR_LAUNCH;
    const long long nv = (long long)num_vertices, nt = (long long)num_triangles, cap = (long long)capacity_segments;
    const Layout l = layout_of(reinterpret_cast<char *>(workspace), nt, cap);
    long long *cnt = reinterpret_cast<long long *>(counts);
    const unsigned face_blocks = (unsigned)tiles_of(nt), segment_blocks = (unsigned)tiles_of(cap);

    // 1 - 2: the faces' level ranges, S and the usable faces
    hipLaunchKernelGGL(faces_kernel, dim3(face_blocks), dim3(kTile), 0, s, positions, temperature, triangles, scalar, lv, nv, nt,
                       l.face_range, l.segment_tiles, l.usable_tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_faces_kernel, dim3(1), dim3(kScan), 0, s, l.segment_tiles, l.usable_tiles, tiles_of(nt), cnt);
    TN_LAUNCH_CHECK();
    if (cap == 0) return TN_OK;  // the sizing call

    // 3 - 5: the segments with their successors and predecessors
    hipLaunchKernelGGL(bases_kernel, dim3(face_blocks), dim3(kTile), 0, s, l.face_range, nt, l.segment_tiles, l.face_base);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(segments_kernel, dim3(face_blocks), dim3(kTile), 0, s, positions, temperature, triangles, scalar, lv, nv, nt, twin,
                       l.face_range, l.face_base, cnt, l.g);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(preds_kernel, dim3(segment_blocks), dim3(kTile), 0, s, cnt, l.g);
    TN_LAUNCH_CHECK();

    // 6 - 8: the first segment of every curve, then the rank of every segment behind it
    const int rounds = jump_rounds(cap);
    int at = 0;  // which of the two jump arrays holds the state
    hipLaunchKernelGGL(sweep1_start_kernel, dim3(segment_blocks), dim3(kTile), 0, s, cnt, l.g);
    TN_LAUNCH_CHECK();
    for (int r = 0; r < rounds; ++r, at ^= 1) {
        hipLaunchKernelGGL(sweep1_kernel, dim3(segment_blocks), dim3(kTile), 0, s, cnt, cap, l.g.jump[at], l.g.jump[at ^ 1]);
        TN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(cut_kernel, dim3(segment_blocks), dim3(kTile), 0, s, cnt, l.g, l.g.jump[at], l.g.jump[at ^ 1]);
    TN_LAUNCH_CHECK();
    at ^= 1;
    for (int r = 0; r < rounds; ++r, at ^= 1) {
        hipLaunchKernelGGL(sweep2_kernel, dim3(segment_blocks), dim3(kTile), 0, s, cnt, cap, l.g.jump[at], l.g.jump[at ^ 1]);
        TN_LAUNCH_CHECK();
    }
    const int2 *ranked = l.g.jump[at];

    // 9 - 10: the curves' lengths, numbers and first points; Q, P and the closed curves
    hipLaunchKernelGGL(lengths_kernel, dim3(segment_blocks), dim3(kTile), 0, s, cnt, l.g, ranked);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(count_curves_kernel, dim3(segment_blocks), dim3(kTile), 0, s, cnt, l.g, l.curve_tiles, l.length_tiles, l.closed_tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_curves_kernel, dim3(1), dim3(kScan), 0, s, l.curve_tiles, l.length_tiles, l.closed_tiles, cap, cnt, l.sums);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(emit_curves_kernel, dim3(segment_blocks), dim3(kTile), 0, s, cnt, l.g, l.curve_tiles, l.length_tiles, l.curve_first);
    TN_LAUNCH_CHECK();

    // 11 - 12: the points, then arc, mean and extremes along every curve
    const Points out = {point_positions, point_temperature, point_arc, point_face, 2 * cap};
    hipLaunchKernelGGL(points_kernel, dim3(segment_blocks), dim3(kTile), 0, s, cnt, l.g, ranked, out);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(walk_kernel, dim3((unsigned)ceil_div(cap * TN_WAVE, kTile)), dim3(kTile), 0, s, cnt, l.g, l.curve_first, out, curves);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

}  // extern "C"
