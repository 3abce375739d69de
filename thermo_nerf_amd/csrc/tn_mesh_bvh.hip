// Ray queries against an indexed triangle list (DESIGN.md "Ray casting"; include/thermonerf_hip.h defines the blob and every output
// to the bit): a linear bounding-volume hierarchy built on the device, and a traversal kernel with one ray per lane.
// tn_mesh_bvh_build, launches on the caller's stream:
//   1. classify     one thread per face: USABLE, the face's box into the extent (a wave's minimum first, then integer atomics on
//                   order-preserving bit patterns)
//   2. codes        one thread per face: the 30-bit Morton code of the box centre against the extent; an unusable face gets 2^30
//   3. header       one thread: the counts, the root, the extent
//   4. sort         tn_sort_pairs over 31 bits: the faces in leaf order, straight into the blob
//   5. nodes        one thread per internal node: Karras's radix tree, ties broken by the position in the sorted list
//   6. fit          kDepthBound launches: a node whose children were done BEFORE this launch takes their boxes and is done
// tn_mesh_raycast: a memset of the counts, the traversal (blocks of one wave, the stack of 64 entries per ray in LDS: the walk is
// tn_mesh_bvh.h's, this file gives it the slab against the best hit so far and the face test), one block that finishes the statistics
// (tn_mesh_bvh.h's finish_one).  No allocation, no host synchronisation, no float atomics, no block ever waits for another; the integer
// atomics (extent, counts) are sums, minima and maxima, which do not depend on the order in which they are taken.
#include "tn_mesh_bvh.h"

using namespace tn;

namespace {

constexpr int kTile = 256;
constexpr int kRays = kLanes;     // rays per traversal block: one wave
constexpr unsigned long long kUnusableKey = 1ull << 30;

// ---- build ------------------------------------------------------------------------------------------------------------------

// extent[0..2]: the smallest f2key of a usable face's lo per axis, extent[3..5]: the largest of its hi; keys[t]: 0 usable, 2^30 not
__global__ void __launch_bounds__(kTile)
bvh_classify_kernel(const float *__restrict__ positions, const float *__restrict__ temperature, const int *__restrict__ triangles,
                    long long num_vertices, long long num_triangles, unsigned long long *__restrict__ keys, unsigned *__restrict__ extent) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    float lo[3], hi[3];
    const bool usable = t < num_triangles && usable_face(positions, temperature, triangles, t, num_vertices, lo, hi);
    if (t < num_triangles) keys[t] = usable ? 0ull : kUnusableKey;
    unsigned kmin[3], kmax[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) kmin[k] = usable ? f2key(lo[k]) : ~0u, kmax[k] = usable ? f2key(hi[k]) : 0u;
#pragma unroll
    for (int o = TN_WAVE / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            kmin[k] = min(kmin[k], (unsigned)__shfl_xor((int)kmin[k], o, TN_WAVE));
            kmax[k] = max(kmax[k], (unsigned)__shfl_xor((int)kmax[k], o, TN_WAVE));
        }
    }
    if (threadIdx.x % TN_WAVE == 0 && kmin[0] != ~0u) {
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicMin(extent + k, kmin[k]), atomicMax(extent + 3 + k, kmax[k]);
    }
}

__device__ __forceinline__ unsigned spread3(unsigned x) {  // 10 bits -> every third bit
    x &= 0x3ffu;
    x = (x | x << 16) & 0x030000ffu;
    x = (x | x << 8) & 0x0300f00fu;
    x = (x | x << 4) & 0x030c30c3u;
    x = (x | x << 2) & 0x09249249u;
    return x;
}

__global__ void __launch_bounds__(kTile)
bvh_codes_kernel(const float *__restrict__ positions, const int *__restrict__ triangles, long long num_vertices, long long num_triangles,
                 const unsigned *__restrict__ extent, unsigned long long *__restrict__ keys, int *__restrict__ num_unusable) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    const bool in = t < num_triangles;
    const bool usable = in && keys[t] == 0ull;
    if (usable) {
        long long i[3];
        float lo[3], hi[3];
        corners(triangles, t, num_vertices, i);
        face_box(positions, i, lo, hi);
        unsigned q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double e0 = (double)key2f(extent[k]), e1 = (double)key2f(extent[3 + k]);
            const double c = __dmul_rn(__dadd_rn((double)lo[k], (double)hi[k]), 0.5);
            const double width = __dsub_rn(e1, e0);
            const double x = floor(__dmul_rn(__ddiv_rn(__dsub_rn(c, e0), width), 1024.0));
            q[k] = width > 0.0 ? (unsigned)(x < 0.0 ? 0.0 : (x > 1023.0 ? 1023.0 : x)) : 0u;
        }
        keys[t] = (unsigned long long)(spread3(q[0]) << 2 | spread3(q[1]) << 1 | spread3(q[2]));
    }
    const unsigned long long bad = __ballot(in && !usable);
    if (threadIdx.x % TN_WAVE == 0 && bad != 0ull) atomicAdd(num_unusable, (int)__popcll(bad));
}

__global__ void bvh_header_kernel(Header *__restrict__ header, const unsigned *__restrict__ extent, const int *__restrict__ num_unusable,
                                  long long num_triangles) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    Header h;
    const int bad = num_triangles > 0 ? *num_unusable : 0;
    h.magic = kMagic, h.version = kVersion;
    h.num_faces = (int)num_triangles, h.num_unusable = bad, h.num_usable = (int)num_triangles - bad;
    h.num_nodes = h.num_usable > 1 ? h.num_usable - 1 : 0;
    h.root = h.num_usable > 1 ? 0 : (h.num_usable == 1 ? ~0 : kNone);
    h.depth = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        h.lo[k] = h.num_usable > 0 ? key2f(extent[k]) : INFINITY;
        h.hi[k] = h.num_usable > 0 ? key2f(extent[3 + k]) : -INFINITY;
    }
    h.pad[0] = h.pad[1] = 0;
    *header = h;
}

// the length of the common prefix of the keys at sorted positions i and j, the position breaking ties; -1 outside [0, n)
__device__ __forceinline__ int delta(const unsigned long long *__restrict__ codes, long long i, long long j, long long n) {
    if (j < 0 || j >= n) return -1;
    const unsigned a = (unsigned)codes[i], b = (unsigned)codes[j];
    return a != b ? __clz((int)(a ^ b)) : 32 + __clz((int)((unsigned)i ^ (unsigned)j));
}

__global__ void __launch_bounds__(kTile)
bvh_nodes_kernel(const unsigned long long *__restrict__ codes, const Header *__restrict__ header, long long num_triangles,
                 Node *__restrict__ nodes) {
    const long long i = (long long)blockIdx.x * kTile + threadIdx.x;
    if (i >= num_triangles - 1) return;
    long long n = header->num_usable;
    n = n < num_triangles ? n : num_triangles;
    Node node;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        node.child[c] = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) node.lo[c][k] = node.hi[c][k] = 0.0f;
    }
    node.level = 0, node.pad = 0;
    if (i < n - 1) {
        const long long d = delta(codes, i, i + 1, n) > delta(codes, i, i - 1, n) ? 1 : -1;
        const int dmin = delta(codes, i, i - d, n);
        long long lmax = 2;
        while (delta(codes, i, i + lmax * d, n) > dmin) lmax *= 2;
        long long l = 0;
        for (long long t = lmax / 2; t >= 1; t /= 2)
            if (delta(codes, i, i + (l + t) * d, n) > dmin) l += t;
        const long long j = i + l * d;
        const int dnode = delta(codes, i, j, n);
        long long s = 0, t = l;
        do {
            t = (t + 1) / 2;
            if (delta(codes, i, i + (s + t) * d, n) > dnode) s += t;
        } while (t > 1);
        const long long split = i + s * d + (d < 0 ? -1 : 0);
        const long long first = i < j ? i : j, last = i < j ? j : i;
        node.child[0] = first == split ? ~(int)split : (int)split;
        node.child[1] = last == split + 1 ? ~(int)(split + 1) : (int)(split + 1);
    }
    nodes[i] = node;
}

// pass p: a node whose children were done before this launch (a leaf always is; an internal node carries a level in 1 .. p - 1)
// takes their boxes and the level p.  A level written during this launch is p, which no reader of this launch accepts: launch
// boundaries alone carry data between blocks.
__global__ void __launch_bounds__(kTile)
bvh_fit_kernel(Header *__restrict__ header, Node *__restrict__ nodes, const int *__restrict__ faces, const float *__restrict__ positions,
               const int *__restrict__ triangles, long long num_vertices, long long num_triangles, int pass) {
    const long long i = (long long)blockIdx.x * kTile + threadIdx.x;
    long long n = header->num_nodes;
    n = n < num_triangles - 1 ? n : num_triangles - 1;
    if (i >= n || nodes[i].level != 0) return;
    const int child[2] = {nodes[i].child[0], nodes[i].child[1]};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (child[c] < 0) continue;
        if (child[c] >= n) return;
        const int level = nodes[child[c]].level;
        if (level < 1 || level >= pass) return;
    }
    float lo[2][3], hi[2][3];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (child[c] < 0) {
            const long long leaf = ~child[c];
            if (leaf >= num_triangles) return;
            const long long t = faces[leaf];
            long long v[3];
            if (t < 0 || t >= num_triangles || !corners(triangles, t, num_vertices, v)) return;
            face_box(positions, v, lo[c], hi[c]);
        } else {
            const Node below = nodes[child[c]];
#pragma unroll
            for (int k = 0; k < 3; ++k) lo[c][k] = min_ord(below.lo[0][k], below.lo[1][k]), hi[c][k] = max_ord(below.hi[0][k], below.hi[1][k]);
        }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) nodes[i].lo[c][k] = lo[c][k], nodes[i].hi[c][k] = hi[c][k];
    nodes[i].level = pass;
    if (i == 0) header->depth = pass;
}

// ---- cast -------------------------------------------------------------------------------------------------------------------

struct Cast {
    const float *positions, *temperature;
    const uint8_t *colors;
    const int *triangles;
    long long num_vertices, num_triangles;
    const char *bvh;
    const float *origins, *directions, *ray_t_max;
    long long num_rays;
    double t_min, t_max;
    int cull, any;
    int *hit_face;
    float *hit_t, *hit_uv, *hit_temperature;
    uint8_t *hit_colors, *hit_any;
    unsigned long long *counts;
};

__global__ void __launch_bounds__(kRays)
bvh_raycast_kernel(Cast a) {
    __shared__ int stack[kStack][kRays];  // entry e of lane l: no two lanes of the wave share a bank
    const int lane = threadIdx.x;
    const long long ray = (long long)blockIdx.x * kRays + lane;
    const Tree tree = open_tree(a.bvh, a.num_triangles, a.num_vertices);

    Ray r;
    bool usable = ray < a.num_rays;
    if (usable) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float o = a.origins[3 * ray + k], d = a.directions[3 * ray + k];
            usable = usable && finite(o) && finite(d);
            r.o[k] = (double)o, r.d[k] = (double)d;
            r.inv[k] = __ddiv_rn(1.0, r.d[k]);
        }
        usable = usable && !(r.d[0] == 0.0 && r.d[1] == 0.0 && r.d[2] == 0.0);
        r.t_min = a.t_min, r.t_end = a.t_max;
        if (a.ray_t_max) {
            const double own = (double)a.ray_t_max[ray];
            r.t_end = own < a.t_max ? own : a.t_max;  // (a NaN leaves t_max)
        }
    }
    int best_face = -1;
    double best_t = INFINITY, best_u = 0.0, best_v = 0.0;
    const bool overflow = walk(
        tree, a.triangles, a.num_vertices, &stack[0][lane], usable,
        [&](const float *lo, const float *hi, double &s) {
            double unused;
            return slab(r, lo, hi, s, unused) && s <= best_t;
        },
        [&](long long t, const long long *i) {
            double ft, fu, fv;
            if (!(face_hit(r, a.positions, i, a.cull, ft, fu, fv) && (ft < best_t || (ft == best_t && (int)t < best_face) || best_face < 0)))
                return false;
            best_face = (int)t, best_t = ft, best_u = fu, best_v = fv;
            return a.any != 0;  // any-hit stops at its first
        });
    const bool hit = best_face >= 0;
    if (ray < a.num_rays) {
        if (a.any) {
            if (a.hit_any) a.hit_any[ray] = hit ? 1 : 0;
        } else {
            float temp = quiet_nan();
            uint8_t rgb[3] = {0, 0, 0};
            if (hit && (a.hit_temperature || a.hit_colors))
                temp = surface_values(a.temperature, a.colors, a.triangles, a.num_vertices, best_face, best_u, best_v, a.hit_colors != nullptr, rgb);
            if (a.hit_face) a.hit_face[ray] = best_face;
            if (a.hit_t) a.hit_t[ray] = hit ? (float)best_t : quiet_nan();
            if (a.hit_uv) a.hit_uv[2 * ray] = hit ? (float)best_u : quiet_nan(), a.hit_uv[2 * ray + 1] = hit ? (float)best_v : quiet_nan();
            if (a.hit_temperature) a.hit_temperature[ray] = temp;
            if (a.hit_colors) {
#pragma unroll
                for (int c = 0; c < 3; ++c) a.hit_colors[3 * ray + c] = rgb[c];
            }
        }
    }
    if (a.counts && !a.any) {
        const unsigned long long hits = __ballot(hit), good = __ballot(usable), over = __ballot(overflow);
        if (lane == 0) {
            if (hits) atomicAdd(a.counts + 0, (unsigned long long)__popcll(hits));
            if (good) atomicAdd(a.counts + 1, (unsigned long long)__popcll(good));
            if (over) atomicAdd(a.counts + 3, (unsigned long long)__popcll(over));
            if (blockIdx.x == 0) a.counts[2] = (unsigned long long)tree.num_usable;
        }
    }
}

// one block: SUM2 of (double)hit_temperature in ray order (a miss, the NaN, counts +0.0), the extremes over the hits.  finish_one
// sums in the order this kernel always had — each run of 256 rays in order, then the runs in order —, here without the squares.
__global__ void __launch_bounds__(kFinish)
bvh_finish_kernel(const float *__restrict__ hit_temperature, long long num_rays, double *__restrict__ stats) {
    __shared__ double partial[kFinish], four[4];
    __shared__ unsigned all_min[kFinish], all_max[kFinish];
    finish_one<false>(hit_temperature, num_rays, partial, nullptr, all_min, all_max, four);
    if (threadIdx.x == 0) stats[0] = four[0], stats[1] = four[2], stats[2] = four[3];
}

inline long long tiles_of(long long n) { return ceil_div(n, kTile); }

inline size_t blob_bytes(long long t) { return sizeof(Header) + faces_bytes(t) + (size_t)(t > 1 ? t - 1 : 0) * sizeof(Node); }

// the workspace, in order: the extent's six keys and the unusable count (64 bytes), the keys as computed, the keys sorted, the sort's own
struct Layout {
    unsigned *extent;
    int *num_unusable;
    unsigned long long *keys, *sorted;
    char *sort;
    size_t sort_bytes, bytes;
};

inline Layout layout_of(char *ws, long long t) {
    Layout l;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        char *p = ws ? ws + at : nullptr;
        at += bytes;
        return p;
    };
    l.extent = reinterpret_cast<unsigned *>(take(64));
    l.num_unusable = reinterpret_cast<int *>(l.extent ? l.extent + 6 : nullptr);
    l.keys = reinterpret_cast<unsigned long long *>(take((size_t)t * sizeof(unsigned long long)));
    l.sorted = reinterpret_cast<unsigned long long *>(take((size_t)t * sizeof(unsigned long long)));
    l.sort_bytes = tn_sort_pairs_workspace_bytes(t);
    l.sort = take(align_up(l.sort_bytes, 8));
    l.bytes = at;
    return l;
}

}  // namespace

extern "C" {

int32_t tn_mesh_bvh_depth_bound(void) { return kDepthBound; }

size_t tn_mesh_bvh_bytes(int64_t num_triangles) {
    if (bad_counts(0, num_triangles)) return 0;
    return blob_bytes((long long)num_triangles);
}

size_t tn_mesh_bvh_workspace_bytes(int64_t num_triangles) {
    if (bad_counts(0, num_triangles)) return 0;
    return layout_of(nullptr, (long long)num_triangles).bytes;
}

int tn_mesh_bvh_build(const float *positions, const float *temperature, const int32_t *triangles, int64_t num_vertices,
                      int64_t num_triangles, void *bvh, size_t bvh_bytes, void *workspace, size_t workspace_bytes, void *stream) {
    if (!bvh) return TN_ERR_NULL;
    if (bad_counts(num_vertices, num_triangles)) return TN_ERR_SHAPE;
    const bool work = num_triangles > 0;
    if (work && (!triangles || !workspace)) return TN_ERR_NULL;
    if (work && num_vertices > 0 && (!positions || !temperature)) return TN_ERR_NULL;
    if (misaligned(positions, 4) || misaligned(temperature, 4) || misaligned(triangles, 4) || misaligned(bvh, 64) || misaligned(workspace, 8))
        return TN_ERR_SHAPE;
    if (bvh_bytes < tn_mesh_bvh_bytes(num_triangles)) return TN_ERR_WORKSPACE;
    if (work && workspace_bytes < tn_mesh_bvh_workspace_bytes(num_triangles)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long long nv = (long long)num_vertices, nt = (long long)num_triangles;
    Header *header = reinterpret_cast<Header *>(bvh);
    if (!work) {
        hipLaunchKernelGGL(bvh_header_kernel, dim3(1), dim3(TN_WAVE), 0, s, header, (const unsigned *)nullptr, (const int *)nullptr, 0LL);
        TN_LAUNCH_CHECK();
        return TN_OK;
    }
    const Layout l = layout_of(reinterpret_cast<char *>(workspace), nt);
    int *faces = reinterpret_cast<int *>(reinterpret_cast<char *>(bvh) + sizeof(Header));
    Node *nodes = reinterpret_cast<Node *>(reinterpret_cast<char *>(bvh) + sizeof(Header) + faces_bytes(nt));
    const unsigned face_blocks = (unsigned)tiles_of(nt);

    // 1 - 3: the extent, the codes, the header (the blob's padding behind the faces is zeroed: two builds are byte-equal)
    if (hipMemsetAsync(l.extent, 0xff, 3 * sizeof(unsigned), s) != hipSuccess) return TN_ERR_LAUNCH;
    if (hipMemsetAsync(l.extent + 3, 0, 64 - 3 * sizeof(unsigned), s) != hipSuccess) return TN_ERR_LAUNCH;
    if (hipMemsetAsync(faces, 0, faces_bytes(nt), s) != hipSuccess) return TN_ERR_LAUNCH;
    hipLaunchKernelGGL(bvh_classify_kernel, dim3(face_blocks), dim3(kTile), 0, s, positions, temperature, triangles, nv, nt, l.keys, l.extent);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(bvh_codes_kernel, dim3(face_blocks), dim3(kTile), 0, s, positions, triangles, nv, nt, l.extent, l.keys, l.num_unusable);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(bvh_header_kernel, dim3(1), dim3(TN_WAVE), 0, s, header, l.extent, l.num_unusable, nt);
    TN_LAUNCH_CHECK();

    // 4: the leaf order
    const int code = tn_sort_pairs(reinterpret_cast<const uint64_t *>(l.keys), nullptr, nt, 31, reinterpret_cast<uint64_t *>(l.sorted), faces,
                                   l.sort, l.sort_bytes, stream);
    if (code != TN_OK) return code;
    if (nt < 2) return TN_OK;

    // 5 - 6: the tree, its boxes bottom-up
    const unsigned node_blocks = (unsigned)tiles_of(nt - 1);
    hipLaunchKernelGGL(bvh_nodes_kernel, dim3(node_blocks), dim3(kTile), 0, s, l.sorted, header, nt, nodes);
    TN_LAUNCH_CHECK();
    for (int pass = 1; pass <= kDepthBound; ++pass) {
        hipLaunchKernelGGL(bvh_fit_kernel, dim3(node_blocks), dim3(kTile), 0, s, header, nodes, faces, positions, triangles, nv, nt, pass);
        TN_LAUNCH_CHECK();
    }
    return TN_OK;
}

int tn_mesh_raycast(const float *positions, const float *temperature, const uint8_t *colors, const int32_t *triangles,
                    int64_t num_vertices, int64_t num_triangles, const void *bvh, size_t bvh_bytes, const float *origins,
                    const float *directions, const float *ray_t_max, int64_t num_rays, const tn_raycast_params *params,
                    int32_t *hit_face, float *hit_t, float *hit_uv, float *hit_temperature, uint8_t *hit_colors, uint8_t *hit_any,
                    int64_t *counts, double *stats, void *stream) {
    if (!params || !bvh) return TN_ERR_NULL;
    if (bad_counts(num_vertices, num_triangles) || num_rays < 0 || 3 * num_rays > 0x7fffffffLL) return TN_ERR_SHAPE;
    if (params->t_min != params->t_min || params->t_max != params->t_max || !(params->t_min >= 0.0) || params->cull < 0 || params->cull > 1 ||
        (params->mode != TN_RAYCAST_CLOSEST && params->mode != TN_RAYCAST_ANY))
        return TN_ERR_UNSUPPORTED;
    const bool any = params->mode == TN_RAYCAST_ANY;
    const bool work = num_vertices > 0 && num_triangles > 0;
    if (work && (!positions || !temperature || !triangles)) return TN_ERR_NULL;
    if (num_rays > 0 && (!origins || !directions)) return TN_ERR_NULL;
    if (!any && hit_colors && !colors) return TN_ERR_NULL;
    if (!any && stats && !hit_temperature && num_rays > 0) return TN_ERR_NULL;
    if (misaligned(positions, 4) || misaligned(temperature, 4) || misaligned(triangles, 4) || misaligned(origins, 4) ||
        misaligned(directions, 4) || misaligned(ray_t_max, 4) || misaligned(hit_face, 4) || misaligned(hit_t, 4) || misaligned(hit_uv, 4) ||
        misaligned(hit_temperature, 4) || misaligned(counts, 8) || misaligned(stats, 8) || misaligned(bvh, 64))
        return TN_ERR_SHAPE;
    if (bvh_bytes < tn_mesh_bvh_bytes(num_triangles)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    Cast a;
    a.positions = positions, a.temperature = temperature, a.colors = colors, a.triangles = triangles;
    a.num_vertices = (long long)num_vertices, a.num_triangles = (long long)num_triangles;
    a.bvh = reinterpret_cast<const char *>(bvh);
    a.origins = origins, a.directions = directions, a.ray_t_max = ray_t_max, a.num_rays = (long long)num_rays;
    a.t_min = params->t_min, a.t_max = params->t_max, a.cull = params->cull, a.any = any ? 1 : 0;
    a.hit_face = hit_face, a.hit_t = hit_t, a.hit_uv = hit_uv, a.hit_temperature = hit_temperature;
    a.hit_colors = any ? nullptr : hit_colors, a.hit_any = hit_any;
    a.counts = reinterpret_cast<unsigned long long *>(counts);
    if (!any && counts) {
        if (hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s) != hipSuccess) return TN_ERR_LAUNCH;
        if (num_rays == 0) {
            hipLaunchKernelGGL(tree_usable_kernel, dim3(1), dim3(TN_WAVE), 0, s, a.bvh, a.num_triangles, a.num_vertices, a.counts);
            TN_LAUNCH_CHECK();
        }
    }
    if (num_rays > 0) {
        hipLaunchKernelGGL(bvh_raycast_kernel, dim3((unsigned)ceil_div(num_rays, kRays)), dim3(kRays), 0, s, a);
        TN_LAUNCH_CHECK();
    }
    if (!any && stats) {
        hipLaunchKernelGGL(bvh_finish_kernel, dim3(1), dim3(kFinish), 0, s, hit_temperature, (long long)num_rays, stats);
        TN_LAUNCH_CHECK();
    }
    return TN_OK;
}

}  // extern "C"
