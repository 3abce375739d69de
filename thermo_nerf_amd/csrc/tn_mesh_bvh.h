// The blob of tn_mesh_bvh_build as its readers see it (include/thermonerf_hip.h "THE BLOB"), the one place for it: the header and
// the node, the constants of the tree and of the per-lane traversal stack, what "usable face" means — the checked corners of a
// face, its box in the numbers' order —, the opened blob (Tree, open_tree: the only header check and the only offsets), THE walk
// (walk: node unpack, nearer child first, the other on the LDS stack, overflow, the step guard — a reader supplies a box test and
// a leaf test), the surface's values at (face, u, v), and the one statistics pass of the finish kernels (finish_one).
// tn_mesh_bvh.hip builds the tree and casts rays through it, tn_mesh_closest.hip walks it for the nearest face, tn_mesh_project.hip
// casts the occlusion rays of a projection: the slab and the face test are here for the two that cast.  tn_mesh_register.hip walks it
// for the nearest face of transformed points: what it shares with tn_mesh_closest.hip is in tn_mesh_closest.h.
#pragma once
#include "tn_device.h"

namespace tn {

constexpr int kDepthBound = 61;   // 30 code bits + 31 index bits: see the header
constexpr int kStack = 64;        // entries per ray, >= kDepthBound
constexpr unsigned kMagic = 0x56424e54u;  // "TNBV"
constexpr int kVersion = 1;
constexpr int kNone = INT32_MIN;  // the root of a tree without a face
static_assert(kStack >= kDepthBound, "the stack covers the depth bound");

struct alignas(64) Header {  // tn_mesh_bvh's first 64 bytes
    unsigned magic;
    int version;
    int num_faces, num_usable, num_unusable, num_nodes;
    int root, depth;
    float lo[3], hi[3];
    int pad[2];
};
static_assert(sizeof(Header) == 64, "one line");

struct alignas(64) Node {
    float lo[2][3], hi[2][3];  // the boxes of child 0 and child 1
    int child[2];              // >= 0: an internal node; < 0: the leaf ~child (a position in the leaf order)
    int level;                 // the node's height: 1 + the larger of its children's, a leaf being 0
    int pad;
};
static_assert(sizeof(Node) == 64, "one fetch decides both children");


// the three vertex indices of face t, checked; false: not VALID or not distinct
__device__ __forceinline__ bool corners(const int *__restrict__ triangles, long long t, long long num_vertices, long long *i) {
    i[0] = triangles[3 * t], i[1] = triangles[3 * t + 1], i[2] = triangles[3 * t + 2];
    const bool ok = i[0] >= 0 && i[0] < num_vertices && i[1] >= 0 && i[1] < num_vertices && i[2] >= 0 && i[2] < num_vertices;
    return ok && i[0] != i[1] && i[1] != i[2] && i[0] != i[2];
}

// the box of a face with checked corners; false: a position is not finite
__device__ __forceinline__ bool face_box(const float *__restrict__ positions, const long long *i, float *lo, float *hi) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = positions[3 * i[0] + k], b = positions[3 * i[1] + k], c = positions[3 * i[2] + k];
        ok = ok && finite(a) && finite(b) && finite(c);
        lo[k] = min_ord(min_ord(a, b), c);
        hi[k] = max_ord(max_ord(a, b), c);
    }
    return ok;
}

__device__ __forceinline__ bool usable_face(const float *__restrict__ positions, const float *__restrict__ temperature,
                                            const int *__restrict__ triangles, long long t, long long num_vertices, float *lo, float *hi) {
    long long i[3];
    if (!corners(triangles, t, num_vertices, i)) return false;
    if (!(finite(temperature[i[0]]) && finite(temperature[i[1]]) && finite(temperature[i[2]]))) return false;
    return face_box(positions, i, lo, hi);
}

// the dot and the cross product in the order the header fixes, every operation rounded on its own
__device__ __forceinline__ double dot3(const double *a, const double *b) {
    return __dadd_rn(__dadd_rn(__dmul_rn(a[0], b[0]), __dmul_rn(a[1], b[1])), __dmul_rn(a[2], b[2]));
}
__device__ __forceinline__ void cross3(const double *a, const double *b, double *c) {
    c[0] = __dsub_rn(__dmul_rn(a[1], b[2]), __dmul_rn(a[2], b[1]));
    c[1] = __dsub_rn(__dmul_rn(a[2], b[0]), __dmul_rn(a[0], b[2]));
    c[2] = __dsub_rn(__dmul_rn(a[0], b[1]), __dmul_rn(a[1], b[0]));
}

// ---- the ray against a box and against a face: the one definition of both readers that cast (tn_mesh_bvh.hip, tn_mesh_project.hip) ----

constexpr double kSlack = 0x1.ffffffffp-1;  // 1 - 2^-32

struct Ray {
    double o[3], d[3], inv[3];
    double t_min, t_end;
};

// the slab of the ray against a box: s = enter shrunk by 2^-32, the exit; true: the box PASSES
__device__ __forceinline__ bool slab(const Ray &r, const float *lo, const float *hi, double &s, double &exit) {
    double enter = r.t_min;
    exit = r.t_end;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double l = (double)lo[k], h = (double)hi[k];
        if (r.d[k] == 0.0) {
            ok = ok && l <= r.o[k] && r.o[k] <= h;
        } else {
            const double a = __dmul_rn(__dsub_rn(l, r.o[k]), r.inv[k]), b = __dmul_rn(__dsub_rn(h, r.o[k]), r.inv[k]);
            enter = fmax(enter, fmin(a, b));
            exit = fmin(exit, fmax(a, b));
        }
    }
    s = __dmul_rn(enter, kSlack);
    return ok && s <= exit;
}

// Moeller-Trumbore in fp64 and the face's own box; true: a HIT
__device__ __forceinline__ bool face_hit(const Ray &r, const float *__restrict__ positions, const long long *i, int cull, double &t,
                                         double &u, double &v) {
    double p0[3], e1[3], e2[3], tv[3], pv[3], qv[3];
    float lo[3], hi[3];
    if (!face_box(positions, i, lo, hi)) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p0[k] = (double)positions[3 * i[0] + k];
        e1[k] = __dsub_rn((double)positions[3 * i[1] + k], p0[k]);
        e2[k] = __dsub_rn((double)positions[3 * i[2] + k], p0[k]);
        tv[k] = __dsub_rn(r.o[k], p0[k]);
    }
    cross3(r.d, e2, pv);
    const double det = dot3(e1, pv);
    if (det == 0.0 || (cull == 1 && det < 0.0)) return false;
    u = __ddiv_rn(dot3(tv, pv), det);
    cross3(tv, e1, qv);
    v = __ddiv_rn(dot3(r.d, qv), det);
    t = __ddiv_rn(dot3(e2, qv), det);
    if (!(u >= 0.0 && v >= 0.0 && __dadd_rn(u, v) <= 1.0 && r.t_min <= t && t <= r.t_end)) return false;
    double s, exit;
    return slab(r, lo, hi, s, exit) && s <= t;
}

// ---- the opened blob and the walk: the one definition of all three readers ----------------------------------------------------

constexpr int kLanes = 64;  // lanes of a walking block, one wave: the stride of a lane's column in the LDS stack

__host__ __device__ inline size_t faces_bytes(long long t) { return ((size_t)t * sizeof(int) + 63) / 64 * 64; }  // host and device: one expression

struct Tree {
    const int *faces;   // the faces in leaf order
    const Node *nodes;
    long long T, num_nodes;  // num_nodes: the header's, at most T - 1; 0 for a blob that is not this mesh's tree
    int root, num_usable;    // kNone and 0 for such a blob
};

__device__ __forceinline__ Tree open_tree(const char *__restrict__ bvh, long long num_triangles, long long num_vertices) {
    const Header *header = reinterpret_cast<const Header *>(bvh);
    const long long T = num_triangles;
    const bool tree = T > 0 && num_vertices > 0 && header->magic == kMagic && header->version == kVersion && header->num_faces == (int)T;
    Tree tr;
    tr.T = T;
    tr.num_nodes = tree ? header->num_nodes : 0;
    tr.num_nodes = tr.num_nodes < T - 1 ? tr.num_nodes : T - 1;
    tr.root = tree ? header->root : kNone;
    tr.num_usable = tree && header->num_usable > 0 ? header->num_usable : 0;
    tr.faces = reinterpret_cast<const int *>(bvh + sizeof(Header));
    tr.nodes = reinterpret_cast<const Node *>(bvh + sizeof(Header) + faces_bytes(T));
    return tr;
}

// The walk of one lane.  box(lo, hi, key) -> the child's box passes, key: what orders two passing children (the smaller first);
// leaf(t, i) -> stop, t a face of the tree with its checked corners i.  A node is one 64-byte fetch and BOTH children's tests
// before either is descended; the farther child goes on the lane's column of the LDS stack (entry e at column[e * kLanes]), on a
// full stack that subtree is not descended and the walk returns true; a popped entry is tested against the callables' state as it is
// by then; a child beyond num_nodes and a leaf out of range are skipped.  The callables hold the kernel's best-so-far by reference.
template <typename Box, typename Leaf>
__device__ __forceinline__ bool walk(const Tree &tr, const int *__restrict__ triangles, long long num_vertices, int *column, bool start,
                                     Box &&box, Leaf &&leaf) {
    bool overflow = false;
    int cur = start ? tr.root : kNone;
    int sp = 0;
    long long steps = 2 * tr.T + 2;  // a tree visits each of its 2U - 1 nodes at most once: a foreign blob with a cycle ends here
    while (cur != kNone && steps-- > 0) {
        int next = kNone;
        if (cur < 0) {
            const long long at = ~cur;
            const long long t = at < tr.T ? tr.faces[at] : -1;
            long long i[3];
            if (t >= 0 && t < tr.T && corners(triangles, t, num_vertices, i) && leaf(t, i)) break;
        } else if (cur < tr.num_nodes) {
            const float4 *q = reinterpret_cast<const float4 *>(tr.nodes + cur);
            const float4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
            const float lo0[3] = {q0.x, q0.y, q0.z}, lo1[3] = {q0.w, q1.x, q1.y};
            const float hi0[3] = {q1.z, q1.w, q2.x}, hi1[3] = {q2.y, q2.z, q2.w};
            const int c0 = __float_as_int(q3.x), c1 = __float_as_int(q3.y);
            double k0, k1;
            const bool go0 = box(lo0, hi0, k0);
            const bool go1 = box(lo1, hi1, k1);
            if (go0 && go1) {
                const bool swap = k1 < k0;  // the nearer child first
                next = swap ? c1 : c0;
                if (sp < kStack) column[sp++ * kLanes] = swap ? c0 : c1;
                else overflow = true;  // that subtree is not descended
            } else if (go0 || go1) {
                next = go0 ? c0 : c1;
            }
        }
        if (next == kNone && sp > 0) next = column[--sp * kLanes];
        cur = next;
    }
    return overflow;
}

// counts[2] of a call without queries
static __global__ void tree_usable_kernel(const char *__restrict__ bvh, long long num_triangles, long long num_vertices,
                                          unsigned long long *counts) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    counts[2] = (unsigned long long)open_tree(bvh, num_triangles, num_vertices).num_usable;
}

// the temperature of the point (u, v) of a face, and with `colour` its colour into rgb: w = 1 - u - v, then (w a + u b) + v c
__device__ __forceinline__ float surface_values(const float *__restrict__ temperature, const uint8_t *__restrict__ colors,
                                                const int *__restrict__ triangles, long long num_vertices, int face, double u, double v,
                                                bool colour, uint8_t *rgb) {
    long long i[3];
    corners(triangles, face, num_vertices, i);
    const double w = __dsub_rn(__dsub_rn(1.0, u), v);
    if (colour) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            rgb[c] = colour_of(__dadd_rn(__dadd_rn(__dmul_rn(w, (double)colors[3 * i[0] + c]), __dmul_rn(u, (double)colors[3 * i[1] + c])),
                                         __dmul_rn(v, (double)colors[3 * i[2] + c])));
    }
    return (float)__dadd_rn(__dadd_rn(__dmul_rn(w, (double)temperature[i[0]]), __dmul_rn(u, (double)temperature[i[1]])),
                            __dmul_rn(v, (double)temperature[i[2]]));
}

// ---- the statistics pass of the finish kernels ----------------------------------------------------------------------------------

constexpr int kFinish = 1024;  // threads of a finish block

// SUM2 of (double)values and of their squares in query order (the NaN of a query without the value counts +0.0), the extremes over
// the queries that have it, into out[0 .. 3]; values == nullptr: no query has the value.  Every thread of the one block calls it;
// partial, partial2, all_min and all_max are kFinish entries of LDS each.  kSquares false: the squares are left out — out[1] is +0.0
// and partial2 is not touched (the cast's statistics have no use for them, and its finish is a third of a closest-hit call's time).
template <bool kSquares = true>
static __device__ void finish_one(const float *__restrict__ values, long long n, double *partial, double *partial2, unsigned *all_min,
                                  unsigned *all_max, double *out) {
    const long long blocks = values ? (n + 255) / 256 : 0;
    double sum = 0.0, sum2 = 0.0;
    unsigned kmin = ~0u, kmax = 0u;
    for (long long first = 0; first < blocks; first += kFinish) {
        const long long b = first + threadIdx.x;
        double own = 0.0, own2 = 0.0;
        if (b < blocks) {
            const long long end = (b + 1) * 256 < n ? (b + 1) * 256 : n;
            for (long long k = b * 256; k < end; ++k) {
                const float x = values[k];
                const bool has = x == x;
                const double d = has ? (double)x : 0.0;
                own = __dadd_rn(own, d);
                if constexpr (kSquares) own2 = __dadd_rn(own2, __dmul_rn(d, d));
                kmin = has ? min(kmin, f2key(x)) : kmin, kmax = has ? max(kmax, f2key(x)) : kmax;
            }
        }
        partial[threadIdx.x] = own;
        if constexpr (kSquares) partial2[threadIdx.x] = own2;
        __syncthreads();
        if (threadIdx.x == 0) {
            const long long here = blocks - first < kFinish ? blocks - first : kFinish;
            for (int k = 0; k < here; ++k) {
                sum = __dadd_rn(sum, partial[k]);
                if constexpr (kSquares) sum2 = __dadd_rn(sum2, partial2[k]);
            }
        }
        __syncthreads();
    }
    all_min[threadIdx.x] = kmin, all_max[threadIdx.x] = kmax;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kFinish; ++k) kmin = min(kmin, all_min[k]), kmax = max(kmax, all_max[k]);
        out[0] = sum, out[1] = sum2;
        out[2] = kmin <= kmax ? (double)key2f(kmin) : (double)INFINITY;
        out[3] = kmin <= kmax ? (double)key2f(kmax) : -(double)INFINITY;
    }
    __syncthreads();
}

}  // namespace tn
