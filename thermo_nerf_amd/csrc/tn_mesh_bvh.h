// The blob of tn_mesh_bvh_build as its readers see it (include/thermonerf_hip.h "THE BLOB"), the one place for it: the header and
// the node, the constants of the tree and of the per-lane traversal stack, and what "usable face" means — the checked corners of a
// face, its box in the numbers' order.  tn_mesh_bvh.hip builds the tree and casts rays through it, tn_mesh_closest.hip walks it for the
// nearest face, tn_mesh_project.hip casts the occlusion rays of a projection: the slab and the face test are here for the two that cast.
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

__device__ __forceinline__ bool finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }  // (a NaN fails)
__device__ __forceinline__ float min_ord(float a, float b) { return f2key(b) < f2key(a) ? b : a; }  // -0.0 below +0.0
__device__ __forceinline__ float max_ord(float a, float b) { return f2key(b) > f2key(a) ? b : a; }

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

__device__ __forceinline__ float quiet_nan() { return __int_as_float(0x7fc00000); }

__device__ __forceinline__ uint8_t colour_of(double c) {
    const double r = floor(__dadd_rn(c, 0.5));
    return (uint8_t)(r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r));
}

}  // namespace tn
