// The nearest point of a face to a point, and the bound of a box against it (include/thermonerf_hip.h "closest point of a face"): the one
// definition of both readers that look for the nearest face — tn_mesh_closest.hip with the point a float widened to fp64,
// tn_mesh_register.hip with the transformed point, any finite fp64.  Nothing here assumes the point fits a float: the header's proof
// (d2 >= b of the face's own box >= b of every ancestor's) uses only that sub, mul and add are monotone.
#pragma once
#include "tn_mesh_bvh.h"

namespace tn {

// b of a box against the point: per axis the gap max(lo - q, q - hi, 0), then the squared length in the order of d2
__device__ __forceinline__ double box_bound(const double *q, const float *lo, const float *hi) {
    double g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = fmax(fmax(__dsub_rn((double)lo[k], q[k]), __dsub_rn(q[k], (double)hi[k])), 0.0);
    return __dadd_rn(__dadd_rn(__dmul_rn(g[0], g[0]), __dmul_rn(g[1], g[1])), __dmul_rn(g[2], g[2]));
}

struct Nearest {
    double d2, u, v, c[3];
};

// a candidate point c with its barycentrics: clamped into the face's box, kept when it is strictly nearer than what `best` holds
__device__ __forceinline__ void consider(const double *q, const float *lo, const float *hi, const double *c, double u, double v, bool &some,
                                         Nearest &best) {
    double x[3], r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double l = (double)lo[k], h = (double)hi[k];
        x[k] = c[k] < l ? l : (c[k] > h ? h : c[k]);
        r[k] = __dsub_rn(q[k], x[k]);
    }
    const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(r[0], r[0]), __dmul_rn(r[1], r[1])), __dmul_rn(r[2], r[2]));
    if (!some || d2 < best.d2) {
        best.d2 = d2, best.u = u, best.v = v;
#pragma unroll
        for (int k = 0; k < 3; ++k) best.c[k] = x[k];
    }
    some = true;
}

// the parameter of the point of the segment a .. a + ab nearest to the point, qa = q - a: in [0, 1], +0.0 for a segment without length
__device__ __forceinline__ double edge_parameter(const double *qa, const double *ab) {
    const double den = dot3(ab, ab);
    const double s = den == 0.0 ? 0.0 : __ddiv_rn(dot3(qa, ab), den);
    return s > 0.0 ? (s > 1.0 ? 1.0 : s) : 0.0;
}

// the closest point of a face with checked corners: the interior candidate and the three edges; false: a position is not finite, or
// b of the face's own box exceeds `limit` (then d2 would: the face can neither win nor tie)
__device__ __forceinline__ bool face_nearest(const double *q, const float *__restrict__ positions, const long long *i, double limit,
                                             Nearest &best) {
    float lo[3], hi[3];
    if (!face_box(positions, i, lo, hi) || box_bound(q, lo, hi) > limit) return false;
    double p0[3], p1[3], e1[3], e2[3], e3[3], w[3], w1[3], n[3], a[3], c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p0[k] = (double)positions[3 * i[0] + k], p1[k] = (double)positions[3 * i[1] + k];
        const double p2 = (double)positions[3 * i[2] + k];
        e1[k] = __dsub_rn(p1[k], p0[k]), e2[k] = __dsub_rn(p2, p0[k]), e3[k] = __dsub_rn(p2, p1[k]);
        w[k] = __dsub_rn(q[k], p0[k]), w1[k] = __dsub_rn(q[k], p1[k]);
    }
    bool some = false;
    cross3(e1, e2, n);
    const double nn = dot3(n, n);
    if (nn != 0.0) {
        cross3(w, e2, a);
        const double u = __ddiv_rn(dot3(a, n), nn);
        cross3(e1, w, a);
        const double v = __ddiv_rn(dot3(a, n), nn);
        if (u >= 0.0 && v >= 0.0 && __dadd_rn(u, v) <= 1.0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = __dadd_rn(__dadd_rn(p0[k], __dmul_rn(u, e1[k])), __dmul_rn(v, e2[k]));
            consider(q, lo, hi, c, u, v, some, best);
        }
    }
    double s = edge_parameter(w, e1);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = __dadd_rn(p0[k], __dmul_rn(s, e1[k]));
    consider(q, lo, hi, c, s, 0.0, some, best);
    s = edge_parameter(w, e2);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = __dadd_rn(p0[k], __dmul_rn(s, e2[k]));
    consider(q, lo, hi, c, 0.0, s, some, best);
    s = edge_parameter(w1, e3);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = __dadd_rn(p1[k], __dmul_rn(s, e3[k]));
    consider(q, lo, hi, c, __dsub_rn(1.0, s), s, some, best);
    return true;
}

// the winner's rule of a walk for the nearest face: `own` of face t replaces `best` when it is nearer, or as near under a lower index
__device__ __forceinline__ void take_nearer(const Nearest &own, long long t, Nearest &best, int &best_face) {
    if (own.d2 < best.d2 || (own.d2 == best.d2 && (best_face < 0 || (int)t < best_face))) best = own, best_face = (int)t;
}

}  // namespace tn
