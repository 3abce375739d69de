// The nearest point of an indexed triangle list to every query point (DESIGN.md "Closest point"; include/thermonerf_hip.h defines
// every output to the bit, without reference to the tree): the second reader of tn_mesh_bvh_build's blob.
// tn_mesh_closest, launches on the caller's stream: a memset of the counts; the walk — blocks of one wave, one point per lane; the
// loop itself is tn_mesh_bvh.h's walk, and this file gives it its two tests: a child's bound b (the squared distance from the point
// to the box) orders the children and a child whose b exceeds the best d2 so far is skipped, also when it is popped later, against
// the best as it is by then; a leaf goes through the bound of its face's own box before any of the face's arithmetic —; one block
// that finishes the statistics (tn_mesh_bvh.h's finish_one).
// No allocation, no host synchronisation, no float atomics, no block ever waits for another; the integer atomics are sums of the
// waves' ballots.
#include "tn_mesh_bvh.h"

using namespace tn;

namespace {

constexpr int kPoints = kLanes;  // points per block: one wave

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

struct Query {
    const float *positions, *temperature;
    const uint8_t *colors;
    const int *triangles;
    long long num_vertices, num_triangles;
    const char *bvh;
    const float *points, *point_temperature;
    long long num_points;
    double r2;
    int *closest_face;
    float *closest_distance, *closest_point, *closest_uv, *closest_temperature;
    uint8_t *closest_colors;
    float *difference;
    unsigned long long *counts;
};

__global__ void __launch_bounds__(kPoints)
bvh_closest_kernel(Query a) {
    __shared__ int stack[kStack][kPoints];      // entry e of lane l: no two lanes of the wave share a bank
    const int lane = threadIdx.x;
    const long long point = (long long)blockIdx.x * kPoints + lane;
    const Tree tree = open_tree(a.bvh, a.num_triangles, a.num_vertices);

    double q[3] = {0.0, 0.0, 0.0};
    bool usable = point < a.num_points;
    if (usable) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float x = a.points[3 * point + k];
            usable = usable && finite(x);
            q[k] = (double)x;
        }
    }
    int best_face = -1;
    Nearest best;
    best.d2 = a.r2, best.u = best.v = 0.0, best.c[0] = best.c[1] = best.c[2] = 0.0;  // d2: the cut until a face is found, then the winner's
    const bool overflow = walk(
        tree, a.triangles, a.num_vertices, &stack[0][lane], usable,
        [&](const float *lo, const float *hi, double &b) {
            b = box_bound(q, lo, hi);
            return !(b > best.d2);  // skipped only when strictly beyond the best, or the cut
        },
        [&](long long t, const long long *i) {
            Nearest own;
            if (face_nearest(q, a.positions, i, best.d2, own) &&
                (own.d2 < best.d2 || (own.d2 == best.d2 && (best_face < 0 || (int)t < best_face)))) {
                best = own, best_face = (int)t;
            }
            return false;
        });
    const bool found = best_face >= 0;
    if (point < a.num_points) {
        float temp = quiet_nan();
        uint8_t rgb[3] = {0, 0, 0};
        if (found && (a.closest_temperature || a.closest_colors || a.difference))
            temp = surface_values(a.temperature, a.colors, a.triangles, a.num_vertices, best_face, best.u, best.v, a.closest_colors != nullptr, rgb);
        if (a.closest_face) a.closest_face[point] = best_face;
        if (a.closest_distance) a.closest_distance[point] = found ? (float)__dsqrt_rn(best.d2) : quiet_nan();
        if (a.closest_point) {
#pragma unroll
            for (int k = 0; k < 3; ++k) a.closest_point[3 * point + k] = found ? (float)best.c[k] : quiet_nan();
        }
        if (a.closest_uv) a.closest_uv[2 * point] = found ? (float)best.u : quiet_nan(), a.closest_uv[2 * point + 1] = found ? (float)best.v : quiet_nan();
        if (a.closest_temperature) a.closest_temperature[point] = temp;
        if (a.closest_colors) {
#pragma unroll
            for (int c = 0; c < 3; ++c) a.closest_colors[3 * point + c] = rgb[c];
        }
        if (a.difference) {
            const float x = (float)__dsub_rn((double)a.point_temperature[point], (double)temp);
            a.difference[point] = x == x ? x : quiet_nan();
        }
    }
    if (a.counts) {
        const unsigned long long with = __ballot(found), good = __ballot(usable), over = __ballot(overflow);
        if (lane == 0) {
            if (with) atomicAdd(a.counts + 0, (unsigned long long)__popcll(with));
            if (good) atomicAdd(a.counts + 1, (unsigned long long)__popcll(good));
            if (over) atomicAdd(a.counts + 3, (unsigned long long)__popcll(over));
            if (blockIdx.x == 0) a.counts[2] = (unsigned long long)tree.num_usable;
        }
    }
}

__global__ void __launch_bounds__(kFinish)
closest_finish_kernel(const float *__restrict__ closest_distance, const float *__restrict__ difference, long long num_points,
                      double *__restrict__ stats) {
    __shared__ double partial[kFinish], partial2[kFinish];
    __shared__ unsigned all_min[kFinish], all_max[kFinish];
    finish_one(closest_distance, num_points, partial, partial2, all_min, all_max, stats);
    finish_one(difference, num_points, partial, partial2, all_min, all_max, stats + 4);
}

}  // namespace

extern "C" {

int tn_mesh_closest(const float *positions, const float *temperature, const uint8_t *colors, const int32_t *triangles, int64_t num_vertices,
                    int64_t num_triangles, const void *bvh, size_t bvh_bytes, const float *points, const float *point_temperature,
                    int64_t num_points, const tn_closest_params *params, int32_t *closest_face, float *closest_distance, float *closest_point,
                    float *closest_uv, float *closest_temperature, uint8_t *closest_colors, float *difference, int64_t *counts, double *stats,
                    void *stream) {
    if (!params || !bvh) return TN_ERR_NULL;
    if (bad_counts(num_vertices, num_triangles) || num_points < 0 || 3 * num_points > 0x7fffffffLL) return TN_ERR_SHAPE;
    if (!(params->max_distance >= 0.0)) return TN_ERR_UNSUPPORTED;  // (a NaN fails)
    const bool work = num_vertices > 0 && num_triangles > 0;
    if (work && (!positions || !temperature || !triangles)) return TN_ERR_NULL;
    if (num_points > 0 && !points) return TN_ERR_NULL;
    if (closest_colors && !colors) return TN_ERR_NULL;
    if (difference && (!closest_temperature || (num_points > 0 && !point_temperature))) return TN_ERR_NULL;
    if (stats && !closest_distance) return TN_ERR_NULL;
    if (misaligned(positions, 4) || misaligned(temperature, 4) || misaligned(triangles, 4) || misaligned(points, 4) ||
        misaligned(point_temperature, 4) || misaligned(closest_face, 4) || misaligned(closest_distance, 4) || misaligned(closest_point, 4) ||
        misaligned(closest_uv, 4) || misaligned(closest_temperature, 4) || misaligned(difference, 4) || misaligned(counts, 8) ||
        misaligned(stats, 8) || misaligned(bvh, 64))
        return TN_ERR_SHAPE;
    if (bvh_bytes < tn_mesh_bvh_bytes(num_triangles)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    Query a;
    a.positions = positions, a.temperature = temperature, a.colors = colors, a.triangles = triangles;
    a.num_vertices = (long long)num_vertices, a.num_triangles = (long long)num_triangles;
    a.bvh = reinterpret_cast<const char *>(bvh);
    a.points = points, a.point_temperature = point_temperature, a.num_points = (long long)num_points;
    a.r2 = params->max_distance * params->max_distance;  // one rounded product (nothing is contracted); +inf stays +inf
    a.closest_face = closest_face, a.closest_distance = closest_distance, a.closest_point = closest_point, a.closest_uv = closest_uv;
    a.closest_temperature = closest_temperature, a.closest_colors = closest_colors, a.difference = difference;
    a.counts = reinterpret_cast<unsigned long long *>(counts);
    if (counts) {
        if (hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s) != hipSuccess) return TN_ERR_LAUNCH;
        if (num_points == 0) {
            hipLaunchKernelGGL(tree_usable_kernel, dim3(1), dim3(TN_WAVE), 0, s, a.bvh, a.num_triangles, a.num_vertices, a.counts);
            TN_LAUNCH_CHECK();
        }
    }
    if (num_points > 0) {
        hipLaunchKernelGGL(bvh_closest_kernel, dim3((unsigned)ceil_div(num_points, kPoints)), dim3(kPoints), 0, s, a);
        TN_LAUNCH_CHECK();
    }
    if (stats) {
        hipLaunchKernelGGL(closest_finish_kernel, dim3(1), dim3(kFinish), 0, s, closest_distance, difference, (long long)num_points, stats);
        TN_LAUNCH_CHECK();
    }
    return TN_OK;
}

}  // extern "C"
