// The nearest point of an indexed triangle list to every query point (DESIGN.md "Closest point"; include/thermonerf_hip.h defines
// every output to the bit, without reference to the tree): the second reader of tn_mesh_bvh_build's blob.
// tn_mesh_closest, launches on the caller's stream: a memset of the counts; the walk — blocks of one wave, one point per lane; the
// loop itself is tn_mesh_bvh.h's walk, and this file gives it its two tests: a child's bound b (the squared distance from the point
// to the box) orders the children and a child whose b exceeds the best d2 so far is skipped, also when it is popped later, against
// the best as it is by then; a leaf goes through the bound of its face's own box before any of the face's arithmetic —; one block
// that finishes the statistics (tn_mesh_bvh.h's finish_one).  The bound and the face's arithmetic are tn_mesh_closest.h's, shared with
// tn_mesh_register.hip.
// No allocation, no host synchronisation, no float atomics, no block ever waits for another; the integer atomics are sums of the
// waves' ballots.
#include "tn_mesh_closest.h"

using namespace tn;

namespace {

constexpr int kPoints = kLanes;  // points per block: one wave

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
            if (face_nearest(q, a.positions, i, best.d2, own)) take_nearer(own, t, best, best_face);
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
