// The measured thermal photos projected onto points of a mesh (DESIGN.md "Projection"; include/thermonerf_hip.h defines every output
// to the bit): the third reader of tn_mesh_bvh_build's blob.
// tn_mesh_project, launches on the caller's stream: a memset of the counts; the projection — blocks of one wave, one point per lane,
// the loop over the cameras INSIDE the thread with the point's sums in registers, so that the order of every sum is the cameras'
// order whatever the schedule; the camera's record is indexed by the loop counter alone and is read once per wave; the cheap clauses
// (behind, outside the image, facing) come before the walk, which is tn_mesh_bvh.h's walk under the slab alone, stopped by the first
// face_hit: the ray cast's any-hit traversal (tn_mesh_bvh.h holds the slab and the face test of both) —; one block that finishes the
// statistics (tn_mesh_bvh.h's finish_one).
// No allocation, no host synchronisation, no float atomics, no block ever waits for another; the integer atomics are sums of the
// waves' counts.
#include "tn_mesh_bvh.h"

using namespace tn;

namespace {

constexpr int kPoints = kLanes;  // points per block: one wave, as tn_mesh_bvh.hip's kRays (16 KiB of stack: ten blocks share a CU's LDS)
constexpr int kMaxSide = 16384;
constexpr double kVisibleFraction = 0x1.ff8p-1;  // 1 - 2^-10: where visible_from stops its rays
static_assert(kVisibleFraction == 1.0 - 1.0 / 1024.0, "include/thermonerf_hip.h, clause 5");

struct Camera {  // tn_project_camera
    float c2w[12];
    float fx, fy, cx, cy;
};
static_assert(sizeof(Camera) == 64, "one line");

struct Project {
    const float *positions;
    const int *triangles;
    long long num_vertices, num_triangles;
    const char *bvh;
    const float *points, *normals, *point_temperature;
    long long num_points;
    const Camera *cameras;
    const uint8_t *images;
    long long num_cameras;
    double t_lo, t_hi, min_cos, near;
    int width, height, two_sided;
    float *measured;
    int *views, *best_camera;
    float *spread, *difference;
    unsigned long long *counts;
};

__device__ __forceinline__ bool usable_camera(const Camera &c) {
    bool ok = c.fx > 0.0f && c.fy > 0.0f && finite(c.fx) && finite(c.fy) && finite(c.cx) && finite(c.cy);
#pragma unroll
    for (int k = 0; k < 12; ++k) ok = ok && finite(c.c2w[k]);
    return ok;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
    for (int o = TN_WAVE / 2; o > 0; o >>= 1) x += (unsigned long long)__shfl_xor((long long)x, o, TN_WAVE);
    return x;
}

__global__ void __launch_bounds__(kPoints)
bvh_project_kernel(Project a) {
    __shared__ int stack[kStack][kPoints];  // entry e of lane l: no two lanes of the wave share a bank
    const int lane = threadIdx.x;
    const long long point = (long long)blockIdx.x * kPoints + lane;
    const Tree tree = open_tree(a.bvh, a.num_triangles, a.num_vertices);
    const int W = a.width, H = a.height;

    float p[3] = {0.0f, 0.0f, 0.0f};
    double n[3] = {0.0, 0.0, 0.0}, nlen = 1.0;
    bool usable = point < a.num_points;
    if (usable) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[k] = a.points[3 * point + k];
            usable = usable && finite(p[k]);
        }
        if (a.normals) {
            bool zero = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float x = a.normals[3 * point + k];
                usable = usable && finite(x);
                zero = zero && x == 0.0f;
                n[k] = (double)x;
            }
            usable = usable && !zero;
            nlen = __dsqrt_rn(dot3(n, n));
        }
    }
    double sw = 0.0, swt = 0.0, tmin = 0.0, tmax = 0.0, best_w = 0.0;
    int views = 0, best = -1;
    unsigned long long reached = 0ull, over = 0ull, good_cameras = 0ull;

    for (long long k = 0; k < a.num_cameras; ++k) {
        const Camera &c = a.cameras[k];  // the address depends on k alone: one read per wave
        if (!usable_camera(c)) continue;
        ++good_cameras;
        // 1 - 2: the ray of visible_from, the point in the camera's frame
        Ray r;
        bool ray_ok = true;
        const float eye[3] = {c.c2w[3], c.c2w[7], c.c2w[11]};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float d32 = __fsub_rn(p[j], eye[j]);
            ray_ok = ray_ok && finite(d32);
            r.o[j] = (double)eye[j], r.d[j] = (double)d32;
        }
        const double col0[3] = {(double)c.c2w[0], (double)c.c2w[4], (double)c.c2w[8]};
        const double col1[3] = {(double)c.c2w[1], (double)c.c2w[5], (double)c.c2w[9]};
        const double col2[3] = {(double)c.c2w[2], (double)c.c2w[6], (double)c.c2w[10]};
        const double xc = dot3(col0, r.d), yc = dot3(col1, r.d), z = -dot3(col2, r.d);
        bool go = usable && z > 0.0 && z >= a.near;
        // 3: the pixel
        const double u = __dadd_rn(__dmul_rn((double)c.fx, __ddiv_rn(xc, z)), (double)c.cx);
        const double v = __dsub_rn((double)c.cy, __dmul_rn((double)c.fy, __ddiv_rn(yc, z)));
        go = go && 0.5 <= u && u <= (double)W - 0.5 && 0.5 <= v && v <= (double)H - 0.5;
        // 4: facing
        const double dist2 = dot3(r.d, r.d);
        double cosine = 1.0;
        if (a.normals) {
            cosine = __ddiv_rn(-dot3(n, r.d), __dmul_rn(__dsqrt_rn(dist2), nlen));
            cosine = a.two_sided ? fabs(cosine) : cosine;
        }
        go = go && cosine >= a.min_cos;
        // 5: occlusion, the any-hit ray (e, d32) over [0, 1 - 2^-10]; an unusable ray meets nothing
        bool hit = false;
        if (go) {
            ++reached;
            ray_ok = ray_ok && !(r.d[0] == 0.0 && r.d[1] == 0.0 && r.d[2] == 0.0);
#pragma unroll
            for (int j = 0; j < 3; ++j) r.inv[j] = __ddiv_rn(1.0, r.d[j]);
            r.t_min = 0.0, r.t_end = kVisibleFraction;
            const bool overflow = walk(
                tree, a.triangles, a.num_vertices, &stack[0][lane], ray_ok,
                [&](const float *lo, const float *hi, double &s) {
                    double unused;
                    return slab(r, lo, hi, s, unused);
                },
                [&](long long, const long long *i) {
                    double ft, fu, fv;
                    return hit = face_hit(r, a.positions, i, 0, ft, fu, fv);  // the first hit ends the walk
                });
            if (overflow) ++over;
        }
        if (!go || hit) continue;
        // 6: the sample, bilinear between the four surrounding pixel centres (u, v are inside their hull: every index is inside)
        const double fu = __dsub_rn(u, 0.5), fv = __dsub_rn(v, 0.5);
        int x0 = (int)floor(fu), y0 = (int)floor(fv);
        x0 = x0 < W - 2 ? x0 : W - 2, y0 = y0 < H - 2 ? y0 : H - 2;
        x0 = x0 > 0 ? x0 : 0, y0 = y0 > 0 ? y0 : 0;  // (never taken: u, v >= 0.5; the guard of the addresses)
        const double fa = __dsub_rn(fu, (double)x0), fb = __dsub_rn(fv, (double)y0);
        const uint8_t *row = a.images + ((size_t)k * (size_t)H + (size_t)y0) * (size_t)W + (size_t)x0;
        const double p00 = (double)row[0], p01 = (double)row[1], p10 = (double)row[W], p11 = (double)row[W + 1];
        const double top = __dadd_rn(p00, __dmul_rn(fa, __dsub_rn(p01, p00)));
        const double bottom = __dadd_rn(p10, __dmul_rn(fa, __dsub_rn(p11, p10)));
        const double s = __dadd_rn(top, __dmul_rn(fb, __dsub_rn(bottom, top)));
        const double t = __dadd_rn(a.t_lo, __dmul_rn(__ddiv_rn(s, 255.0), __dsub_rn(a.t_hi, a.t_lo)));
        // 7: the weight, and the point's sums in the cameras' order
        const double w = __ddiv_rn(cosine, dist2);
        sw = __dadd_rn(sw, w), swt = __dadd_rn(swt, __dmul_rn(w, t));
        if (views == 0) {
            tmin = tmax = t, best_w = w, best = (int)k;
        } else {
            tmin = t < tmin ? t : tmin, tmax = t > tmax ? t : tmax;
            if (w > best_w) best_w = w, best = (int)k;
        }
        ++views;
    }
    if (point < a.num_points) {
        const bool seen = views > 0;
        const float m = seen ? (float)__ddiv_rn(swt, sw) : quiet_nan();
        if (a.measured) a.measured[point] = m == m ? m : quiet_nan();
        if (a.views) a.views[point] = views;
        if (a.best_camera) a.best_camera[point] = best;
        if (a.spread) a.spread[point] = seen ? (float)__dsub_rn(tmax, tmin) : quiet_nan();
        if (a.difference) {
            const float x = (float)__dsub_rn((double)a.point_temperature[point], (double)m);
            a.difference[point] = x == x ? x : quiet_nan();
        }
    }
    if (a.counts) {
        const unsigned long long seen = wave_sum(views > 0 ? 1ull : 0ull), good = wave_sum(usable ? 1ull : 0ull);
        const unsigned long long tested = wave_sum(reached), accepted = wave_sum((unsigned long long)views), limit = wave_sum(over);
        if (lane == 0) {
            if (seen) atomicAdd(a.counts + 0, seen);
            if (good) atomicAdd(a.counts + 1, good);
            if (tested) atomicAdd(a.counts + 3, tested);
            if (accepted) atomicAdd(a.counts + 4, accepted);
            if (limit) atomicAdd(a.counts + 5, limit);
            if (blockIdx.x == 0) a.counts[2] = good_cameras;
        }
    }
}

// counts[2] of a call without a point
__global__ void project_cameras_kernel(const Camera *__restrict__ cameras, long long num_cameras, unsigned long long *counts) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    unsigned long long good = 0ull;
    for (long long k = 0; k < num_cameras; ++k) good += usable_camera(cameras[k]) ? 1ull : 0ull;
    counts[2] = good;
}

__global__ void __launch_bounds__(kFinish)
project_finish_kernel(const float *__restrict__ difference, const float *__restrict__ spread, const float *__restrict__ measured,
                      long long num_points, double *__restrict__ stats) {
    __shared__ double partial[kFinish], partial2[kFinish], four[4];
    __shared__ unsigned all_min[kFinish], all_max[kFinish];
    finish_one(difference, num_points, partial, partial2, all_min, all_max, stats);
    finish_one(spread, num_points, partial, partial2, all_min, all_max, four);
    if (threadIdx.x == 0) stats[4] = four[0], stats[5] = four[3];
    __syncthreads();
    finish_one(measured, num_points, partial, partial2, all_min, all_max, four);
    if (threadIdx.x == 0) stats[6] = four[0], stats[7] = 0.0;
}

inline bool is_finite(double x) { return x - x == 0.0; }

}  // namespace

extern "C" {

int tn_mesh_project(const float *positions, const float *temperature, const int32_t *triangles, int64_t num_vertices, int64_t num_triangles,
                    const void *bvh, size_t bvh_bytes, const float *points, const float *normals, const float *point_temperature,
                    int64_t num_points, const tn_project_camera *cameras, const uint8_t *images, int64_t num_cameras,
                    const tn_project_params *params, float *measured, int32_t *views, int32_t *best_camera, float *spread, float *difference,
                    int64_t *counts, double *stats, void *stream) {
    if (!params || !bvh) return TN_ERR_NULL;
    if (bad_counts(num_vertices, num_triangles) || num_points < 0 || 3 * num_points > 0x7fffffffLL || num_cameras < 0 ||
        num_cameras > 0x7fffffffLL || params->width < 2 || params->width > kMaxSide || params->height < 2 || params->height > kMaxSide)
        return TN_ERR_SHAPE;
    if (!(params->min_cos > 0.0 && params->min_cos <= 1.0) || !(params->near >= 0.0) || !is_finite(params->t_lo) || !is_finite(params->t_hi))
        return TN_ERR_UNSUPPORTED;  // (a NaN fails each)
    const bool work = num_vertices > 0 && num_triangles > 0;
    if (work && (!positions || !temperature || !triangles)) return TN_ERR_NULL;
    if (num_points > 0 && !points) return TN_ERR_NULL;
    if (num_cameras > 0 && (!cameras || !images)) return TN_ERR_NULL;
    if (difference && num_points > 0 && !point_temperature) return TN_ERR_NULL;
    if (misaligned(positions, 4) || misaligned(temperature, 4) || misaligned(triangles, 4) || misaligned(points, 4) || misaligned(normals, 4) ||
        misaligned(point_temperature, 4) || misaligned(cameras, 4) || misaligned(measured, 4) || misaligned(views, 4) ||
        misaligned(best_camera, 4) || misaligned(spread, 4) || misaligned(difference, 4) || misaligned(counts, 8) || misaligned(stats, 8) ||
        misaligned(bvh, 64))
        return TN_ERR_SHAPE;
    if (bvh_bytes < tn_mesh_bvh_bytes(num_triangles)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    Project a;
    a.positions = positions, a.triangles = triangles;
    a.num_vertices = (long long)num_vertices, a.num_triangles = (long long)num_triangles;
    a.bvh = reinterpret_cast<const char *>(bvh);
    a.points = points, a.normals = normals, a.point_temperature = point_temperature, a.num_points = (long long)num_points;
    a.cameras = reinterpret_cast<const Camera *>(cameras), a.images = images, a.num_cameras = (long long)num_cameras;
    a.t_lo = params->t_lo, a.t_hi = params->t_hi, a.min_cos = params->min_cos, a.near = params->near;
    a.width = params->width, a.height = params->height, a.two_sided = params->two_sided ? 1 : 0;
    a.measured = measured, a.views = views, a.best_camera = best_camera, a.spread = spread, a.difference = difference;
    a.counts = reinterpret_cast<unsigned long long *>(counts);
    if (counts) {
        if (hipMemsetAsync(counts, 0, 6 * sizeof(int64_t), s) != hipSuccess) return TN_ERR_LAUNCH;
        if (num_points == 0 && num_cameras > 0) {
            hipLaunchKernelGGL(project_cameras_kernel, dim3(1), dim3(TN_WAVE), 0, s, a.cameras, a.num_cameras, a.counts);
            TN_LAUNCH_CHECK();
        }
    }
    if (num_points > 0) {
        hipLaunchKernelGGL(bvh_project_kernel, dim3((unsigned)ceil_div(num_points, kPoints)), dim3(kPoints), 0, s, a);
        TN_LAUNCH_CHECK();
    }
    if (stats) {
        hipLaunchKernelGGL(project_finish_kernel, dim3(1), dim3(kFinish), 0, s, difference, spread, measured, (long long)num_points, stats);
        TN_LAUNCH_CHECK();
    }
    return TN_OK;
}

}  // extern "C"
