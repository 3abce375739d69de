// Registration of a point cloud to a mesh (DESIGN.md "Registration"; include/thermonerf_hip.h defines every output to the bit,
// without reference to the tree): iterated closest points with a Gauss-Newton step, the fourth reader of tn_mesh_bvh_build's blob.
// tn_mesh_register, launches on the caller's stream: a memset of the control words; then per iteration the walk — blocks of one wave,
// one point per lane, tn_mesh_bvh.h's walk with tn_mesh_closest.h's bound and face arithmetic from the TRANSFORMED point, after it the
// point's rows, the 36 sums of the wave through the fixed adjacent-pair tree, one partial per wave — and one block that sums the
// partials in finish_one's order, solves the 6 or 7 unknowns with one thread, writes the new transform in place, the history row and
// the result.  A finished run sets a device flag that the later iterations' kernels read and return on.
// No allocation, no host synchronisation, no host read, no float atomics, no block ever waits for another.
#include "tn_mesh_closest.h"

using namespace tn;

namespace {

constexpr int kPoints = kLanes;   // points per block: one wave
constexpr int kSums = 36;         // the upper triangle of sum g g^T (28), sum g r (7), sum r r (1)
constexpr int kWords = 40;        // doubles of a wave's partial: the sums, matched, usable, without a normal, +0.0
constexpr int kRun = 256;         // waves of a run of the finish
constexpr int kSlots = kFinish / kWords;  // runs summed at once by the finish block
constexpr int kControl = 64;      // bytes of the control words in front of the partials: [0] done
constexpr int kMaxIterations = 1024;
constexpr double kNotRun = -1.0;  // a history entry of an iteration that did not run, or of an update that was refused

__device__ __forceinline__ bool finite64(double x) { return fabs(x) < (double)INFINITY; }

struct Walk {
    const float *positions;
    const int *triangles;
    long long num_vertices, num_triangles;
    const char *bvh;
    const float *points;
    long long num_points;
    double r2, center[3];
    int metric;
    const double *transform;
    const long long *control;
    double *partials;
};

__global__ void __launch_bounds__(kPoints)
register_walk_kernel(Walk a) {
    __shared__ int stack[kStack][kPoints];      // entry e of lane l: no two lanes of the wave share a bank
    if (a.control[0] != 0) return;              // the run is done
    const int lane = threadIdx.x;
    const long long point = (long long)blockIdx.x * kPoints + lane;
    const Tree tree = open_tree(a.bvh, a.num_triangles, a.num_vertices);

    double q[3] = {0.0, 0.0, 0.0};
    bool usable = point < a.num_points;
    if (usable) {
        double p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float x = a.points[3 * point + k];
            usable = usable && finite(x);
            p[k] = (double)x;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double *m = a.transform + 4 * k;
            q[k] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[0], p[0]), __dmul_rn(m[1], p[1])), __dmul_rn(m[2], p[2])), m[3]);
        }
        usable = usable && finite64(q[0]) && finite64(q[1]) && finite64(q[2]);
    }
    int best_face = -1;
    Nearest best;
    best.d2 = a.r2, best.u = best.v = 0.0, best.c[0] = best.c[1] = best.c[2] = 0.0;  // d2: the cut until a face is found, then the winner's
    walk(
        tree, a.triangles, a.num_vertices, &stack[0][lane], usable,
        [&](const float *lo, const float *hi, double &b) {
            b = box_bound(q, lo, hi);
            return !(b > best.d2);
        },
        [&](long long t, const long long *i) {
            Nearest own;
            if (face_nearest(q, a.positions, i, best.d2, own)) take_nearer(own, t, best, best_face);
            return false;
        });

    // the rows of the point: only from here on do the 36 sums exist
    const bool found = best_face >= 0;
    double n[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    int rows = found ? 3 : 0;
    bool flat = false;
    if (found && a.metric == 1) {
        long long i[3];
        corners(a.triangles, best_face, a.num_vertices, i);
        double e1[3], e2[3], c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double p0 = (double)a.positions[3 * i[0] + k];
            e1[k] = __dsub_rn((double)a.positions[3 * i[1] + k], p0), e2[k] = __dsub_rn((double)a.positions[3 * i[2] + k], p0);
        }
        cross3(e1, e2, c);
        const double nn = dot3(c, c);
        flat = nn == 0.0;
        rows = flat ? 0 : 1;
        const double length = flat ? 1.0 : __dsqrt_rn(nn);
#pragma unroll
        for (int k = 0; k < 3; ++k) n[0][k] = __ddiv_rn(c[k], length);
    }
    double y[3], e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) y[k] = __dsub_rn(q[k], a.center[k]), e[k] = __dsub_rn(q[k], best.c[k]);
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
#pragma unroll
    for (int row = 0; row < 3; ++row) {
        if (row < rows) {
            double g[7];
            cross3(y, n[row], g);
#pragma unroll
            for (int k = 0; k < 3; ++k) g[3 + k] = n[row][k];
            g[6] = dot3(n[row], y);
            const double r = dot3(n[row], e);
            int at = 0;
#pragma unroll
            for (int i = 0; i < 7; ++i) {
#pragma unroll
                for (int j = i; j < 7; ++j, ++at) acc[at] = __dadd_rn(acc[at], __dmul_rn(g[i], g[j]));
            }
#pragma unroll
            for (int i = 0; i < 7; ++i) acc[28 + i] = __dadd_rn(acc[28 + i], __dmul_rn(g[i], r));
            acc[35] = __dadd_rn(acc[35], __dmul_rn(r, r));
        }
    }
    // the adjacent-pair tree over the 64 lanes: (0 + 1), (2 + 3), ..., then pairs of those; an fp64 add is commutative, so the
    // butterfly gives every lane the tree's sum
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
#pragma unroll
        for (int off = 1; off < kLanes; off *= 2) acc[k] = __dadd_rn(acc[k], __shfl_xor(acc[k], off, kLanes));
    }
    const unsigned long long matched = __ballot(rows > 0), good = __ballot(usable), none = __ballot(flat);
    if (lane == 0) {
        double *out = a.partials + (long long)blockIdx.x * kWords;
#pragma unroll
        for (int k = 0; k < kSums; ++k) out[k] = acc[k];
        out[36] = (double)__popcll(matched), out[37] = (double)__popcll(good), out[38] = (double)__popcll(none), out[39] = 0.0;
    }
}

struct Finish {
    const double *partials;
    long long waves;
    long long *control;
    double *transform, *history;
    long long *result;
    double center[3], length, damping, tolerance;
    int iteration, iterations, with_scale, min_pairs;
};

// the step of one thread: the damped normal equations by LDL^T in the header's written order, the Cayley update of the transform in
// place, the history row and the result
__device__ void solve_and_update(const double *total, const Finish &s, double (*A)[7], double (*L)[7], double *d, double *z) {
    const int k = s.with_scale ? 7 : 6;
    const double m = total[36], rr = total[35];
    double *row = s.history + 4 * (long long)s.iteration;
    int status = TN_REGISTER_ITERATIONS;
    bool refused = false;
    double delta[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (m < (double)s.min_pairs) {
        status = TN_REGISTER_TOO_FEW, refused = true;
    } else {
        int at = 0;
        for (int i = 0; i < 7; ++i)
            for (int j = i; j < 7; ++j, ++at) A[i][j] = A[j][i] = total[at];
        const double l2 = __dmul_rn(s.length, s.length), lambda = __dmul_rn(s.damping, m);
        for (int i = 0; i < 7; ++i) A[i][i] = __dadd_rn(A[i][i], __dmul_rn(lambda, (i >= 3 && i < 6) ? 1.0 : l2));
        for (int j = 0; j < k && !refused; ++j) {
            double dj = A[j][j];
            for (int p = 0; p < j; ++p) dj = __dsub_rn(dj, __dmul_rn(L[j][p], __dmul_rn(L[j][p], d[p])));
            if (!(dj > 0.0) || !finite64(dj)) {
                refused = true;
                break;
            }
            d[j] = dj;
            for (int i = j + 1; i < k; ++i) {
                double v = A[j][i];
                for (int p = 0; p < j; ++p) v = __dsub_rn(v, __dmul_rn(L[i][p], __dmul_rn(L[j][p], d[p])));
                L[i][j] = __ddiv_rn(v, dj);
            }
        }
        if (!refused) {
            for (int i = 0; i < k; ++i) {
                double v = -total[28 + i];
                for (int p = 0; p < i; ++p) v = __dsub_rn(v, __dmul_rn(L[i][p], z[p]));
                z[i] = v;
            }
            for (int i = 0; i < k; ++i) z[i] = __ddiv_rn(z[i], d[i]);
            for (int i = k - 1; i >= 0; --i) {
                double v = z[i];
                for (int p = i + 1; p < k; ++p) v = __dsub_rn(v, __dmul_rn(L[p][i], delta[p]));
                delta[i] = v;
                refused = refused || !finite64(v);
            }
        }
        if (refused) status = TN_REGISTER_DEGENERATE;
    }
    row[0] = m, row[1] = rr;
    if (refused) {
        row[2] = row[3] = kNotRun;
    } else {
        const double a[3] = {__dmul_rn(0.5, delta[0]), __dmul_rn(0.5, delta[1]), __dmul_rn(0.5, delta[2])};
        const double aa = dot3(a, a), f = __ddiv_rn(2.0, __dadd_rn(1.0, aa)), scale = __dadd_rn(1.0, delta[6]);
        const double K[3][3] = {{0.0, -a[2], a[1]}, {a[2], 0.0, -a[0]}, {-a[1], a[0], 0.0}};
        double U[3][3], M[12], t[3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double k2 = i == j ? __dsub_rn(__dmul_rn(a[i], a[i]), aa) : __dmul_rn(a[i], a[j]);
                U[i][j] = __dmul_rn(scale, __dadd_rn(i == j ? 1.0 : 0.0, __dmul_rn(f, __dadd_rn(K[i][j], k2))));
            }
        for (int i = 0; i < 12; ++i) M[i] = s.transform[i];
        for (int j = 0; j < 3; ++j) t[j] = __dsub_rn(M[4 * j + 3], s.center[j]);
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) {
                const double column[3] = {M[j], M[4 + j], M[8 + j]};
                s.transform[4 * i + j] = dot3(U[i], column);
            }
            s.transform[4 * i + 3] = __dadd_rn(__dadd_rn(s.center[i], dot3(U[i], t)), delta[3 + i]);
        }
        const double turn = fmax(fmax(fabs(delta[0]), fabs(delta[1])), fmax(fabs(delta[2]), fabs(delta[6])));
        const double shift = __ddiv_rn(fmax(fmax(fabs(delta[3]), fabs(delta[4])), fabs(delta[5])), s.length);
        row[2] = turn, row[3] = shift;
        if (turn <= s.tolerance && shift <= s.tolerance) status = TN_REGISTER_CONVERGED;
    }
    if (status != TN_REGISTER_ITERATIONS) s.control[0] = 1;
    s.result[0] = status, s.result[1] = s.iteration + 1, s.result[2] = (long long)m, s.result[3] = (long long)total[37];
}

__global__ void __launch_bounds__(kFinish)
register_finish_kernel(Finish s) {
    __shared__ double run_sum[kSlots][kWords], total[kWords];
    __shared__ double A[7][7], L[7][7], d[7], z[7];
    const int tid = threadIdx.x;
    if (s.control[0] != 0) {  // done before this iteration: its row says so
        if (tid < 4) s.history[4 * (long long)s.iteration + tid] = kNotRun;
        return;
    }
    const int j = tid % kWords, slot = tid / kWords;
    const long long runs = (s.waves + kRun - 1) / kRun;
    double sum = 0.0;
    for (long long first = 0; first < runs; first += kSlots) {
        const long long b = first + slot;
        if (slot < kSlots && b < runs) {
            const long long end = (b + 1) * kRun < s.waves ? (b + 1) * kRun : s.waves;
            double own = 0.0;
            for (long long w = b * kRun; w < end; ++w) own = __dadd_rn(own, s.partials[w * kWords + j]);
            run_sum[slot][j] = own;
        }
        __syncthreads();
        if (slot == 0) {
            const long long here = runs - first < kSlots ? runs - first : kSlots;
            for (int r = 0; r < here; ++r) sum = __dadd_rn(sum, run_sum[r][j]);
        }
        __syncthreads();
    }
    if (slot == 0) total[j] = sum;
    __syncthreads();
    if (tid == 0) solve_and_update(total, s, A, L, d, z);
}

}  // namespace

extern "C" {

size_t tn_mesh_register_workspace_bytes(int64_t num_points) {
    if (num_points < 0) return 0;
    return (size_t)kControl + (size_t)ceil_div(num_points, kPoints) * kWords * sizeof(double);
}

int tn_mesh_register(const float *positions, const float *temperature, const int32_t *triangles, int64_t num_vertices, int64_t num_triangles,
                     const void *bvh, size_t bvh_bytes, const float *points, int64_t num_points, const tn_register_params *params,
                     double *transform, double *history, int64_t *result, void *workspace, size_t workspace_bytes, void *stream) {
    if (!params || !bvh || !transform || !history || !result || !workspace) return TN_ERR_NULL;
    if (bad_counts(num_vertices, num_triangles) || num_points < 0 || 3 * num_points > 0x7fffffffLL) return TN_ERR_SHAPE;
    const tn_register_params &P = *params;
    const auto number = [](double x) { return x - x == 0.0; };  // finite (a NaN and an infinity fail)
    if (!(P.max_distance >= 0.0) || !number(P.center[0]) || !number(P.center[1]) || !number(P.center[2]) || !(P.length > 0.0) ||
        !number(P.length) || !(P.damping >= 0.0) || !number(P.damping) || !(P.tolerance >= 0.0) || P.iterations < 1 ||
        P.iterations > kMaxIterations || (P.metric != TN_REGISTER_POINT && P.metric != TN_REGISTER_PLANE) ||
        (P.with_scale != 0 && P.with_scale != 1) || P.min_pairs < 0)
        return TN_ERR_UNSUPPORTED;
    const bool work = num_vertices > 0 && num_triangles > 0;
    if (work && (!positions || !temperature || !triangles)) return TN_ERR_NULL;
    if (num_points > 0 && !points) return TN_ERR_NULL;
    if (misaligned(positions, 4) || misaligned(temperature, 4) || misaligned(triangles, 4) || misaligned(points, 4) || misaligned(transform, 8) ||
        misaligned(history, 8) || misaligned(result, 8) || misaligned(workspace, 8) || misaligned(bvh, 64))
        return TN_ERR_SHAPE;
    if (bvh_bytes < tn_mesh_bvh_bytes(num_triangles) || workspace_bytes < tn_mesh_register_workspace_bytes(num_points)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long long waves = ceil_div(num_points, kPoints);
    long long *control = reinterpret_cast<long long *>(workspace);
    double *partials = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + kControl);
    Walk a;
    a.positions = positions, a.triangles = triangles, a.num_vertices = (long long)num_vertices, a.num_triangles = (long long)num_triangles;
    a.bvh = reinterpret_cast<const char *>(bvh);
    a.points = points, a.num_points = (long long)num_points;
    a.r2 = P.max_distance * P.max_distance;  // one rounded product (nothing is contracted); +inf stays +inf
    a.metric = P.metric;
    a.transform = transform, a.control = control, a.partials = partials;
    Finish f;
    f.partials = partials, f.waves = waves, f.control = control, f.transform = transform, f.history = history;
    f.result = reinterpret_cast<long long *>(result);
    for (int k = 0; k < 3; ++k) a.center[k] = f.center[k] = P.center[k];
    f.length = P.length, f.damping = P.damping, f.tolerance = P.tolerance;
    f.iterations = P.iterations, f.with_scale = P.with_scale, f.min_pairs = P.min_pairs;
    if (hipMemsetAsync(control, 0, kControl, s) != hipSuccess) return TN_ERR_LAUNCH;
    for (int it = 0; it < P.iterations; ++it) {
        if (waves > 0) {
            hipLaunchKernelGGL(register_walk_kernel, dim3((unsigned)waves), dim3(kPoints), 0, s, a);
            TN_LAUNCH_CHECK();
        }
        f.iteration = it;
        hipLaunchKernelGGL(register_finish_kernel, dim3(1), dim3(kFinish), 0, s, f);
        TN_LAUNCH_CHECK();
    }
    return TN_OK;
}

}  // extern "C"
