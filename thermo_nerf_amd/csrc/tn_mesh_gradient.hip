// The surface gradient of a per-vertex scalar (degrees Celsius per world unit: where the temperature changes fastest) and the
// NaN-aware Jacobi filter of such a scalar, on tn_mesh_incidence's corner lists (DESIGN.md "Mesh export": gradient and scalar
// smoothing; include/thermonerf_hip.h defines every output to the bit).
//
// tn_mesh_scalar_smooth, one launch per pass, one thread per vertex: the mean of the FINITE values at the partners of the vertex's
// corners, in list order in fp64; a finite vertex moves towards it by the pass's factor, a vertex without a value takes it when
// `fill` is set — a hole closes by one ring per pass.  Jacobi: a pass only reads src and only writes dst, in -> scratch -> out ->
// scratch ..., and an odd number of passes ends with a device copy scratch -> out.
// tn_mesh_scalar_gradient, on the caller's stream:
//   1. faces    one thread per face: load_face (tn_group_sum.h: the one definition of placed, finite, the edges, the cross product and
//               n2), the gradient of the linear interpolant, the row of face_gradient, the face's record (w, w |g|, |g|, 1)
//   2. vertices one thread per vertex: the usable faces among its corners in list order, S += w g, W += w, then G = S / W and |G|.
//               The gradient of a corner's face is RECOMPUTED from the positions and the values: reading the rows of step 1 back
//               gives the same bits and took twice as long (profiles/micro/mesh_gradient.txt has both times)
//   3. totals   one thread per 256 faces joins their records in face order (join_run of tn_group_sum.h, the walk of every ordered sum
//               of the mesh layer), then one thread joins the partials in block order, out of LDS, where its block stages them
// No allocation, no host synchronisation, no float atomics, every error code before any launch, and no block ever waits for another.
// The kernels check what they dereference: a list is clipped to [0, 3T], a corner outside it is skipped, load_face reads a vertex only
// where the face's indices allow it — a foreign index gives other numbers, never an access outside the arrays.
#include <cmath>

#include "tn_device.h"
#include "tn_group_sum.h"
#include "tn_mesh_lists.h"

using namespace tn;

namespace {

constexpr int kTile = 256;  // faces / vertices / 256-blocks per thread block of every kernel here

__device__ __forceinline__ double quiet_nan64() { return __longlong_as_double(0x7ff8000000000000LL); }

// add(add(mul(x, x), mul(y, y)), mul(z, z)), then the root: |g| of a face, |G| of a vertex
__device__ __forceinline__ double length_of(const double g[3]) {
    return __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(g[0], g[0]), __dmul_rn(g[1], g[1])), __dmul_rn(g[2], g[2])));
}

// the gradient of the linear interpolant of f's three values over f, and its weight w = sqrt(n2), twice the area; false: not USABLE
__device__ __forceinline__ bool face_gradient_of(const Face &f, double g[3], double &w) {
    if (!(f.placed && f.warm && f.n2 > 0.0 && f.n2 < (double)INFINITY)) return false;
    const double a = __dsub_rn((double)f.c[1], (double)f.c[0]), b = __dsub_rn((double)f.c[2], (double)f.c[0]);
    const double *e1 = f.e1, *e2 = f.e2, *n = f.cr;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int y = (c + 1) % 3, z = (c + 2) % 3;  // the cross products' component order: (yz - zy, zx - xz, xy - yx)
        const double A = __dsub_rn(__dmul_rn(e2[y], n[z]), __dmul_rn(e2[z], n[y]));  // e2 x n
        const double B = __dsub_rn(__dmul_rn(n[y], e1[z]), __dmul_rn(n[z], e1[y]));  // n x e1
        g[c] = __ddiv_rn(__dadd_rn(__dmul_rn(a, A), __dmul_rn(b, B)), f.n2);
    }
    w = f.len;
    return true;
}

// a face's record, a 256-block's partial and the mesh's accumulator: two ordered sums, the order-free maximum and count
struct alignas(16) Sum {
    double s[2];    // w, w |g|
    double steepest;  // max |g|; |g| >= +0.0 and never a NaN for a usable face
    long long faces;  // the usable faces
    static constexpr int kAhead = 8;  // 8 registers a record: the walks are few threads, round trips are what they pay
    static __device__ __forceinline__ Sum empty() { return Sum{{0.0, 0.0}, 0.0, 0}; }
    __device__ __forceinline__ void join(const Sum &r) {
        s[0] = __dadd_rn(s[0], r.s[0]);
        s[1] = __dadd_rn(s[1], r.s[1]);
        steepest = r.steepest > steepest ? r.steepest : steepest;
        faces += r.faces;
    }
};
static_assert(sizeof(Sum) == 32, "two 16-byte loads");

__global__ void __launch_bounds__(kTile)
gradient_faces_kernel(const float *__restrict__ positions, const float *__restrict__ values, const int *__restrict__ triangles,
                      long long num_vertices, long long num_triangles, double *__restrict__ face_gradient, Sum *__restrict__ records) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    if (t >= num_triangles) return;
    const Face f = load_face(positions, values, triangles, num_vertices, t);
    double g[3] = {quiet_nan64(), quiet_nan64(), quiet_nan64()}, w = 0.0;
    Sum r = Sum::empty();
    if (face_gradient_of(f, g, w)) {
        const double steep = length_of(g);
        r.s[0] = w, r.s[1] = __dmul_rn(w, steep), r.steepest = steep, r.faces = 1;
    }
    records[t] = r;
    if (!face_gradient) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) face_gradient[3 * t + c] = g[c];
}

__global__ void __launch_bounds__(kTile)
gradient_vertices_kernel(const float *__restrict__ positions, const float *__restrict__ values, const int *__restrict__ triangles,
                         long long num_triangles, long long num_vertices, const int *__restrict__ offsets,
                         const int *__restrict__ corners, float *__restrict__ vertex_gradient, float *__restrict__ vertex_magnitude) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    if (v >= num_vertices) return;
    const long long num_corners = 3 * num_triangles;
    long long begin, end;
    list_of(offsets, v, num_corners, begin, end);
    double S[3] = {0.0, 0.0, 0.0}, W = 0.0;
    bool any = false;
    for (long long k = begin; k < end; ++k) {
        const long long c = corners[k];
        if (c < 0 || c >= num_corners) continue;
        double g[3], w;
        if (!face_gradient_of(load_face(positions, values, triangles, num_vertices, c / 3), g, w)) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) S[a] = __dadd_rn(S[a], __dmul_rn(w, g[a]));
        W = __dadd_rn(W, w);
        any = true;
    }
    float out[3] = {quiet_nan(), quiet_nan(), quiet_nan()}, magnitude = quiet_nan();
    if (any) {
        double G[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) G[a] = __ddiv_rn(S[a], W), out[a] = (float)G[a];
        magnitude = (float)length_of(G);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) vertex_gradient[3 * v + a] = out[a];
    vertex_magnitude[v] = magnitude;
}

// ONE THREAD PER 256 FACES joins their records in face order into one partial
__global__ void __launch_bounds__(kTile)
gradient_block_sums_kernel(const Sum *__restrict__ records, long long num_triangles, long long num_blocks, Sum *__restrict__ partials) {
    const long long b = (long long)blockIdx.x * kTile + threadIdx.x;
    if (b >= num_blocks) return;
    const long long first = b * kSumBlock, end = first + kSumBlock < num_triangles ? first + kSumBlock : num_triangles;
    partials[b] = join_run<Sum>(first, end, [&](long long t) -> const Sum * { return records + t; });
}

// ONE THREAD joins the partials in block order.  Alone it would pay a trip to memory for every few partials (8192 of them at 2 M
// faces: 0.82 ms measured); so its block brings them into LDS kStage at a time, coalesced, and the one thread joins them from there,
// record after record as join_run would
constexpr int kStage = 1024;

__global__ void __launch_bounds__(kTile)
gradient_totals_kernel(const Sum *__restrict__ partials, long long num_blocks, double *__restrict__ totals) {
    __shared__ Sum stage[kStage];
    Sum a = Sum::empty();
    for (long long first = 0; first < num_blocks; first += kStage) {  // (uniform over the block: the barriers are met by all)
        const long long n = num_blocks - first < kStage ? num_blocks - first : kStage;
        for (long long k = threadIdx.x; k < n; k += kTile) stage[k] = partials[first + k];
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll 8
            for (int k = 0; k < (int)n; ++k) a.join(stage[k]);  // LDS reads that depend on no sum: they run ahead of the additions
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    totals[0] = (double)a.faces;
    totals[1] = a.s[0];
    totals[2] = a.s[1];
    totals[3] = a.steepest;
}

// one Jacobi pass with factor k over the finite values: dst[v] = src[v] + k (mean of the finite partners - src[v]), or the mean
// itself for a vertex without a value when `fill` is set
__global__ void __launch_bounds__(kTile)
scalar_pass_kernel(const float *__restrict__ src, const int *__restrict__ tri, long long num_corners, int num_vertices,
                   const int *__restrict__ offsets, const int *__restrict__ corners, float k, bool fill, float *__restrict__ dst) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    if (v >= num_vertices) return;
    long long begin, end;
    list_of(offsets, v, num_corners, begin, end);
    double s = 0.0;
    unsigned n = 0;  // <= 2 * 3T < 2^32
    for (long long i = begin; i < end; ++i) {
        const long long c = corners[i];
        if (c < 0 || c >= num_corners) continue;
        const long long t = c / 3;
        const int j = (int)(c - 3 * t);
        const Tri tr = load_triangle(tri, t);
        if (!valid_triangle(tr, num_vertices)) continue;
        const float q = src[j == 0 ? tr.v[1] : (j == 1 ? tr.v[2] : tr.v[0])];  // index (j + 1) % 3
        const float r = src[j == 0 ? tr.v[2] : (j == 1 ? tr.v[0] : tr.v[1])];  // index (j + 2) % 3
        if (finite(q)) s = __dadd_rn(s, (double)q), ++n;
        if (finite(r)) s = __dadd_rn(s, (double)r), ++n;
    }
    const float p = src[v];
    float out = p;  // the same bits: no partner with a value, or a hole that is not to be filled
    if (n != 0) {
        const double m = __ddiv_rn(s, (double)n);
        if (finite(p)) out = (float)__dadd_rn((double)p, __dmul_rn((double)k, __dsub_rn(m, (double)p)));
        else if (fill) out = (float)m;
    }
    dst[v] = out;
}

inline long long tiles_of(long long items) { return ceil_div(items, kTile); }

// the workspace, in order: up to 8 bytes of slack (the records are 16-byte aligned), the face records, the 256-blocks' partials
struct Layout {
    Sum *records, *partials;
    long long blocks;
    size_t bytes;
};

inline Layout layout_of(char *ws, long long t) {
    Layout l;
    l.blocks = ceil_div(t, kSumBlock);
    char *at = ws ? ws + reinterpret_cast<uintptr_t>(ws) % 16 : nullptr;  // ws is 8-byte aligned: 0 or 8
    const size_t records = (size_t)t * sizeof(Sum), partials = (size_t)l.blocks * sizeof(Sum);
    l.records = reinterpret_cast<Sum *>(at);
    l.partials = reinterpret_cast<Sum *>(at ? at + records : nullptr);
    l.bytes = 16 + records + partials;
    return l;
}

}  // namespace

extern "C" {

int tn_mesh_scalar_smooth(const float *values_in, const int32_t *triangles, int64_t num_triangles, int64_t num_vertices,
                          const int32_t *offsets, const int32_t *corners, int32_t iterations, float lambda, float mu, int32_t fill,
                          float *values_out, float *scratch, void *stream) {
    const int code = check_indexed_mesh(values_in, triangles, num_triangles, num_vertices, offsets, corners, values_out);
    if (code != TN_OK) return code;
    if (num_vertices > 0 && iterations > 0 && !scratch) return TN_ERR_NULL;
    if (iterations < 0 || iterations > 0x3fffffff || misaligned(scratch, 4)) return TN_ERR_SHAPE;
    if (!std::isfinite(lambda) || !std::isfinite(mu)) return TN_ERR_UNSUPPORTED;
    const size_t bytes = (size_t)num_vertices * sizeof(float);
    if (values_out != values_in && overlap(values_in, values_out, bytes)) return TN_ERR_SHAPE;
    if (iterations > 0 && (overlap(scratch, values_in, bytes) || overlap(scratch, values_out, bytes))) return TN_ERR_SHAPE;
    if (num_vertices == 0) return TN_OK;
    hipStream_t s = (hipStream_t)stream;
    if (iterations == 0) {
        if (values_out == values_in) return TN_OK;
        return hipMemcpyAsync(values_out, values_in, bytes, hipMemcpyDeviceToDevice, s) == hipSuccess ? TN_OK : TN_ERR_LAUNCH;
    }
    const bool pairs = mu != 0.0f;  // mu == 0: an iteration is its lambda pass alone
    const int passes = pairs ? 2 * iterations : iterations;
    const unsigned blocks = (unsigned)tiles_of(num_vertices);
    const long long n = 3 * (long long)num_triangles;
    const float *src = values_in;
    for (int pass = 0; pass < passes; ++pass) {
        float *dst = pass % 2 == 0 ? scratch : values_out;
        hipLaunchKernelGGL(scalar_pass_kernel, dim3(blocks), dim3(kTile), 0, s, src, triangles, n, (int)num_vertices, offsets, corners,
                           pairs && pass % 2 == 1 ? mu : lambda, fill != 0, dst);
        TN_LAUNCH_CHECK();
        src = dst;
    }
    if (passes % 2 == 1)  // the last pass wrote scratch
        return hipMemcpyAsync(values_out, scratch, bytes, hipMemcpyDeviceToDevice, s) == hipSuccess ? TN_OK : TN_ERR_LAUNCH;
    return TN_OK;
}

size_t tn_mesh_scalar_gradient_workspace_bytes(int64_t num_vertices, int64_t num_triangles) {
    if (bad_counts(num_vertices, num_triangles)) return 0;
    return layout_of(nullptr, (long long)num_triangles).bytes;
}

int tn_mesh_scalar_gradient(const float *positions, const float *values, const int32_t *triangles, int64_t num_triangles,
                            int64_t num_vertices, const int32_t *offsets, const int32_t *corners, double *face_gradient,
                            float *vertex_gradient, float *vertex_magnitude, double *totals, void *workspace, size_t workspace_bytes,
                            void *stream) {
    if (!totals) return TN_ERR_NULL;
    if (num_vertices > 0 && (!positions || !values || !offsets || !vertex_gradient || !vertex_magnitude)) return TN_ERR_NULL;
    if (num_triangles > 0 && (!triangles || !workspace)) return TN_ERR_NULL;
    if (num_vertices > 0 && num_triangles > 0 && !corners) return TN_ERR_NULL;
    if (bad_counts(num_vertices, num_triangles)) return TN_ERR_SHAPE;
    if (misaligned(positions, 4) || misaligned(values, 4) || misaligned(triangles, 4) || misaligned(offsets, 4) || misaligned(corners, 4) ||
        misaligned(vertex_gradient, 4) || misaligned(vertex_magnitude, 4) || misaligned(face_gradient, 8) || misaligned(totals, 8) ||
        misaligned(workspace, 8))
        return TN_ERR_SHAPE;
    if (num_triangles > 0 && workspace_bytes < tn_mesh_scalar_gradient_workspace_bytes(num_vertices, num_triangles)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long long nv = (long long)num_vertices, nt = (long long)num_triangles;
    const Layout l = layout_of(nt > 0 ? reinterpret_cast<char *>(workspace) : nullptr, nt);
    if (nt > 0) {
        hipLaunchKernelGGL(gradient_faces_kernel, dim3((unsigned)tiles_of(nt)), dim3(kTile), 0, s, positions, values, triangles, nv, nt,
                           face_gradient, l.records);
        TN_LAUNCH_CHECK();
    }
    if (nv > 0) {
        hipLaunchKernelGGL(gradient_vertices_kernel, dim3((unsigned)tiles_of(nv)), dim3(kTile), 0, s, positions, values, triangles, nt, nv,
                           offsets, corners, vertex_gradient, vertex_magnitude);
        TN_LAUNCH_CHECK();
    }
    if (nt == 0) return hipMemsetAsync(totals, 0, 4 * sizeof(double), s) == hipSuccess ? TN_OK : TN_ERR_LAUNCH;
    hipLaunchKernelGGL(gradient_block_sums_kernel, dim3((unsigned)tiles_of(l.blocks)), dim3(kTile), 0, s, l.records, nt, l.blocks,
                       l.partials);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(gradient_totals_kernel, dim3(1), dim3(kTile), 0, s, l.partials, l.blocks, totals);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

}  // extern "C"
