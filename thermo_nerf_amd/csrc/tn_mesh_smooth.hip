// Vertex normals and Taubin smoothing of an indexed triangle list on a device incidence index (DESIGN.md "Mesh export": normals and
// smoothing; include/thermonerf_hip.h defines every output to the bit).  Both need, per vertex, the list of its incident triangle
// corners in a FIXED order: then a vertex's sum is one thread's loop over its own list — no float atomics, and the same bits on
// every run.  Corner c = 3 t + j is index j of triangle t.
//
// tn_mesh_incidence, on the caller's stream:
//   1. keys     one thread per corner: the vertex it names if its triangle is valid (all three indices in [0, V)), else V
//   2. sort     tn_sort_pairs (tn_sort.hip) of (key, 0 .. 3T-1) over max(1, bit_length(V)) key bits, stable: `corners` = the corner
//               numbers in ascending key, equal keys in ascending corner; the corners of invalid triangles come last
//   3. offsets  one thread per v = 0 .. V: offsets[v] = the number of keys < v, a binary search in the sorted keys — no atomics and
//               no serial fill over runs of unreferenced vertices
// tn_mesh_vertex_normals, one launch, one thread per vertex: the area-weighted sum of its corners' face vectors in list order,
// normalised.  tn_mesh_smooth, two launches per iteration (a pass with lambda, a pass with mu), one thread per vertex, Jacobi: a
// pass only reads src and only writes dst, in -> scratch -> out -> scratch -> out ..., so the result is in positions_out for every
// iteration count and positions_out may be positions_in.
// No allocation, no host synchronisation, every error code before any launch, and NO block ever waits for another block (no
// look-back, no grid barrier, no cooperative launch).  Every fp32 operation is one correctly rounded add_rn / sub_rn / mul_rn /
// div_rn / sqrt_rn of tn_device.h.
//
// A surface-nets vertex has 4 - 8 incident triangles: the lists are short and even, the lanes of a wave run alike.  A star of
// thousands of corners makes ONE lane run long and nothing else.  The per-vertex loops hold a handful of scalars (no array indexed
// at run time: corner j's two partners are picked by selects), so nothing lands in scratch.  A triangle's indices are one 12-byte
// load, a position three dwords of one row.  The two per-vertex kernels never dereference an index they have not checked: a list
// is clipped to [0, 3T], a corner outside it or of an invalid triangle is skipped — for the index tn_mesh_incidence built from the
// same triangles no check ever fires.
#include <cmath>

#include "tn_device.h"
#include "tn_mesh_lists.h"

using namespace tn;

namespace {

constexpr int kTile = 256;  // corners / vertices per block of every kernel here (tn_mesh_tile())

struct Vec {
    float x, y, z;
};

__device__ __forceinline__ Vec load_position(const float *__restrict__ positions, int v) {
    const float *p = positions + 3 * (long long)v;
    return {p[0], p[1], p[2]};
}

__device__ __forceinline__ void store_position(float *__restrict__ positions, long long v, const Vec &p) {
    float *d = positions + 3 * v;
    d[0] = p.x, d[1] = p.y, d[2] = p.z;
}

__global__ void __launch_bounds__(kTile)
keys_kernel(const int *__restrict__ tri, long long num_corners, int num_vertices, unsigned long long *__restrict__ keys) {
    const long long c = (long long)blockIdx.x * kTile + threadIdx.x;
    if (c >= num_corners) return;
    const long long t = c / 3;
    const Tri tr = load_triangle(tri, t);
    const int j = (int)(c - 3 * t);
    const int named = j == 0 ? tr.v[0] : (j == 1 ? tr.v[1] : tr.v[2]);
    keys[c] = (unsigned long long)(valid_triangle(tr, num_vertices) ? named : num_vertices);
}

// offsets[v] = the number of sorted keys < v (v = 0 .. V): the lower bound
__global__ void __launch_bounds__(kTile)
offsets_kernel(const unsigned long long *__restrict__ sorted_keys, long long num_corners, long long num_vertices,
               int *__restrict__ offsets) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    if (v > num_vertices) return;
    long long lo = 0, hi = num_corners;  // keys[lo - 1] < v <= keys[hi]
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (sorted_keys[mid] < (unsigned long long)v) lo = mid + 1; else hi = mid;
    }
    offsets[v] = (int)lo;  // <= 3T <= 2^31 - 1
}

__global__ void __launch_bounds__(kTile)
normals_kernel(const float *__restrict__ positions, const int *__restrict__ tri, long long num_corners, int num_vertices,
               const int *__restrict__ offsets, const int *__restrict__ corners, float *__restrict__ normals) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    if (v >= num_vertices) return;
    long long begin, end;
    list_of(offsets, v, num_corners, begin, end);
    Vec s = {0.0f, 0.0f, 0.0f};
    for (long long k = begin; k < end; ++k) {
        const int c = corners[k];
        if ((unsigned)c >= (unsigned long long)num_corners) continue;
        const Tri tr = load_triangle(tri, c / 3);
        if (!valid_triangle(tr, num_vertices)) continue;
        const Vec p0 = load_position(positions, tr.v[0]), p1 = load_position(positions, tr.v[1]), p2 = load_position(positions, tr.v[2]);
        const Vec e1 = {sub_rn(p1.x, p0.x), sub_rn(p1.y, p0.y), sub_rn(p1.z, p0.z)};
        const Vec e2 = {sub_rn(p2.x, p0.x), sub_rn(p2.y, p0.y), sub_rn(p2.z, p0.z)};
        s.x = add_rn(s.x, sub_rn(mul_rn(e1.y, e2.z), mul_rn(e1.z, e2.y)));
        s.y = add_rn(s.y, sub_rn(mul_rn(e1.z, e2.x), mul_rn(e1.x, e2.z)));
        s.z = add_rn(s.z, sub_rn(mul_rn(e1.x, e2.y), mul_rn(e1.y, e2.x)));
    }
    const float len = sqrt_rn(add_rn(add_rn(mul_rn(s.x, s.x), mul_rn(s.y, s.y)), mul_rn(s.z, s.z)));
    const bool unit = len > 0.0f && len < INFINITY;  // false for a NaN, too
    store_position(normals, v, unit ? Vec{div_rn(s.x, len), div_rn(s.y, len), div_rn(s.z, len)} : Vec{0.0f, 0.0f, 0.0f});
}

// one Jacobi pass with factor k: dst[v] = src[v] + k (mean of the corners' partner vertices - src[v])
__global__ void __launch_bounds__(kTile)
smooth_pass_kernel(const float *__restrict__ src, const int *__restrict__ tri, long long num_corners, int num_vertices,
                   const int *__restrict__ offsets, const int *__restrict__ corners, float k, float *__restrict__ dst) {
    const long long v = (long long)blockIdx.x * kTile + threadIdx.x;
    if (v >= num_vertices) return;
    long long begin, end;
    list_of(offsets, v, num_corners, begin, end);
    Vec s = {0.0f, 0.0f, 0.0f};
    unsigned n = 0;  // <= 2 * 3T < 2^32
    for (long long i = begin; i < end; ++i) {
        const int c = corners[i];
        if ((unsigned)c >= (unsigned long long)num_corners) continue;
        const int t = c / 3, j = c - 3 * t;
        const Tri tr = load_triangle(tri, t);
        if (!valid_triangle(tr, num_vertices)) continue;
        const int qi = j == 0 ? tr.v[1] : (j == 1 ? tr.v[2] : tr.v[0]);  // index (j + 1) % 3
        const int ri = j == 0 ? tr.v[2] : (j == 1 ? tr.v[0] : tr.v[1]);  // index (j + 2) % 3
        const Vec q = load_position(src, qi), r = load_position(src, ri);
        s.x = add_rn(add_rn(s.x, q.x), r.x);
        s.y = add_rn(add_rn(s.y, q.y), r.y);
        s.z = add_rn(add_rn(s.z, q.z), r.z);
        n += 2;
    }
    Vec p = load_position(src, (int)v);
    if (n != 0) {
        const float count = (float)n;
        p.x = add_rn(p.x, mul_rn(k, sub_rn(div_rn(s.x, count), p.x)));
        p.y = add_rn(p.y, mul_rn(k, sub_rn(div_rn(s.y, count), p.y)));
        p.z = add_rn(p.z, mul_rn(k, sub_rn(div_rn(s.z, count), p.z)));
    }
    store_position(dst, v, p);
}

inline long long tiles_of(long long items) { return ceil_div(items, kTile); }

inline size_t keys_bytes(long long n) { return (size_t)n * sizeof(unsigned long long); }

inline bool bad_count(int64_t n) { return n < 0 || n > 0x7fffffffLL; }

inline bool bad_mesh(int64_t num_vertices, int64_t num_triangles) {
    return bad_count(num_vertices) || num_triangles < 0 || num_triangles > 0x7fffffffLL / 3;  // 3T <= 2^31 - 1
}

inline int bit_length(unsigned long long x) {
    int bits = 0;
    for (; x; x >>= 1) ++bits;
    return bits;
}

}  // namespace

extern "C" {

// the keys, the sorted keys, the sort's own workspace
size_t tn_mesh_incidence_workspace_bytes(int64_t num_vertices, int64_t num_triangles) {
    if (bad_mesh(num_vertices, num_triangles)) return 0;
    return 2 * keys_bytes(3 * num_triangles) + tn_sort_pairs_workspace_bytes(3 * num_triangles);
}

int tn_mesh_incidence(const int32_t *triangles, int64_t num_triangles, int64_t num_vertices, int32_t *offsets, int32_t *corners,
                      void *workspace, size_t workspace_bytes, void *stream) {
    if (!offsets) return TN_ERR_NULL;
    if (bad_mesh(num_vertices, num_triangles)) return TN_ERR_SHAPE;
    if (misaligned(triangles, 4) || misaligned(offsets, 4) || misaligned(corners, 4) || misaligned(workspace, 8)) return TN_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    if (num_vertices == 0 || num_triangles == 0)
        return hipMemsetAsync(offsets, 0, (size_t)(num_vertices + 1) * sizeof(int32_t), s) == hipSuccess ? TN_OK : TN_ERR_LAUNCH;
    if (!triangles || !corners || !workspace) return TN_ERR_NULL;
    if (workspace_bytes < tn_mesh_incidence_workspace_bytes(num_vertices, num_triangles)) return TN_ERR_WORKSPACE;
    const int nv = (int)num_vertices;
    const long long n = 3 * (long long)num_triangles;
    char *ws = reinterpret_cast<char *>(workspace);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws);
    unsigned long long *sorted_keys = reinterpret_cast<unsigned long long *>(ws + keys_bytes(n));
    void *sort_ws = ws + 2 * keys_bytes(n);
    hipLaunchKernelGGL(keys_kernel, dim3((unsigned)tiles_of(n)), dim3(kTile), 0, s, triangles, n, nv, keys);
    TN_LAUNCH_CHECK();
    const int bits = bit_length((unsigned long long)nv);  // >= 1: nv > 0
    const int code = tn_sort_pairs(reinterpret_cast<const uint64_t *>(keys), nullptr, n, bits, reinterpret_cast<uint64_t *>(sorted_keys),
                                   corners, sort_ws, tn_sort_pairs_workspace_bytes(n), stream);
    if (code != TN_OK) return code;
    hipLaunchKernelGGL(offsets_kernel, dim3((unsigned)tiles_of((long long)nv + 1)), dim3(kTile), 0, s, sorted_keys, n, (long long)nv,
                       offsets);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

int tn_mesh_vertex_normals(const float *positions, const int32_t *triangles, int64_t num_triangles, int64_t num_vertices,
                           const int32_t *offsets, const int32_t *corners, float *normals, void *stream) {
    const int code = check_indexed_mesh(positions, triangles, num_triangles, num_vertices, offsets, corners, normals);
    if (code != TN_OK) return code;
    if (num_vertices == 0) return TN_OK;
    hipLaunchKernelGGL(normals_kernel, dim3((unsigned)tiles_of(num_vertices)), dim3(kTile), 0, (hipStream_t)stream, positions, triangles,
                       3 * (long long)num_triangles, (int)num_vertices, offsets, corners, normals);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

int tn_mesh_smooth(const float *positions_in, const int32_t *triangles, int64_t num_triangles, int64_t num_vertices,
                   const int32_t *offsets, const int32_t *corners, int32_t iterations, float lambda, float mu, float *positions_out,
                   float *scratch, void *stream) {
    const int code = check_indexed_mesh(positions_in, triangles, num_triangles, num_vertices, offsets, corners, positions_out);
    if (code != TN_OK) return code;
    if (num_vertices > 0 && iterations > 0 && !scratch) return TN_ERR_NULL;
    if (iterations < 0 || misaligned(scratch, 4)) return TN_ERR_SHAPE;
    if (!std::isfinite(lambda) || !std::isfinite(mu)) return TN_ERR_UNSUPPORTED;
    const size_t bytes = (size_t)num_vertices * 3 * sizeof(float);
    if (positions_out != positions_in && overlap(positions_in, positions_out, bytes)) return TN_ERR_SHAPE;
    if (iterations > 0 && (overlap(scratch, positions_in, bytes) || overlap(scratch, positions_out, bytes))) return TN_ERR_SHAPE;
    if (num_vertices == 0) return TN_OK;
    hipStream_t s = (hipStream_t)stream;
    if (iterations == 0) {
        if (positions_out == positions_in) return TN_OK;
        return hipMemcpyAsync(positions_out, positions_in, bytes, hipMemcpyDeviceToDevice, s) == hipSuccess ? TN_OK : TN_ERR_LAUNCH;
    }
    const unsigned blocks = (unsigned)tiles_of(num_vertices);
    const long long n = 3 * (long long)num_triangles;
    const float *src = positions_in;
    for (int pass = 0; pass < 2 * iterations; ++pass) {  // an even number of passes: the last one writes positions_out
        float *dst = pass % 2 == 0 ? scratch : positions_out;
        hipLaunchKernelGGL(smooth_pass_kernel, dim3(blocks), dim3(kTile), 0, s, src, triangles, n, (int)num_vertices, offsets, corners,
                           pass % 2 == 0 ? lambda : mu, dst);
        TN_LAUNCH_CHECK();
        src = dst;
    }
    return TN_OK;
}

}  // extern "C"
