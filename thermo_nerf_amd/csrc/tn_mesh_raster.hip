// Orthographic thermogram of an indexed triangle list (DESIGN.md "Thermograms"; include/thermonerf_hip.h defines every output to the
// bit): a z-buffered rasteriser on a uint64 key plane, key = ord(depth) << 32 | face, the pixel shows the smallest key.  Launches on
// the caller's stream:
//   1. clear        the key plane <- all ones (a memset)
//   2. faces        one thread per face: the three vertices into fixed point, USABLE / DRAWN, the face record, the box of pixel
//                   centres clipped to the image; a face with a SMALL box is rasterised here, by its thread (a TSDF mesh at any
//                   sensible pixel size: every face); the tile counts of the usable, the drawn and the large faces
//   3. scan         one block: the three exclusive scans -> counts[2], counts[1], the number of large faces
//   4. large list   the faces with a larger box compacted in face order
//   5. sweep        kSweepShare blocks of 256 threads per large face walk its box in 16 x 16 pixel tiles, a tile skipped whole when
//                   one edge function is negative at its four corners (a simplified mesh: one face may span thousands of pixels)
//   6. resolve      one thread per pixel: the key's face, the barycentrics again from its record, the four arrays; per 256 pixels
//                   one partial: the block's ordered sum (one thread walks it), extremes and covered count
//   7. finish       one block: the partials in order (SUM2's second level), the extremes, the covered count
// No allocation, no host synchronisation, no float atomics, and no block ever waits for another.  The only atomic is the 64-bit
// integer minimum on the key plane, and a minimum does not depend on the order in which it is taken: the small / large threshold,
// the grid sizes and the schedule cannot change a bit of the output.
#include "tn_device.h"
#include "tn_scan.h"

using namespace tn;

namespace {

constexpr int kTile = 256;        // faces / pixels per thread block
constexpr int kBlock = 256;       // entries per block of SUM2 (== kTile: a resolve block is a SUM2 block)
constexpr int kSmallBox = 8;      // a box of at most this many pixels on both sides is rasterised by the face's own thread
constexpr int kSweep = 16;        // the side of a sweep tile: kSweep x kSweep == kTile
constexpr int kSweepShare = 8;    // blocks that share the tiles of one large face
constexpr int kFinishChunk = 1024;
constexpr int kMaxSide = 16384;
constexpr unsigned long long kEmpty = ~0ull;  // (ord of a depth is never 0xffffffff: that is a NaN's pattern)
static_assert(kSweep * kSweep == kTile && kBlock == kTile, "one thread per pixel of a tile; one resolve block per SUM2 block");

struct View {  // tn_raster_view by value
    double origin[3], right[3], down[3], forward[3];
    double pixel_size, near, far;
    int width, height, cull, small_box;
};

// a drawn face after the exchange: area2 > 0 (0: not drawn)
struct alignas(8) Face {
    double z[3];
    long long area2;
    int x[3], y[3];  // |X|, |Y| <= 2^29
    int v[3];
    int pad;
};
static_assert(sizeof(Face) == 72, "nine 8-byte loads");

struct alignas(8) Partial {  // of 256 pixels
    double sum;
    unsigned kmin, kmax;  // f2key of the extremes; ~0 and 0 without a covered pixel
    int covered, pad;
};

using tn::finite;  // (float), beside the double of this file
__device__ __forceinline__ bool finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

__device__ __forceinline__ double along(const double *q, const double *a) {
    return __dadd_rn(__dadd_rn(__dmul_rn(q[0], a[0]), __dmul_rn(q[1], a[1])), __dmul_rn(q[2], a[2]));
}

// vertex p into fixed point; false: not rasterable
__device__ __forceinline__ bool transform(const float *p, const View &view, long long &X, long long &Y, double &z) {
    double q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = __dsub_rn((double)p[k], view.origin[k]);
    const double x = __ddiv_rn(along(q, view.right), view.pixel_size), y = __ddiv_rn(along(q, view.down), view.pixel_size);
    z = along(q, view.forward);
    const double fx = __dmul_rn(x, 256.0), fy = __dmul_rn(y, 256.0);
    const bool ok = finite(x) && finite(y) && finite(z) && fabs(fx) <= 536870912.0 && fabs(fy) <= 536870912.0;
    X = ok ? (long long)rint(fx) : 0;
    Y = ok ? (long long)rint(fy) : 0;
    return ok;
}

__device__ __forceinline__ long long edge(long long ax, long long ay, long long bx, long long by, long long px, long long py) {
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}
__device__ __forceinline__ bool top_left(long long ax, long long ay, long long bx, long long by) {
    return by - ay < 0 || (by - ay == 0 && bx - ax > 0);
}

// is pixel (row j, col i) covered by f; its barycentrics
__device__ __forceinline__ bool cover(const Face &f, long long i, long long j, double *l) {
    const long long px = 256 * i + 128, py = 256 * j + 128;
    const long long w0 = edge(f.x[1], f.y[1], f.x[2], f.y[2], px, py), w1 = edge(f.x[2], f.y[2], f.x[0], f.y[0], px, py),
                    w2 = edge(f.x[0], f.y[0], f.x[1], f.y[1], px, py);
    const bool in = (w0 > 0 || (w0 == 0 && top_left(f.x[1], f.y[1], f.x[2], f.y[2]))) &&
                    (w1 > 0 || (w1 == 0 && top_left(f.x[2], f.y[2], f.x[0], f.y[0]))) &&
                    (w2 > 0 || (w2 == 0 && top_left(f.x[0], f.y[0], f.x[1], f.y[1])));
    if (!in) return false;
    const double a = (double)f.area2;
    l[0] = __ddiv_rn((double)w0, a);
    l[1] = __ddiv_rn((double)w1, a);
    l[2] = __ddiv_rn((double)w2, a);
    return true;
}

__device__ __forceinline__ double blend(const double *l, double a0, double a1, double a2) {
    return __dadd_rn(__dadd_rn(__dmul_rn(l[0], a0), __dmul_rn(l[1], a1)), __dmul_rn(l[2], a2));
}

__device__ __forceinline__ float depth_of(double zp) {
    const float d = (float)zp;
    return d == 0.0f ? 0.0f : d;  // -0.0 -> +0.0
}

// the sample of face t at pixel (j, i), if there is one, joins the key plane
__device__ __forceinline__ void sample(const Face &f, long long t, long long i, long long j, const View &view,
                                       unsigned long long *__restrict__ keys) {
    double l[3];
    if (!cover(f, i, j, l)) return;
    const double zp = blend(l, f.z[0], f.z[1], f.z[2]);
    if (!(view.near <= zp && zp <= view.far)) return;
    const unsigned long long key = (unsigned long long)f2key(depth_of(zp)) << 32 | (unsigned long long)t;
    unsigned long long *slot = keys + (size_t)j * (size_t)view.width + (size_t)i;
    if (key < *slot) atomicMin(slot, key);  // a stale load is an older, larger key: the skip is safe
}

// the pixels whose centres lie in the face's box, clipped to the image; false: none
__device__ __forceinline__ bool box_of(const Face &f, const View &view, int &i0, int &i1, int &j0, int &j1) {
    const long long xl = min(min(f.x[0], f.x[1]), f.x[2]), xh = max(max(f.x[0], f.x[1]), f.x[2]);
    const long long yl = min(min(f.y[0], f.y[1]), f.y[2]), yh = max(max(f.y[0], f.y[1]), f.y[2]);
    // 256 i + 128 >= xl  <=>  i >= ceil((xl - 128) / 256);  256 i + 128 <= xh  <=>  i <= floor((xh - 128) / 256)
    const long long a0 = max((xl + 127) >> 8, 0LL), a1 = min((xh - 128) >> 8, (long long)view.width - 1);
    const long long b0 = max((yl + 127) >> 8, 0LL), b1 = min((yh - 128) >> 8, (long long)view.height - 1);
    i0 = (int)a0, i1 = (int)a1, j0 = (int)b0, j1 = (int)b1;
    return a0 <= a1 && b0 <= b1;
}

constexpr int kUsable = 1, kDrawn = 2, kLarge = 4;

__global__ void __launch_bounds__(kTile)
raster_faces_kernel(const float *__restrict__ positions, const float *__restrict__ temperature, const int *__restrict__ triangles,
                    long long num_vertices, long long num_triangles, View view, Face *__restrict__ records, int *__restrict__ flags,
                    unsigned long long *__restrict__ keys, long long *__restrict__ usable_tiles, long long *__restrict__ drawn_tiles,
                    long long *__restrict__ large_tiles) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    int flag = 0;
    if (t < num_triangles) {
        const long long i[3] = {triangles[3 * t], triangles[3 * t + 1], triangles[3 * t + 2]};
        bool ok = i[0] >= 0 && i[0] < num_vertices && i[1] >= 0 && i[1] < num_vertices && i[2] >= 0 && i[2] < num_vertices;
        ok = ok && i[0] != i[1] && i[1] != i[2] && i[0] != i[2];
        long long X[3] = {0, 0, 0}, Y[3] = {0, 0, 0};
        double z[3] = {0.0, 0.0, 0.0};
        if (ok) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                ok = ok && finite(temperature[i[a]]);
                const float p[3] = {positions[3 * i[a]], positions[3 * i[a] + 1], positions[3 * i[a] + 2]};
                ok = transform(p, view, X[a], Y[a], z[a]) && ok;
            }
        }
        Face f;
        f.area2 = 0;
        f.pad = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) f.x[a] = f.y[a] = 0, f.v[a] = -1, f.z[a] = 0.0;
        if (ok) {
            flag = kUsable;
            const long long area2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]);
            if (area2 != 0 && !(view.cull == 1 && area2 > 0)) {
                flag |= kDrawn;
                const int b = area2 < 0 ? 2 : 1, c = area2 < 0 ? 1 : 2;  // the exchange
                const int order[3] = {0, b, c};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    f.x[a] = (int)X[order[a]], f.y[a] = (int)Y[order[a]], f.z[a] = z[order[a]], f.v[a] = (int)i[order[a]];
                }
                f.area2 = area2 < 0 ? -area2 : area2;
                int i0, i1, j0, j1;
                if (box_of(f, view, i0, i1, j0, j1)) {
                    if (i1 - i0 < view.small_box && j1 - j0 < view.small_box) {
                        for (int j = j0; j <= j1; ++j)
                            for (int k = i0; k <= i1; ++k) sample(f, t, k, j, view, keys);
                    } else {
                        flag |= kLarge;
                    }
                }
            }
        }
        records[t] = f;
        flags[t] = flag;
    }
    uint32_t total;
    block_rank<kTile>((flag & kUsable) != 0, total);
    if (threadIdx.x == 0) usable_tiles[blockIdx.x] = (long long)total;
    __syncthreads();  // block_rank's LDS is rewritten by the next call
    block_rank<kTile>((flag & kDrawn) != 0, total);
    if (threadIdx.x == 0) drawn_tiles[blockIdx.x] = (long long)total;
    __syncthreads();
    block_rank<kTile>((flag & kLarge) != 0, total);
    if (threadIdx.x == 0) large_tiles[blockIdx.x] = (long long)total;
}

__global__ void __launch_bounds__(kScan)
raster_scan_kernel(long long *__restrict__ usable_tiles, long long *__restrict__ drawn_tiles, long long *__restrict__ large_tiles,
                   long long num_tiles, long long *__restrict__ counts, long long *__restrict__ num_large) {
    scan_tiles<false>(usable_tiles, num_tiles, counts + 2);
    __syncthreads();
    scan_tiles<false>(drawn_tiles, num_tiles, counts + 1);
    __syncthreads();
    scan_tiles<false>(large_tiles, num_tiles, num_large);
}

__global__ void __launch_bounds__(kTile)
raster_large_list_kernel(const int *__restrict__ flags, long long num_triangles, const long long *__restrict__ large_tiles,
                         int *__restrict__ large_list) {
    const long long t = (long long)blockIdx.x * kTile + threadIdx.x;
    const bool large = t < num_triangles && (flags[t] & kLarge) != 0;
    uint32_t unused;
    const uint32_t before = block_rank<kTile>(large, unused);
    if (!large) return;
    const long long o = large_tiles[blockIdx.x] + (long long)before;  // <= t
    if (o >= 0 && o < num_triangles) large_list[o] = (int)t;
}

// blockIdx.x strides over the large faces, blockIdx.y over the tiles of a face; a thread per pixel of the tile, 16 neighbours of a
// row side by side (128 bytes of the key plane)
__global__ void __launch_bounds__(kTile)
raster_sweep_kernel(const int *__restrict__ large_list, const long long *__restrict__ num_large, long long num_triangles,
                    const Face *__restrict__ records, View view, unsigned long long *__restrict__ keys) {
    long long n = num_large[0];
    n = n < num_triangles ? n : num_triangles;
    const int di = threadIdx.x % kSweep, dj = threadIdx.x / kSweep;
    for (long long k = blockIdx.x; k < n; k += gridDim.x) {
        const long long t = large_list[k];
        if (t < 0 || t >= num_triangles) continue;
        const Face f = records[t];
        int i0, i1, j0, j1;
        if (f.area2 <= 0 || !box_of(f, view, i0, i1, j0, j1)) continue;
        const long long tiles_x = (i1 - i0) / kSweep + 1, tiles_y = (j1 - j0) / kSweep + 1;
        for (long long tile = blockIdx.y; tile < tiles_x * tiles_y; tile += gridDim.y) {
            const long long ti = i0 + (tile % tiles_x) * kSweep, tj = j0 + (tile / tiles_x) * kSweep;
            // an edge function is linear: negative at the four corner centres, negative at every centre of the tile
            const long long xa = 256 * ti + 128, xb = xa + 256 * (kSweep - 1), ya = 256 * tj + 128, yb = ya + 256 * (kSweep - 1);
            bool out = false;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const int a = (e + 1) % 3, b = (e + 2) % 3;
                const long long ax = f.x[a], ay = f.y[a], bx = f.x[b], by = f.y[b];
                out = out || (edge(ax, ay, bx, by, xa, ya) < 0 && edge(ax, ay, bx, by, xb, ya) < 0 && edge(ax, ay, bx, by, xa, yb) < 0 &&
                              edge(ax, ay, bx, by, xb, yb) < 0);
            }
            if (out) continue;
            const long long i = ti + di, j = tj + dj;
            if (i <= i1 && j <= j1) sample(f, t, i, j, view, keys);
        }
    }
}

__global__ void __launch_bounds__(kTile)
raster_resolve_kernel(const unsigned long long *__restrict__ keys, long long num_pixels, int width, const Face *__restrict__ records,
                      long long num_triangles, long long num_vertices, const float *__restrict__ temperature,
                      const uint8_t *__restrict__ colors, int *__restrict__ pixel_face, float *__restrict__ pixel_depth,
                      float *__restrict__ pixel_temperature, uint8_t *__restrict__ pixel_colors, Partial *__restrict__ partials) {
    __shared__ double values[kTile];
    __shared__ unsigned wave_min[kTile / TN_WAVE], wave_max[kTile / TN_WAVE];
    const long long p = (long long)blockIdx.x * kTile + threadIdx.x;
    bool covered = false;
    int face = -1;
    float depth = quiet_nan(), temp = quiet_nan();
    uint8_t rgb[3] = {0, 0, 0};
    if (p < num_pixels) {
        const unsigned long long key = keys[p];
        const long long t = (long long)(key & 0xffffffffull);
        if (key != kEmpty && t < num_triangles) {
            const Face f = records[t];
            double l[3];
            const bool inside = f.v[0] >= 0 && f.v[0] < num_vertices && f.v[1] >= 0 && f.v[1] < num_vertices && f.v[2] >= 0 &&
                                f.v[2] < num_vertices;
            if (f.area2 > 0 && inside && cover(f, p % width, p / width, l)) {
                covered = true;
                face = (int)t;
                depth = depth_of(blend(l, f.z[0], f.z[1], f.z[2]));
                temp = (float)blend(l, (double)temperature[f.v[0]], (double)temperature[f.v[1]], (double)temperature[f.v[2]]);
                if (pixel_colors) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        rgb[c] = colour_of(blend(l, (double)colors[3 * (long long)f.v[0] + c], (double)colors[3 * (long long)f.v[1] + c],
                                                 (double)colors[3 * (long long)f.v[2] + c]));
                }
            }
        }
        if (pixel_face) pixel_face[p] = face;
        if (pixel_depth) pixel_depth[p] = depth;
        if (pixel_temperature) pixel_temperature[p] = temp;
        if (pixel_colors) {
#pragma unroll
            for (int c = 0; c < 3; ++c) pixel_colors[3 * p + c] = rgb[c];
        }
    }
    // the block's partial: the ordered sum is one thread's walk, the extremes and the count are order-free
    values[threadIdx.x] = covered ? (double)temp : 0.0;
    unsigned kmin = covered ? f2key(temp) : ~0u, kmax = covered ? f2key(temp) : 0u;
#pragma unroll
    for (int o = TN_WAVE / 2; o > 0; o >>= 1) {
        kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o, TN_WAVE));
        kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o, TN_WAVE));
    }
    if (threadIdx.x % TN_WAVE == 0) wave_min[threadIdx.x / TN_WAVE] = kmin, wave_max[threadIdx.x / TN_WAVE] = kmax;
    uint32_t total;
    block_rank<kTile>(covered, total);  // (its barrier orders the three LDS arrays above)
    if (threadIdx.x != 0) return;
    Partial out;
    out.sum = 0.0;
    out.kmin = ~0u, out.kmax = 0u;
    out.covered = (int)total, out.pad = 0;
    if (total > 0) {
        for (int k = 0; k < kTile; ++k) out.sum = __dadd_rn(out.sum, values[k]);
#pragma unroll
        for (int w = 0; w < kTile / TN_WAVE; ++w) out.kmin = min(out.kmin, wave_min[w]), out.kmax = max(out.kmax, wave_max[w]);
    }
    partials[blockIdx.x] = out;
}

__global__ void __launch_bounds__(kTile)
raster_finish_kernel(const Partial *__restrict__ partials, long long num_blocks, long long *__restrict__ counts,
                     double *__restrict__ stats) {
    __shared__ double chunk[kFinishChunk];
    __shared__ unsigned all_min[kTile], all_max[kTile];
    __shared__ long long all_covered[kTile];
    double sum = 0.0;
    unsigned kmin = ~0u, kmax = 0u;
    long long covered = 0;
    for (long long first = 0; first < num_blocks; first += kFinishChunk) {
        const long long here = num_blocks - first < kFinishChunk ? num_blocks - first : kFinishChunk;
        for (int k = threadIdx.x; k < here; k += kTile) {
            const Partial q = partials[first + k];
            chunk[k] = q.sum;
            kmin = min(kmin, q.kmin), kmax = max(kmax, q.kmax);
            covered += q.covered;
        }
        __syncthreads();
        if (threadIdx.x == 0)  // (reading eight values ahead of the chain by hand measured slower: 175 against 150 us for 16 384 partials)
            for (int k = 0; k < here; ++k) sum = __dadd_rn(sum, chunk[k]);
        __syncthreads();
    }
    all_min[threadIdx.x] = kmin, all_max[threadIdx.x] = kmax, all_covered[threadIdx.x] = covered;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < kTile; ++k) kmin = min(kmin, all_min[k]), kmax = max(kmax, all_max[k]), covered += all_covered[k];
    counts[0] = covered;
    stats[0] = sum;
    stats[1] = covered > 0 ? (double)key2f(kmin) : (double)INFINITY;
    stats[2] = covered > 0 ? (double)key2f(kmax) : -(double)INFINITY;
}

// V == 0 or T == 0: counts and stats of an empty image
__global__ void raster_empty_kernel(long long *__restrict__ counts, double *__restrict__ stats) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    counts[0] = counts[1] = counts[2] = 0;
    stats[0] = 0.0;
    stats[1] = (double)INFINITY;
    stats[2] = -(double)INFINITY;
}

inline bool bad_side(int32_t n) { return n < 1 || n > kMaxSide; }
inline bool host_finite(double x) { return x - x == 0.0; }

inline long long tiles_of(long long n) { return ceil_div(n, kTile); }

// the workspace, in order: the key plane, the face records, the partials, three arrays of tile counts, the number of large faces,
// the flags and the list of the large faces
struct Layout {
    unsigned long long *keys;
    Face *records;
    Partial *partials;
    long long *usable_tiles, *drawn_tiles, *large_tiles, *num_large;
    int *flags, *large_list;
    long long num_pixels, num_blocks;
    size_t bytes;
};

inline Layout layout_of(char *ws, long long t, long long width, long long height) {
    Layout l;
    size_t at = 0;
    auto take = [&](size_t bytes) {  // (ws == NULL: the sizes alone)
        char *p = ws ? ws + at : nullptr;
        at += bytes;
        return p;
    };
    l.num_pixels = width * height;
    l.num_blocks = ceil_div(l.num_pixels, kBlock);
    l.keys = reinterpret_cast<unsigned long long *>(take((size_t)l.num_pixels * sizeof(unsigned long long)));
    l.records = reinterpret_cast<Face *>(take((size_t)t * sizeof(Face)));
    l.partials = reinterpret_cast<Partial *>(take((size_t)l.num_blocks * sizeof(Partial)));
    long long **tiles[3] = {&l.usable_tiles, &l.drawn_tiles, &l.large_tiles};
    for (auto p : tiles) *p = reinterpret_cast<long long *>(take((size_t)tiles_of(t) * sizeof(long long)));
    l.num_large = reinterpret_cast<long long *>(take(sizeof(long long)));
    l.flags = reinterpret_cast<int *>(take(ints_bytes(t)));
    l.large_list = reinterpret_cast<int *>(take(ints_bytes(t)));
    l.bytes = at;
    return l;
}

}  // namespace

extern "C" {

int32_t tn_mesh_raster_small_box(void) { return kSmallBox; }

size_t tn_mesh_rasterize_workspace_bytes(int64_t num_triangles, int32_t width, int32_t height) {
    if (bad_counts(0, num_triangles) || bad_side(width) || bad_side(height)) return 0;
    return layout_of(nullptr, (long long)num_triangles, width, height).bytes;
}

int tn_mesh_rasterize(const float *positions, const float *temperature, const uint8_t *colors, const int32_t *triangles,
                      int64_t num_vertices, int64_t num_triangles, const tn_raster_view *view, int32_t *pixel_face, float *pixel_depth,
                      float *pixel_temperature, uint8_t *pixel_colors, int64_t *counts, double *stats, void *workspace,
                      size_t workspace_bytes, void *stream) {
    if (!view || !counts || !stats) return TN_ERR_NULL;
    if (bad_counts(num_vertices, num_triangles) || bad_side(view->width) || bad_side(view->height)) return TN_ERR_SHAPE;
    if (!host_finite(view->pixel_size) || !(view->pixel_size > 0.0)) return TN_ERR_SHAPE;
    for (int k = 0; k < 3; ++k)
        if (!host_finite(view->origin[k]) || !host_finite(view->right[k]) || !host_finite(view->down[k]) || !host_finite(view->forward[k]))
            return TN_ERR_SHAPE;
    if (view->near != view->near || view->far != view->far || view->cull < 0 || view->cull > 1 || view->reserved < 0 ||
        view->reserved > kMaxSide)
        return TN_ERR_UNSUPPORTED;
    const bool work = num_vertices > 0 && num_triangles > 0;
    if (work && (!positions || !temperature || !workspace)) return TN_ERR_NULL;
    if (num_triangles > 0 && !triangles) return TN_ERR_NULL;
    if (pixel_colors && !colors) return TN_ERR_NULL;
    if (misaligned(positions, 4) || misaligned(temperature, 4) || misaligned(triangles, 4) || misaligned(pixel_face, 4) ||
        misaligned(pixel_depth, 4) || misaligned(pixel_temperature, 4) || misaligned(counts, 8) || misaligned(stats, 8) ||
        misaligned(workspace, 8))
        return TN_ERR_SHAPE;
    if (work && workspace_bytes < tn_mesh_rasterize_workspace_bytes(num_triangles, view->width, view->height)) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long long nv = (long long)num_vertices, nt = (long long)num_triangles;
    long long *cnt = reinterpret_cast<long long *>(counts);
    const size_t pixels = (size_t)view->width * (size_t)view->height;
    if (!work) {
        if (pixel_face && hipMemsetAsync(pixel_face, 0xff, pixels * sizeof(int32_t), s) != hipSuccess) return TN_ERR_LAUNCH;
        if (pixel_depth && hipMemsetD32Async((hipDeviceptr_t)pixel_depth, 0x7fc00000, pixels, s) != hipSuccess) return TN_ERR_LAUNCH;
        if (pixel_temperature && hipMemsetD32Async((hipDeviceptr_t)pixel_temperature, 0x7fc00000, pixels, s) != hipSuccess)
            return TN_ERR_LAUNCH;
        if (pixel_colors && hipMemsetAsync(pixel_colors, 0, 3 * pixels, s) != hipSuccess) return TN_ERR_LAUNCH;
        hipLaunchKernelGGL(raster_empty_kernel, dim3(1), dim3(TN_WAVE), 0, s, cnt, stats);
        TN_LAUNCH_CHECK();
        return TN_OK;
    }
    View v;
    for (int k = 0; k < 3; ++k)
        v.origin[k] = view->origin[k], v.right[k] = view->right[k], v.down[k] = view->down[k], v.forward[k] = view->forward[k];
    v.pixel_size = view->pixel_size, v.near = view->near, v.far = view->far;
    v.width = view->width, v.height = view->height, v.cull = view->cull;
    v.small_box = view->reserved > 0 ? view->reserved : kSmallBox;
    const Layout l = layout_of(reinterpret_cast<char *>(workspace), nt, v.width, v.height);
    const unsigned face_blocks = (unsigned)tiles_of(nt);

    // 1 - 2: the empty plane; the faces, the small ones rasterised
    if (hipMemsetAsync(l.keys, 0xff, pixels * sizeof(unsigned long long), s) != hipSuccess) return TN_ERR_LAUNCH;
    hipLaunchKernelGGL(raster_faces_kernel, dim3(face_blocks), dim3(kTile), 0, s, positions, temperature, triangles, nv, nt, v, l.records,
                       l.flags, l.keys, l.usable_tiles, l.drawn_tiles, l.large_tiles);
    TN_LAUNCH_CHECK();

    // 3 - 5: the large faces in face order, swept in tiles
    hipLaunchKernelGGL(raster_scan_kernel, dim3(1), dim3(kScan), 0, s, l.usable_tiles, l.drawn_tiles, l.large_tiles, tiles_of(nt), cnt,
                       l.num_large);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(raster_large_list_kernel, dim3(face_blocks), dim3(kTile), 0, s, l.flags, nt, l.large_tiles, l.large_list);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(raster_sweep_kernel, dim3(tn_grid_blocks(nt, 1, 4 * kCUs), kSweepShare), dim3(kTile), 0, s, l.large_list,
                       l.num_large, nt, l.records, v, l.keys);
    TN_LAUNCH_CHECK();

    // 6 - 7: the image, its partials, its statistics
    hipLaunchKernelGGL(raster_resolve_kernel, dim3((unsigned)l.num_blocks), dim3(kTile), 0, s, l.keys, l.num_pixels, v.width, l.records, nt,
                       nv, temperature, colors, pixel_face, pixel_depth, pixel_temperature, pixel_colors, l.partials);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(raster_finish_kernel, dim3(1), dim3(kTile), 0, s, l.partials, l.num_blocks, cnt, stats);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

}  // extern "C"
