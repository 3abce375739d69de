// k nearest neighbours of every point of a cloud, and normals from them (DESIGN.md "Point-cloud export": outlier removal and
// normals).  The list of (d2, index) pairs of a point is defined bit for bit (include/thermonerf_hip.h): every step of d2 is ONE
// correctly rounded fp32 operation, ties in d2 go to the lower index, so the result does not depend on how the search walks.
//
// A uniform grid over the bounding box of the finite points makes the search local.  Launches per call, no host
// synchronisation, no allocation:
//   1. box      per-block min / max over the finite points (fp32 min / max: exact and order-free) -> partials
//   2. setup    ONE block: the partials -> the box, the cell size, the grid's dims — on the device, nothing is read back
//   3. (memset) the cell counters <- 0
//   4. bin      a point's cell (stored per point) and an integer atomicAdd on its counter; a non-finite point writes its own
//               all -1 / +inf row here and takes no further part
//   5. tiles    one block per tile of kCellTile cells: the tile's number of points (block_exclusive's total, tn_scan.h)
//   6. scan     ONE block (scan_tiles): tile -> the number of points before it; the total = the number of finite points
//   7. offsets  one block per tile: every cell <- the position of its first point (block_exclusive again)
//   8. scatter  a point takes the next position of its cell (atomicAdd) and stores (x, y, z, index) there; afterwards a
//               cell's counter is the END of its range and the START of the next cell's
//   9. search   one thread per query, queries in cell order (a wave reads neighbouring cells): shells of cells of Chebyshev
//               radius r = 0, 1, 2, ... around the query's cell, the best k pairs in a sorted list in LDS
// The atomics are integer adds that no block waits for; the order in which points arrive inside a cell is arbitrary, and
// nothing in the defined output depends on it, because the list is ordered by (d2, index) and the stop rule below never
// leaves out a candidate that belongs to it.  No look-back, no grid barrier, no cooperative launch, no spinning (§5.5d).
//
// THE STOP RULE.  After shell r the search has seen every point whose cell differs from the query's by at most r on every
// axis.  A point j it has not seen differs by more than r on some axis c.  Cells are assigned by
//     u = fl64(fl64((double)p_c - (double)lo_c) * inv_h),   cell_c = min(int(u), dims_c - 1)
// (lo = the box minimum, so u >= 0).  Call u* = (p_c - lo_c) * inv_h the same expression in real numbers: |u - u*| <=
// 2^-52 u* < 2^-42 (two roundings, u* < 513).  On the high side cell_j >= cell_i + r + 1 gives u_j >= cell_i + r + 1 (the upper
// clamp only lowers a cell index), on the low side cell_j <= cell_i - r - 1 gives u_j < cell_i - r (a clamped cell_j would be
// the last cell, which is not below cell_i).  Hence, in real numbers,
//     |p_j - p_i| >= |p_jc - p_ic| = |u*_j - u*_i| / inv_h >= (gap - 2^-41) / inv_h,
//     gap = min over the axes and sides that still have cells outside the visited cube of
//           (cell_i + r + 1) - u_i  (high side)   or   u_i - (cell_i - r)  (low side).
// The computed fp32 d2 is not the real one: a difference, three squares and two sums of non-negative terms lose at most
// (1 - 2^-24)^5 > 1 - 2^-21 relative, and a square that underflows at most 2^-149 absolute each.  So with
//     D = (gap - 2^-40) * h,  h = fl64(1 / inv_h),   bound = D * D * (1 - 2^-20)
// every unseen point has a computed d2 >= bound whenever bound > 2^-100 (the margin 2^-21 D^2 then exceeds both the
// absolute underflow error and the fp64 roundings of D, h and the product, which are below 2^-50 relative).  The search
// stops after shell r iff the list is full and its worst d2 is STRICTLY below bound — an unseen point at exactly the worst d2
// with a lower index would belong in the list, and cannot exist when worst < bound <= its d2 — or when the cube covers the
// grid.  A bound that is not positive, or not above 2^-100, never stops the search.
// An isolated point walks many empty shells before its list fills: accepted (the exporter's box bounds the extent and such
// points are few); there is no inexact cut-off.
#include <math.h>

#include "tn_device.h"
#include "tn_scan.h"

using namespace tn;

namespace {

constexpr int kBlock = 256;       // threads of the box / bin / tiles / offsets / scatter / normals kernels
constexpr int kWaves = kBlock / TN_WAVE;
constexpr int kBoxBlocks = 1024;  // at most this many blocks of partial boxes (grid-stride beyond)
constexpr int kCellTile = 4 * kBlock;  // cells per tile: four consecutive cells per thread
constexpr int kSearch = 128;      // threads per search block: k * 8 B * 128 <= 32 KiB of LDS
constexpr int kMaxK = 32;
constexpr int kMaxRes = 512;

struct GridInfo {  // written by the setup block, read by everything after it
    double inv_h, h;
    float lo[3];
    int dims[3];
    int pad[2];
};
static_assert(sizeof(GridInfo) == 48, "GridInfo layout");

struct Layout {  // byte offsets inside the workspace; every part is 16-byte aligned
    size_t sorted, info, partials, count, tiles, cells, point_cell, total;
    long long num_tiles, num_cells;
};

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

inline int choose_resolution(long long n) {  // grid_resolution == 0: about one point per cell of the cube
    long long r = llround(cbrt((double)n));  // then exactly the smallest r with r^3 >= n, up to 256
    while (r * r * r < n) ++r;
    while (r > 1 && (r - 1) * (r - 1) * (r - 1) >= n) --r;
    return (int)(r < 1 ? 1 : (r > 256 ? 256 : r));
}

inline Layout layout_of(long long n, int res) {
    Layout l;
    l.num_cells = (long long)res * res * res;
    l.num_tiles = ceil_div(l.num_cells, kCellTile);
    size_t o = 0;
    l.sorted = o;     o += align16((size_t)n * sizeof(float4));
    l.info = o;       o += align16(sizeof(GridInfo));
    l.partials = o;   o += align16((size_t)kBoxBlocks * 6 * sizeof(float));
    l.count = o;      o += 16;
    l.tiles = o;      o += align16((size_t)l.num_tiles * sizeof(long long));
    l.cells = o;      o += (size_t)l.num_tiles * kCellTile * sizeof(uint32_t);  // padded to whole tiles
    l.point_cell = o; o += align16((size_t)n * sizeof(int32_t));
    l.total = o;
    return l;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;  // false for a NaN
}

// ---- 1. 2. the box of the finite points and the grid ---------------------------------------------------------------------------
__device__ __forceinline__ void box_reduce(float (&mn)[3], float (&mx)[3], float *out) {
    __shared__ float part[kWaves][6];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn[c] = fminf(mn[c], __shfl_xor(mn[c], o, TN_WAVE));
            mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o, TN_WAVE));
        }
    if (threadIdx.x % TN_WAVE == 0)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            part[threadIdx.x / TN_WAVE][c] = mn[c];
            part[threadIdx.x / TN_WAVE][3 + c] = mx[c];
        }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v = threadIdx.x < 3 ? fminf(v, part[w][threadIdx.x]) : fmaxf(v, part[w][threadIdx.x]);
        out[threadIdx.x] = v;
    }
}

__global__ void __launch_bounds__(kBlock)
box_kernel(const float *__restrict__ positions, long long n, float *__restrict__ partials) {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        const float p[3] = {positions[3 * i], positions[3 * i + 1], positions[3 * i + 2]};
        if (!finite3(p[0], p[1], p[2])) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            mn[c] = fminf(mn[c], p[c]);
            mx[c] = fmaxf(mx[c], p[c]);
        }
    }
    box_reduce(mn, mx, partials + 6 * (size_t)blockIdx.x);
}

__global__ void __launch_bounds__(kBlock)
setup_kernel(const float *__restrict__ partials, int num_partials, int res, GridInfo *__restrict__ info) {
    __shared__ float box[6];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < num_partials; b += kBlock)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            mn[c] = fminf(mn[c], partials[6 * b + c]);
            mx[c] = fmaxf(mx[c], partials[6 * b + 3 + c]);
        }
    box_reduce(mn, mx, box);
    __syncthreads();
    if (threadIdx.x != 0) return;
    GridInfo g;
    double ext[3], longest = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ext[c] = box[c] <= box[3 + c] ? (double)box[3 + c] - (double)box[c] : 0.0;  // no finite point: an empty box
        longest = fmax(longest, ext[c]);
        g.lo[c] = box[c] <= box[3 + c] ? box[c] : 0.0f;
    }
    if (longest > 0.0) {
        g.inv_h = 1.0 / (longest / (double)res);
        g.h = 1.0 / g.inv_h;
    } else {  // one position only: one cell, which the first cube covers
        g.inv_h = 0.0;
        g.h = 0.0;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) g.dims[c] = (int)fmin((double)(res - 1), floor(ext[c] * g.inv_h)) + 1;
    g.pad[0] = g.pad[1] = 0;
    *info = g;
}

// the unclamped cell coordinate of the stop rule's argument (>= 0: lo is the minimum)
__device__ __forceinline__ double cell_coordinate(float p, float lo, double inv_h) { return ((double)p - (double)lo) * inv_h; }
__device__ __forceinline__ int cell_of(double u, int dim) { return (int)fmax(fmin(u, (double)(dim - 1)), 0.0); }

// ---- 4. bin --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
bin_kernel(const float *__restrict__ positions, long long n, int k, const GridInfo *__restrict__ info, uint32_t *__restrict__ cells,
           int32_t *__restrict__ point_cell, int32_t *__restrict__ neighbor_index, float *__restrict__ neighbor_d2,
           double *__restrict__ mean_distance) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float x = positions[3 * i], y = positions[3 * i + 1], z = positions[3 * i + 2];
    if (!finite3(x, y, z)) {  // nobody's neighbour; its own row is empty
        point_cell[i] = -1;
        for (int m = 0; m < k; ++m) {
            if (neighbor_index) neighbor_index[i * k + m] = -1;
            if (neighbor_d2) neighbor_d2[i * k + m] = INFINITY;
        }
        if (mean_distance) mean_distance[i] = INFINITY;
        return;
    }
    const GridInfo g = *info;
    const int cx = cell_of(cell_coordinate(x, g.lo[0], g.inv_h), g.dims[0]);
    const int cy = cell_of(cell_coordinate(y, g.lo[1], g.inv_h), g.dims[1]);
    const int cz = cell_of(cell_coordinate(z, g.lo[2], g.inv_h), g.dims[2]);
    const int cell = (cz * g.dims[1] + cy) * g.dims[0] + cx;  // x fastest: a row of cells along x is one range of points
    point_cell[i] = cell;
    atomicAdd(&cells[cell], 1u);
}

// ---- 5. 6. 7. cell counts -> cell starts --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
tiles_kernel(const uint32_t *__restrict__ cells, long long *__restrict__ tiles) {
    const uint4 v = reinterpret_cast<const uint4 *>(cells)[(size_t)blockIdx.x * kBlock + threadIdx.x];
    uint32_t total;
    block_exclusive<kBlock>(v.x + v.y + v.z + v.w, total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = (long long)total;
}

__global__ void __launch_bounds__(kScan)
scan_kernel(long long *__restrict__ tiles, long long num_tiles, long long *__restrict__ count) {
    scan_tiles<false>(tiles, num_tiles, count);  // a pass sums at most all N < 2^31 points
}

__global__ void __launch_bounds__(kBlock)
offsets_kernel(uint32_t *__restrict__ cells, const long long *__restrict__ tiles) {
    uint4 *slot = reinterpret_cast<uint4 *>(cells) + (size_t)blockIdx.x * kBlock + threadIdx.x;
    const uint4 v = *slot;
    uint32_t total;
    uint4 start;
    start.x = (uint32_t)tiles[blockIdx.x] + block_exclusive<kBlock>(v.x + v.y + v.z + v.w, total);
    start.y = start.x + v.x;
    start.z = start.y + v.y;
    start.w = start.z + v.z;
    *slot = start;
}

// ---- 8. scatter ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
scatter_kernel(const float *__restrict__ positions, long long n, const int32_t *__restrict__ point_cell, uint32_t *__restrict__ cells,
               float4 *__restrict__ sorted) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int cell = point_cell[i];
    if (cell < 0) return;
    const uint32_t at = atomicAdd(&cells[cell], 1u);  // < the number of finite points <= n: inside `sorted`
    sorted[at] = make_float4(positions[3 * i], positions[3 * i + 1], positions[3 * i + 2], __int_as_float((int)i));
}

// ---- 9. search -----------------------------------------------------------------------------------------------------------------
struct Best {  // one lane's sorted list, slot m of lane t at [m * kSearch + t]: a wave's accesses to one slot fall on 64 banks
    float *d2;
    int *index;
    int k, count;
    float worst_d2;
    int worst_index;
    __device__ __forceinline__ void offer(float d, int j) {
        if (count == k && !(d < worst_d2 || (d == worst_d2 && j < worst_index))) return;
        int m = count < k ? count : k - 1;  // a full list drops its worst
        while (m > 0) {
            const float pd = d2[(m - 1) * kSearch];
            const int pj = index[(m - 1) * kSearch];
            if (pd < d || (pd == d && pj < j)) break;
            d2[m * kSearch] = pd;
            index[m * kSearch] = pj;
            --m;
        }
        d2[m * kSearch] = d;
        index[m * kSearch] = j;
        if (count < k) ++count;
        if (count == k) {
            worst_d2 = d2[(k - 1) * kSearch];
            worst_index = index[(k - 1) * kSearch];
        }
    }
};

__global__ void __launch_bounds__(kSearch)
search_kernel(const float4 *__restrict__ sorted, const long long *__restrict__ num_finite, int k, const GridInfo *__restrict__ info,
              const uint32_t *__restrict__ cells, int32_t *__restrict__ neighbor_index, float *__restrict__ neighbor_d2,
              double *__restrict__ mean_distance) {
    extern __shared__ float lists[];  // [k][kSearch] d2, then [k][kSearch] index
    const long long t = (long long)blockIdx.x * kSearch + threadIdx.x;
    if (t >= num_finite[0]) return;  // (no barrier below)
    const GridInfo g = *info;
    const float4 q = sorted[t];
    const int i = __float_as_int(q.w);
    Best best;
    best.d2 = lists + threadIdx.x;
    best.index = reinterpret_cast<int *>(lists + k * kSearch) + threadIdx.x;
    best.k = k;
    best.count = 0;
    best.worst_d2 = INFINITY;
    best.worst_index = 0x7fffffff;
    const double ux = cell_coordinate(q.x, g.lo[0], g.inv_h), uy = cell_coordinate(q.y, g.lo[1], g.inv_h),
                 uz = cell_coordinate(q.z, g.lo[2], g.inv_h);
    const int nx = g.dims[0], ny = g.dims[1], nz = g.dims[2];
    const int cx = cell_of(ux, nx), cy = cell_of(uy, ny), cz = cell_of(uz, nz);

    auto scan = [&](uint32_t begin, uint32_t end) {  // the points at [begin, end) of the cell order
        for (uint32_t p = begin; p < end; ++p) {
            const float4 c = sorted[p];
            const int j = __float_as_int(c.w);
            if (j == i) continue;
            const float dx = sub_rn(q.x, c.x), dy = sub_rn(q.y, c.y), dz = sub_rn(q.z, c.z);
            best.offer(add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz)), j);
        }
    };
    // cells xa .. xb (consecutive cells: ONE range of points) of the rows ya .. yb of plane z.  The ranges of four rows are
    // fetched before any is scanned: an isolated query walks thousands of empty rows, and their loads must not queue up
    // one round trip after the other.
    auto visit_rows = [&](int z, int ya, int yb, int xa, int xb) {
        for (int y = ya; y <= yb; y += 4) {
            uint32_t begin[4], end[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int first = (z * ny + min(y + u, yb)) * nx + xa;
                begin[u] = first > 0 ? cells[first - 1] : 0u;
                end[u] = y + u <= yb ? cells[first + (xb - xa)] : 0u;  // (a row past yb: an empty range)
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) scan(begin[u], end[u]);
        }
    };

    for (int r = 0;; ++r) {
        const int x0 = max(cx - r, 0), x1 = min(cx + r, nx - 1);
        const int y0 = max(cy - r, 0), y1 = min(cy + r, ny - 1);
        const int z0 = max(cz - r, 0), z1 = min(cz + r, nz - 1);
        for (int z = z0; z <= z1; ++z) {
            if (z == cz - r || z == cz + r) {  // a z face of the shell: every row, whole
                visit_rows(z, y0, y1, x0, x1);
                continue;
            }
            if (cy - r >= 0) visit_rows(z, cy - r, cy - r, x0, x1);  // the y faces: whole rows
            if (cy + r <= ny - 1) visit_rows(z, cy + r, cy + r, x0, x1);
            const int ya = max(cy - r + 1, 0), yb = min(cy + r - 1, ny - 1);  // between them: the two end cells, where the grid has them
            if (cx - r >= 0) visit_rows(z, ya, yb, cx - r, cx - r);
            if (cx + r <= nx - 1) visit_rows(z, ya, yb, cx + r, cx + r);
        }
        // the distance, in cells, to the nearest face of the visited cube that still has cells beyond it
        double gap = INFINITY;
        if (cx + r + 1 <= nx - 1) gap = fmin(gap, (double)(cx + r + 1) - ux);
        if (cx - r - 1 >= 0) gap = fmin(gap, ux - (double)(cx - r));
        if (cy + r + 1 <= ny - 1) gap = fmin(gap, (double)(cy + r + 1) - uy);
        if (cy - r - 1 >= 0) gap = fmin(gap, uy - (double)(cy - r));
        if (cz + r + 1 <= nz - 1) gap = fmin(gap, (double)(cz + r + 1) - uz);
        if (cz - r - 1 >= 0) gap = fmin(gap, uz - (double)(cz - r));
        if (gap == INFINITY) break;  // the cube covers the grid
        if (best.count == k) {
            const double d = (gap - 0x1p-40) * g.h;
            const double bound = d * d * (1.0 - 0x1p-20);
            if (d > 0.0 && bound > 0x1p-100 && (double)best.worst_d2 < bound) break;
        }
    }

    double sum = 0.0;
    for (int m = 0; m < k; ++m) {
        const bool have = m < best.count;
        const float d = have ? best.d2[m * kSearch] : INFINITY;
        if (neighbor_index) neighbor_index[(long long)i * k + m] = have ? best.index[m * kSearch] : -1;
        if (neighbor_d2) neighbor_d2[(long long)i * k + m] = d;
        sum = __dadd_rn(sum, __dsqrt_rn((double)d));
    }
    if (mean_distance) mean_distance[i] = best.count == k ? __ddiv_rn(sum, (double)k) : (double)INFINITY;
}

// ---- normals -------------------------------------------------------------------------------------------------------------------
// one cyclic Jacobi rotation that zeroes a[P][Q] of the symmetric 3 x 3 matrix a; v accumulates the eigenvectors in its columns
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&v)[3][3]) {
    constexpr int R = 3 - P - Q;
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));  // the smaller root: |angle| <= pi / 4
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double arp = a[R][P], arq = a[R][Q];
    a[P][P] -= t * apq;
    a[Q][Q] += t * apq;
    a[P][Q] = a[Q][P] = 0.0;
    a[R][P] = a[P][R] = c * arp - s * arq;
    a[R][Q] = a[Q][R] = s * arp + c * arq;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double vp = v[r][P], vq = v[r][Q];
        v[r][P] = c * vp - s * vq;
        v[r][Q] = s * vp + c * vq;
    }
}

__global__ void __launch_bounds__(kBlock)
normals_kernel(const float *__restrict__ positions, const int32_t *__restrict__ neighbor_index, long long n, int k,
               const float *__restrict__ viewpoints, float *__restrict__ normals) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float px = positions[3 * i], py = positions[3 * i + 1], pz = positions[3 * i + 2];
    const int32_t *row = neighbor_index + i * k;
    auto valid = [&](int j) { return j >= 0 && (long long)j < n; };
    int members = 0;
    double sx = (double)px, sy = (double)py, sz = (double)pz;  // 0 + p
    for (int m = 0; m < k; ++m) {
        const int j = row[m];
        if (!valid(j)) continue;
        ++members;
        sx += (double)positions[3 * (long long)j];
        sy += (double)positions[3 * (long long)j + 1];
        sz += (double)positions[3 * (long long)j + 2];
    }
    if (!finite3(px, py, pz) || members < 2) {
        normals[3 * i] = normals[3 * i + 1] = normals[3 * i + 2] = 0.0f;
        return;
    }
    const double count = (double)(members + 1);
    const double mx = sx / count, my = sy / count, mz = sz / count;
    double a[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    auto add = [&](double x, double y, double z) {
        const double dx = x - mx, dy = y - my, dz = z - mz;
        a[0][0] += dx * dx; a[0][1] += dx * dy; a[0][2] += dx * dz;
        a[1][1] += dy * dy; a[1][2] += dy * dz; a[2][2] += dz * dz;
    };
    add((double)px, (double)py, (double)pz);
    for (int m = 0; m < k; ++m) {
        const int j = row[m];
        if (valid(j)) add((double)positions[3 * (long long)j], (double)positions[3 * (long long)j + 1], (double)positions[3 * (long long)j + 2]);
    }
    a[1][0] = a[0][1]; a[2][0] = a[0][2]; a[2][1] = a[1][2];
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll 1
    for (int sweep = 0; sweep < 8; ++sweep) {  // converges quadratically; 8 sweeps leave the off-diagonal at rounding level
        jacobi_rotate<0, 1>(a, v);
        jacobi_rotate<0, 2>(a, v);
        jacobi_rotate<1, 2>(a, v);
    }
    const int e = a[1][1] < a[0][0] ? (a[2][2] < a[1][1] ? 2 : 1) : (a[2][2] < a[0][0] ? 2 : 0);  // smallest; lowest on a tie
    double nv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) nv[c] = e == 0 ? v[c][0] : (e == 1 ? v[c][1] : v[c][2]);
    const double len = sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) nv[c] /= len;
    double s = 0.0;
    if (viewpoints) {
        const float vx = viewpoints[3 * i], vy = viewpoints[3 * i + 1], vz = viewpoints[3 * i + 2];
        if (finite3(vx, vy, vz))
            s = nv[0] * ((double)vx - (double)px) + nv[1] * ((double)vy - (double)py) + nv[2] * ((double)vz - (double)pz);
    }
    bool flip = s < 0.0;
    if (!(s < 0.0) && !(s > 0.0)) {  // no usable viewpoint: the component of largest magnitude (lowest on a tie) is positive
        const double ax = fabs(nv[0]), ay = fabs(nv[1]), az = fabs(nv[2]);
        const int big = ay > ax ? (az > ay ? 2 : 1) : (az > ax ? 2 : 0);
        flip = (big == 0 ? nv[0] : (big == 1 ? nv[1] : nv[2])) < 0.0;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) normals[3 * i + c] = (float)(flip ? -nv[c] : nv[c]);
}

inline bool bad_resolution(int32_t r) { return r < 0 || r > kMaxRes; }

}  // namespace

extern "C" {

int32_t tn_knn_grid_resolution(int64_t num_points) { return num_points > 0 ? choose_resolution(num_points) : 0; }

size_t tn_knn_workspace_bytes(int64_t num_points, int32_t grid_resolution) {
    if (num_points <= 0 || num_points > 0x7fffffffLL || bad_resolution(grid_resolution)) return 0;
    return layout_of(num_points, grid_resolution > 0 ? grid_resolution : choose_resolution(num_points)).total;
}

int tn_knn(const float *positions, int64_t num_points, int32_t k, int32_t grid_resolution, int32_t *neighbor_index,
           float *neighbor_d2, double *mean_distance, void *workspace, size_t workspace_bytes, void *stream) {
    if (k < 1 || k > kMaxK) return TN_ERR_UNSUPPORTED;
    if (num_points < 0 || num_points > 0x7fffffffLL || bad_resolution(grid_resolution)) return TN_ERR_SHAPE;
    if (misaligned(positions, 4) || misaligned(neighbor_index, 4) || misaligned(neighbor_d2, 4) || misaligned(mean_distance, 8) ||
        misaligned(workspace, 16))
        return TN_ERR_SHAPE;
    if (num_points == 0) return TN_OK;
    if (!positions || !workspace) return TN_ERR_NULL;
    const long long n = num_points;
    const int res = grid_resolution > 0 ? grid_resolution : choose_resolution(n);
    const Layout l = layout_of(n, res);
    if (workspace_bytes < l.total) return TN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(workspace);
    float4 *sorted = reinterpret_cast<float4 *>(ws + l.sorted);
    GridInfo *info = reinterpret_cast<GridInfo *>(ws + l.info);
    float *partials = reinterpret_cast<float *>(ws + l.partials);
    long long *count = reinterpret_cast<long long *>(ws + l.count);
    long long *tiles = reinterpret_cast<long long *>(ws + l.tiles);
    uint32_t *cells = reinterpret_cast<uint32_t *>(ws + l.cells);
    int32_t *point_cell = reinterpret_cast<int32_t *>(ws + l.point_cell);
    const long long point_blocks = ceil_div(n, kBlock);
    const int box_blocks = (int)(point_blocks < kBoxBlocks ? point_blocks : kBoxBlocks);
    hipLaunchKernelGGL(box_kernel, dim3(box_blocks), dim3(kBlock), 0, s, positions, n, partials);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(setup_kernel, dim3(1), dim3(kBlock), 0, s, partials, box_blocks, res, info);
    TN_LAUNCH_CHECK();
    if (hipMemsetAsync(cells, 0, (size_t)l.num_tiles * kCellTile * sizeof(uint32_t), s) != hipSuccess) return TN_ERR_LAUNCH;
    hipLaunchKernelGGL(bin_kernel, dim3((unsigned)point_blocks), dim3(kBlock), 0, s, positions, n, (int)k, info, cells, point_cell,
                       neighbor_index, neighbor_d2, mean_distance);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(tiles_kernel, dim3((unsigned)l.num_tiles), dim3(kBlock), 0, s, cells, tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kScan), 0, s, tiles, l.num_tiles, count);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(offsets_kernel, dim3((unsigned)l.num_tiles), dim3(kBlock), 0, s, cells, tiles);
    TN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)point_blocks), dim3(kBlock), 0, s, positions, n, point_cell, cells, sorted);
    TN_LAUNCH_CHECK();
    const long long search_blocks = ceil_div(n, kSearch);
    hipLaunchKernelGGL(search_kernel, dim3((unsigned)search_blocks), dim3(kSearch), (size_t)k * kSearch * 8, s, sorted, count, (int)k, info,
                       cells, neighbor_index, neighbor_d2, mean_distance);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

int tn_pointcloud_normals(const float *positions, const int32_t *neighbor_index, int64_t num_points, int32_t k,
                          const float *viewpoints, float *normals, void *stream) {
    if (k < 1 || k > kMaxK) return TN_ERR_UNSUPPORTED;
    if (num_points < 0 || num_points > 0x7fffffffLL) return TN_ERR_SHAPE;
    if (misaligned(positions, 4) || misaligned(neighbor_index, 4) || misaligned(viewpoints, 4) || misaligned(normals, 4))
        return TN_ERR_SHAPE;
    if (num_points == 0) return TN_OK;
    if (!positions || !neighbor_index || !normals) return TN_ERR_NULL;
    const long long n = num_points;
    hipLaunchKernelGGL(normals_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, positions,
                       neighbor_index, n, (int)k, viewpoints, normals);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

}  // extern "C"
