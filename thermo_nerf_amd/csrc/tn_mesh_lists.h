// What the per-vertex readers of tn_mesh_incidence's lists share (tn_mesh_smooth.hip: the normals and the position passes;
// tn_mesh_gradient.hip: the scalar passes and the vertex gradient): a triangle's indices as one load, what makes it VALID, the list
// of a vertex clipped to the corners that exist, and the argument checks of their entries.  A reader never dereferences an index it
// has not checked: a list is clipped to [0, 3T], a corner outside it or of an invalid triangle is skipped — for the index
// tn_mesh_incidence built from the same triangles no check ever fires.
#pragma once
#include "tn_device.h"

namespace tn {

struct Tri {
    int v[3];
};

__device__ __forceinline__ Tri load_triangle(const int *__restrict__ tri, long long t) {
    return *reinterpret_cast<const Tri *>(tri + 3 * t);  // 12 bytes, 4-byte aligned: one global_load_dwordx3
}

__device__ __forceinline__ bool valid_triangle(const Tri &t, int num_vertices) {
    const unsigned n = (unsigned)num_vertices;
    return (unsigned)t.v[0] < n && (unsigned)t.v[1] < n && (unsigned)t.v[2] < n;
}

// the list of vertex v, clipped to the corners that exist
__device__ __forceinline__ void list_of(const int *__restrict__ offsets, long long v, long long num_corners, long long &begin,
                                        long long &end) {
    begin = offsets[v], end = offsets[v + 1];
    begin = begin < 0 ? 0 : begin;
    end = end > num_corners ? num_corners : end;
}

inline bool overlap(const void *a, const void *b, size_t bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bytes && y < x + bytes;
}

// what the per-vertex entries share: TN_OK, or the code of the first argument that is wrong (`values`: the per-vertex input, `out`:
// the per-vertex output)
inline int check_indexed_mesh(const float *values, const int32_t *triangles, int64_t num_triangles, int64_t num_vertices,
                              const int32_t *offsets, const int32_t *corners, const float *out) {
    if (num_vertices > 0 && (!values || !offsets || !out)) return TN_ERR_NULL;
    if (num_vertices > 0 && num_triangles > 0 && (!triangles || !corners)) return TN_ERR_NULL;
    if (bad_counts(num_vertices, num_triangles)) return TN_ERR_SHAPE;
    if (misaligned(values, 4) || misaligned(triangles, 4) || misaligned(offsets, 4) || misaligned(corners, 4) || misaligned(out, 4))
        return TN_ERR_SHAPE;
    return TN_OK;
}

}  // namespace tn
