// The voxel grid of tn_voxel_params, the one place for it: the key of a point, the heads of the runs of equal keys in a sorted key
// list, and the ordered means of a run (include/thermonerf_hip.h defines each to the bit).  tn_voxel.hip averages a point cloud with
// them, tn_mesh_simplify.hip the vertices of a triangle mesh.
#pragma once
#include "tn_device.h"

namespace tn {

struct VoxelGrid {
    double origin[3];
    double inv;       // 1.0 / (double)voxel_size
    double limit[3];  // (double)dims
    unsigned long long dims_x, dims_y, total;
};

// the key of point i, or `total` (behind every voxel) for a point that is dropped
__device__ __forceinline__ unsigned long long voxel_key(const float *__restrict__ positions, long long i, const VoxelGrid &g) {
    unsigned long long c[3];
    bool member = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = positions[3 * i + a];
        const double u = __dmul_rn(__dsub_rn((double)p, g.origin[a]), g.inv);
        member = member && isfinite(p) && u >= 0.0 && u < g.limit[a];  // (a NaN fails)
        c[a] = member ? (unsigned long long)(long long)u : 0ull;
    }
    return member ? (c[2] * g.dims_y + c[1]) * g.dims_x + c[0] : g.total;
}

// sorted position j starts the run of a voxel
__device__ __forceinline__ bool voxel_head(const unsigned long long *__restrict__ keys, long long j, long long n, unsigned long long total) {
    if (j >= n) return false;
    const unsigned long long k = keys[j];
    return k < total && (j == 0 || k != keys[j - 1]);
}

__device__ __forceinline__ uint8_t rounded_mean(unsigned long long sum, unsigned long long members) {
    return (uint8_t)((2ull * sum + members) / (2ull * members));  // round half up; at most 255
}

struct VoxelInputs {
    const float *positions, *temperature;
    const uint8_t *colors, *thermal_colors;  // thermal_colors may be NULL
};

struct VoxelOutputs {
    float *positions, *temperature;
    uint8_t *colors, *thermal_colors;  // thermal_colors may be NULL
    int *count;
};

// One thread: the means of the run that starts at sorted position `start`, its members taken in list order (ascending index: the
// sort is stable), into row v of the outputs.  Sequential, because the fp64 sums are ordered by definition.
__device__ __forceinline__ void voxel_average(const unsigned long long *__restrict__ keys, const int *__restrict__ order, long long n,
                                              long long start, const VoxelInputs &in, const VoxelOutputs &out, long long v) {
    const unsigned long long key = keys[start];
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    unsigned long long rgb[3] = {0, 0, 0}, thermal_rgb[3] = {0, 0, 0};
    long long j = start;
    for (; j < n && keys[j] == key; ++j) {
        const long long i = order[j];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            sum[a] = __dadd_rn(sum[a], (double)in.positions[3 * i + a]);
            rgb[a] += in.colors[3 * i + a];
        }
        sum[3] = __dadd_rn(sum[3], (double)in.temperature[i]);
        if (in.thermal_colors) {
#pragma unroll
            for (int a = 0; a < 3; ++a) thermal_rgb[a] += in.thermal_colors[3 * i + a];
        }
    }
    const unsigned long long members = (unsigned long long)(j - start);  // >= 1: a head is a member
    const double m = (double)members;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        out.positions[3 * v + a] = (float)__ddiv_rn(sum[a], m);
        out.colors[3 * v + a] = rounded_mean(rgb[a], members);
    }
    out.temperature[v] = (float)__ddiv_rn(sum[3], m);
    if (out.thermal_colors) {
#pragma unroll
        for (int a = 0; a < 3; ++a) out.thermal_colors[3 * v + a] = rounded_mean(thermal_rgb[a], members);
    }
    out.count[v] = (int)members;
}

inline bool voxel_params_unsupported(const tn_voxel_params *params) {
    if (!(params->voxel_size > 0.0f) || !(params->voxel_size <= 3.402823466e+38f)) return true;  // (a NaN fails the first)
    for (int a = 0; a < 3; ++a)
        if (params->dims[a] < 1 || params->dims[a] > (1 << 21)) return true;
    return false;
}

inline VoxelGrid voxel_grid_of(const tn_voxel_params *params) {
    VoxelGrid g;
    for (int a = 0; a < 3; ++a) {
        g.origin[a] = (double)params->origin[a];
        g.limit[a] = (double)params->dims[a];
    }
    g.inv = 1.0 / (double)params->voxel_size;
    g.dims_x = (unsigned long long)params->dims[0];
    g.dims_y = (unsigned long long)params->dims[1];
    g.total = g.dims_x * g.dims_y * (unsigned long long)params->dims[2];  // <= 2^63
    return g;
}

inline int bit_length(unsigned long long x) {
    int bits = 0;
    for (; x; x >>= 1) ++bits;
    return bits;
}

}  // namespace tn
