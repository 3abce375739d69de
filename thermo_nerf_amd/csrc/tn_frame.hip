// Frame finishing of the inference harness: a rendered float image -> the 8-bit RGB frame the reference's Renderer.render keeps
// [REF thermo_nerf/render/renderer.py:189-199]: replicate one channel to three, colour-map (matplotlib ListedColormap lookup) or
// scale by 255, cast to uint8 — plus nerfstudio's apply_depth_colormap as an opt-in for depth.  Every step is ONE correctly
// rounded fp32 operation (explicit *_rn intrinsics), so a frame is defined bit for bit (DESIGN.md "Frame finishing").
//
//   SCALE  v = x * 255                      -> byte = trunc(v) saturated to [0, 255], NaN -> 0         (x in [0,1]: numpy's cast)
//   LUT    i = trunc(x * 256), 256 -> 255   -> table_u8[i]; x < 0 -> entry 0, i > 255 -> entry 255, NaN -> (0,0,0)
//   DEPTH  t = clip((d - near) / ((far - near) + 1e-10), 0, 1), NaN -> 0;  c = table_f32[trunc(t * 255)];
//          byte = SCALE(c * acc + (1 - acc))   (multiply, subtract, add: three roundings)
//
// A thread owns 4 consecutive pixels: one float4 load per channel quarter (C = 1: one, C = 3: three) and 12 output bytes as
// three whole dwords.  dst need not be 4-byte aligned (a frame piece may start at any pixel): the first (dst & 3) pixels — the
// count that brings 3 * pixel to a multiple of 4 — and the last (n - head) % 4 go through a scalar path of block 0.  The table
// is read from LDS (one packed dword per entry in LUT mode).  Traffic is n (4 C [+ 4] + 3) bytes: the kernel is launch- and
// latency-bound and not a tuning target.
#include "tn_device.h"

using namespace tn;

namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;  // grid-stride beyond

struct DepthArgs {
    float near, denom;
};

// one pixel -> r | g << 8 | b << 16.  x: the pixel's C floats; a: its accumulation (DEPTH only)
template <int MODE, int C>
__device__ __forceinline__ uint32_t finish_pixel(const float *x, float a, const uint32_t *lut, const float *lutf, DepthArgs da) {
    if (MODE == TN_FRAME_SCALE) {
        if (C == 1) return quantise(mul_rn(x[0], 255.0f)) * 0x010101u;
        return quantise(mul_rn(x[0], 255.0f)) | quantise(mul_rn(x[1], 255.0f)) << 8 | quantise(mul_rn(x[2], 255.0f)) << 16;
    }
    if (MODE == TN_FRAME_LUT) return lut_entry_nan(lut, x[0]);  // (the reference looks channel 0 up: cmap(image[:, :, 0]))
    float t = __fdiv_rn(sub_rn(x[0], da.near), da.denom);
    t = fminf(fmaxf(t, 0.0f), 1.0f);  // clip; NaN -> 0
    const int i = (int)mul_rn(t, 255.0f);
    const float om = sub_rn(1.0f, a);
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) out |= quantise(mul_rn(add_rn(mul_rn(lutf[3 * i + c], a), om), 255.0f)) << (8 * c);
    return out;
}

template <int MODE, int C>
__global__ void __launch_bounds__(kBlock)
frame_to_rgb8_kernel(const float *__restrict__ src, const float *__restrict__ acc, const float *__restrict__ near_far,
                     const void *__restrict__ table, uint8_t *__restrict__ dst, long long n, int head, int src_vec, int acc_vec) {
    __shared__ uint32_t lut[MODE == TN_FRAME_LUT ? 256 : 1];
    __shared__ float lutf[MODE == TN_FRAME_DEPTH ? 768 : 1];
    DepthArgs da{0.0f, 1.0f};
    if (MODE == TN_FRAME_LUT) {
        load_lut<kBlock>(lut, reinterpret_cast<const uint8_t *>(table));
        __syncthreads();
    }
    if (MODE == TN_FRAME_DEPTH) {
        const float *t = reinterpret_cast<const float *>(table);
        for (int e = threadIdx.x; e < 768; e += kBlock) lutf[e] = t[e];
        __syncthreads();
        da.near = near_far[0];
        da.denom = add_rn(sub_rn(near_far[1], da.near), 1e-10f);
    }
    const long long groups = (n - head) / 4;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (long long)gridDim.x * kBlock) {
        const long long p = head + 4 * g;
        float x[4 * C], a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const float *s = src + p * C;
        if (src_vec) {
#pragma unroll
            for (int q = 0; q < C; ++q) {
                const float4 v = reinterpret_cast<const float4 *>(s)[q];
                x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4 * C; ++q) x[q] = s[q];
        }
        if (MODE == TN_FRAME_DEPTH) {
            if (acc_vec) {
                const float4 v = *reinterpret_cast<const float4 *>(acc + p);
                a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) a[q] = acc[p + q];
            }
        }
        uint32_t c[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] = finish_pixel<MODE, C>(x + q * C, a[q], lut, lutf, da);
        uint32_t *o = reinterpret_cast<uint32_t *>(dst + 3 * p);  // 3 (head + 4 g) + (dst & 3) is a multiple of 4
        o[0] = c[0] | c[1] << 24;
        o[1] = c[1] >> 8 | c[2] << 16;
        o[2] = c[2] >> 16 | c[3] << 8;
    }
    // the unaligned head and the n % 4 tail, a pixel per thread (at most 3 + 3)
    const int tail = (int)(n - head - 4 * groups);
    if (blockIdx.x == 0 && (int)threadIdx.x < head + tail) {
        const long long p = (int)threadIdx.x < head ? threadIdx.x : head + 4 * groups + ((int)threadIdx.x - head);
        float x[C];
#pragma unroll
        for (int q = 0; q < C; ++q) x[q] = src[p * C + q];
        store_rgb8(dst + 3 * p, finish_pixel<MODE, C>(x, MODE == TN_FRAME_DEPTH ? acc[p] : 0.0f, lut, lutf, da));
    }
}

template <int MODE, int C>
int launch(const float *src, const float *acc, const float *near_far, const void *table, uint8_t *dst, long long n, hipStream_t s) {
    const int head = (int)min((long long)(reinterpret_cast<uintptr_t>(dst) & 3), n);
    const long long groups = (n - head) / 4;
    const int blocks = (int)max(1LL, min((groups + kBlock - 1) / kBlock, (long long)kMaxBlocks));
    const int src_vec = reinterpret_cast<uintptr_t>(src + (long long)head * C) % 16 == 0;
    const int acc_vec = acc && reinterpret_cast<uintptr_t>(acc + head) % 16 == 0;
    hipLaunchKernelGGL((frame_to_rgb8_kernel<MODE, C>), dim3(blocks), dim3(kBlock), 0, s, src, acc, near_far, table, dst, n, head,
                       src_vec, acc_vec);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

}  // namespace

extern "C" {

int tn_frame_to_rgb8(const float *src, int64_t num_pixels, int32_t channels, int32_t mode, const void *table, const float *acc,
                     const float *near_far, uint8_t *dst, void *stream) {
    if (!src || !dst) return TN_ERR_NULL;
    if (num_pixels < 0 || (channels != 1 && channels != 3)) return TN_ERR_SHAPE;
    if (mode != TN_FRAME_SCALE && mode != TN_FRAME_LUT && mode != TN_FRAME_DEPTH) return TN_ERR_UNSUPPORTED;
    if (mode != TN_FRAME_SCALE && !table) return TN_ERR_NULL;
    if (mode == TN_FRAME_DEPTH && (!acc || !near_far)) return TN_ERR_NULL;
    if (reinterpret_cast<uintptr_t>(src) % 4 != 0 || (acc && reinterpret_cast<uintptr_t>(acc) % 4 != 0)) return TN_ERR_SHAPE;
    if (num_pixels == 0) return TN_OK;
    hipStream_t s = (hipStream_t)stream;
    const long long n = num_pixels;
    if (mode == TN_FRAME_SCALE)
        return channels == 1 ? launch<TN_FRAME_SCALE, 1>(src, nullptr, nullptr, nullptr, dst, n, s)
                             : launch<TN_FRAME_SCALE, 3>(src, nullptr, nullptr, nullptr, dst, n, s);
    if (mode == TN_FRAME_LUT)
        return channels == 1 ? launch<TN_FRAME_LUT, 1>(src, nullptr, nullptr, table, dst, n, s)
                             : launch<TN_FRAME_LUT, 3>(src, nullptr, nullptr, table, dst, n, s);
    return channels == 1 ? launch<TN_FRAME_DEPTH, 1>(src, acc, near_far, table, dst, n, s)
                         : launch<TN_FRAME_DEPTH, 3>(src, acc, near_far, table, dst, n, s);
}

}  // extern "C"
