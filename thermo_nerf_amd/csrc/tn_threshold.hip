// Foreground threshold of the evaluation harness [REF thermo_nerf/thermal_nerf/calculate_threshold.py:29-38]: per grey image,
// the 256-bin histogram and the Otsu threshold OpenCV's cv2.threshold(..., THRESH_BINARY + THRESH_OTSU) returns; the reference
// averages them over a dataset (host side, thermo_nerf_amd/thermal_nerf/calculate_threshold.py).  Two launches per call, no
// host synchronisation: the result is defined bit for bit (DESIGN.md 5.5c "Foreground threshold").
//
// Image extents: a HOST array of N + 1 pixel offsets into the packed byte stream, handed to the kernel BY VALUE in batches of
// kBatch images, as tn_adam_step hands its tensor descriptors (tn_optim.hip).  A device array would leave the host unable to
// refuse an image of 2^32 pixels or to size the grid without reading it back; by value costs nothing and needs no copy.
//
// Histogram pass (the only part that touches every pixel): a block owns a slice of ONE image.  The image's unaligned head
// (up to 15 bytes, to the next 16-byte address) and its tail go through a scalar path of the image's first block, as in
// tn_frame.hip; in between a lane loads 16 pixels as one uint4.  Thermal images are mostly flat background: a lane merges runs
// of equal pixels (across its loads as well — only the count matters) and issues one integer LDS atomic per run into its WAVE's
// 256 bins, so a constant image costs one atomic per lane instead of one per pixel on one bank.  The four waves' bins are
// summed and the non-zero ones flushed with integer global atomics.  Integer sums: order-independent, exact.
//
// Threshold pass: one lane per image walks the recurrence of OpenCV 4.x getThreshVal_Otsu_8u (imgproc/thresh.cpp) [recall:
// restated from memory, OpenCV is not a dependency] in fp64, every step ONE correctly rounded operation in the order written
// in include/thermonerf_hip.h.  Images with empty bins have plateaus of mathematically equal sigma, where the last bit decides
// which index the strict > keeps: the association is part of the definition.
#include "tn_device.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / TN_WAVE;
constexpr int kBatch = 128;               // images per histogram launch
constexpr int kGroupsPerThread = 4;       // 16-pixel groups a thread should at least find: 16 KB of pixels per block
constexpr int kMaxBlocksPerImage = 256;   // grid-stride beyond

struct Batch {
    long long start[kBatch + 1];   // pixel offsets of the batch's images in the packed stream
    int first_block[kBatch + 1];   // blocks [first_block[k], first_block[k + 1]) work on image k
    int count;
    int first_image;               // row of the first image in the histogram array
};

struct Run {  // a lane's current run of equal pixels
    uint32_t value, count;
};

__device__ __forceinline__ void push(Run &r, uint32_t v, uint32_t *bins) {
    if (v == r.value) {
        ++r.count;
    } else {
        if (r.count) atomicAdd(&bins[r.value], r.count);
        r.value = v;
        r.count = 1;
    }
}

__global__ void __launch_bounds__(kBlock)
histogram_kernel(const uint8_t *__restrict__ pixels, Batch b, uint32_t *__restrict__ histograms) {
    __shared__ uint32_t bins[kWaves][256];
    for (int e = threadIdx.x; e < kWaves * 256; e += kBlock) (&bins[0][0])[e] = 0u;
    __syncthreads();
    // which image: a binary search over <= kBatch block offsets (uniform per block)
    int lo = 0, hi = b.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int)blockIdx.x >= b.first_block[mid]) lo = mid; else hi = mid;
    }
    const int k = lo;
    const int slot = (int)blockIdx.x - b.first_block[k], slots = b.first_block[k + 1] - b.first_block[k];
    const uint8_t *img = pixels + b.start[k];
    const long long n = b.start[k + 1] - b.start[k];
    const long long to_aligned = (long long)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(img) & 15u)) & 15u);
    const long long head = to_aligned < n ? to_aligned : n;
    const long long groups = (n - head) / 16;
    uint32_t *mine = bins[threadIdx.x / TN_WAVE];

    Run r{0u, 0u};
    const uint4 *vec = reinterpret_cast<const uint4 *>(img + head);  // 16-byte aligned; group g < groups ends inside the image
    for (long long g = (long long)slot * kBlock + threadIdx.x; g < groups; g += (long long)slots * kBlock) {
        const uint4 v = vec[g];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            // a dword of one value (the flat background) is one compare
            const uint32_t first = w[q] & 0xffu;
            if (w[q] == first * 0x01010101u) {
                if (first == r.value) {
                    r.count += 4;
                } else {
                    if (r.count) atomicAdd(&mine[r.value], r.count);
                    r.value = first;
                    r.count = 4;
                }
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) push(r, (w[q] >> (8 * s)) & 0xffu, mine);
            }
        }
    }
    if (r.count) atomicAdd(&mine[r.value], r.count);
    // the unaligned head and the tail behind the last whole group, a pixel per thread (at most 15 + 15)
    const int tail = (int)(n - head - 16 * groups);
    if (slot == 0 && (int)threadIdx.x < (int)head + tail) {
        const long long p = (int)threadIdx.x < (int)head ? (long long)threadIdx.x : head + 16 * groups + ((int)threadIdx.x - (int)head);
        atomicAdd(&mine[img[p]], 1u);
    }
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) sum += bins[w][threadIdx.x];  // kBlock == 256: a thread per bin
    if (sum) atomicAdd(&histograms[(size_t)(b.first_image + k) * 256 + threadIdx.x], sum);
}

// OpenCV 4.x getThreshVal_Otsu_8u [recall], one image per lane
__global__ void __launch_bounds__(TN_WAVE)
otsu_kernel(const uint32_t *__restrict__ histograms, int num_images, int32_t *__restrict__ thresholds) {
    const int k = blockIdx.x * TN_WAVE + threadIdx.x;
    if (k >= num_images) return;
    const uint32_t *h = histograms + (size_t)k * 256;
    double n = 0.0, mu = 0.0;
    for (int i = 0; i < 256; ++i) {  // both sums are exact: integers below 2^53
        const double hi = (double)h[i];
        n = __dadd_rn(n, hi);
        mu = __dadd_rn(mu, __dmul_rn((double)i, hi));
    }
    const double scale = __ddiv_rn(1.0, n);
    mu = __dmul_rn(mu, scale);
    const double eps = (double)1.1920928955078125e-7f;  // FLT_EPSILON
    const double one_minus_eps = __dsub_rn(1.0, eps);
    double mu1 = 0.0, q1 = 0.0, max_sigma = 0.0;
    int max_val = 0;
    for (int i = 0; i < 256; ++i) {
        const double p = __dmul_rn((double)h[i], scale);
        mu1 = __dmul_rn(mu1, q1);
        q1 = __dadd_rn(q1, p);
        const double q2 = __dsub_rn(1.0, q1);
        if (fmin(q1, q2) < eps || fmax(q1, q2) > one_minus_eps) continue;  // (mu1 stays multiplied: OpenCV's own behaviour)
        mu1 = __ddiv_rn(__dadd_rn(mu1, __dmul_rn((double)i, p)), q1);
        const double mu2 = __ddiv_rn(__dsub_rn(mu, __dmul_rn(q1, mu1)), q2);
        const double d = __dsub_rn(mu1, mu2);
        const double sigma = __dmul_rn(__dmul_rn(__dmul_rn(q1, q2), d), d);
        if (sigma > max_sigma) {
            max_sigma = sigma;
            max_val = i;
        }
    }
    thresholds[k] = max_val;
}

}  // namespace

extern "C" int tn_otsu_thresholds(const uint8_t *pixels, const int64_t *offsets, int32_t num_images, uint32_t *histograms,
                                  int32_t *thresholds, void *stream) {
    if (!pixels || !offsets || !histograms || !thresholds) return TN_ERR_NULL;
    if (num_images < 1) return TN_ERR_SHAPE;
    if (offsets[0] < 0) return TN_ERR_SHAPE;
    for (int k = 0; k < num_images; ++k) {
        const int64_t n = offsets[k + 1] - offsets[k];
        if (n < 1) return TN_ERR_SHAPE;                     // (an image without pixels has no histogram to normalise)
        if (n >= (int64_t)1 << 32) return TN_ERR_UNSUPPORTED;  // a bin is 32 bits wide
    }
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(histograms, 0, (size_t)num_images * 256 * sizeof(uint32_t), s) != hipSuccess) return TN_ERR_LAUNCH;
    for (int first = 0; first < num_images; first += kBatch) {
        Batch b;
        b.count = num_images - first < kBatch ? num_images - first : kBatch;
        b.first_image = first;
        int blocks = 0;
        for (int k = 0; k < b.count; ++k) {
            b.start[k] = offsets[first + k];
            b.first_block[k] = blocks;
            // (the head is at most 15 pixels: sizing by n / 16 is within one group of the kernel's own count)
            const long long per_block = (long long)kBlock * kGroupsPerThread;
            const long long nb = ((offsets[first + k + 1] - offsets[first + k]) / 16 + per_block - 1) / per_block;
            blocks += (int)(nb < 1 ? 1 : nb < kMaxBlocksPerImage ? nb : kMaxBlocksPerImage);
        }
        b.start[b.count] = offsets[first + b.count];
        b.first_block[b.count] = blocks;
        for (int k = b.count + 1; k <= kBatch; ++k) {  // (unused entries: defined values)
            b.start[k] = b.start[b.count];
            b.first_block[k] = blocks;
        }
        hipLaunchKernelGGL(histogram_kernel, dim3(blocks), dim3(kBlock), 0, s, pixels, b, histograms);
        TN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(otsu_kernel, dim3((num_images + TN_WAVE - 1) / TN_WAVE), dim3(TN_WAVE), 0, s, histograms, (int)num_images,
                       thresholds);
    TN_LAUNCH_CHECK();
    return TN_OK;
}
