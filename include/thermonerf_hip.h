/*
 * thermonerf_hip.h — C-ABI of libthermonerf_hip.so: the MI355X (gfx950) drop-in for ThermoNeRF's
 * volumetric-rendering hot path.
 *
 * The reference is 100 % Python (a nerfstudio plugin) and has no FFI of its own; the entry points below are
 * what a ctypes binding placed behind the reference's plugin surface binds (INTEGRATION.md shows the stub).
 * Each entry point cites the reference interface it replaces:
 *   REF = /root/reference/thermo_nerf/...        NS = nerfstudio 1.1.5 symbol invoked from that REF line.
 *
 * Conventions
 *   - every pointer named  *_dev / inside the structs  is a DEVICE pointer to contiguous row-major fp32
 *     (int32 where stated); the caller (PyTorch-ROCm) owns every buffer; nothing is allocated or freed here.
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it and the device is never synchronised.
 *   - return value: TN_OK or a negative TN_ERR_* code; no exceptions cross the boundary.
 *   - re-entrant across devices/streams: the library keeps no mutable global state.
 *   - `training` != 0 selects nerfstudio's train-mode semantics (no nan_to_num / clamp in the renderers).
 */
#ifndef THERMONERF_HIP_H
#define THERMONERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TN_OK 0
#define TN_ERR_NULL (-1)        /* a required pointer is NULL                           */
#define TN_ERR_SHAPE (-2)       /* a dimension is out of the supported range            */
#define TN_ERR_UNSUPPORTED (-3) /* configuration not implemented by the kernels         */
#define TN_ERR_WORKSPACE (-4)   /* workspace too small (see tn_render_workspace_bytes)  */
#define TN_ERR_LAUNCH (-5)      /* hipGetLastError() != hipSuccess after a launch       */

#define TN_MAX_LEVELS 16

/* NS HashEncoding (torch path): table [L*T, 2], per-level scalings taken from the module's `scalings`
 * buffer (never recomputed here — SURVEY.md §8c). Built at REF thermal_nerf/thermal_field.py:62-88 (main
 * field, via NerfactoField) and REF thermal_nerf/thermal_nerf_model.py:136-149 (proposal nets). */
typedef struct tn_hashgrid {
    const float *table;            /* [num_levels << log2_hashmap_size, 2]                         */
    float scalings[TN_MAX_LEVELS]; /* HashEncoding.scalings                                        */
    int32_t num_levels;            /* 1..16                                                        */
    int32_t log2_hashmap_size;     /* 1..24                                                        */
    /* optional re-laid ("dense") copy of the coarse levels produced by tn_hashgrid_prepare: for level
     * l < num_dense_levels, dense + dense_offset[l] holds a [(res+2)^3] x-major / z-fastest grid of
     * 16-byte elements derived from table[hash(x,y,z)].  What an element holds is a PRIVATE layout
     * between tn_hashgrid_prepare and the kernels (today: the entry and the difference to its
     * x-neighbour); callers only allocate the buffer and pass the struct on.  Results are
     * bit-identical to the hashed tables'.                                                          */
    const float *dense;
    int64_t dense_offset[TN_MAX_LEVELS]; /* in float2 elements                                      */
    int32_t dense_res[TN_MAX_LEVELS];    /* grid side (= scalings[l] + 2)                           */
    int32_t num_dense_levels;
    int32_t _pad;
} tn_hashgrid;

/* torch.nn.Linear: weight [out_dim, in_dim], bias [out_dim]. */
typedef struct tn_linear {
    const float *weight;
    const float *bias;
    int32_t in_dim;
    int32_t out_dim;
} tn_linear;

/* Position normalisation shared by both density fields (NS NerfactoField.get_density /
 * HashMLPDensityField.get_density): contraction != 0 -> SceneContraction(order=inf) then (x+2)/4
 * [REF thermal_nerf_model.py:91-94]; else (x - aabb_min) / (aabb_max - aabb_min). */
typedef struct tn_space {
    int32_t contraction;
    float aabb_min[3];
    float aabb_max[3];
    int32_t _pad;
} tn_space;

/* NS HashMLPDensityField(num_layers=2, hidden_dim=16, use_linear=False), REF thermal_nerf_model.py:140-149. */
typedef struct tn_density_field {
    tn_hashgrid grid;
    tn_linear l0; /* [hidden, 2*L] + ReLU */
    tn_linear l1; /* [1, hidden]          */
    tn_space space;
    float average_init_density; /* 1.0 */
    int32_t _pad;
} tn_density_field;

/* ThermalNerfactoTField, REF thermal_nerf/thermal_field.py:33-201 (NerfactoField base + thermal branch). */
typedef struct tn_thermal_field {
    tn_hashgrid grid;
    tn_linear base0;  /* mlp_base.mlp.layers.0  [64, 32]  ReLU                    */
    tn_linear base1;  /* mlp_base.mlp.layers.1  [1+geo, 64]                        */
    tn_linear head0;  /* mlp_head.layers.0      [64, 16+geo+app] ReLU              */
    tn_linear head1;  /* mlp_head.layers.1      [64, 64] ReLU                      */
    tn_linear head2;  /* mlp_head.layers.2      [3, 64]  Sigmoid                   */
    tn_linear th0;    /* mlp_thermal.layers.0   [64, geo] ReLU          REF :90-98 */
    tn_linear th1;    /* mlp_thermal.layers.1   [64, 64] Sigmoid        REF :90-98 */
    tn_linear thead;  /* field_head_thermal.net [1, 64] no activation   REF :100-102, thermal_field_head.py:50-51 */
    const float *appearance; /* embedding_appearance.embedding.weight [num_images, app_dim]        */
    int32_t num_images;
    int32_t app_dim;       /* 32 */
    int32_t geo_feat_dim;  /* 15 */
    int32_t use_average_appearance; /* eval: mean(embedding) if != 0 else zeros   REF :128-137 */
    int32_t sh_shifted;    /* 1: SH evaluated on (d+1)/2 (torch fallback), 0: on d */
    tn_space space;
    float average_init_density; /* 1.0, REF thermal_field.py:86 */
    /* optional blob produced by tn_field_prepare (MFMA-fragment-ordered MLP weights); NULL = raw path */
    const float *prepared;
    /* optional blob produced by tn_field_prepare_f16x3: every fp32 weight split into two f16 halves so that the eval
     * field kernel can evaluate each fp32 product as three f16 MFMA products accumulated in fp32 (~2^-22 relative
     * product error, needs |activation| < 65504).  Takes precedence over `prepared` for eval calls when non-NULL. */
    const float *prepared_f16x3;
    /* optional blob produced by tn_field_prepare_bf16x6: every fp32 weight as THREE bf16 pieces (24 significand bits: the split is
     * exact) so that the eval field kernel can evaluate each fp32 product as the six piece products of order <= 2, accumulated in
     * fp32: a per-product error of 2^-23 relative — fp32's own rounding size — at the matrix cores' bf16 rate.  Takes precedence
     * over `prepared_f16x3` and `prepared` for eval calls when non-NULL.
     * ABI NOTE (round 4 appended this member): ZERO-INITIALISE the struct (`tn_thermal_field f = {0};` / memset) before filling it
     * — the three `prepared*` pointers are optional and a non-NULL one is dereferenced; a caller compiled against the older,
     * shorter struct must be recompiled.  RANGE NOTE (tests/test_gpu_parity.py::test_bf16x6_split_is_exact_...): x = p1 + p2 + p3
     * exactly for 2^-110 <= |x| <= (2 - 2^-8) 2^127 = 3.396e38.  Below, the third piece falls under bf16's smallest sub-normal
     * (2^-133) and the sum is off by < 2^-133 absolute; above, bf16(x) rounds to infinity (the field's activations are O(1)).
     * gfx950's bf16 MFMA takes sub-normal bf16 INPUTS as they are (test_bf16_mfma_takes_subnormal_inputs_as_they_are), so the small
     * pieces of small operands still contribute.  Measured on 1e6 random pairs over 60 binades: the six-product sum is within
     * 0.77 x 2^-23 of the fp64 product. */
    const float *prepared_bf16x6;
} tn_thermal_field;

/* ------------------------------------------------------------------------------------------------------
 * Per-sample entry points (the Field plugin surface)
 * ---------------------------------------------------------------------------------------------------- */

/* NS Cameras.generate_rays for one perspective camera, as called by the reference's harnesses
 * [REF thermo_nerf/render/renderer.py:182-184; thermo_nerf/evaluator/evaluator.py:68-70]: pixels
 * [first_pixel, first_pixel + num_pixels) of the row-major H x W image (pixel centres at +0.5) ->
 * origins [n,3], unit directions [n,3], pixel_area [n] (may be NULL).  c2w_host = 12 HOST floats, row-major [3,4].
 * distortion_host = 6 HOST floats (k1, k2, k3, k4, p1, p2: NS get_distortion_params order) or NULL; when any is non-zero
 * the normalised pixel coordinates go through NS camera_utils.radial_and_tangential_undistort (10 Newton steps). */
int tn_generate_rays(const float *c2w_host, float fx, float fy, float cx, float cy, int32_t height, int32_t width,
                     const float *distortion_host, int64_t first_pixel, int64_t num_pixels, float *origins,
                     float *directions, float *pixel_area, void *stream);

/* NS Frustums.get_positions: pos = origins + directions * (starts + ends) / 2.
 * origins/directions [R,3]; starts/ends [R,n]; positions out [R,n,3]. */
int tn_frustum_positions(const float *origins, const float *directions, const float *starts, const float *ends,
                         int64_t num_rays, int32_t n, float *positions, void *stream);

/* The same positions straight from a level's bin edges eucl_bins [R,n+1] (RaySamples.frustums.starts / .ends are its two
 * edge columns, NS Sampler.generate_ray_samples via get_ray_samples), also writing the contiguous starts / ends / deltas
 * [R,n] the training step's adjoint kernels read: one launch for the level's geometry. */
int tn_frustum_from_edges(const float *origins, const float *directions, const float *eucl_bins, int64_t num_rays,
                          int32_t n, float *positions, float *starts, float *ends, float *deltas, void *stream);

/* HashMLPDensityField.density_fn(positions) [REF thermal_nerf_model.py:146-149,222-224]:
 * positions [N,3] -> density [N]. */
int tn_density_fwd(const tn_density_field *field, const float *positions, int64_t n, float *density, void *stream);

/* NerfactoField.get_density as used by ThermalNerfactoTField.forward [REF thermal_field.py:186-190]:
 * positions [N,3] -> density [N], geo embedding [N, geo_feat_dim]. */
int tn_field_density_fwd(const tn_thermal_field *field, const float *positions, int64_t n, float *density,
                         float *geo, void *stream);

/* ThermalNerfactoTField.get_outputs [REF thermal_field.py:108-181]:
 * directions [N,3] (un-normalised to [0,1]; the kernel applies (d+1)/2), geo [N,geo], camera_indices [N] int32
 * (only read when training != 0) -> rgb [N,3], thermal [N]. */
int tn_field_heads_fwd(const tn_thermal_field *field, const float *directions, const float *geo,
                       const int32_t *camera_indices, int64_t n, int32_t training, float *rgb, float *thermal,
                       void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Samplers and weights (NS ray_samplers.py / RaySamples.get_weights, invoked at
 * REF thermal_nerf_model.py:172-179,222-224,233)
 * ---------------------------------------------------------------------------------------------------- */

/* The proposal sampler's initial sampler [REF thermal_nerf_model.py:164-170]: UniformLinDispPiecewiseSampler
 * (uniform_spacing == 0, the reference default) or UniformSampler (uniform_spacing == 1; spacing_fn and its inverse are the
 * identity).  spacing bins [n+1] (= torch.linspace(0,1,n+1), host-computed, device resident) (+ optional per-ray
 * stratified jitter t_rand [R], NULL in eval) -> spacing_bins [R,n+1], euclidean bins [R,n+1]. nears/fars [R].
 * Bit 1 of uniform_spacing (value 2, round 5) = NS single_jitter=False: t_rand is [R,n+1], one draw per bin edge. */
int tn_sample_initial(const float *lin_bins, const float *t_rand, const float *nears, const float *fars,
                      int64_t num_rays, int32_t n, int32_t uniform_spacing, float *spacing_bins, float *eucl_bins,
                      void *stream);

/* RaySamples.get_weights: deltas [R,n], densities [R,n] -> weights [R,n]. */
int tn_weights_fwd(const float *deltas, const float *densities, int64_t num_rays, int32_t n, float *weights,
                   void *stream);

/* PDFSampler.generate_ray_samples (histogram_padding 0.01, eps 1e-5): weights [R,n_in] (already annealed),
 * existing spacing bins [R,n_in+1], u [n_out+1] (host-computed eval positions) or u_rand [R] jitter (training;
 * NULL in eval), nears/fars [R] -> spacing_bins [R,n_out+1], eucl_bins [R,n_out+1].  uniform_spacing = the initial
 * sampler's spacing function, which PDFSampler reuses for the new bins (see tn_sample_initial); its bit 1 (value 2) =
 * single_jitter=False: u_rand is [R,n_out+1], one draw per new bin edge. */
int tn_sample_pdf(const float *weights, const float *existing_bins, const float *u, const float *u_rand,
                  const float *nears, const float *fars, int64_t num_rays, int32_t n_in, int32_t n_out,
                  int32_t uniform_spacing, float *spacing_bins, float *eucl_bins, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Renderers
 * ---------------------------------------------------------------------------------------------------- */

/* ThermalRenderer.forward [REF thermal_renderer.py:113-149] and NS RGBRenderer(background "last_sample")
 * [witness REF rgb_concat/rgbt_renderer.py:62-81,159-174]: values [R,n,C], weights [R,n] -> out [R,C]
 * = sum_s w*v + v[last]*(1 - sum_s w); eval (training == 0): nan_to_num(values) first, clamp [0,1] last. */
int tn_composite_fwd(const float *values, const float *weights, int64_t num_rays, int32_t n, int32_t channels,
                     int32_t training, float *out, void *stream);

/* NS AccumulationRenderer + DepthRenderer("median") + DepthRenderer("expected") in one pass
 * [REF thermal_nerf_model.py:238-243,267-270]. weights/starts/ends [R,n]; any output may be NULL.
 * expected depth is clipped to the call-global [min(steps), max(steps)] exactly as the reference does;
 * `minmax_scratch` = 2 floats of device scratch (required when expected != NULL). */
int tn_depth_fwd(const float *weights, const float *starts, const float *ends, int64_t num_rays, int32_t n,
                 float *accumulation, float *median, float *expected, float *minmax_scratch, void *stream);

/* torchmetrics.functional.structural_similarity_index_measure with its defaults (gaussian 11 x 11, sigma 1.5, k1 0.01,
 * k2 0.03; torchmetrics 1.7.2, uv.lock:5468-5469) as the reference's models call it on a rendered frame
 * [REF thermal_nerf_model.py:195,363; NS NerfactoModel.get_image_metrics_and_images]: pred / target [H,W,C] device floats
 * (the renderers' layout), data_range = what torchmetrics derives when none is given, max(pred.max() - pred.min(),
 * target.max() - target.min()); out[0] = mean index over the windows inside the image and the channels.
 * height, width >= 11.  workspace: tn_ssim_workspace_bytes(height, width, channels) bytes of device scratch. */
size_t tn_ssim_workspace_bytes(int32_t height, int32_t width, int32_t channels);
int tn_ssim_fwd(const float *pred, const float *target, int32_t height, int32_t width, int32_t channels, float data_range,
                void *workspace, size_t workspace_bytes, float *out, void *stream);

/* Frame finishing of the inference harness [REF thermo_nerf/render/renderer.py:189-199]: src [n, channels] device floats
 * (channels 1 or 3) -> dst [n, 3] uint8, on the device, every step one correctly rounded fp32 operation:
 *   TN_FRAME_SCALE  `(x * 255).astype(np.uint8)`, one channel replicated to three [REF :191-192,198]; outside [0, 256), where
 *                   numpy's cast is undefined: saturated to [0, 255], NaN -> 0.
 *   TN_FRAME_LUT    `(cmap(x[:, :, 0])[:, :, :3] * 255).astype(np.uint8)` for a 256-entry matplotlib ListedColormap [REF :193-196]:
 *                   i = trunc(x * 256) (256 -> 255), dst = table[i]; x < 0 -> entry 0, i > 255 -> entry 255, NaN -> (0, 0, 0);
 *                   `table` = uint8 [256, 3] = trunc(colours * 255).  Channel 0 is looked up.
 *   TN_FRAME_DEPTH  NS colormaps.apply_depth_colormap: t = clip((d - near) / ((far - near) + 1e-10), 0, 1), NaN -> 0;
 *                   c = table[trunc(t * 255)] (`table` = float [256, 3]); TN_FRAME_SCALE of c * acc + (1 - acc).
 *                   near_far = 2 device floats (near, far), acc [n] device floats; both NULL otherwise.
 * dst may start at any byte (a piece of a frame): whole dwords are written wherever 4 pixels share three of them. */
#define TN_FRAME_SCALE 0
#define TN_FRAME_LUT 1
#define TN_FRAME_DEPTH 2
int tn_frame_to_rgb8(const float *src, int64_t num_pixels, int32_t channels, int32_t mode, const void *table, const float *acc,
                     const float *near_far, uint8_t *dst, void *stream);

/* Foreground threshold of the evaluation harness [REF thermo_nerf/thermal_nerf/calculate_threshold.py:29-38]: for each of
 * num_images grey images, the Otsu threshold cv2.threshold(image, 0, 255, THRESH_BINARY + THRESH_OTSU) returns — an integer
 * in [0, 255]; the reference averages them over the dataset and divides by 255 (the host does that part).
 *   pixels      device bytes of all images back to back; an image may start at any byte alignment.
 *   offsets     HOST array of num_images + 1 increasing pixel offsets into `pixels` (image k = [offsets[k], offsets[k+1])),
 *               read during the call and handed to the kernels by value, as the Adam step's descriptors are: the host can
 *               refuse an unsupported extent and size the grid without a device read-back.
 *   histograms  device uint32 [num_images, 256], caller-provided scratch AND output: cleared by the call itself, then the
 *               exact count of every grey level (integer atomics: independent of the order of arrival).
 *   thresholds  device int32 [num_images].
 * Queued on `stream`; no host synchronisation inside the call.
 * The threshold is the recurrence of OpenCV 4.x getThreshVal_Otsu_8u (imgproc/thresh.cpp) [recall], h = the histogram:
 *     n = sum h[i];  scale = 1.0 / n;  mu = (sum over i = 0..255 ascending of i * h[i]) * scale
 *     mu1 = 0, q1 = 0, max_sigma = 0, max_val = 0
 *     for i = 0 .. 255:
 *         p = h[i] * scale;  mu1 = mu1 * q1;  q1 = q1 + p;  q2 = 1 - q1
 *         if min(q1, q2) < FLT_EPSILON or max(q1, q2) > 1 - FLT_EPSILON: continue      (mu1 stays multiplied)
 *         mu1 = (mu1 + i * p) / q1;  mu2 = (mu - q1 * mu1) / q2
 *         sigma = ((q1 * q2) * (mu1 - mu2)) * (mu1 - mu2)
 *         if sigma > max_sigma: max_sigma = sigma; max_val = i
 *     threshold = max_val
 * in fp64, every step ONE correctly rounded operation in the order and association written.  Histograms with empty bins have
 * plateaus of mathematically equal sigma on which the last bit decides which index the strict > keeps: the order of
 * operations is part of the definition.  A constant image gives 0.
 * TN_ERR_SHAPE: num_images < 1, a negative or decreasing offset, an image without pixels; TN_ERR_UNSUPPORTED: an image of
 * 2^32 pixels or more (a bin is 32 bits wide). */
int tn_otsu_thresholds(const uint8_t *pixels, const int64_t *offsets, int32_t num_images, uint32_t *histograms,
                       int32_t *thresholds, void *stream);

/* Point-cloud export (what nerfstudio's point-cloud exporter does with rendered depth, plus a temperature per point): the
 * per-ray outputs of a rendered pose -> the surviving points, appended in ray order behind a device-resident counter.
 * Every step is one correctly rounded fp32 operation in the order and association written.  For ray i of num_rays:
 *     p[c] = origins[i][c] + directions[i][c] * depth[i]                                   (multiply, add), c = 0..2
 *     kept iff  accumulation[i] > min_accumulation
 *          and  p[c] > box_min[c] and p[c] < box_max[c] for every c                        (on p, BEFORE to_world)
 *          and  thermal[i] > thermal_lo and thermal[i] < thermal_hi
 *   all comparisons strict; a NaN in depth, accumulation, thermal or p makes one false, so the ray is dropped; a bound of
 *   -inf / +inf switches its test off.  For a kept ray, at index k = count_in + #{kept j < i} (count_in = count[0] as the call
 *   finds it on the stream):
 *     positions[k][c]   = ((M[c][0] * p[0] + M[c][1] * p[1]) + M[c][2] * p[2]) + M[c][3],  M = to_world, row-major 3 x 4
 *     temperature[k]    = thermal[i] * temperature_span + temperature_min                  (degrees; span = max - min)
 *     colors[k]         = TN_FRAME_SCALE of rgb[i]          (trunc(x * 255) saturated to [0, 255], NaN -> 0)
 *     thermal_colors[k] = TN_FRAME_LUT of thermal[i] through thermal_table (uint8 [256, 3]), as tn_frame_to_rgb8 defines it
 *     source[k]         = source_base + i
 *   and count[0] = count_in + kept — the FULL number: nothing is written at an index >= capacity, and the host detects an
 *   overflow as count > capacity after its one read-back.  thermal_colors (with its table) and source may be NULL.
 * origins / directions / rgb [num_rays, 3], depth / accumulation / thermal [num_rays] device floats that may start at any
 * ray of a larger allocation (4-byte alignment is all that is assumed); positions [capacity, 3] floats, colors /
 * thermal_colors [capacity, 3] bytes, temperature [capacity] floats, source [capacity] int64, count 1 device int64.
 * workspace: tn_pointcloud_workspace_bytes(num_rays) bytes of device scratch, 8-byte aligned (one int64 per tile).
 * Three launches on `stream` (per-tile count, a one-block scan of the tile counts, emit), no host synchronisation, no
 * allocation; the output order is a prefix sum and never depends on atomics, and no block waits for another.
 * tn_pointcloud_tile_rays / tn_pointcloud_scan_width: rays per tile, and tile counts per pass of the scan block (the sizes at
 * which the kernels change path; for tests).
 * TN_ERR_NULL: a required pointer is NULL (the outputs are required when capacity > 0, the workspace when num_rays > 0);
 * TN_ERR_SHAPE: num_rays or capacity negative, a float pointer not 4-byte aligned, count / source / workspace not 8-byte
 * aligned; TN_ERR_WORKSPACE: workspace_bytes too small.  num_rays == 0: TN_OK, nothing is launched, count is untouched. */
typedef struct tn_pointcloud_params {
    float min_accumulation;
    float box_min[3], box_max[3];
    float thermal_lo, thermal_hi;
    float temperature_span, temperature_min;
    float to_world[12]; /* row-major 3 x 4 */
} tn_pointcloud_params;
int32_t tn_pointcloud_tile_rays(void);
int32_t tn_pointcloud_scan_width(void);
size_t tn_pointcloud_workspace_bytes(int64_t num_rays);
int tn_pointcloud_append(const float *origins, const float *directions, const float *depth, const float *accumulation,
                         const float *rgb, const float *thermal, int64_t num_rays, int64_t source_base,
                         const tn_pointcloud_params *params, const uint8_t *thermal_table, float *positions, uint8_t *colors,
                         float *temperature, uint8_t *thermal_colors, int64_t *source, int64_t capacity, int64_t *count,
                         void *workspace, size_t workspace_bytes, void *stream);

/* k nearest neighbours of every point of a cloud (what the exporter's outlier removal and normals are built on).  The list
 * of (d2, index) pairs of a point is defined bit for bit.  positions: [num_points, 3] device floats; a point is FINITE iff
 * its three coordinates are.  For finite points i != j, every step ONE correctly rounded fp32 operation:
 *     dx = x_i - x_j,  dy = y_i - y_j,  dz = z_i - z_j;     d2 = (dx * dx + dy * dy) + dz * dz
 * The neighbours of i are the k other finite points with the smallest (d2, j) in lexicographic order: a tie in d2 goes to
 * the lower index.  A point is never its own neighbour; a duplicate at the same position is one, with d2 = 0.  Row i of
 * neighbor_index (int32 [num_points, k]) and neighbor_d2 (float [num_points, k]) holds them in ascending (d2, j) order;
 * where fewer than k other finite points exist the remaining slots hold -1 and +inf.  A non-finite point is nobody's
 * neighbour and its own row is all -1 and +inf.  mean_distance (double [num_points]): for a finite point with a full row
 *     (sqrt((double)d2_0) + sqrt((double)d2_1) + ... ) / k       summed in fp64 from 0 in row order,
 * +inf for every other point.  Any of the three outputs may be NULL.
 * grid_resolution: the number of cells, along the longest side of the finite points' bounding box, of the uniform grid
 * that makes the search local: 0 lets the library choose from num_points (tn_knn_grid_resolution tells what it chooses),
 * 1 .. 512 forces it.  THE OUTPUTS DO NOT DEPEND ON IT: the search leaves a shell of cells only when the list is full and
 * its worst d2 is strictly below a lower bound, valid for the COMPUTED fp32 d2, on anything it has not seen
 * (thermo_nerf_amd/csrc/tn_knn.hip and DESIGN.md state the argument).  An isolated point costs many empty shells.
 * workspace: tn_knn_workspace_bytes(num_points, grid_resolution) device bytes, 16-byte aligned.  Eight launches and one
 * memset on `stream`, no host synchronisation, no allocation.  Points are counted into cells with integer atomic adds; no
 * block waits for another, and nothing in the outputs depends on the order of arrival.
 * TN_ERR_UNSUPPORTED: k < 1 or k > 32; TN_ERR_SHAPE: num_points < 0 or > 2^31 - 1, grid_resolution < 0 or > 512, a
 * misaligned pointer; num_points == 0: TN_OK, nothing is launched or written; then TN_ERR_NULL: positions or workspace is
 * NULL; TN_ERR_WORKSPACE: workspace_bytes too small.  All are returned before any launch.
 *
 * tn_pointcloud_normals: a normal per point from its neighbour rows.  Point i's neighbourhood is i itself followed by the
 * valid entries (0 <= j < num_points) of row i of neighbor_index, in row order.  A non-finite point, or one with fewer than 2
 * valid neighbours, gets (0, 0, 0).  Otherwise, in fp64, every step one correctly rounded operation, summed from 0 in
 * neighbourhood order:  c = (sum of q) / count;  C[a][b] = sum of (q_a - c_a) * (q_b - c_b)  — the covariance, defined bit
 * for bit.  The normal is the unit eigenvector of C's smallest eigenvalue (cyclic Jacobi in fp64; the eigenvector is
 * defined to a tolerance, not to the bit), rounded once to fp32.  Sign, with viewpoints [num_points, 3] floats or NULL:
 * s = sum over c of n_c * (v_c - p_c) in fp64; the normal is negated iff s < 0; if s == 0, the viewpoint is non-finite or
 * viewpoints is NULL, the component of largest |n_c| (the lowest c on a tie) is made positive.  One launch.
 * TN_ERR_UNSUPPORTED: k < 1 or k > 32; TN_ERR_SHAPE: num_points out of range, a misaligned pointer; num_points == 0: TN_OK;
 * TN_ERR_NULL: positions, neighbor_index or normals is NULL. */
int32_t tn_knn_grid_resolution(int64_t num_points);
size_t tn_knn_workspace_bytes(int64_t num_points, int32_t grid_resolution);
int tn_knn(const float *positions, int64_t num_points, int32_t k, int32_t grid_resolution, int32_t *neighbor_index,
           float *neighbor_d2, double *mean_distance, void *workspace, size_t workspace_bytes, void *stream);
int tn_pointcloud_normals(const float *positions, const int32_t *neighbor_index, int64_t num_points, int32_t k,
                          const float *viewpoints, float *normals, void *stream);

/* Mesh export(what nerfstudio's TSDF exporter does with rendered depth, plus a temperature per vertex): rendered poses are
 * fused into a voxel volume, and the volume becomes an indexed triangle list by SURFACE NETS — one vertex per sign-changing
 * cell, one quad per sign-changing grid edge.  Every step is one correctly rounded fp32 operation in the order and association
 * written, `/` and sqrt included.
 *
 * The volume: one contiguous float [7, Nz, Ny, Nx], zeroed by the caller; voxel (i, j, k) of a plane sits at (k Ny + j) Nx + i.
 * Planes: 0 tsdf_sum, 1 weight, 2 thermal_sum, 3..5 r / g / b_sum, 6 colour_weight (weights are fp32 counts).  Grid point
 * (i, j, k) is at p[c] = lo[c] + float(idx[c]) * step[c]; (Nx, Ny, Nz) = dims, every one >= 2 (TN_ERR_SHAPE otherwise) and
 * Nx Ny Nz <= 2^31 - 1 (TN_ERR_UNSUPPORTED beyond: vertex indices are int32).
 *
 * tn_tsdf_integrate fuses ONE pose: depth / accumulation / thermal [height * width] and rgb [height * width, 3] device floats as
 * RayRenderEngine.render leaves them (4-byte alignment is all that is assumed), a PINHOLE camera fx, fy, cx, cy and
 * w2c = [R^T | -R^T t] (row-major 3 x 4) of its camera-to-world [R | t].  Per voxel, m = w2c:
 *     q[r] = ((m[r][0] * p[0] + m[r][1] * p[1]) + m[r][2] * p[2]) + m[r][3],  r = 0..2
 *     zc = -q[2]                                  (the camera looks along -z);  skipped unless zc > 0
 *     u = (fx * q[0]) / zc + cx;   v = (fy * -q[1]) / zc + cy;   skipped unless 0 <= u < width and 0 <= v < height
 *     pix = int(v) * width + int(u)               (the nearest pixel, centres at +0.5; never bilinear)
 *     skipped unless accumulation[pix] > min_accumulation
 *     dist = sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);   sdf = depth[pix] - dist    (depth is a distance along the ray)
 *     skipped unless sdf >= -truncation and sdf < +inf
 *     tsdf_sum += min(1, sdf * inv_truncation);   weight += 1
 *     if sdf <= truncation:  thermal_sum += thermal[pix];  r/g/b_sum += rgb[pix][c];  colour_weight += 1
 *   A NaN makes a comparison false (skipped); a skipped voxel writes nothing.  One launch on `stream`, one thread per voxel.
 *
 * tn_mesh_extract.  A grid point is OBSERVED iff weight > 0, its value is f = tsdf_sum / weight, it is INSIDE iff observed
 * and f < 0.  Cells are (Nx-1)(Ny-1)(Nz-1), x fastest; a cell is ACTIVE iff its 8 corners are all observed and neither all
 * inside nor all outside.  A CROSSING edge: both ends observed, different insideness.
 *   Vertices, one per active cell in ascending cell order; cell_index[cell] (the first int32 per cell of the workspace) = its
 *   vertex index or -1, written for EVERY cell.  For cell (i, j, k), walk its 12 edges — axis a = 0, 1, 2, and within an axis the
 *   offsets on the two other axes (ascending) run (0,0) (1,0) (0,1) (1,1) — with s[0..2] = 0, n = 0, and for each crossing edge
 *   from corner A to B = A + e_a:   s[a] += f_A / (f_A - f_B);  s[other] += offset (0 or 1);  n += 1.  Then
 *     local[c] = s[c] / n;   p[c] = lo[c] + (float(idx[c]) + local[c]) * step[c]
 *     positions[k][c]   = ((M[c][0] * p[0] + M[c][1] * p[1]) + M[c][2] * p[2]) + M[c][3],  M = to_world
 *   attributes: planes 2..6 each summed over the 8 corners from 0, x-fastest corner order; mean = sum / summed colour_weight;
 *     temperature[k]    = mean_thermal * temperature_span + temperature_min
 *     colors[k]         = TN_FRAME_SCALE of the mean rgb;  thermal_colors[k] = TN_FRAME_LUT of mean_thermal (may be NULL)
 *   Triangles, in ascending (grid point, axis) order: for grid point p and axis a, with b = (a+1)%3, c = (a+2)%3, the edge
 *   p -> p + e_a gives a quad iff it is crossing and the four cells at offsets (-1,-1) (0,-1) (0,0) (-1,0) in (b, c) from p's own
 *   cell coordinates all exist and are active; v0..v3 = their cell_index in that order, reversed to v0 v3 v2 v1 when p + e_a is
 *   the inside end (normals point from inside to outside); two triangles (v0 v1 v2), (v0 v2 v3).
 *   counts[0], counts[1] (device int64) are OVERWRITTEN with the full numbers of vertices and triangles; vertex data is written
 *   only below capacity_vertices, triangles only below capacity_triangles (both 0 with NULL outputs: the sizing call).
 * positions [capacity_vertices, 3] floats, colors / thermal_colors [., 3] bytes, temperature floats, triangles
 * [capacity_triangles, 3] int32.  workspace: tn_mesh_workspace_bytes(Nx, Ny, Nz) bytes, 8-byte aligned.  Six launches on
 * `stream` (count, one-block scan, emit; twice), no atomics, no host synchronisation, no allocation; no block waits for another.
 * tn_mesh_tile / tn_mesh_scan_width: cells or grid points per tile, tile counts per pass of the scan block (for tests).
 * TN_ERR_NULL: a required pointer is NULL (outputs are required when their capacity > 0, the table with thermal_colors);
 * TN_ERR_SHAPE: a dim < 2, height or width < 1, a negative capacity, a misaligned pointer; TN_ERR_WORKSPACE: workspace_bytes
 * too small.  All are returned before any launch. */
typedef struct tn_mesh_params {
    float fx, fy, cx, cy;
    float w2c[12]; /* row-major 3 x 4 */
    float truncation, inv_truncation, min_accumulation;
    float lo[3], step[3];
    int32_t dims[3]; /* Nx, Ny, Nz */
    float temperature_span, temperature_min;
    float to_world[12]; /* row-major 3 x 4 */
} tn_mesh_params;
int32_t tn_mesh_tile(void);
int32_t tn_mesh_scan_width(void);
size_t tn_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int tn_tsdf_integrate(const float *depth, const float *accumulation, const float *thermal, const float *rgb, int32_t height,
                      int32_t width, const tn_mesh_params *params, float *volume, void *stream);
int tn_mesh_extract(const float *volume, const tn_mesh_params *params, const uint8_t *thermal_table, float *positions,
                    uint8_t *colors, float *temperature, uint8_t *thermal_colors, int64_t capacity_vertices, int32_t *triangles,
                    int64_t capacity_triangles, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);

/* Connected components of an indexed triangle list and the removal of small ones (what a viewer's "remove small connected
 * components" does to the islands a TSDF volume makes of floaters).  triangles: [T, 3] device int32, V = num_vertices,
 * T = num_triangles.  Every output is an integer defined to the bit.
 *   A triangle is VALID iff its three indices are all in [0, V).  An invalid triangle connects nothing and is never emitted; a
 *   valid one with a repeated index still connects and is still counted.
 *   Two vertices are CONNECTED iff a chain of valid triangles joins them, consecutive triangles sharing at least ONE vertex: this
 *   is vertex connectivity, not edge adjacency — a floater that touches the wall at one vertex is part of the wall — and it is
 *   what an indexed list makes cheap (a triangle unites its three indices; no edge table).
 * tn_mesh_components:
 *   labels[v] (int32 [V]): the smallest vertex index in v's component; a vertex in no valid triangle is its own component.
 *   component_triangles[r] (int32 [V]): where labels[r] == r, the number of valid triangles whose FIRST index has label r; 0 at
 *   every other r.
 *   summary (device int64 [3], OVERWRITTEN): [0] the number of components (labels[v] == v), isolated vertices included; [1] the
 *   largest component_triangles value; [2] the label that holds it, the lowest label on a tie.  With T == 0 or no valid triangle
 *   [1] is 0 and [2] is 0.
 * tn_mesh_filter_components, on the three outputs above.  A component is KEPT iff
 *     component_triangles[label] >= max(min_triangles, 1)   and   (largest_only == 0 or label == summary[2])
 *   (summary is read on the device; it may be NULL iff largest_only == 0).  A vertex is kept iff its component is — a vertex in no
 *   triangle therefore always goes —, a triangle iff it is valid and its component is kept.
 *   vertex_source (int32 [capacity_vertices]): the old indices of the kept vertices, ascending.
 *   triangles_out (int32 [capacity_triangles, 3]): the kept triangles in their input order, every index rewritten to its rank among
 *   the kept vertices.
 *   counts (device int64 [2], OVERWRITTEN): the full numbers of kept vertices and kept triangles; writes happen only below the
 *   capacities (both 0 with NULL outputs: the sizing call).
 *   workspace: tn_mesh_components_workspace_bytes(V, T) bytes, 8-byte aligned; its first int32 per vertex is vertex_map (the new
 *   index or -1).
 * Labelling is a lock-free union-find (hook with compare-and-swap of the higher root under the lower, path halving), then a
 * flatten pass; thermo_nerf_amd/csrc/tn_mesh_components.hip and DESIGN.md state why it ends and why the labels do not depend on
 * the schedule.  At most six launches each on `stream` (tn_mesh_components: init, hook, flatten, count, summarise, unpack; the
 * filter: count, one-block scan, emit, twice, with the tile and scan widths of tn_mesh_tile / tn_mesh_scan_width), no host
 * synchronisation, no allocation.  Integer atomics only (compare-and-swap, add, a 64-bit max of (count << 32) | (0x7fffffff -
 * label)); no block waits for another, and nothing in any output depends on the order of arrival.
 * TN_ERR_NULL: a required pointer is NULL (summary of tn_mesh_components and counts always; labels, component_triangles and the
 * workspace when V > 0; triangles when T > 0; an output when its capacity > 0; summary with largest_only); TN_ERR_SHAPE: V or T
 * negative or above 2^31 - 1, a negative capacity or min_triangles, a misaligned pointer; TN_ERR_WORKSPACE: workspace_bytes too
 * small.  All are returned before any launch.  V == 0: TN_OK, summary / counts are zeroed by a memset, nothing else is launched.
 * T == 0 with V > 0: every vertex is its own label.  tn_mesh_components_workspace_bytes is 0 for counts out of range. */
size_t tn_mesh_components_workspace_bytes(int64_t num_vertices, int64_t num_triangles);
int tn_mesh_components(const int32_t *triangles, int64_t num_triangles, int64_t num_vertices, int32_t *labels,
                       int32_t *component_triangles, int64_t *summary, void *stream);
int tn_mesh_filter_components(const int32_t *triangles, int64_t num_triangles, int64_t num_vertices, const int32_t *labels,
                              const int32_t *component_triangles, const int64_t *summary, int64_t min_triangles,
                              int32_t largest_only, int32_t *vertex_source, int64_t capacity_vertices, int32_t *triangles_out,
                              int64_t capacity_triangles, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);

/* Vertex normals and Taubin smoothing of an indexed triangle list, on a device incidence index: per vertex, the list of its incident
 * triangle corners in a fixed order.  A vertex's sum is then one thread's loop over its own list, so every float below is defined to
 * the bit and the same on every run; there are no float atomics.  positions [V, 3] device floats, triangles [T, 3] device int32,
 * V = num_vertices, T = num_triangles; CORNER c = 3 t + j is index j of triangle t.  add / sub / mul / div / sqrt below are single
 * correctly rounded fp32 operations, nothing is contracted.
 * tn_mesh_incidence: offsets (int32 [V + 1]) and corners (int32 [3 T]).
 *   A triangle is VALID as in tn_mesh_components: all three indices in [0, V).  A valid triangle with a repeated index is listed
 *   once per corner.
 *   The KEY of corner c is the vertex index it names if its triangle is valid, else V.
 *   corners: the corner numbers 0 .. 3T-1 in ascending key order, equal keys in ascending corner order — tn_sort_pairs with
 *   values_in = NULL over max(1, bit_length(V)) key bits, i.e. numpy's argsort(keys, kind="stable").  The rows at and beyond
 *   offsets[V] therefore hold the corners of the invalid triangles in ascending order: every row is defined.
 *   offsets[v], v = 0 .. V: the number of keys < v (the lower bound in the sorted keys; one thread per v, a binary search).  The
 *   list of vertex v is corners[offsets[v] .. offsets[v + 1]).
 *   V == 0 or T == 0: offsets (V + 1 entries) is zeroed by a memset, nothing is launched, corners is untouched.
 *   workspace: tn_mesh_incidence_workspace_bytes(V, T) device bytes, 8-byte aligned (the keys, the sorted keys, the sort's own
 *   workspace); 0 for counts out of range.  Launches on `stream`: keys, tn_sort_pairs, offsets.
 * tn_mesh_vertex_normals: normals (float [V, 3]), one thread per vertex.
 *   face vector of t: e1 = sub(p1, p0), e2 = sub(p2, p0) per component (p0 p1 p2 = the positions of its indices 0 1 2), then
 *   f = (sub(mul(e1y, e2z), mul(e1z, e2y)), sub(mul(e1z, e2x), mul(e1x, e2z)), sub(mul(e1x, e2y), mul(e1y, e2x))).  Its length is
 *   twice the area (area weighting); it points outward, because the extraction winds its triangles that way; it is exactly 0 for
 *   a repeated index.
 *   vertex sum: s = 0; for the corners of v's list in list order, s_c = add(s_c, f_c) with f of the corner's triangle.
 *   normal: len = sqrt(add(add(mul(sx, sx), mul(sy, sy)), mul(sz, sz))); if len > 0 and len < +inf, n_c = div(s_c, len), otherwise
 *   (0, 0, 0) — which also covers a NaN and a vertex in no valid triangle.
 * tn_mesh_smooth: positions_out (float [V, 3]) = positions_in after `iterations` >= 0 iterations; scratch: float [V, 3].
 *   A PASS with factor k, src -> dst (Jacobi: src is only read, dst only written, one thread per vertex): s = 0, n = 0; for the
 *   corners of v's list in list order, corner (t, j): q = src[t[(j + 1) % 3]], r = src[t[(j + 2) % 3]], s_c = add(add(s_c, q_c),
 *   r_c), n += 2.  If n == 0, dst[v] = src[v].  Otherwise m_c = div(s_c, float(n)) and dst_c = add(p_c, mul(k, sub(m_c, p_c)))
 *   with p = src[v].
 *   Why corner weights: in the interior of a manifold mesh every edge neighbour is met in exactly two triangles, so this is the
 *   uniform umbrella operator; on an open border the two border neighbours weigh half.  No per-vertex de-duplication is needed,
 *   and every value is defined by the list order.
 *   An ITERATION is a pass with lambda, then a pass with mu (Taubin's non-shrinking filter: lambda > 0, mu < -lambda).  Any finite
 *   pair is accepted.  The passes alternate in -> scratch -> out -> scratch -> out ..., so the result is in positions_out for every
 *   iteration count; iterations == 0 is a device copy.  positions_out == positions_in is allowed; otherwise the two must not
 *   overlap, and scratch must overlap neither.  Only positions move: a vertex keeps the colour and temperature it was born with.
 * offsets / corners of the two per-vertex entries are tn_mesh_incidence's of the SAME triangles and V.  The kernels check what they
 * dereference (a list is clipped to [0, 3T], a corner outside it or of an invalid triangle is skipped), so a foreign index gives
 * other numbers, never an access outside the arrays.
 * All launches are plain, 256-thread blocks on `stream`; no allocation, no host synchronisation, no float atomics, and no block
 * ever waits for another (no look-back, no grid barrier, no cooperative launch).  The loop of a vertex is sequential because the
 * sums are ordered by definition: a star of 10^5 corners is 10^5 steps of one thread (a surface-nets vertex has 4 - 8).
 * TN_ERR_NULL: a required pointer is NULL (offsets always for tn_mesh_incidence, and with V > 0 and T > 0 triangles, corners, the
 * workspace; for the other two, with V > 0: positions, offsets, the output, and with T > 0 triangles and corners; scratch with
 * V > 0 and iterations > 0); TN_ERR_SHAPE: V < 0 or > 2^31 - 1, T < 0 or 3T > 2^31 - 1, iterations < 0, a pointer not 4-byte
 * aligned, the workspace not 8-byte aligned, buffers of tn_mesh_smooth that overlap; TN_ERR_UNSUPPORTED: lambda or mu not finite;
 * TN_ERR_WORKSPACE: workspace_bytes too small.  All are returned before any launch.  V == 0: TN_OK, nothing is launched. */
size_t tn_mesh_incidence_workspace_bytes(int64_t num_vertices, int64_t num_triangles);
int tn_mesh_incidence(const int32_t *triangles, int64_t num_triangles, int64_t num_vertices, int32_t *offsets, int32_t *corners,
                      void *workspace, size_t workspace_bytes, void *stream);
int tn_mesh_vertex_normals(const float *positions, const int32_t *triangles, int64_t num_triangles, int64_t num_vertices,
                           const int32_t *offsets, const int32_t *corners, float *normals, void *stream);
int tn_mesh_smooth(const float *positions_in, const int32_t *triangles, int64_t num_triangles, int64_t num_vertices,
                   const int32_t *offsets, const int32_t *corners, int32_t iterations, float lambda, float mu, float *positions_out,
                   float *scratch, void *stream);

/* The NaN-aware smoothing of a per-vertex scalar and its surface gradient (degrees Celsius per world unit: where the temperature
 * changes fastest), on tn_mesh_incidence's lists: offsets / corners are tn_mesh_incidence's of the SAME triangles and V.  positions
 * [V, 3] floats, values [V] floats, triangles [T, 3] int32, V = num_vertices, T = num_triangles.  Every output is defined to the bit.
 * add / sub / mul / div / sqrt below are single correctly rounded fp64 operations, nothing is contracted; (double) of a float is
 * exact, (float) of a double rounds to nearest even.  FINITE: neither a NaN nor an infinity.
 * tn_mesh_scalar_smooth: values_out (float [V]) = values_in after `iterations` >= 0 iterations; scratch: float [V].
 *   A PASS with factor k, src -> dst (Jacobi: src is only read, dst only written, one thread per vertex): s = +0.0, n = 0; for the
 *   corners of v's list in list order, corner (t, j) — skipped, as in tn_mesh_smooth, when it lies outside [0, 3T) or its triangle
 *   is not VALID (all three indices in [0, V)) —: q = src[t[(j + 1) % 3]], r = src[t[(j + 2) % 3]]; for each of the two that is
 *   finite, q first: s = add(s, (double)x), n += 1.  With p = src[v]:
 *     n == 0                       dst[v] = p, the same bits
 *     otherwise m = div(s, (double)n), and
 *       p finite                   dst[v] = (float)add((double)p, mul((double)k, sub(m, (double)p)))
 *       p not finite, fill != 0    dst[v] = (float)m
 *       p not finite, fill == 0    dst[v] = p, the same bits
 *   A value that is not finite is never a partner: a NaN spreads nowhere, and with `fill` a hole closes by one ring of vertices
 *   per pass — each pass reads only src, so the order in which it closes depends on no schedule.  A vertex in no valid triangle
 *   and an island all of whose vertices lack a value stay as they are.
 *   An ITERATION is a pass with lambda, then a pass with mu; with mu == 0 it is the pass with lambda alone (plain diffusion, the
 *   low-pass a noisy scalar wants; the pair with lambda > 0, mu < -lambda is Taubin's filter, which keeps amplitudes).  Any finite
 *   pair is accepted.  lambda == 0 and mu == 0 with `fill` fills the holes and moves no other value: add(p, mul(0, d)) is the
 *   number p for finite p and d (p == -0.0 becomes +0.0 where the product is +0.0; every other p keeps its bits).
 *   The passes alternate in -> scratch -> out -> scratch -> out ...; where their number is odd a device copy scratch -> out follows
 *   the last, so the result is in values_out for every count; iterations == 0 is a device copy.  values_out == values_in is
 *   allowed; otherwise the two must not overlap, and scratch must overlap neither.
 * tn_mesh_scalar_gradient: the gradient of the piecewise linear interpolant of `values`, per face and per vertex.
 *   face t is loaded as tn_mesh_regions loads it: VALID, the indices distinct, e1 = sub(p1, p0), e2 = sub(p2, p0), the face vector
 *   n = e1 x e2 = (sub(mul(e1y, e2z), mul(e1z, e2y)), sub(mul(e1z, e2x), mul(e1x, e2z)), sub(mul(e1x, e2y), mul(e1y, e2x))) and
 *   n2 = add(add(mul(nx, nx), mul(ny, ny)), mul(nz, nz)), all in fp64.
 *     USABLE    valid, the indices distinct, all nine coordinates finite, the three values u0 u1 u2 finite, n2 > 0 and n2 < +inf.
 *     g         a = sub((double)u1, (double)u0), b = sub((double)u2, (double)u0); A = e2 x n and B = n x e1, every component
 *               sub(mul, mul) in the component order of n above (Ax = sub(mul(e2y, nz), mul(e2z, ny)), Bx = sub(mul(ny, e1z),
 *               mul(nz, e1y)), ...); g_c = div(add(mul(a, A_c), mul(b, B_c)), n2).  In exact arithmetic g . e1 = u1 - u0,
 *               g . e2 = u2 - u0 and g . n = 0.
 *     |x|       of a vector x: sqrt(add(add(mul(xx, xx), mul(xy, xy)), mul(xz, xz)))
 *     w         sqrt(n2), twice the area
 *   face_gradient (double [T, 3], may be NULL): g of a usable face; the row of every other face is three times the NaN
 *               0x7ff8000000000000.
 *   vertex_gradient (float [V, 3]), vertex_magnitude (float [V]), one thread per vertex: S = (+0.0, +0.0, +0.0), W = +0.0; for
 *               the corners of v's list in list order (a corner outside [0, 3T) is skipped) whose face is usable: S_c = add(S_c,
 *               mul(w, g_c)), W = add(W, w).  (A face is listed once per corner, and a usable face has no repeated index.)  With no
 *               usable face: the NaN 0x7fc00000 in all four floats.  Otherwise G_c = div(S_c, W), vertex_gradient[v] = (float)G_c
 *               and vertex_magnitude[v] = (float)|G|.
 *   totals (double [4], OVERWRITTEN): [0] the number of usable faces, [1] SUM2(w_f), [2] SUM2(mul(w_f, |g_f|)), [3] the largest
 *               |g_f| of a usable face, +0.0 if there is none.  SUM2 is the ordered sum of tn_mesh_regions over the list of ALL T
 *               faces in ascending face index — consecutive blocks of 256 faces, each accumulated from +0.0, then the block sums
 *               from +0.0 in block order — in which a face that is not usable stands for +0.0.  [2] / [1] is the area-weighted
 *               mean of |g|.  T == 0: all four are +0.0 (a memset).
 *   How: one thread per face writes the row and a 32-byte record (w, w |g|, |g|, 1); one thread per vertex walks its list and
 *   recomputes the gradient of each corner's face from the positions and the values (measured against reading the rows back:
 *   profiles/micro/mesh_gradient.txt); one thread per 256 faces joins their records, one thread the partials.  workspace:
 *   tn_mesh_scalar_gradient_workspace_bytes(V, T) device bytes, 8-byte aligned (the records and the partials); 0 for counts out of
 *   range, positive otherwise.
 * The kernels check what they dereference (a list is clipped to [0, 3T], a corner outside it or of an invalid triangle is skipped, a
 * vertex is read only where the face's indices allow it), so a foreign index gives other numbers, never an access outside the arrays.
 * All launches are plain, 256-thread blocks on `stream`; no allocation, no host synchronisation, no float atomics, and no block
 * ever waits for another.
 * TN_ERR_NULL: a required pointer is NULL (tn_mesh_scalar_smooth, with V > 0: values_in, offsets, values_out, with T > 0 triangles
 * and corners, scratch with iterations > 0; tn_mesh_scalar_gradient: totals always; with V > 0 positions, values, offsets,
 * vertex_gradient, vertex_magnitude; with T > 0 triangles and the workspace; with V > 0 and T > 0 corners); TN_ERR_SHAPE: V < 0 or
 * > 2^31 - 1, T < 0 or 3T > 2^31 - 1, iterations < 0 or > 2^30 - 1, a float / int32 pointer not 4-byte aligned, face_gradient /
 * totals / workspace not 8-byte aligned, buffers of tn_mesh_scalar_smooth that overlap; TN_ERR_UNSUPPORTED: lambda or mu not finite;
 * TN_ERR_WORKSPACE: workspace_bytes too small (with T > 0).  All are returned before any launch.  tn_mesh_scalar_smooth with
 * V == 0: TN_OK, nothing is launched.  tn_mesh_scalar_gradient: the faces and the totals are launched with T > 0 (V == 0: no face
 * is usable), the vertices with V > 0 (T == 0: every vertex gets the NaN). */
int tn_mesh_scalar_smooth(const float *values_in, const int32_t *triangles, int64_t num_triangles, int64_t num_vertices,
                          const int32_t *offsets, const int32_t *corners, int32_t iterations, float lambda, float mu, int32_t fill,
                          float *values_out, float *scratch, void *stream);
size_t tn_mesh_scalar_gradient_workspace_bytes(int64_t num_vertices, int64_t num_triangles);
int tn_mesh_scalar_gradient(const float *positions, const float *values, const int32_t *triangles, int64_t num_triangles,
                            int64_t num_vertices, const int32_t *offsets, const int32_t *corners, double *face_gradient,
                            float *vertex_gradient, float *vertex_magnitude, double *totals, void *workspace, size_t workspace_bytes,
                            void *stream);

/* A stable sort of n (uint64 key, int32 value) pairs on the device: a least-significant-digit radix sort, 8 bits per pass.
 *   The ORDERING BITS of a key are its low 8 * ceil(key_bits / 8) bits.  keys_out / values_out hold the input pairs in ascending
 *   order of their ordering bits; pairs whose ordering bits are equal keep their input order (the sort is stable).  Higher key
 *   bits travel with the key and do not order.  The output is therefore unique: with m = keys_in masked to the ordering bits and
 *   o = numpy's argsort(m, kind="stable"), keys_out = keys_in[o] and values_out = values_in[o] — or o itself when values_in is
 *   NULL, which stands for the values 0 .. n-1.
 *   keys_in / values_in are only read and must not overlap the outputs or the workspace.  The result is in keys_out / values_out
 *   for every pass count, odd or even: the ping-pong partner of the output buffers lives in the workspace.
 * workspace: tn_sort_pairs_workspace_bytes(n) device bytes, 8-byte aligned (partner keys and values, 256 counts per tile of
 * tn_sort_tile() keys); it depends on n only.  Three launches per pass on `stream` (per-tile digit histogram, a one-block scan of
 * the 256 * tiles counts, scatter), no allocation, no host synchronisation; no block waits for another (no decoupled look-back, no
 * grid barrier).  The histogram counts with integer LDS atomics; nothing in the output depends on the order of arrival.
 * TN_ERR_UNSUPPORTED: key_bits < 1 or > 64; TN_ERR_SHAPE: n < 0 or n > 2^31 - 1; n == 0: TN_OK, nothing is launched or written;
 * then TN_ERR_NULL: keys_in, keys_out, values_out or workspace is NULL; TN_ERR_SHAPE: a key pointer or the workspace not 8-byte
 * aligned, a value pointer not 4-byte aligned; TN_ERR_WORKSPACE: workspace_bytes too small.  All are returned before any launch.
 * tn_sort_pairs_workspace_bytes is 0 for n < 0 or n > 2^31 - 1. */
int32_t tn_sort_tile(void);
size_t tn_sort_pairs_workspace_bytes(int64_t n);
int tn_sort_pairs(const uint64_t *keys_in, const int32_t *values_in, int64_t n, int key_bits, uint64_t *keys_out,
                  int32_t *values_out, void *workspace, size_t workspace_bytes, void *stream);

/* Voxel down-sampling of a point cloud (the voxel grid filter of open3d / CloudCompare, with a temperature): one output point per
 * occupied voxel, every attribute the mean over the voxel's members, defined to the bit.
 *   parameters   origin[3] floats, voxel_size a float > 0 and finite, dims[3] int32, each in [1, 2^21] (TN_ERR_UNSUPPORTED
 *                otherwise); total = dims_x * dims_y * dims_z (at most 2^63).
 *   coordinate   inv = 1.0 / (double)voxel_size;  u_a = ((double)p_a - (double)origin_a) * inv — fp64, one correctly rounded
 *                operation per step.
 *   member       point i is a MEMBER iff its three coordinates are finite and 0 <= u_a < (double)dims_a on every axis (a NaN
 *                fails); then c_a = (int64)u_a (truncation).  Every other point is dropped.
 *   key          (c_z * dims_y + c_y) * dims_x + c_x; a dropped point gets `total`, which sorts behind every voxel.  The keys are
 *                sorted with the point indices by tn_sort_pairs over key_bits = bit_length(total).
 *   voxel        the members with one key, in ascending point index — the order the stable sort leaves them in.  Voxels are
 *                written in ascending key.
 *   positions_out, temperature_out   per component the fp64 sum from 0 in that order, divided by (double)n (n = the voxel's
 *                members), rounded once to fp32.
 *   colors_out, thermal_colors_out (uint8)   per channel the exact integer sum S, then (2 S + n) / (2 n) in integer division
 *                (round half up).  thermal_colors_out may be NULL, and must be if thermal_colors is.
 *   source_out   the source of the voxel's first member (its lowest point index); may be NULL, and must be if source is.
 *   voxel_count  int32 n per output point.
 *   count[0] (device int64) is OVERWRITTEN with the number of occupied voxels — the FULL number; nothing is written at or beyond
 *   `capacity` (0 with NULL outputs: the sizing call).
 * positions [num_points, 3] floats, colors / thermal_colors [num_points, 3] bytes, temperature [num_points] floats, source
 * [num_points] int64; the outputs likewise over `capacity` rows.  workspace: tn_voxel_downsample_workspace_bytes(num_points) device
 * bytes, 8-byte aligned.  Launches on `stream`: keys, tn_sort_pairs, then the heads of the runs compacted in order (count, one-block
 * scan, emit), then one thread per voxel that walks its run; no atomics, no allocation, no host synchronisation, no block waits
 * for another.  The walk is sequential per voxel (the sums are ordered by definition): a voxel of 10^5 members is 10^5 steps of
 * one thread.
 * TN_ERR_NULL: params or count is NULL; positions, colors, temperature or the workspace with num_points > 0; positions_out,
 * colors_out, temperature_out or voxel_count with capacity > 0; thermal_colors_out without thermal_colors, source_out without
 * source (with num_points > 0); TN_ERR_SHAPE: num_points < 0 or > 2^31 - 1, capacity < 0, a float / int32 pointer not 4-byte aligned, source /
 * source_out / count / workspace not 8-byte aligned; TN_ERR_WORKSPACE: workspace_bytes too small.  All are returned before any
 * launch.  num_points == 0: count[0] is zeroed by a memset, nothing is launched.  tn_voxel_downsample_workspace_bytes is 0 for
 * num_points < 0 or > 2^31 - 1. */
typedef struct tn_voxel_params {
    float origin[3];
    float voxel_size;
    int32_t dims[3];
} tn_voxel_params;
size_t tn_voxel_downsample_workspace_bytes(int64_t num_points);
int tn_voxel_downsample(const float *positions, const uint8_t *colors, const float *temperature, const uint8_t *thermal_colors,
                        const int64_t *source, int64_t num_points, const tn_voxel_params *params, float *positions_out,
                        uint8_t *colors_out, float *temperature_out, uint8_t *thermal_colors_out, int64_t *source_out,
                        int32_t *voxel_count, int64_t capacity, int64_t *count, void *workspace, size_t workspace_bytes, void *stream);

/* Vertex-clustering simplification of an indexed triangle list: the vertices that fall in one cell of a grid become one vertex, the
 * triangles are re-indexed, and those that collapse or repeat go.  positions [V, 3] floats, colors / thermal_colors [V, 3] bytes,
 * temperature [V] floats, triangles [T, 3] int32, V = num_vertices, T = num_triangles.  Every output is defined to the bit.
 *   parameters   tn_voxel_params as in tn_voxel_downsample: origin, voxel_size (the cell edge), dims; the same limits and the same
 *                TN_ERR_UNSUPPORTED.
 *   member, cell, key   exactly tn_voxel_downsample's: u_a = ((double)p_a - (double)origin_a) * (1.0 / (double)voxel_size); a
 *                vertex is a MEMBER iff its three coordinates are finite and 0 <= u_a < dims_a on every axis; c_a = (int64)u_a;
 *                key = (c_z * dims_y + c_y) * dims_x + c_x.  A CLUSTER is the set of members with one key.
 *   triangle     VALID iff its three indices are in [0, V) and all three vertices are members.  Its cluster triple is (A, B, C), the
 *                clusters of its corners in corner order; it is DEGENERATE iff two of them are equal.  Its CANONICAL triple is the
 *                cyclic rotation of (A, B, C) that puts the smallest cluster first; orientation is kept: (A, B, C) and (A, C, B)
 *                are different triples.  Among the valid, non-degenerate triangles with one canonical triple the one with the
 *                lowest input index is KEPT, the others are DUPLICATES.
 *   vertices     a cluster is USED iff a kept triangle names it.  One output vertex per used cluster, in ascending key; an unused
 *                cluster (vertices in no triangle, an island that collapsed into one cell) gives nothing.
 *   positions_out, temperature_out   per component the fp64 sum from 0 over ALL members of the cluster in ascending vertex index
 *                (unreferenced members count too), divided by (double)n, rounded once to fp32.
 *   colors_out, thermal_colors_out (uint8)   per channel the exact integer sum S, then (2 S + n) / (2 n) in integer division
 *                (round half up).  thermal_colors_out may be NULL, and must be if thermal_colors is.
 *   cluster_count   int32 n per output vertex.
 *   triangles_out (int32 [capacity_triangles, 3])   the kept triangles in ascending input index, every corner rewritten to the
 *                output vertex of its cluster; the corner order is the input's, not the canonical rotation.
 *   triangle_source (int32 [capacity_triangles], may be NULL)   the input index of every output triangle.
 *   vertex_map (int32 [V], may be NULL)   per input vertex the output vertex of its cluster; -1 for a non-member and for a member of
 *                an unused cluster.
 *   counts (device int64 [4], OVERWRITTEN)   [0] output vertices, [1] output triangles, [2] triangles dropped as invalid or
 *                degenerate, [3] triangles dropped as duplicates; [1] + [2] + [3] = T.  The FULL numbers: nothing is written at
 *                or beyond a capacity (both 0 with NULL outputs: the sizing call).
 * How: the vertex keys are sorted with the vertex indices by tn_sort_pairs and the heads of the runs compacted (count, one-block
 * scan, emit), which ranks the clusters; one thread per triangle forms the canonical triple of ranks; with b = bit_length(V) the
 * triples are sorted with the triangle indices as ONE key of 3 b + 1 bits if that fits 64 (V < 2^21), otherwise by TWO stable sorts
 * (the third rank, then the first two), so that equal triples are adjacent in ascending triangle index; the head of a run is kept
 * and flags its three clusters; two more compactions (triangles in input order, clusters in key order); one thread per used cluster
 * walks its run for the means.  workspace: tn_mesh_simplify_workspace_bytes(V, T) device bytes, 8-byte aligned; 0 for counts out of
 * range.  Launches on `stream` only: no allocation, no host synchronisation, no float atomics, no block waits for another.  The
 * integer atomics (the sort's LDS histogram, one add per block to counts[2]) and the same-value flag stores leave nothing in any
 * output that depends on the order of arrival.  The walk is sequential per cluster (the sums are ordered by definition): a cluster
 * of 10^5 members is 10^5 steps of one thread.
 * TN_ERR_NULL: params or counts is NULL; positions, colors, temperature or the workspace with V > 0; triangles with T > 0;
 * positions_out, colors_out, temperature_out or cluster_count with capacity_vertices > 0; triangles_out with capacity_triangles > 0;
 * thermal_colors_out without thermal_colors; TN_ERR_SHAPE: V < 0 or > 2^31 - 1, T < 0 or 3T > 2^31 - 1, a negative capacity, a
 * float / int32 pointer not 4-byte aligned, counts / workspace not 8-byte aligned; TN_ERR_WORKSPACE: workspace_bytes too small.
 * All are returned before any launch.  V == 0: TN_OK, counts is zeroed by a memset, nothing is launched (the one case in which the
 * triangles, all of them invalid, are not counted in [2]).  T == 0 with V > 0: counts is zeroed and vertex_map filled with -1, by
 * memsets. */
size_t tn_mesh_simplify_workspace_bytes(int64_t num_vertices, int64_t num_triangles);
int tn_mesh_simplify(const float *positions, const uint8_t *colors, const float *temperature, const uint8_t *thermal_colors,
                     const int32_t *triangles, int64_t num_vertices, int64_t num_triangles, const tn_voxel_params *params,
                     float *positions_out, uint8_t *colors_out, float *temperature_out, uint8_t *thermal_colors_out,
                     int32_t *cluster_count, int64_t capacity_vertices, int32_t *triangles_out, int32_t *triangle_source,
                     int64_t capacity_triangles, int32_t *vertex_map, int64_t *counts, void *workspace, size_t workspace_bytes,
                     void *stream);

/* Thermal regions of an indexed triangle list: the faces whose temperature lies in a window, joined through shared vertices, and per
 * region its area, area-weighted mean temperature and centroid, extremes, bounds and hottest / coldest vertex.  positions [V, 3]
 * floats, temperature [V] floats, triangles [T, 3] int32, V = num_vertices, T = num_triangles.  Every output is defined to the bit.
 * add / sub / mul / div / sqrt below are single correctly rounded fp64 operations, nothing is contracted; (double) of a float is
 * exact, (float) of a double rounds to nearest even.
 *   face t, indices i0 i1 i2, positions p0 p1 p2, temperatures t0 t1 t2:
 *     VALID     all three indices in [0, V).
 *     USABLE    valid, the three indices distinct, all nine coordinates finite, all three temperatures finite.
 *     tf        (float)div(add(add((double)t0, (double)t1), (double)t2), 3.0)
 *     area      e1 = sub(p1, p0), e2 = sub(p2, p0) per component; c = (sub(mul(e1y, e2z), mul(e1z, e2y)), sub(mul(e1z, e2x),
 *               mul(e1x, e2z)), sub(mul(e1x, e2y), mul(e1y, e2x))) — the face vector of tn_mesh_vertex_normals in fp64;
 *               n2 = add(add(mul(cx, cx), mul(cy, cy)), mul(cz, cz)); area = mul(0.5, sqrt(n2)).
 *     centroid  per axis div(add(add(p0, p1), p2), 3.0)
 *     SELECTED  usable and min_temperature <= tf <= max_temperature, compared in fp32.  Either bound may be infinite; min > max
 *               selects nothing.
 *   face_area (double [T], may be NULL): the area of a usable face, +0.0 of every other.
 *   regions     two selected faces that share a vertex are connected (the connectivity of tn_mesh_components, over the selected
 *               faces only).  A region's LABEL is the smallest vertex index among its faces' vertices; regions are numbered
 *               r = 0 .. R-1 in ascending label; a region's faces are taken in ascending face index.
 *   face_region (int32 [T], always fully written): r of a selected face, -1 of every other.
 *   SUM2(list)  the ordered sum: the list is cut into consecutive blocks of 256 entries from its start (the last may be short); each
 *               block is accumulated from +0.0 in list order, s = add(s, x); the block sums are then accumulated from +0.0 in block
 *               order.  (A thread walks 256 entries, then n / 256 partials: one region may be the whole mesh.)
 *   tn_mesh_region, row r of `regions` (72 bytes), over the region's faces f:
 *     area              SUM2(area_f)
 *     label, faces      as above; the number of its faces
 *     mean_temperature  (float)div(SUM2(mul(area_f, (double)tf_f)), area)
 *     centroid[a]       (float)div(SUM2(mul(area_f, centroid_f,a)), area); with area == 0 the mean and the centroid are the NaN
 *                       0x7fc00000
 *     min_temperature, max_temperature   of tf_f;  bounds: min x y z, max x y z over the positions of the region's vertices.  Both
 *                       in the numbers' order with -0.0 below +0.0, so that they do not depend on any order of evaluation.
 *     hottest_vertex    the vertex of the region with the highest temperature, compared as numbers (-0.0 == +0.0), the lowest index
 *                       on a tie; coldest_vertex likewise for the lowest.
 *   totals (double [2], OVERWRITTEN): [0] SUM2 of area_f over the usable faces in ascending face index (the mesh's area), [1] the
 *               same over the selected faces.
 *   counts (device int64 [3], OVERWRITTEN): [0] R — the FULL number; rows at or beyond capacity_regions are not written (0 with
 *               regions NULL: the sizing call) —, [1] the selected faces, [2] the usable faces.
 * How: one thread per face writes a 96-byte record (the five products, tf, the face's box, its hottest and coldest corner) and a
 * copy of the index list in which a face outside the window is invalid; the usable and the selected faces are compacted in order
 * (count, one-block scan, emit); tn_mesh_components labels the copy; tn_sort_pairs of (label, face) puts a region's faces side by side in
 * face order, the regions in ascending label; the first position of every run is numbered by a count / scan / emit over the sorted
 * positions (a region's faces are the distance to the next run), the 256-blocks by one over the regions; one thread per 256-block
 * walks its records into a partial, one thread per region walks its partials; the two totals take the same two steps over the two
 * compacted lists.  workspace: tn_mesh_regions_workspace_bytes(V, T) device bytes,
 * 8-byte aligned; 0 for counts out of range.  Launches on `stream` only: no allocation, no host synchronisation, no float atomics
 * (the integer ones are tn_mesh_components' and the sort's), no block waits for another.  The kernels check what they dereference:
 * a foreign index gives other numbers, never an access outside the arrays.
 * TN_ERR_NULL: counts or totals is NULL; positions, temperature or the workspace with V > 0 and T > 0; triangles or face_region
 * with T > 0; regions with capacity_regions > 0; TN_ERR_SHAPE: V < 0 or > 2^31 - 1, T < 0 or 3T > 2^31 - 1, a negative capacity, a
 * float / int32 pointer not 4-byte aligned, regions / face_area / totals / counts / workspace not 8-byte aligned;
 * TN_ERR_UNSUPPORTED: a NaN bound; TN_ERR_WORKSPACE: workspace_bytes too small (with V > 0 and T > 0).  All are returned before any
 * launch.  V == 0 or T == 0: TN_OK, counts and totals are zeroed, face_region filled with -1 and face_area with +0.0 by memsets,
 * nothing is launched. */
typedef struct tn_mesh_region {
    double area;
    int32_t label;
    int32_t faces;
    float mean_temperature;
    float min_temperature, max_temperature;
    float centroid[3];
    float bounds[6];
    int32_t coldest_vertex, hottest_vertex;
} tn_mesh_region;
size_t tn_mesh_regions_workspace_bytes(int64_t num_vertices, int64_t num_triangles);
int tn_mesh_regions(const float *positions, const float *temperature, const int32_t *triangles, int64_t num_vertices,
                    int64_t num_triangles, float min_temperature, float max_temperature, tn_mesh_region *regions,
                    int64_t capacity_regions, int32_t *face_region, double *face_area, int64_t *counts, double *totals,
                    void *workspace, size_t workspace_bytes, void *stream);

/* Orthographic thermogram of an indexed triangle list: a z-buffered rasteriser.  Every pixel of the image has a known size in world
 * units, the face it shows, its depth, its temperature and (optionally) its colour.  positions [V, 3] floats, temperature [V] floats,
 * colors [V, 3] bytes (may be NULL), triangles [T, 3] int32, V = num_vertices, T = num_triangles; `view` is read on the HOST.  Every
 * output is defined to the bit.  add / sub / mul / div below are single correctly rounded fp64 operations, nothing is contracted;
 * (double) of a float is exact, (double) of an int64 and (float) of a double round to nearest even.
 *   tn_raster_view: `origin` is the world position of the top-left CORNER of pixel (row 0, col 0) on the image plane; `right`, `down`
 *     and `forward` are unit and orthogonal with right x down = forward and are TAKEN AS GIVEN; `pixel_size` world units per pixel;
 *     faces are kept where near <= z <= far (either may be infinite; near > far keeps nothing); width, height in 1 .. 16384; cull 0:
 *     both sides, 1: faces seen from behind are dropped; reserved: 0, or — for measurements only, it cannot change a bit of the output
 *     — the small / large box threshold to use in place of tn_mesh_raster_small_box(), 1 .. 16384.
 *   vertex p:
 *     q = sub((double)p, origin) per component
 *     x = div(add(add(mul(qx, rx), mul(qy, ry)), mul(qz, rz)), pixel_size) with r = right; y the same with down; z the same with
 *         forward, without the division
 *     X = (int64) of mul(x, 256.0) rounded half to even, Y likewise: fixed point with 8 sub-pixel bits
 *     RASTERABLE  x, y and z finite, |mul(x, 256.0)| <= 2^29 and |mul(y, 256.0)| <= 2^29 (every edge function below then fits an int64
 *         exactly)
 *   face t, indices i0 i1 i2:
 *     VALID   all three indices in [0, V).   USABLE  valid, the three indices distinct, all three temperatures finite, all three
 *             vertices rasterable.
 *     area2   (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0), exact.  area2 > 0: the normal (p1 - p0) x (p2 - p0) points along `forward`, away
 *             from the viewer.
 *     DRAWN   usable, area2 != 0, and not (cull == 1 and area2 > 0).
 *     If area2 < 0 the face's second and third vertex are exchanged, with everything that belongs to them, and area2 is negated: from
 *     here on area2 > 0 and the vertices are v0 v1 v2.
 *   coverage of pixel (row j, col i), centre P = (256 i + 128, 256 j + 128):
 *     E(a, b) = (bx - ax)(Py - ay) - (by - ay)(Px - ax);  w0 = E(v1, v2), w1 = E(v2, v0), w2 = E(v0, v1)  (w0 + w1 + w2 = area2)
 *     the pixel is COVERED when for every k: wk > 0, or wk == 0 and that edge a -> b is top-left: by - ay < 0, or by - ay == 0 and
 *     bx - ax > 0.  A pixel centre on an edge shared by two faces, of either winding, belongs to exactly one of them.
 *   depth and attributes of a covered pixel:
 *     lk = div((double)wk, (double)area2);  B(a0, a1, a2) = add(add(mul(l0, a0), mul(l1, a1)), mul(l2, a2))
 *     zp = B(z0, z1, z2); the sample is DROPPED unless near <= zp <= far, compared in fp64
 *     depth = (float)zp, with -0.0 written as +0.0;  temperature = (float)B((double)t0, (double)t1, (double)t2)
 *     colour channel c = floor(add(B((double)c0, (double)c1, (double)c2), 0.5)) clamped to [0, 255]
 *   winner: key = (ord(depth) << 32) | t, ord the order-preserving map of fp32 bits to uint32 (b -> ~b with the sign bit set, b |
 *     0x80000000 without), t the face's index in the list AS GIVEN.  The pixel shows the sample with the smallest key: the nearest
 *     surface, and on equal fp32 depth the lowest face index.  A minimum does not depend on the order in which it is taken.
 *   outputs, row-major [height, width], each of the four pixel arrays may be NULL:
 *     pixel_face (int32)   the face index; -1 on an empty pixel
 *     pixel_depth, pixel_temperature (float)   the NaN 0x7fc00000 on an empty pixel
 *     pixel_colors (uint8 [H, W, 3])   0 on an empty pixel; must be NULL when colors is NULL
 *     counts (device int64 [3], OVERWRITTEN)   [0] covered pixels, [1] drawn faces, [2] usable faces
 *     stats (device double [3], OVERWRITTEN)   [0] SUM2, as tn_mesh_regions defines it (blocks of 256), over ALL pixels in row-major
 *         order of (double)temperature, an empty pixel contributing +0.0; [1], [2] the minimum and the maximum of (double)temperature
 *         over the covered pixels in the numbers' order with -0.0 below +0.0; +inf and -inf without a covered pixel.
 * How: one thread per face transforms its vertices, classifies it, writes a 72-byte record (the fixed-point corners, the three
 * depths, area2, the indices after the exchange) and clips its box of pixel centres to the image.  A face whose box is at most
 * tn_mesh_raster_small_box() pixels on both sides is rasterised by that thread, straight into a uint64 key plane in the workspace
 * with a 64-bit integer atomic minimum; a plain load of the current key skips the atomic when the sample cannot win (a minimum
 * only falls).  The faces with a larger box are compacted in face order (count, one-block scan, emit) and swept in 16 x 16 pixel
 * tiles by blocks of 256 threads, a tile being skipped whole when one edge function is negative at its four corners.  A resolve
 * pass, one thread per pixel, decodes the key, recomputes the barycentrics from the record and writes the four arrays and one
 * partial per 256 pixels; one block finishes SUM2, the extremes and the covered count.  workspace:
 * tn_mesh_rasterize_workspace_bytes(T, width, height) device bytes, 8-byte aligned; 0 for arguments out of range.  Launches on
 * `stream` only: no allocation, no host synchronisation, no float atomics, no block waits for another.  The kernels check what they
 * dereference: a foreign index gives an unusable face, never an access outside the arrays.
 * TN_ERR_NULL: view, counts or stats is NULL; positions, temperature or the workspace with V > 0 and T > 0; triangles with T > 0;
 * colors with pixel_colors; TN_ERR_SHAPE: V < 0 or > 2^31 - 1, T < 0 or 3T > 2^31 - 1, width or height outside 1 .. 16384,
 * pixel_size not a finite positive number, a non-finite origin or axis component, a float / int32 pointer not 4-byte aligned, counts /
 * stats / workspace not 8-byte aligned; TN_ERR_UNSUPPORTED: a NaN near or far, cull outside {0, 1}, reserved outside 0 .. 16384;
 * TN_ERR_WORKSPACE: workspace_bytes too small (with V > 0 and T > 0).  All are returned before any launch, in the siblings' order:
 * NULL of view / counts / stats, SHAPE of the numbers, UNSUPPORTED, NULL of the arrays, SHAPE of the alignment, WORKSPACE.
 * V == 0 or T == 0: TN_OK, the pixel arrays are filled with their empty values, counts are zeroed, stats = (+0.0, +inf, -inf). */
typedef struct tn_raster_view {
    double origin[3];
    double right[3], down[3], forward[3];
    double pixel_size;
    double near, far;
    int32_t width, height;
    int32_t cull;
    int32_t reserved;
} tn_raster_view;
int32_t tn_mesh_raster_small_box(void);
size_t tn_mesh_rasterize_workspace_bytes(int64_t num_triangles, int32_t width, int32_t height);
int tn_mesh_rasterize(const float *positions, const float *temperature, const uint8_t *colors, const int32_t *triangles,
                      int64_t num_vertices, int64_t num_triangles, const tn_raster_view *view, int32_t *pixel_face, float *pixel_depth,
                      float *pixel_temperature, uint8_t *pixel_colors, int64_t *counts, double *stats, void *workspace,
                      size_t workspace_bytes, void *stream);

/* Ray queries against an indexed triangle list: a linear bounding-volume hierarchy (LBVH) built on the device, and a traversal that
 * gives every ray the face it meets first, where, and the temperature and colour there.  positions [V, 3] floats, temperature [V]
 * floats, colors [V, 3] bytes (may be NULL), triangles [T, 3] int32, V = num_vertices, T = num_triangles.  Every output is defined to
 * the bit, and WITHOUT reference to the tree.  add / sub / mul / div below are single correctly rounded fp64 operations, nothing is
 * contracted; (double) of a float is exact, (float) of a double rounds to nearest even.  min and max of floats are taken in the
 * numbers' order with -0.0 below +0.0.
 *   face t, indices i0 i1 i2:
 *     USABLE  all three indices in [0, V) and distinct, the nine coordinates finite, the three temperatures finite (tn_mesh_rasterize's
 *             USABLE without "rasterable").
 *     box     lo = min, hi = max of its three fp32 corners per axis: exact.
 *
 * THE BLOB (tn_mesh_bvh_build writes it, tn_mesh_raycast reads it; tn_mesh_bvh_bytes(T) = 64 + 64 ceil(4 T / 64) + 64 max(T - 1, 0)
 * device bytes, 64-byte aligned; little endian):
 *   header, 64 bytes   uint32 magic 0x56424e54; int32 version 1; int32 num_faces = T; int32 num_usable = U; int32 num_unusable = T - U;
 *                      int32 num_nodes = max(U - 1, 0); int32 root; int32 depth; float lo[3], hi[3]: the EXTENT, min of lo and max of hi
 *                      over the usable faces (+inf and -inf when U == 0); two zero int32.
 *                      root: U >= 2: 0, the internal node 0; U == 1: -1, the leaf 0; U == 0: INT32_MIN, there is nothing to meet.
 *                      depth: the height of the root (the internal nodes on the longest way down to a leaf); 0 when U < 2.
 *   faces              int32 [T], padded with zeros to a multiple of 64 bytes: the face indices in LEAF ORDER — ascending key, equal
 *                      keys in ascending face index (tn_sort_pairs over 31 bits).  The first U are the usable faces, leaf k is faces[k].
 *   nodes              [max(T - 1, 0)] x 64 bytes, the first num_nodes are the tree, the rest are zero:
 *                      float lo[2][3], hi[2][3]: the boxes of child 0 and of child 1; int32 child[2]: c >= 0 is the internal node c,
 *                      c < 0 the leaf ~c; int32 level: the node's height, 1 + the larger of its children's, a leaf being 0; a zero int32.
 *                      The box of a leaf is its face's; the box of an internal node is the min / max of its two children's boxes.
 *   key of a face      usable: the 30-bit Morton code of q, bit 3 b + 2 - k of the code = bit b of q_k (k = 0 x, 1 y, 2 z), with
 *                      c_k = mul(add((double)lo_k, (double)hi_k), 0.5) the box centre, w_k = sub((double)HI_k, (double)LO_k) the
 *                      extent's width, q_k = 0 when w_k == 0, else floor(mul(div(sub(c_k, (double)LO_k), w_k), 1024.0)) clamped to
 *                      [0, 1023].  Unusable: 2^30, above every code.
 *   tree               Karras's radix tree (Maximizing parallelism in the construction of BVHs, octrees and k-d trees, 2012) over the
 *                      first U entries of the leaf order with delta(i, j) = clz32(key_i ^ key_j) for different keys and
 *                      32 + clz32(i ^ j) for equal ones (i, j positions in the leaf order): all keys are distinct, the tree is unique.
 *                      Internal node i covers the positions first .. last, one of them i; child 0 covers first .. split, child 1
 *                      split + 1 .. last; a child that covers one position is that leaf, otherwise child 0 is node split and child 1
 *                      node split + 1.
 *   DEPTH BOUND        tn_mesh_bvh_depth_bound() = 61.  Proof: delta(first, last) of a node is the length of the common prefix of the
 *                      (key, position) strings it covers, and it grows strictly from a node to its internal child.  Between different
 *                      keys it is clz32 of a non-zero number below 2^30: one of the 30 values 2 .. 31.  Between equal keys it is
 *                      32 + clz32 of a non-zero number below 2^31: one of the 31 values 33 .. 63.  A way down passes at most 30 + 31
 *                      internal nodes.
 *   The blob is deterministic: two builds of one mesh are byte-equal.
 * How it is built: one thread per face classifies it and folds its box into the extent (a wave's minimum first, then integer atomic
 * min / max on the order-preserving bit patterns of the floats; no float atomics); one thread per face computes its key; tn_sort_pairs
 * writes the leaf order into the blob; one thread per internal node finds its range and split; then tn_mesh_bvh_depth_bound()
 * launches fit the boxes bottom-up: in launch p a node whose two children were done BEFORE the launch (a leaf always is; an internal
 * child carries a level in 1 .. p - 1) takes their boxes and the level p, so level = height.  Launch boundaries carry the data
 * between blocks: no block hands data to another inside a launch, nothing waits, there is no fence.  workspace:
 * tn_mesh_bvh_workspace_bytes(T) device bytes, 8-byte aligned.  Launches on `stream` only, no allocation, no host synchronisation.
 * tn_mesh_bvh_build: TN_ERR_NULL: bvh; TN_ERR_SHAPE: V < 0 or > 2^31 - 1, T < 0 or 3T > 2^31 - 1; TN_ERR_NULL: with T > 0 triangles
 * or the workspace, with T > 0 and V > 0 positions or temperature; TN_ERR_SHAPE: a float / int32 pointer not 4-byte aligned, bvh not
 * 64-byte aligned, the workspace not 8-byte aligned; TN_ERR_WORKSPACE: bvh_bytes or workspace_bytes too small.  All are returned
 * before any launch.  T == 0: TN_OK, the header alone is written.  Both size functions are 0 for T out of range.
 *
 * THE CAST.  origins, directions [N, 3] floats, ray_t_max [N] floats or NULL, N = num_rays, 3N <= 2^31 - 1; `params` is read on the HOST:
 * 0 <= t_min, t_max may be +inf (t_min > t_max meets nothing); cull 0: both sides, 1: faces seen from behind are dropped; mode
 * TN_RAYCAST_CLOSEST or TN_RAYCAST_ANY.
 *   ray i     USABLE when its six floats are finite and its direction is not (0, 0, 0).  o, d = (double) of them; directions are NOT
 *             normalised, t is in units of the direction.  t_end = t_max, or with ray_t_max: r = (double)ray_t_max[i],
 *             t_end = r < t_max ? r : t_max (a NaN leaves t_max).  An unusable ray is a miss.
 *   slab of the ray against a box lo .. hi, per axis k:
 *             d_k == 0: the axis PASSES iff lo_k <= o_k <= hi_k, and gives no bound.  Otherwise inv_k = div(1, d_k),
 *             a = mul(sub(lo_k, o_k), inv_k), b = mul(sub(hi_k, o_k), inv_k), near_k = min(a, b), far_k = max(a, b).
 *             enter = max(t_min, near_k ...), exit = min(t_end, far_k ...), s = mul(enter, 1 - 2^-32).
 *             The box PASSES iff every zero axis passes and s <= exit.  (The slack does real work: rays through the vertices and
 *             edge midpoints of an axis-aligned cube graze boxes of zero thickness, where the rounding of a and b can put enter
 *             above exit by an ulp; without the slack thousands of true hits of such a scene fail the test, with it none.)
 *   face test, Moeller-Trumbore in fp64 with p0 p1 p2 = (double) of the corners, dot(a, b) = add(add(mul(ax, bx), mul(ay, by)),
 *             mul(az, bz)), cross(a, b) = (sub(mul(ay, bz), mul(az, by)), sub(mul(az, bx), mul(ax, bz)), sub(mul(ax, by), mul(ay, bx))):
 *             e1 = sub(p1, p0), e2 = sub(p2, p0), pv = cross(d, e2), det = dot(e1, pv).  det == 0 is a miss.  det = -dot(d, n) with
 *             n = (p1 - p0) x (p2 - p0): det < 0 is a face whose normal points along the ray, away from the viewer — SEEN FROM
 *             BEHIND in tn_mesh_rasterize's sense (its area2 > 0) — and cull == 1 drops it.
 *             tv = sub(o, p0), u = div(dot(tv, pv), det), qv = cross(tv, e1), v = div(dot(d, qv), det), t = div(dot(e2, qv), det).
 *   HIT       a usable face with u >= 0, v >= 0, add(u, v) <= 1, t_min <= t <= t_end, whose own box passes with s <= t.
 *   winner    the HIT with the smallest t in fp64, then the lowest face index in the list AS GIVEN.
 * Why the tree cannot change the output: the computed slab bounds are monotone under box inclusion — inv_k is the ray's, sub and mul
 * round monotonically, so a larger box has near_k no larger and far_k no smaller on every axis, a zero axis that passes the smaller
 * box passes the larger, and mul(enter, 1 - 2^-32) is monotone in enter.  The box of every ancestor of a face contains the face's box
 * (exact fp32 min / max), so when a face is a HIT every ancestor passes and its s is at most the face's s, which is at most t.  A
 * traversal that skips a node when it does not pass, or when its s exceeds the best t so far, therefore never skips the winner — nor
 * any HIT with the winner's t, so the index tie-break is safe as well.
 *   outputs, each array may be NULL:
 *     hit_face (int32 [N])   the winner's face index; -1 on a miss
 *     hit_t (float [N])      (float)t; the NaN 0x7fc00000 on a miss
 *     hit_uv (float [N, 2])  (float)u, (float)v; the NaN on a miss
 *     hit_temperature (float [N])   (float)add(add(mul(sub(sub(1, u), v), T0), mul(u, T1)), mul(v, T2)) with Tk = (double)temperature
 *                            of the face's corner k; the NaN on a miss
 *     hit_colors (uint8 [N, 3])   per channel floor(add(add(add(mul(sub(sub(1, u), v), c0), mul(u, c1)), mul(v, c2)), 0.5)) clamped to
 *                            [0, 255], tn_mesh_rasterize's rounding; 0 on a miss; needs colors
 *     hit_any (uint8 [N])    TN_RAYCAST_ANY only, and then the ONLY array written: 1 iff some HIT exists (the traversal stops at the
 *                            first it finds)
 *     counts (device int64 [4], OVERWRITTEN, CLOSEST only)   [0] rays that hit, [1] usable rays, [2] usable faces (the header's),
 *                            [3] rays that reached the limit of the traversal stack
 *     stats (device double [3], OVERWRITTEN, CLOSEST only; needs hit_temperature)   as tn_mesh_rasterize defines them: [0] SUM2
 *                            (blocks of 256) over ALL rays in ray order of (double)hit_temperature, a miss contributing +0.0;
 *                            [1], [2] the minimum and the maximum over the hits; +inf and -inf without a hit.
 * How: one ray per lane, blocks of one wave.  A node is one 64-byte fetch that decides both children; the nearer child (the smaller
 * s) is descended first and the other pushed on a stack of 64 entries per ray in LDS (16 KiB per wave).  A way down pushes at most
 * one entry per internal node: 61 <= 64, so counts[3] is 0 for every blob this library builds.  The kernel never writes past its
 * stack: a ray that reaches the limit does not descend that subtree and is counted.  The kernel checks what it dereferences: a
 * header that does not carry the magic, the version and T is a tree without a face; node and leaf numbers are compared against
 * num_nodes and T, face and vertex indices against T and V; the number of steps is bounded by 2 T + 2, which a tree never reaches.  A
 * foreign blob gives other numbers, never an access outside the arrays.  The counts are integer atomic sums of the waves' ballots; one
 * block finishes the statistics from hit_temperature.  Launches on `stream` only, no allocation, no host synchronisation, no float
 * atomics, no block waits for another.
 * tn_mesh_raycast: TN_ERR_NULL: params or bvh; TN_ERR_SHAPE: V, T out of range (as above), N < 0 or 3N > 2^31 - 1;
 * TN_ERR_UNSUPPORTED: t_min or t_max a NaN, t_min < 0, cull outside {0, 1}, an unknown mode; TN_ERR_NULL: positions, temperature or
 * triangles with V > 0 and T > 0; origins or directions with N > 0; and in CLOSEST mode colors with hit_colors, hit_temperature with
 * stats and N > 0; TN_ERR_SHAPE: a float / int32 pointer not 4-byte aligned, counts / stats not 8-byte aligned, bvh not 64-byte
 * aligned; TN_ERR_WORKSPACE: bvh_bytes < tn_mesh_bvh_bytes(T).  All are returned before any launch, in the siblings' order. */
#define TN_RAYCAST_CLOSEST 0
#define TN_RAYCAST_ANY 1
typedef struct tn_raycast_params {
    double t_min, t_max;
    int32_t cull;
    int32_t mode;
} tn_raycast_params;
int32_t tn_mesh_bvh_depth_bound(void);
size_t tn_mesh_bvh_bytes(int64_t num_triangles);
size_t tn_mesh_bvh_workspace_bytes(int64_t num_triangles);
int tn_mesh_bvh_build(const float *positions, const float *temperature, const int32_t *triangles, int64_t num_vertices,
                      int64_t num_triangles, void *bvh, size_t bvh_bytes, void *workspace, size_t workspace_bytes, void *stream);
int tn_mesh_raycast(const float *positions, const float *temperature, const uint8_t *colors, const int32_t *triangles,
                    int64_t num_vertices, int64_t num_triangles, const void *bvh, size_t bvh_bytes, const float *origins,
                    const float *directions, const float *ray_t_max, int64_t num_rays, const tn_raycast_params *params,
                    int32_t *hit_face, float *hit_t, float *hit_uv, float *hit_temperature, uint8_t *hit_colors, uint8_t *hit_any,
                    int64_t *counts, double *stats, void *stream);

/* The nearest point of the mesh to every query point: the other walk through tn_mesh_bvh_build's blob.  The mesh arrays, V, T, bvh and
 * bvh_bytes are the ray cast's; points [N, 3] floats, point_temperature [N] floats or NULL, N = num_points, 3N <= 2^31 - 1; `params` is
 * read on the HOST: max_distance = R >= 0, which may be +inf; reserved: write 0.  Every output is defined to the bit, and WITHOUT
 * reference to the tree, in the ray cast's conventions: add / sub / mul / div / sqrt are single correctly rounded fp64 operations,
 * nothing is contracted, (double) of a float is exact, (float) of a double rounds to nearest even, dot and cross are the ray cast's.
 *   point i   USABLE when its three floats are finite; Q = (double) of them.  Faces are USABLE as for the ray cast.
 *   bound of a box lo .. hi (fp32) against Q:
 *             g_k = max(sub((double)lo_k, Q_k), sub(Q_k, (double)hi_k), 0) per axis, b = add(add(mul(g0, g0), mul(g1, g1)), mul(g2, g2)).
 *   closest point of a face, p0 p1 p2 = (double) of its corners, lo .. hi its own box: up to four CANDIDATES (C, u, v), in this order:
 *     interior  e1 = sub(p1, p0), e2 = sub(p2, p0), n = cross(e1, e2), nn = dot(n, n).  Left out when nn == 0.  w = sub(Q, p0),
 *               u = div(dot(cross(w, e2), n), nn), v = div(dot(cross(e1, w), n), nn).  A candidate iff u >= 0, v >= 0 and
 *               add(u, v) <= 1; then C_k = add(add(p0_k, mul(u, e1_k)), mul(v, e2_k)).
 *     edges     of a segment a -> b: ab = sub(b, a), den = dot(ab, ab), s = 0 when den == 0, else div(dot(sub(Q, a), ab), den); then
 *               s = 1 when s > 1, s = +0.0 unless s > 0 (a -0.0 becomes +0.0).  C_k = add(a_k, mul(s, ab_k)).
 *               p0 -> p1 with (u, v) = (s, 0); p0 -> p2 with (0, s); p1 -> p2 with (sub(1, s), s).
 *     clamp     every candidate's C is clamped per axis into the face's own box: C_k = lo_k when C_k < lo_k, hi_k when C_k > hi_k
 *               (exact).  r_k = sub(Q_k, C_k), d2 = add(add(mul(r0, r0), mul(r1, r1)), mul(r2, r2)).
 *     The face's closest point is the candidate with the smallest d2, the first in the order above on a tie.  A usable face without
 *     area (collinear or coincident corner positions under distinct indices) has nn == 0 and is the segment or the point its edges
 *     are: no division by zero is taken, no NaN can arise (every operand is finite and no product of them leaves the fp64 range).
 *   winner    among the usable faces with d2 <= R2, R2 = mul(R, R): the smallest d2 in fp64, then the lowest face index in the list AS
 *             GIVEN.
 * Why the tree cannot change the output: after the clamp C_k lies in [lo_k, hi_k], and sub is monotone and odd, so on every axis
 * |r_k| >= g_k of the face's own box — where Q_k < lo_k: sub(Q_k, C_k) <= sub(Q_k, lo_k) = -sub(lo_k, Q_k) <= 0; likewise above hi_k;
 * in between g_k = 0.  mul and add are monotone, and d2 and b add in the same order: d2 >= b of the face's own box.  The box of every
 * ancestor contains the face's box (exact fp32 min / max), a larger box has g_k no larger on every axis, so b is monotone under box
 * inclusion: every ancestor's b <= the face's own b <= d2.  A traversal that skips a node only when its b > the best d2 so far,
 * strictly, or when b > R2, therefore never skips the winner — nor a face that ties with it, so the index tie-break is safe as well.
 *   outputs, each array may be NULL:
 *     closest_face (int32 [N])        the winner's face index; -1 when the point is unusable, there is no usable face, or none lies
 *                                     within R
 *     closest_distance (float [N])    (float)sqrt(d2)
 *     closest_point (float [N, 3])    (float)C, the clamped candidate
 *     closest_uv (float [N, 2])       (float)u, (float)v
 *     closest_temperature (float [N]), closest_colors (uint8 [N, 3])   from (u, v) exactly as hit_temperature and hit_colors from theirs;
 *                                     closest_colors needs colors
 *     difference (float [N])          (float)sub((double)point_temperature[i], (double)closest_temperature[i]), from the ROUNDED
 *                                     float: the point minus the surface.  Needs point_temperature and closest_temperature.  The NaN
 *                                     0x7fc00000 whenever the result is a NaN (either is one).
 *     Without a face the floats are the NaN 0x7fc00000 and the colours 0.
 *     counts (device int64 [4], OVERWRITTEN)   [0] points with a face, [1] usable points, [2] usable faces (the header's), [3] points
 *                                     that reached the limit of the traversal stack
 *     stats (device double [8], OVERWRITTEN; needs closest_distance)   sums are SUM2 (blocks of 256, as tn_mesh_rasterize defines it)
 *                                     over ALL points in order of x = (double) of the rounded float output, +0.0 where the point has no
 *                                     value (the output is a NaN): [0] of closest_distance, [1] of mul(x, x) of it, [2], [3] its minimum
 *                                     and maximum over the points that have one, in the numbers' order with -0.0 below +0.0; [4] .. [7]
 *                                     the same of difference.  +inf and -inf where no point has the value; [4] .. [7] are (+0.0, +0.0,
 *                                     +inf, -inf) with difference NULL.
 * How: one point per lane, blocks of one wave.  A node is one 64-byte fetch that gives both children's b; a child with b > the best
 * d2 so far (R2 until a face is found) is skipped, of two that stay the one with the smaller b is descended first and the other is
 * pushed on a stack of 64 entries per point in LDS ([entry][lane], 16 KiB per wave, as the ray cast's).  A popped entry is tested
 * again, against the best d2 by then: an internal node through the b of its two children, a leaf through the b of its face's own box,
 * before any of the face's arithmetic.  The depth bound 61 <= 64: counts[3] is 0 for every blob this library builds, and
 * the kernel never writes past its stack — a point that reaches the limit does not descend that subtree and is counted.  The kernel
 * checks what it dereferences as the ray cast does: the header's magic, version and T; node and leaf numbers against num_nodes and T, face and vertex indices
 * against T and V; at most 2 T + 2 steps.  A foreign or zeroed blob gives other numbers or no face, never an access outside the
 * arrays.  The counts are integer atomic sums of the waves' ballots; one block finishes the statistics from closest_distance and
 * difference.  Launches on `stream` only, no allocation, no host synchronisation, no float atomics, no block waits for another.
 * tn_mesh_closest: TN_ERR_NULL: params or bvh; TN_ERR_SHAPE: V, T out of range (as above), N < 0 or 3N > 2^31 - 1;
 * TN_ERR_UNSUPPORTED: max_distance a NaN or < 0; TN_ERR_NULL: positions, temperature or triangles with V > 0 and T > 0; points with
 * N > 0; colors with closest_colors; closest_temperature with difference, and point_temperature with difference and N > 0;
 * closest_distance with stats; TN_ERR_SHAPE: a float / int32 pointer not 4-byte aligned, counts / stats not 8-byte aligned, bvh not
 * 64-byte aligned;
 * TN_ERR_WORKSPACE: bvh_bytes < tn_mesh_bvh_bytes(T).  All are returned before any launch, in the siblings' order.  N == 0 or T == 0:
 * TN_OK, counts and stats are written, every point is without a face. */
typedef struct tn_closest_params {
    double max_distance;
    int32_t reserved[2];
} tn_closest_params;
int tn_mesh_closest(const float *positions, const float *temperature, const uint8_t *colors, const int32_t *triangles,
                    int64_t num_vertices, int64_t num_triangles, const void *bvh, size_t bvh_bytes, const float *points,
                    const float *point_temperature, int64_t num_points, const tn_closest_params *params, int32_t *closest_face,
                    float *closest_distance, float *closest_point, float *closest_uv, float *closest_temperature,
                    uint8_t *closest_colors, float *difference, int64_t *counts, double *stats, void *stream);

/* The measured thermal photos projected onto points of the mesh: what the cameras MEASURED at every point, from how many photos, how
 * far these agree, and where the model differs.  The third reader of tn_mesh_bvh_build's blob.  positions, temperature, triangles, V, T,
 * bvh and bvh_bytes are the ray cast's (temperature decides which faces are USABLE and is not read otherwise); points [P, 3] floats,
 * normals [P, 3] floats or NULL (no facing test: cos = 1), point_temperature [P] floats or NULL, P = num_points, 3P <= 2^31 - 1;
 * cameras: K = num_cameras <= 2^31 - 1 DEVICE records of 64 bytes, c2w the row-major 3 x 4 camera-to-world in tn_generate_rays'
 * convention (the camera looks along its -z, +y is up), fx fy cx cy in pixels; images [K, H, W] DEVICE bytes, the 8-bit thermal
 * photos, all of one size; `params` is read on the HOST: t_lo, t_hi the temperatures of byte 0 and byte 255 (finite, in any order),
 * 0 < min_cos <= 1, near >= 0, width = W and height = H in 2 .. 16384, two_sided 0 or not, reserved: write 0.  Every output is
 * defined to the bit, in the ray cast's conventions: add / sub / mul / div / sqrt are single correctly rounded fp64 operations unless
 * marked fp32, nothing is contracted, (double) of a float or a byte is exact, (float) of a double rounds to nearest even, dot is the
 * ray cast's dot, -x is exact.
 *   point i    USABLE when its three floats are finite and, with normals, its normal's three floats are finite and not all zero.
 *              p = its floats, n = (double) of its normal.  An unusable point is seen by no camera.
 *   camera k   USABLE when its sixteen floats are finite and fx > 0, fy > 0.  An unusable camera is skipped.
 *   PAIR (i, k) of a usable point and a usable camera, the clauses in this order; the pair is ACCEPTED when none rejects it:
 *     1 ray    e = (c2w[3], c2w[7], c2w[11]) fp32, d32_j = fp32 sub(p_j, e_j), d = (double)d32: the ray (e, d32) is the one
 *              visible_from casts at the point, t = 1 is the point.
 *     2 depth  xc = dot(c0, d), yc = dot(c1, d), zc = dot(c2, d) with c_j = (double)(c2w[j], c2w[4 + j], c2w[8 + j]), column j of the
 *              rotation; z = -zc.  Rejected (BEHIND) unless z > 0 and z >= near.
 *     3 pixel  u = add(mul(fx, div(xc, z)), cx), v = sub(cy, mul(fy, div(yc, z))): the centre of pixel (row r, column c) is
 *              (u, v) = (c + 0.5, r + 0.5), as tn_generate_rays places it.  Rejected (OUTSIDE) unless 0.5 <= u <= W - 0.5 and
 *              0.5 <= v <= H - 0.5: the hull of the pixel centres; nothing is extrapolated into the half-pixel border.
 *     4 facing dist2 = dot(d, d), dist = sqrt(dist2); cos = div(-dot(n, d), mul(dist, sqrt(dot(n, n)))), |cos| with two_sided; 1
 *              without normals.  Rejected (FACING) unless cos >= min_cos: equality is inside.
 *     5 occlusion   the pair has REACHED the occlusion test.  The ray o = (double)e, direction d, 0 <= t <= 1 - 2^-10, no culling,
 *              against the usable faces exactly as THE CAST defines a HIT (the ray is unusable, and meets nothing, when d32 is not
 *              finite or is (0, 0, 0)).  Rejected (HIDDEN) when some HIT exists.
 *     6 sample a = sub(u, 0.5), x0 = min((int)floor(a), W - 2), fa = sub(a, x0); b = sub(v, 0.5), y0 = min((int)floor(b), H - 2),
 *              fb = sub(b, y0).  With B(r, c) = (double)images[k][r][c]: top = add(B(y0, x0), mul(fa, sub(B(y0, x0 + 1), B(y0, x0)))),
 *              bottom = add(B(y0 + 1, x0), mul(fa, sub(B(y0 + 1, x0 + 1), B(y0 + 1, x0)))), s = add(top, mul(fb, sub(bottom, top))),
 *              Tk = add(t_lo, mul(div(s, 255), sub(t_hi, t_lo))).
 *     7 weight w = div(cos, dist2): up to the camera's constant the reciprocal of the surface area one pixel covers there — a
 *              near, frontal photo outweighs a far, oblique one.
 *   fusion of point i over its accepted pairs in ASCENDING k, from sw = swt = +0.0: sw = add(sw, w), swt = add(swt, mul(w, Tk)),
 *              views += 1; the first accepted pair sets lo = hi = Tk and best = k with its w, a later one sets lo = Tk when Tk < lo,
 *              hi = Tk when Tk > hi, and best = k when its w > the best's w, strictly: the lower index wins a tie.
 *   outputs, each array may be NULL:
 *     measured (float [P])      (float)div(swt, sw); the NaN 0x7fc00000 when views == 0 (or the quotient is a NaN)
 *     views (int32 [P])         the accepted pairs of the point
 *     best_camera (int32 [P])   best; -1 when views == 0
 *     spread (float [P])        (float)sub(hi, lo): how far the photos disagree — a hot spot that moves with the viewpoint is a
 *                               reflection; the NaN when views == 0
 *     difference (float [P])    (float)sub((double)point_temperature[i], (double)measured_i) from the ROUNDED float measured_i, whether
 *                               or not the measured array is given: model minus measurement.  Needs point_temperature.  The NaN
 *                               0x7fc00000 whenever the result is a NaN (either is one).
 *     counts (device int64 [6], OVERWRITTEN)   [0] points with views > 0, [1] usable points, [2] usable cameras, [3] pairs that
 *                               reached the occlusion test, [4] pairs accepted, [5] pairs whose walk reached the limit of the
 *                               traversal stack
 *     stats (device double [8], OVERWRITTEN)   sums are SUM2 (blocks of 256, as tn_mesh_rasterize defines it) over ALL points in
 *                               order of x = (double) of the rounded float output, +0.0 where the output is a NaN: [0] of
 *                               difference, [1] of mul(x, x) of it, [2], [3] its minimum and maximum over the points that have
 *                               one (in the numbers' order, -0.0 below +0.0); [4] of spread, [5] the maximum of spread; [6] of
 *                               measured; [7] +0.0, reserved.  Each is taken from its output array: with that array NULL, or no
 *                               point with the value, a sum is +0.0, a minimum +inf and a maximum -inf.
 * Why the order is fixed: one lane owns one point and walks the cameras in ascending k with sw, swt, lo, hi and best in registers.
 * No sum is shared between lanes, so there is no atomic and no reduction whose order a schedule could change: two calls, on any
 * device state, write the same bytes.
 * How: one point per lane, blocks of one wave.  The camera's record is addressed by k alone, so a wave reads it once.  Clauses 2 - 4
 * cost a few dozen operations and come first; only the pairs they leave walk the tree, with the ray cast's own slab and face test
 * (one definition in the source) in its any-hit traversal: a node is one 64-byte fetch that decides both children, the nearer
 * child (the smaller s) first, the other on a stack of 64 entries per lane in LDS ([entry][lane], 16 KiB per wave), the walk ends
 * at the first HIT.  Which HIT ends it cannot matter: clause 5 asks only whether one exists, and THE CAST's proof shows that the
 * traversal skips no HIT.  The kernel checks what it dereferences as the ray cast does; x0, y0 are also clamped at 0 (never
 * taken inside the hull).  The counts are integer atomic sums of the waves' sums; one block finishes the statistics from the
 * difference, spread and measured arrays.  Launches on `stream` only, no allocation, no host synchronisation, no float atomics,
 * no block waits for another.
 * tn_mesh_project: TN_ERR_NULL: params or bvh; TN_ERR_SHAPE: V, T out of range (as above), P < 0 or 3P > 2^31 - 1, K < 0 or
 * > 2^31 - 1, width or height outside 2 .. 16384; TN_ERR_UNSUPPORTED: min_cos not in (0, 1], near < 0, t_lo or t_hi not finite (a NaN
 * fails each); TN_ERR_NULL: positions, temperature or triangles with V > 0 and T > 0; points with P > 0; cameras or images with K > 0;
 * point_temperature with difference and P > 0; TN_ERR_SHAPE: a float / int32 pointer or cameras not 4-byte aligned, counts / stats not
 * 8-byte aligned, bvh not 64-byte aligned; TN_ERR_WORKSPACE: bvh_bytes < tn_mesh_bvh_bytes(T).  All are returned before any launch,
 * in the siblings' order.  P == 0 or K == 0 or T == 0: TN_OK, counts and stats are written; without a camera no point is seen,
 * without a face nothing hides one. */
typedef struct tn_project_camera {
    float c2w[12];
    float fx, fy, cx, cy;
} tn_project_camera;
typedef struct tn_project_params {
    double t_lo, t_hi;
    double min_cos;
    double near;
    int32_t width, height;
    int32_t two_sided;
    int32_t reserved;
} tn_project_params;
int tn_mesh_project(const float *positions, const float *temperature, const int32_t *triangles, int64_t num_vertices,
                    int64_t num_triangles, const void *bvh, size_t bvh_bytes, const float *points, const float *normals,
                    const float *point_temperature, int64_t num_points, const tn_project_camera *cameras, const uint8_t *images,
                    int64_t num_cameras, const tn_project_params *params, float *measured, int32_t *views, int32_t *best_camera,
                    float *spread, float *difference, int64_t *counts, double *stats, void *stream);

/* Registration of a point cloud to the mesh: iterated closest points with a damped Gauss-Newton step, a whole run queued without a host
 * read.  The fourth reader of tn_mesh_bvh_build's blob.  positions, temperature, triangles, V, T, bvh and bvh_bytes are the closest-point
 * query's (temperature decides which faces are USABLE and is not read otherwise); points [N, 3] floats, the MOVING cloud, N = num_points,
 * 3N <= 2^31 - 1; `params` is read on the HOST: max_distance = R >= 0, which may be +inf; center c and length L > 0, finite: the point the
 * rotation and the scale act about, and the unit in which a translation is compared with the tolerance; damping >= 0, finite; tolerance
 * >= 0, which may be +inf; 1 <= iterations <= 1024; metric TN_REGISTER_POINT or TN_REGISTER_PLANE; with_scale 0 or 1; min_pairs >= 0;
 * reserved: write 0.  transform (DEVICE double [12], the row-major 3 x 4 matrix M that takes a point of the cloud into the mesh's frame)
 * is read as the start and OVERWRITTEN with the result; history (device double [iterations, 4]), result (device int64 [4]) and the
 * workspace are overwritten.  Every output is defined to the bit, and WITHOUT reference to the tree, in the ray cast's conventions: add /
 * sub / mul / div / sqrt are single correctly rounded fp64 operations, nothing is contracted, no library function is called, (double) of a
 * float is exact, dot and cross are the ray cast's, -x, |x|, max and mul by 0.5 are exact.
 * ONE ITERATION i = 0, 1, ..., from the transform M as it is by then:
 *   point j   p = (double) of its floats, x_k = add(add(add(mul(M[k][0], p0), mul(M[k][1], p1)), mul(M[k][2], p2)), M[k][3]).  USABLE when
 *             the three floats and the three x_k are finite.
 *   pair      of a usable point: the closest-point query's definition with Q = x — the fp64 numbers, NOT rounded to float — and
 *             R2 = mul(R, R): the winner (face, C, d2) among the usable faces with d2 <= R2, the lowest face index on a tie.  The proof
 *             given there holds for this Q as it stands: it uses only that sub, mul and add are monotone and that sub is odd, for
 *             which Q may be any fp64 number; a sum that overflows becomes +inf on both sides of d2 >= b, and no NaN arises in d2 or b (C
 *             is finite: u, v, s lie in [0, 1], and a NaN quotient fails the interior's test and gives an edge's s = +0.0).
 *   rows      y = sub(x, c), e = sub(x, C), both per axis.  A direction n gives the row g = (cross(y, n), n, dot(n, y)), seven numbers,
 *             and r = dot(n, e).  Metric POINT: three rows, n = (1, 0, 0), (0, 1, 0), (0, 0, 1) in this order, through the same cross
 *             and dot (the products with 0 are taken, not skipped).  Metric PLANE: one row; e1 = sub(p1, p0), e2 = sub(p2, p0) of the
 *             winning face, w = cross(e1, e2), nn = dot(w, w), n_k = div(w_k, sqrt(nn)).  A winner with nn == 0 is WITHOUT A NORMAL: the
 *             point has no row and is counted.  A point is MATCHED when it has a row.
 *   a point's 36 numbers   from +0.0 each, its rows in order: S[i][j] = add(S[i][j], mul(g_i, g_j)) for 0 <= i <= j < 7 (28 numbers,
 *             row-major), then B[i] = add(B[i], mul(g_i, r)) (7), then E = add(E, mul(r, r)).  A point without a row holds 36 times +0.0.
 *   wave w    the points 64 w .. 64 w + 63, beyond N as points without a row.  Each of the 36 numbers is summed over the wave's lanes
 *             in the adjacent-pair tree: (0 + 1), (2 + 3), ..., (62 + 63), then adjacent pairs of these sums, six levels.  The wave's
 *             PARTIAL is 40 doubles: the 36 sums, then its matched points, its usable points, its points without a normal as doubles,
 *             then +0.0.  The partial of wave w is left at byte 64 + 320 w of the workspace (of the last iteration that ran).
 *   totals    each of the 40 as SUM2 over the waves with runs of 256 (as tn_mesh_rasterize defines it): a run's waves ascending from
 *             +0.0, then the runs' sums ascending from +0.0.  m = the matched points.
 *   refusal   m < min_pairs: status TOO_FEW.
 *   system    k = 7 with_scale, else 6: the leading k x k block of the symmetric S and the first k of B.  lambda = mul(damping, m),
 *             L2 = mul(L, L); D[i] = add(S[i][i], mul(lambda, L2)) for i = 0, 1, 2, 6 and add(S[i][i], mul(lambda, 1)) for i = 3, 4, 5:
 *             the damping is ADDITIVE, in units in which every unknown moves a point by about L.  Column by column, j = 0 .. k - 1:
 *             d_j = D[j], then for p = 0 .. j - 1 ascending d_j = sub(d_j, mul(l[j][p], mul(l[j][p], d_p))); a d_j that is not > 0 or not
 *             finite: status DEGENERATE; for i = j + 1 .. k - 1: v = S[j][i], for p = 0 .. j - 1 ascending v = sub(v, mul(l[i][p],
 *             mul(l[j][p], d_p))), l[i][j] = div(v, d_j).  Then z_i = -B[i], for p = 0 .. i - 1 ascending z_i = sub(z_i, mul(l[i][p], z_p)),
 *             i ascending; z_i = div(z_i, d_i); delta_i = z_i, for p = i + 1 .. k - 1 ascending delta_i = sub(delta_i, mul(l[p][i],
 *             delta_p)), i DESCENDING.  A delta_i that is not finite: status DEGENERATE.  delta = (omega (3), tau (3), sigma); sigma = +0.0
 *             without scale.
 *   update    the Cayley map, no trigonometry: a = mul(0.5, omega), aa = dot(a, a), f = div(2, add(1, aa)); K = [a]x =
 *             ((0, -a2, a1), (a2, 0, -a0), (-a1, a0, 0)) with +0.0 on the diagonal; Q[i][j] = mul(a_i, a_j) off the diagonal and
 *             sub(mul(a_i, a_i), aa) on it; U[i][j] = mul(add(1, sigma), add(I[i][j], mul(f, add(K[i][j], Q[i][j])))).  New linear part
 *             M'[i][j] = dot(U[i], column j of M's linear part); new translation M'[i][3] = add(add(c_i, dot(U[i], t - c)), tau_i) with
 *             (t - c)_k = sub(M[k][3], c_k).  A refused iteration leaves M as it was.
 *   history row i   (m, E, turn, shift): turn = max(|omega_0|, |omega_1|, |omega_2|, |sigma|), shift = div(max_k |tau_k|, L); -1.0 for
 *             both in a refused iteration.  turn <= tolerance and shift <= tolerance: status CONVERGED (the update is applied).
 *   A run ends with the first iteration whose status is CONVERGED, TOO_FEW or DEGENERATE; otherwise after `iterations` of them with
 *   status ITERATIONS.  The history rows of iterations that did not run are four times -1.0.
 *   result    [0] the status, [1] the iterations that ran, [2] m and [3] the usable points of the last one that ran.
 * With N == 0 or T == 0 nothing is matched: TOO_FEW (min_pairs > 0) or DEGENERATE in iteration 0.
 * Why the order is fixed: no sum is taken by an atomic; the wave's tree, the runs and the one thread's solve are written orders, so
 * two calls, on any device state, write the same bytes.
 * How: per iteration two launches.  The walk: one point per lane, blocks of one wave, the closest-point query's traversal (one
 * definition in the source) from x; the 36 sums exist only after the walk, are reduced by lane exchanges and leave as one partial
 * per wave.  The finish: one block sums the partials in the order above, one thread solves and writes M, the row and the result; a run
 * that has ended sets a device flag on which the later iterations' kernels return at once.  The kernels check what they dereference as
 * the closest-point query does.  Launches on `stream` only: iterations x (walk, finish) behind one memset of the flag; no allocation, no
 * host synchronisation, no host read, no float atomics, no block waits for another.
 * tn_mesh_register: TN_ERR_NULL: params, bvh, transform, history, result or workspace; TN_ERR_SHAPE: V, T out of range (as above),
 * N < 0 or 3N > 2^31 - 1; TN_ERR_UNSUPPORTED: a parameter outside what is written above (a NaN fails each); TN_ERR_NULL: positions,
 * temperature or triangles with V > 0 and T > 0; points with N > 0; TN_ERR_SHAPE: a float / int32 pointer not 4-byte aligned, transform
 * / history / result / workspace not 8-byte aligned, bvh not 64-byte aligned; TN_ERR_WORKSPACE: bvh_bytes < tn_mesh_bvh_bytes(T) or
 * workspace_bytes < tn_mesh_register_workspace_bytes(N) = 64 + 320 ceil(N / 64).  All are returned before any launch, in the siblings'
 * order. */
#define TN_REGISTER_POINT 0
#define TN_REGISTER_PLANE 1
#define TN_REGISTER_CONVERGED 0
#define TN_REGISTER_ITERATIONS 1
#define TN_REGISTER_TOO_FEW 2
#define TN_REGISTER_DEGENERATE 3
typedef struct tn_register_params {
    double max_distance;
    double center[3];
    double length;
    double damping;
    double tolerance;
    int32_t iterations;
    int32_t metric;
    int32_t with_scale;
    int32_t min_pairs;
    int32_t reserved[2];
} tn_register_params;
size_t tn_mesh_register_workspace_bytes(int64_t num_points);
int tn_mesh_register(const float *positions, const float *temperature, const int32_t *triangles, int64_t num_vertices,
                     int64_t num_triangles, const void *bvh, size_t bvh_bytes, const float *points, int64_t num_points,
                     const tn_register_params *params, double *transform, double *history, int64_t *result, void *workspace,
                     size_t workspace_bytes, void *stream);

/* Half-edge twins of an indexed triangle list: face adjacency across edges, and whether the mesh is closed, manifold and consistently
 * oriented.  triangles [T, 3] int32, V = num_vertices, T = num_triangles.  Every output is defined to the bit.
 *   half-edge h = 3 f + j runs from tri[f][j] to tri[f][(j + 1) % 3].
 *   STRUCTURAL   a face whose three indices lie in [0, V) and are distinct.
 *   edge class   the half-edges of structural faces with the same unordered vertex pair.
 *   twin (int32 [3T], always fully written): the other half-edge of a class that has exactly two members running in opposite
 *               directions; -1 for every other half-edge, the three half-edges of a non-structural face included.
 *   counts (device int64 [4], OVERWRITTEN): [0] the classes (edges), [1] the classes of one member (boundary edges), [2] the classes of
 *               three or more members (non-manifold edges), [3] the classes of two members that run in the same direction
 *               (inconsistent orientation).  A closed, manifold, consistently oriented mesh has [1] = [2] = [3] = 0.
 * How: one uint64 key lo * V + hi per half-edge (V * V for a non-structural face: above every class), key_bits = the bit length of
 * V * V; the stable device sort of the pairs (key, h); one thread per sorted position: the head of a class looks at its next two
 * neighbours, writes the twins and counts (one integer atomic per block and count).  Nothing in the outputs depends on the order inside
 * a class.  workspace: tn_mesh_half_edges_workspace_bytes(V, T) device bytes, 8-byte aligned; 0 for counts out of range.  Launches on
 * `stream` only: no allocation, no host synchronisation, no float atomics, no block waits for another.
 * TN_ERR_NULL: counts is NULL; triangles, twin or the workspace with T > 0; TN_ERR_SHAPE: V < 0 or > 2^31 - 1, T < 0 or 3T > 2^31 - 1,
 * triangles / twin not 4-byte aligned, counts / workspace not 8-byte aligned; TN_ERR_WORKSPACE: workspace_bytes too small (with T > 0).
 * All are returned before any launch.  T == 0: TN_OK, counts are zeroed, nothing else is written. */
size_t tn_mesh_half_edges_workspace_bytes(int64_t num_vertices, int64_t num_triangles);
int tn_mesh_half_edges(const int32_t *triangles, int64_t num_triangles, int64_t num_vertices, int32_t *twin, int64_t *counts,
                       void *workspace, size_t workspace_bytes, void *stream);

/* Level-set curves of a per-vertex scalar on an indexed triangle list, chained into ordered polylines: isotherms (the scalar is the
 * temperature itself) and plane sections (the scalar is the signed distance to a plane).  positions [V, 3] floats, temperature [V]
 * floats, triangles [T, 3] int32, twin [3T] int32 as tn_mesh_half_edges writes it, V = num_vertices, T = num_triangles.  `params` is a
 * HOST struct, read before the call returns: 1 <= num_levels = K <= 256 levels, finite and strictly ascending, and the plane's normal.
 * `scalar` is NULL for plane mode or a device float [V] for scalar mode (isotherms pass the temperature array itself).  Every output is
 * defined to the bit.  add / sub / mul / div / sqrt below are single correctly rounded fp64 operations, nothing is contracted; (double)
 * of a float is exact, (float) of a double rounds to nearest even.
 *   scalar s_v   scalar mode: (double)scalar[v]; plane mode: add(add(mul(nx, px), mul(ny, py)), mul(nz, pz)) with the position widened
 *                to double.
 *   USABLE       a structural face (see tn_mesh_half_edges) with all nine coordinates, all three temperatures and all three scalars
 *                finite (a plane scalar is finite unless the normal is beyond 1e269).
 *   HIGH         vertex v at level L when s_v >= L, compared in fp64.  A usable face with scalar minimum m and maximum M carries one
 *                segment for every level k with m < L_k <= M: the levels first_f .. last_f - 1, first = #{L <= m}, last = #{L <= M}.  A
 *                vertex exactly on a level is HIGH, so every crossing lies on exactly two edges of the face (curves through vertices
 *                stay consistent, possibly with segments of length zero).
 *   numbering    face-major: seg = base_f + (k - first_f), base_f the exclusive prefix of the faces' segment counts in ascending face
 *                index; S is the total.
 *   direction    rotate the corners so that c0 is the corner whose class differs from the other two; the crossed half-edges are
 *                hA = c0 -> c1 and hB = c2 -> c0.  With c0 HIGH the segment starts on hA and ends on hB, otherwise it starts on hB and
 *                ends on hA: the high side lies on the left, seen against the face's orientation.
 *   crossing     of half-edge h between vertices a and b at level L, lo the vertex that is not HIGH and hi the HIGH one:
 *                w = div(sub(L, s_lo), sub(s_hi, s_lo)); position per axis (float)add(p_lo, mul(w, sub(p_hi, p_lo))); temperature
 *                (float)add(t_lo, mul(w, sub(t_hi, t_lo))).  It depends on (lo, hi, L) only: both faces of an edge compute the same bits.
 *   successor    g = twin[the end half-edge]; none when g is outside [0, 3T), face g / 3 is not usable or does not carry level k;
 *                otherwise segment base_{g/3} + (k - first_{g/3}).  The predecessor of a segment is the segment it succeeds.  With a twin
 *                table of this mesh in- and out-degree are at most 1: the segments form paths and cycles.
 *   curves       a path is an OPEN curve and starts at its head (the segment without a predecessor); a cycle is a CLOSED curve and starts
 *                at its lowest-numbered segment.  Curves are numbered q = 0 .. Q-1 in ascending number of their first segment.  A curve
 *                of n segments has n + 1 points: the start of its first segment, then the end of every segment in order (a closed curve
 *                repeats its first point bit for bit).  Its points begin at first_point = (the segments of earlier curves) + q;
 *                P = S + Q.
 *   per point    point_positions [P, 3], point_temperature [P]; point_face: the face of the segment that starts there, for the last
 *                point of a curve the face of the last segment; point_arc: +0.0 at first_point, arc[j+1] = add(arc[j], len_j),
 *                len_j = sqrt(add(add(mul(dx, dx), mul(dy, dy)), mul(dz, dz))), d the per-axis sub of the rounded fp32 points j + 1 and
 *                j in fp64: a sequential sum in point order.
 *   tn_mesh_curve, row q of `curves` (40 bytes):
 *     length            arc of the last point
 *     level             k;  first_point, points = n + 1;  closed 0 or 1;  first_face: the face of the first segment
 *     mean_temperature  (float)div(W, length), W accumulated from +0.0 in point order, W = add(W, mul(len_j, mul(0.5, add(t_j, t_j+1))))
 *                       with t the fp32 point temperatures widened to double; with length == 0 the NaN 0x7fc00000
 *     min_temperature, max_temperature   over the curve's points, in the numbers' order with -0.0 below +0.0
 *   counts (device int64 [5], OVERWRITTEN): [0] S, the FULL number of segments, [1] Q, [2] P, [3] the closed curves, [4] the usable
 *                faces.  With S > capacity_segments (0: the sizing call, in which every output pointer but counts may be NULL) [1], [2]
 *                and [3] are 0 and no output array is written; the kernels decide that on the device.  Otherwise the point arrays need
 *                room for 2 * capacity_segments rows and curves for capacity_segments rows.
 * How: count per face by binary search over the levels, one-block scan, emit the segments with their successors; the predecessors by
 * one scatter; list ranking by pointer jumping over ping-pong arrays, ceil(log2(max(2, capacity_segments))) launches per sweep, each
 * reading one array and writing the other: a first sweep carries (ancestor, lowest segment seen) and finds every path's head and every
 * cycle's lowest member, the cycles are cut there, a second sweep yields the ranks; the last segment of a curve writes the curve's
 * segment count to its first segment; count / scan / emit over the first segments numbers and places the curves; every segment writes
 * its points to first_point + rank; one wave per curve adds 64 lengths at a time lane by lane.  workspace:
 * tn_mesh_isolines_workspace_bytes(V, T, capacity_segments) device bytes, 8-byte aligned; 0 for counts out of range.  Launches on
 * `stream` only: no allocation, no host synchronisation, no atomics, no block waits for another.  The kernels check what they
 * dereference: foreign indices and foreign twin values give other numbers, never an access outside the arrays.
 * TN_ERR_NULL: params or counts is NULL; TN_ERR_SHAPE: V < 0 or > 2^31 - 1, T < 0 or 3T > 2^31 - 1, capacity_segments < 0 or > 2^30,
 * K outside [1, 256], a float / int32 pointer not 4-byte aligned, point_arc / curves / counts / workspace not 8-byte aligned;
 * TN_ERR_UNSUPPORTED: a level that is not finite or not above its predecessor, in plane mode a normal that is not finite or all zero;
 * TN_ERR_NULL: with V > 0 and T > 0 positions, temperature, triangles, twin or the workspace, and with capacity_segments > 0 an output
 * array; TN_ERR_WORKSPACE: workspace_bytes too small (with V > 0 and T > 0).  All are returned before any launch.  V == 0 or T == 0:
 * TN_OK, counts are zeroed, nothing is launched. */
typedef struct tn_mesh_curve {
    double length;
    int32_t level, first_point, points, closed;
    float mean_temperature, min_temperature, max_temperature;
    int32_t first_face;
} tn_mesh_curve;
typedef struct tn_isoline_params {
    double normal[3]; /* plane mode: the scalar is the signed distance along it (in units of its length) */
    int32_t num_levels;
    int32_t reserved;
    double levels[256];
} tn_isoline_params;
size_t tn_mesh_isolines_workspace_bytes(int64_t num_vertices, int64_t num_triangles, int64_t capacity_segments);
int tn_mesh_isolines(const float *positions, const float *temperature, const int32_t *triangles, int64_t num_vertices,
                     int64_t num_triangles, const int32_t *twin, const float *scalar, const tn_isoline_params *params,
                     float *point_positions, float *point_temperature, double *point_arc, int32_t *point_face,
                     tn_mesh_curve *curves, int64_t capacity_segments, int64_t *counts, void *workspace, size_t workspace_bytes,
                     void *stream);

/* Planar patches of an indexed triangle list: the faces joined across edges while the angle between their normals stays under a
 * limit (walls, floors, roof planes), and per patch its fitted plane, area, flatness, deviation from the plane and area-weighted mean /
 * min / max temperature.  With min_cos = -1 the patches are the EDGE-connected components (tn_mesh_components is vertex connectivity).
 * positions [V, 3] floats, temperature [V] floats, triangles [T, 3] int32, twin [3T] int32 as tn_mesh_half_edges writes it (foreign
 * data: a value is used as an index only inside [0, 3T)), V = num_vertices, T = num_triangles.  min_cos is the cosine of the largest
 * angle between the normals of two joined faces, taken on the host: the device never calls libm.  Every output is defined to the bit.
 * add / sub / mul / div / sqrt below are single correctly rounded fp64 operations, nothing is contracted; (double) of a float is
 * exact, (float) of a double rounds to nearest even.
 *   face f, indices i0 i1 i2, positions p0 p1 p2, temperatures t0 t1 t2:
 *     c, n2, area, centroid m, tf   the expressions of tn_mesh_regions: e1 = sub(p1, p0), e2 = sub(p2, p0) per component; c = (sub(
 *               mul(e1y, e2z), mul(e1z, e2y)), sub(mul(e1z, e2x), mul(e1x, e2z)), sub(mul(e1x, e2y), mul(e1y, e2x))); n2 = add(add(
 *               mul(cx, cx), mul(cy, cy)), mul(cz, cz)); area = mul(0.5, sqrt(n2)); m per axis div(add(add(p0, p1), p2), 3.0);
 *               tf = (float)div(add(add((double)t0, (double)t1), (double)t2), 3.0).
 *     GEOMETRIC the three indices in [0, V) and distinct, all nine coordinates finite, n2 > 0.
 *     THERMAL   geometric and all three temperatures finite.  A face with a NaN temperature is still part of its wall.
 *     u         the unit normal: len = sqrt(n2), u = (div(cx, len), div(cy, len), div(cz, len)).
 *   JOINED      faces f != g are joined iff both are geometric, some half-edge h of one has twin[h] in [0, 3T) with twin[h] / 3 the
 *               other, and add(add(mul(ufx, ugx), mul(ufy, ugy)), mul(ufz, ugz)) >= min_cos (symmetric in f and g).
 *   patches     a patch is a class of the transitive closure of JOINED over the geometric faces; a lone geometric face is a patch.  Its
 *               LABEL is the smallest face index in it; patches are numbered q = 0 .. Q-1 in ascending label; a patch's faces are
 *               taken in ascending face index.  The criterion is adjacency chaining: a gently curved surface whose neighbouring faces
 *               all stay under the angle is ONE patch; flatness and rms_deviation show it.
 *   face_patch  (int32 [T], always fully written): q of a geometric face, -1 of every other.
 *   SUM2(list)  the ordered sum of tn_mesh_regions: consecutive blocks of 256 entries from the list's start (the last may be short),
 *               each accumulated from +0.0 in list order, s = add(s, x); the block sums then accumulated from +0.0 in block order.
 *   tn_mesh_patch, row q of `patches` (136 bytes), over the patch's faces f:
 *     area              SUM2(area_f)
 *     thermal_area      SUM2(area_f of a thermal face, +0.0 of every other)
 *     N (not stored)    the vector area, per axis a: SUM2(mul(0.5, c_f,a))
 *     centroid[a]       div(SUM2(mul(area_f, m_f,a)), area)
 *     plane             nn = add(add(mul(Nx, Nx), mul(Ny, Ny)), mul(Nz, Nz)).  With nn > 0: plane[a] = div(N_a, sqrt(nn)) for a = 0, 1, 2,
 *                       plane[3] = add(add(mul(plane[0], centroid[0]), mul(plane[1], centroid[1])), mul(plane[2], centroid[2])): the
 *                       points x of the plane have dot(plane[0..2], x) = plane[3].  With nn == 0: four +0.0.
 *     flatness          (float)div(sqrt(nn), area): 1 for a flat patch, 0 for a closed surface; +0.0 with nn == 0
 *     rms_deviation     per face and corner i: e_i = add(add(mul(nx, sub(p_ix, cx)), mul(ny, sub(p_iy, cy))), mul(nz, sub(p_iz, cz)))
 *                       with n = plane[0..2], c = centroid and the position widened to double; s = add(add(e0, e1), e2);
 *                       term_f = mul(div(area_f, 12.0), add(add(add(mul(e0, e0), mul(e1, e1)), mul(e2, e2)), mul(s, s))) — the
 *                       integral of the squared distance over the triangle, not just its centroid;
 *                       rms_deviation = (float)sqrt(div(SUM2(term_f), area))
 *     max_deviation     (float) of the largest |e_i| over the patch's faces and corners (a maximum is order-free).  With nn == 0 both
 *                       deviations are the NaN 0x7fc00000.
 *     mean_temperature  (float)div(SUM2(mul(area_f, (double)tf_f) of a thermal face, +0.0 of every other), thermal_area)
 *     min_temperature, max_temperature   of tf_f over the thermal faces;  bounds: min x y z, max x y z over the positions of the
 *                       patch's vertices.  Both in the numbers' order with -0.0 below +0.0.  With thermal_area == 0 the mean and both
 *                       extremes are the NaN 0x7fc00000.
 *     label, faces, thermal_faces   as above; the numbers of its faces and of its thermal faces;  reserved = 0
 *   totals (double [2], OVERWRITTEN): [0] SUM2 of area_f over the geometric faces in ascending face index (the mesh's area), [1] the
 *               same over the thermal faces.
 *   counts (device int64 [3], OVERWRITTEN): [0] Q — the FULL number; rows at or beyond capacity_patches are not written (0 with
 *               patches NULL: the sizing call) —, [1] the geometric faces, [2] the half-edges h whose face is joined with the face of
 *               twin[h] (twice the joining edges of a symmetric table).
 * How: one thread per face writes a 112-byte record (the nine products, tf, the face's box) and its unit normal; the geometric and the
 * thermal faces are compacted in order (count, one-block scan, emit); one thread per half-edge hooks joined faces in a lock-free
 * union-find over the T faces (relaxed agent-scope loads, compare-and-swap of the higher root under the lower), a flatten gives every
 * face its label; tn_sort_pairs of (label, face) puts a patch's faces side by side in face order and the patches in label order, so
 * count / scan / emit over the heads of the runs numbers the patches and finds their faces without an atomic; one thread per
 * 256-block walks its records into a partial, one thread per patch walks its partials (its faces when they are at most 256) and
 * writes centroid and plane; one thread per face measures its corners against its row's plane, and the same two levels finish the
 * row.  The totals take the two steps over the two compacted lists.  workspace: tn_mesh_patches_workspace_bytes(V, T) device bytes,
 * 8-byte aligned; 0 for counts out of range.  Launches on `stream` only: no allocation, no host synchronisation, no float atomics
 * (the integer ones are the union-find's, the count of [2] — one per block — and the sort's), no block waits for another.  The
 * kernels check what they dereference: a foreign index or twin value gives other numbers, never an access outside the arrays.
 * TN_ERR_NULL: counts or totals is NULL; positions, temperature, twin or the workspace with V > 0 and T > 0; triangles or face_patch
 * with T > 0; patches with capacity_patches > 0; TN_ERR_SHAPE: V < 0 or > 2^31 - 1, T < 0 or 3T > 2^31 - 1, a negative capacity, a
 * float / int32 pointer not 4-byte aligned, patches / totals / counts / workspace not 8-byte aligned; TN_ERR_UNSUPPORTED: min_cos a
 * NaN or outside [-1, 1]; TN_ERR_WORKSPACE: workspace_bytes too small (with V > 0 and T > 0).  All are returned before any launch,
 * and in the order of the code: counts / totals, the shape, min_cos, the other pointers, the alignment, the workspace.  V == 0 or
 * T == 0: TN_OK, counts and totals are zeroed and face_patch filled with -1 by memsets, nothing is launched. */
typedef struct tn_mesh_patch {
    double area, thermal_area;
    double plane[4];
    double centroid[3];
    float flatness, rms_deviation, max_deviation;
    float mean_temperature, min_temperature, max_temperature;
    float bounds[6];
    int32_t label, faces, thermal_faces, reserved;
} tn_mesh_patch;
size_t tn_mesh_patches_workspace_bytes(int64_t num_vertices, int64_t num_triangles);
int tn_mesh_patches(const float *positions, const float *temperature, const int32_t *triangles, int64_t num_vertices,
                    int64_t num_triangles, const int32_t *twin, double min_cos, tn_mesh_patch *patches, int64_t capacity_patches,
                    int32_t *face_patch, int64_t *counts, double *totals, void *workspace, size_t workspace_bytes, void *stream);

/* Thermal hot spots of an indexed triangle list: the local maxima of the per-vertex temperature, their basins, the saddles between
 * adjacent basins, the 0-dimensional persistence of the basins (every peak's prominence in degrees) and, per spot that stands out, the
 * extent and the row of a thermal region.  Cold spots are the same with the order reversed.  temperature [V] floats, triangles [T, 3]
 * int32, V = num_vertices, T = num_triangles; offsets / corners are tn_mesh_incidence's of the SAME triangles and V.  Every output is
 * defined to the bit, and all but the rows' floats are integers.
 *   ORDER       a vertex is FINITE if its temperature is neither a NaN nor infinite.  HOT order (coldest == 0): u is ABOVE v iff
 *               T[u] > T[v] compared as numbers (-0.0 == +0.0), or T[u] == T[v] and u < v.  With coldest != 0 the comparison of the
 *               temperatures is reversed, the tie rule is not.  rank[v] (int32 [V]) is v's position in that order, 0 the top; the
 *               vertices that are not finite follow all finite ones in ascending index.  It is one tn_sort_pairs of (key, 0 .. V-1)
 *               over 32 key bits: with k the monotone 32-bit key of the float (-0.0 taken as +0.0; the sign bit set for a positive
 *               float, all bits flipped for a negative one) the key is ~k for HOT, k for COLD and 0xffffffff for a vertex that is
 *               not finite — finite floats have k and ~k in [0x00800000, 0xff7fffff].  Everything below compares ranks, never floats.
 *   NEIGHBOURS  of a finite vertex v: the finite vertices t[(j + 1) % 3] and t[(j + 2) % 3], where they differ from v, over the
 *               corners (t, j) of v's list — clipped and checked as tn_mesh_scalar_smooth does it, VALID triangles only (all three
 *               indices in [0, V)).  A vertex that is not finite is nobody's neighbour and belongs to nothing: -1 in vertex_basin.
 *   ASCENT      up[v] = the neighbour of the smallest rank if that rank is below rank[v], else v itself: v is then a PEAK.  peak[v] is
 *               the fixed point of up, reached by pointer jumping in ceil(log2(max(2, V))) launches over two arrays, each launch
 *               reading one and writing the other.
 *   BASINS      numbered b = 0 .. B-1 in ascending peak vertex (count / scan / emit over the peak flags).  vertex_basin (int32 [V],
 *               always fully written): b, or -1.  basin_peak (int32, capacity_basins rows): the peak vertex of basin b.
 *   SADDLES     for every half-edge (u, w) = (t[j], t[(j + 1) % 3]) of a valid triangle with both ends finite and vertex_basin[u] = a
 *               != vertex_basin[w] = b, the edge's PASS is max(rank[u], rank[w]): its lower end.  The saddle of the unordered pair
 *               {a, b} is the smallest pass over all half-edges between them.  saddles (tn_mesh_saddle, capacity_saddles rows): one
 *               row per adjacent pair in ascending (a, b) with a < b: the pair, pass_vertex (the vertex of that rank) and pass_rank.
 *   counts (device int64 [3], OVERWRITTEN): [0] B and [1] S, the number of adjacent pairs — the FULL numbers; rows at or beyond a
 *               capacity are not written (capacity 0 with a NULL table: the sizing call) —, [2] the finite vertices.
 * tn_mesh_peaks, how: the keys and the sort; one thread per rank writes rank[v]; one thread per vertex walks its list (a minimum over
 * integers is order-free); the jumps; count, one-block scan, emit over the peak flags; one thread per half-edge writes the key
 * (min(a, b), max(a, b)) in 2 bit_length(V) bits, or the key of no pair; tn_sort_pairs puts a pair's half-edges side by side and the
 * pairs in order; count / scan / emit over the heads of the runs, and the head's thread walks its run for the smallest pass.
 * workspace: tn_mesh_peaks_workspace_bytes(V, T) device bytes, 8-byte aligned; 0 for counts out of range.  V == 0: counts is zeroed by a
 * memset, nothing is launched.  T == 0: every finite vertex is a peak, S = 0, the saddle steps are not launched.
 * TN_ERR_NULL: counts is NULL; with V > 0 temperature, offsets, rank, vertex_basin or the workspace; with V > 0 and T > 0 triangles or
 * corners; basin_peak / saddles with a capacity > 0; TN_ERR_SHAPE: V < 0 or > 2^31 - 1, T < 0 or 3T > 2^31 - 1, a negative capacity, a
 * float / int32 pointer or saddles not 4-byte aligned, counts / workspace not 8-byte aligned; TN_ERR_WORKSPACE: workspace_bytes too
 * small (with V > 0).  All are returned before any launch, in the order of the code: counts, the shape, the other pointers, the
 * alignment, the workspace.
 *
 * tn_basin_persistence, ON THE HOST, every pointer a HOST pointer, integers only: basin_rank (int32 [B]) = rank[basin_peak[b]];
 * saddles [S] as above, in the table's order.  The saddles are taken in ascending pass_rank; all saddles of one pass_rank are a BATCH,
 * taken in ascending row.  A union-find over the basins keeps as a component's representative the member with the smallest peak rank.
 * A saddle that joins two different components kills the representative with the larger peak rank: death_saddle[it] = the row.  After
 * the batch parent[d] = find(d) for every basin d that died in it: the eldest of everything joined at that pass vertex.  A basin that
 * never dies keeps death_saddle = parent = -1: there is one per connected component of the finite graph.  death_saddle, parent: int32
 * [B], fully written.  It allocates its two index arrays (S + B ints) and nothing else; O(S log S).
 * TN_ERR_SHAPE: B or S negative or > 2^31 - 1, a pointer not 4-byte aligned; TN_ERR_NULL: basin_rank, death_saddle or parent with
 * B > 0, saddles with S > 0; TN_ERR_UNSUPPORTED: a row names a basin outside [0, B) or one basin twice (nothing is written);
 * TN_ERR_WORKSPACE: the two arrays could not be allocated.
 * The PROMINENCE of basin b is (float)sub((double)T[peak], (double)T[pass_vertex]) of its death saddle — the operands swapped for
 * coldest —, +inf for a basin that never dies; the caller computes it.
 *
 * tn_mesh_spots: the caller has chosen the K spots (the basins whose prominence exceeds its threshold, every other basin joined to the
 * first survivor on its parent chain) and uploads basin_spot (int32 [B]: the spot k of every basin, -1 of a basin in none), and per
 * spot spot_peak (the peak vertex), spot_limit (int32: pass_rank of the spot's own death saddle; any value >= V for a spot that never
 * dies) and spot_bound (float: (float)sub((double)T[peak], (double)extent_drop) for HOT, (float)add(...) for COLD; -inf / +inf for no
 * drop).  rank and vertex_basin are tn_mesh_peaks' of the same temperature and order.
 *   EXTENT of spot k: the finite vertices v with vertex_basin[v] = b in [0, B), basin_spot[b] = k in [0, K), rank[v] < spot_limit[k]
 *               — strictly above the spot's saddle — and T[v] >= spot_bound[k] (coldest != 0: T[v] <= spot_bound[k]), compared in
 *               fp32.  The bound is "the spot within X degrees of its peak"; connectivity is NOT re-checked: with a bound the extent
 *               may fall into several pieces, which stay one spot.
 *   vertex_spot (int32 [V], always fully written): k or -1.
 *   face_spot (int32 [T], always fully written): k iff face t is USABLE as tn_mesh_regions defines it and all three vertices lie in
 *               the extent of k; -1 otherwise.
 *   tn_mesh_spot, row k of `spots` (80 bytes, K rows, all written): the fields of tn_mesh_region over the spot's faces in ascending
 *               face index, by the same definitions and the same SUM2 — area, faces, mean_temperature, centroid, min_temperature /
 *               max_temperature, bounds, hottest_vertex / coldest_vertex (over the faces' vertices) —; label = spot_peak[k];
 *               vertices = the number of vertices in the extent; reserved = 0.  A spot whose extent holds no whole face has area
 *               +0.0, faces 0, hottest_vertex = coldest_vertex = -1 and the NaN 0x7fc00000 in every float; with faces of area 0
 *               alone the mean and the centroid are that NaN, as in a region of area 0.
 *   counts (device int64 [3], OVERWRITTEN): [0] the spots that have a face, [1] the faces that belong to a spot, [2] the usable faces.
 * How: one thread per vertex writes vertex_spot and counts its spot's vertices (an integer atomic); one thread per face writes the
 * 96-byte record of tn_mesh_regions, face_spot and the key; then the steps of tn_mesh_regions with the spot as the label: the two
 * compacted lists, tn_sort_pairs of (spot, face), the heads, the 256-blocks, the partials; one thread per spot joins its partials.
 * workspace: tn_mesh_spots_workspace_bytes(V, T, K) device bytes, 8-byte aligned; 0 for counts out of range or K > V.  V == 0: counts
 * is zeroed and face_spot filled with -1 by memsets, nothing is launched.  T == 0: vertex_spot and the rows (all empty, with their
 * vertex counts) are written.  K == 0: vertex_spot and face_spot are -1, counts[2] is still counted.
 * TN_ERR_NULL: counts is NULL; with V > 0 positions, temperature, rank, vertex_basin, vertex_spot or the workspace; with T > 0
 * triangles or face_spot; with B > 0 basin_spot; with K > 0 spot_peak, spot_limit, spot_bound or spots; TN_ERR_SHAPE: V or T out of
 * range as above, B < 0 or > V, K < 0 or > B, a float / int32 pointer not 4-byte aligned, spots / counts / workspace not 8-byte
 * aligned; TN_ERR_WORKSPACE: workspace_bytes too small (with V > 0).  All are returned before any launch, in the order of the code:
 * counts, the shape, the other pointers, the alignment, the workspace.
 * Both device entries launch plain 256-thread blocks (the scans: one block of 1024) on `stream` only: no allocation, no host
 * synchronisation, no float atomics (the integer ones: counts[2] of tn_mesh_peaks, one per block; a spot's vertices; the sort's), no
 * block waits for another.  The kernels check what they dereference — a list is clipped to [0, 3T], a corner outside it or of an
 * invalid triangle is skipped, a rank, a basin, a spot and a sorted position are used only inside their arrays —, so a foreign index
 * or table gives other numbers, never an access outside the arrays.  Inputs and outputs must not overlap. */
typedef struct tn_mesh_saddle {
    int32_t a, b;
    int32_t pass_vertex, pass_rank;
} tn_mesh_saddle;
typedef struct tn_mesh_spot {
    double area;
    int32_t label;
    int32_t faces;
    float mean_temperature;
    float min_temperature, max_temperature;
    float centroid[3];
    float bounds[6];
    int32_t coldest_vertex, hottest_vertex;
    int32_t vertices, reserved;
} tn_mesh_spot;
size_t tn_mesh_peaks_workspace_bytes(int64_t num_vertices, int64_t num_triangles);
int tn_mesh_peaks(const float *temperature, const int32_t *triangles, int64_t num_triangles, int64_t num_vertices,
                  const int32_t *offsets, const int32_t *corners, int32_t coldest, int32_t *rank, int32_t *vertex_basin,
                  int32_t *basin_peak, int64_t capacity_basins, tn_mesh_saddle *saddles, int64_t capacity_saddles, int64_t *counts,
                  void *workspace, size_t workspace_bytes, void *stream);
int tn_basin_persistence(const int32_t *basin_rank, int64_t num_basins, const tn_mesh_saddle *saddles, int64_t num_saddles,
                         int32_t *death_saddle, int32_t *parent);
size_t tn_mesh_spots_workspace_bytes(int64_t num_vertices, int64_t num_triangles, int64_t num_spots);
int tn_mesh_spots(const float *positions, const float *temperature, const int32_t *triangles, int64_t num_vertices,
                  int64_t num_triangles, const int32_t *rank, const int32_t *vertex_basin, const int32_t *basin_spot, int64_t num_basins,
                  const int32_t *spot_peak, const int32_t *spot_limit, const float *spot_bound, int64_t num_spots, int32_t coldest,
                  int32_t *vertex_spot, int32_t *face_spot, tn_mesh_spot *spots, int64_t *counts, void *workspace,
                  size_t workspace_bytes, void *stream);

/* Geodesic distance on an indexed triangle list: the distance ALONG THE SURFACE from a set of seeds to every vertex, and the decay
 * profile — area and temperature per band of that distance.  positions [V, 3] floats, triangles [T, 3] int32; offsets / corners are
 * tn_mesh_incidence's of the SAME triangles and V.  The solver is a Jacobi fixed point of the eikonal equation on the triangles with
 * the "virtual source" update: first order, exact on a plane from a point, no unfolding of obtuse triangles.  Every output is defined
 * to the bit: all arithmetic is fp64 from the fp32 positions, one rounded operation per named step (add, sub, mul, div, sqrt:
 * __dadd_rn ... __dsqrt_rn), no contraction; dot(x, y) = add(add(mul(x0, y0), mul(x1, y1)), mul(x2, y2)), norm(x) = sqrt(dot(x, x)).
 *   STATE       distance (fp64 [V]) and nearest_seed (int32 [V]): D and L below; counts (device int64 [2], KEPT between calls): [0] the
 *               rounds that changed a vertex, [1] 1 once a round has changed nothing.
 *   RESTART     (restart != 0) counts = 0; every D = +inf, L = -1; then for the seeds i = 0 .. num_seeds - 1 ascending, with
 *               v = seed_vertex[i] and o = add(seed_offset[i], 0.0) (-0.0 is +0.0): where o < D[v], D[v] = o and L[v] = i.  A repeated
 *               vertex so keeps its smallest offset and, among equal offsets, the lowest i.  A seed with v outside [0, V) or an offset
 *               that is not finite or below zero is ignored.  (Two integer atomic minima: the offset's bit pattern, then i.)
 *   ROUND       reads D_k, L_k only and writes D_k+1, L_k+1 only (two arrays of each; never in place).  For vertex c: best = D_k[c],
 *               label = L_k[c].  If c's three coordinates are finite, the corners (t, j) of c's list in list order — the list clipped
 *               to [0, 3T], a corner outside it skipped — with triangle t VALID (three indices in [0, V)), t[j] == c, the three indices
 *               distinct and the coordinates of a = t[(j + 1) % 3] and b = t[(j + 2) % 3] finite give three candidates, in this order:
 *                 ac = c - a, bc = c - b, ab = b - a (sub per coordinate)
 *                 via a    add(D[a], norm(ac)), label L[a]
 *                 via b    add(D[b], norm(bc)), label L[b]
 *                 face     only with D[a] and D[b] finite, u = norm(ab) > 0 and cy > 0, where
 *                          cr = ab x ac: cr0 = sub(mul(ab1, ac2), mul(ab2, ac1)), cr1 = sub(mul(ab2, ac0), mul(ab0, ac2)),
 *                                        cr2 = sub(mul(ab0, ac1), mul(ab1, ac0))
 *                          cx = div(dot(ab, ac), u), cy = div(norm(cr), u)
 *                          A = mul(D[a], D[a]); sx = div(sub(add(mul(u, u), A), mul(D[b], D[b])), mul(2, u))
 *                          sy2 = sub(A, mul(sx, sx)), which must be >= 0; sy = sqrt(sy2)
 *                          dx = sub(cx, sx), h = add(cy, sy); xs = add(sx, div(mul(dx, sy), h)), which must lie in 0 < xs < u
 *                          the candidate is sqrt(add(mul(dx, dx), mul(h, h))), its label L[a] if D[a] <= D[b], else L[b]
 *               A candidate replaces best and label iff cand < best and cand <= max_distance: ties keep the earlier candidate, a NaN
 *               never wins.  D_k+1[c] = best, L_k+1[c] = label.  A value only ever decreases; a round that changes no vertex ends the
 *               solve.  The number of rounds is about the number of edge hops to the farthest vertex.
 * tn_mesh_geodesic queues, on `stream`, the restart (if asked) and `rounds` rounds (0 .. 4096).  Once a round has changed nothing the
 * remaining queued rounds return on a device flag, as tn_mesh_register's iterations do.  After the call distance / nearest_seed hold
 * the latest iterate whatever the parity (a last launch copies it from the workspace if the number of rounds that changed something
 * in this call is odd).  restart == 0 continues the solve of the last call: the SAME distance, nearest_seed, counts and workspace,
 * unchanged in between.  Every vertex is evaluated in every round.
 * workspace: tn_mesh_geodesic_workspace_bytes(V, T) device bytes, 8-byte aligned; 0 for counts out of range.  V == 0: TN_OK, nothing is
 * launched or written.  T == 0: the seeds keep their offsets, the first round changes nothing.
 * Errors, all before any launch, in this order: tn_mesh_smooth's set for an indexed mesh (TN_ERR_NULL: with V > 0 positions, offsets
 * or distance, with V > 0 and T > 0 triangles or corners; TN_ERR_SHAPE: V or T out of range, a pointer not 4-byte aligned); TN_ERR_NULL:
 * with V > 0 nearest_seed, counts or the workspace; with V > 0, restart != 0 and num_seeds > 0 seed_vertex or seed_offset; TN_ERR_SHAPE:
 * num_seeds < 0 or > 2^31 - 1, max_distance negative or a NaN (+inf: no limit), rounds < 0 or > 4096, distance / seed_offset / counts /
 * workspace not 8-byte aligned, nearest_seed / seed_vertex not 4-byte aligned; TN_ERR_WORKSPACE: workspace_bytes too small (with V > 0).
 *
 * tn_mesh_distance_bands: the decay profile of `temperature` (floats [V]) over `distance`.  width (fp64, finite, > 0), bands = K in
 * 1 .. 4096, cell: -1 for every face, otherwise only faces whose three vertices have nearest_seed == cell.  Face t TAKES PART iff it is
 * PLACED as tn_mesh_regions defines it (indices distinct and in [0, V), nine finite coordinates), its three distances d0, d1, d2 are
 * finite, the cell admits it, and q = div(div(add(add(d0, d1), d2), 3), width) satisfies 0 <= q < K; its band is floor(q).
 *   tn_mesh_band, row k of `rows` (40 bytes, no padding, K rows, all written): area = SUM2 of the areas of the band's faces;
 *               warm_area = SUM2 of the areas of its faces that have a face temperature tf (three finite temperatures; a face
 *               without one enters these two sums as +0.0); mean_temperature = (float)div(SUM2 of mul(area, (double)tf), warm_area),
 *               the NaN 0x7fc00000 unless warm_area > 0; min_temperature / max_temperature of tf, that NaN without a warm face;
 *               faces, warm_faces; reserved = 0.  area, tf and SUM2 — the stable device sort of (band, face), the records joined in
 *               ascending face index, 256 at a time, then the partials in block order — are tn_mesh_regions'.  An empty band is a
 *               row of zeros with that NaN in its three floats.
 *   counts (device int64 [3], OVERWRITTEN): [0] the bands that have a face, [1] the faces that take part, [2] the placed faces with
 *               three finite distances that the cell admits (those beyond the last band included).
 * workspace: tn_mesh_distance_bands_workspace_bytes(V, T, K) device bytes, 8-byte aligned; 0 for counts or K out of range.  V == 0 or
 * T == 0: the rows are all empty.  TN_ERR_NULL: rows, counts or the workspace; with V > 0 positions, temperature, distance or
 * nearest_seed; with T > 0 triangles; TN_ERR_SHAPE: V or T out of range, K < 1 or > 4096, width not finite or not > 0, cell < -1, a
 * float / int32 pointer not 4-byte aligned, distance / rows / counts / workspace not 8-byte aligned; TN_ERR_WORKSPACE.  All before any
 * launch, in the order of the code: rows / counts / workspace, the shape, the other pointers, the alignment, the workspace.
 * Both entries launch plain 256-thread blocks (the scans: one block of 1024) on `stream` only: no allocation, no host synchronisation,
 * no float atomics (the integer ones: the seeds', the tally's, the sort's), no block waits for another.  The kernels check what they
 * dereference.  Inputs and outputs must not overlap. */
typedef struct tn_mesh_band {
    double area, warm_area;
    float mean_temperature;
    float min_temperature, max_temperature;
    int32_t faces, warm_faces;
    int32_t reserved;
} tn_mesh_band;
size_t tn_mesh_geodesic_workspace_bytes(int64_t num_vertices, int64_t num_triangles);
int tn_mesh_geodesic(const float *positions, const int32_t *triangles, int64_t num_triangles, int64_t num_vertices,
                     const int32_t *offsets, const int32_t *corners, const int32_t *seed_vertex, const double *seed_offset,
                     int64_t num_seeds, double max_distance, int32_t restart, int32_t rounds, double *distance,
                     int32_t *nearest_seed, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);
size_t tn_mesh_distance_bands_workspace_bytes(int64_t num_vertices, int64_t num_triangles, int64_t bands);
int tn_mesh_distance_bands(const float *positions, const float *temperature, const int32_t *triangles, int64_t num_vertices,
                           int64_t num_triangles, const double *distance, const int32_t *nearest_seed, double width, int64_t bands,
                           int32_t cell, tn_mesh_band *rows, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Fused forward: Model.forward (collider) + ThermalNerfModel.get_outputs
 * [REF thermal_nerf_model.py:210-275]
 * ---------------------------------------------------------------------------------------------------- */

typedef struct tn_render_config {
    int32_t num_proposal_samples[2]; /* (256, 96); 1..1024 each       */
    int32_t num_nerf_samples;        /* 48 | 64 | 192 ...; 1..1024    */
    int32_t training;                /* eval == 0                     */
    float pdf_anneal;                /* ProposalNetworkSampler._anneal (1.0 at inference) */
    /* eval only, 0 = off (exact): a wave of 64 rays stops marching once EVERY ray's transmittance is below this value
     * (wave-wide vote).  Skipped samples carry weights < eps each; rgb/thermal/accumulation move by <= eps, the
     * expected depth by <= eps * far.  The reference has no such switch: 0 reproduces it. */
    float early_stop_transmittance;
    /* 0 = choose by call size (tn_render_kernel_form: lane = ray — a wavefront marches 64 consecutive rays — from 24 576 rays in
     * the proposal pass and from 8 192 in the field pass, whose tiles a small call marches in segments (sample_split); one ray
     * per wave below), 1 = lane = ray, 2 = one ray per wave. */
    int32_t kernel_family;
    /* ProposalNetworkSampler's initial sampler [REF thermal_nerf_model.py:164-170]: 0 = UniformLinDispPiecewiseSampler
     * ("piecewise", the default), 1 = UniformSampler ("uniform").  Every level's spacing -> euclidean map follows it. */
    int32_t initial_sampler;
    /* Sample-split tiles of the exact-fp32 lane = ray field kernel (eval; round 5 — APPENDED: zero-initialise the struct, 0 keeps
     * every older caller's meaning of "the library decides").  A 64-ray tile marches its S samples serially, so a call of T tiles
     * lasts ceil(T / 2048) marches however few tiles there are; with k segments per tile it lasts ceil(k T / 2048) marches of S / k
     * samples, each segment composited with its own transmittance and chained by a second pass (w_i = T_j w_i_local: the
     * reference's weights [NS RaySamples.get_weights, called at REF thermal_nerf_model.py:233] in another association — same
     * tolerance, other last bits than the serial march).  0 = by call size (tn_render_sample_split; 1 from ~400 k rays up),
     * 1 = never, k > 1 = k segments (capped so that the records fit the workspace: tn_render_sample_split reports the value used).
     * Ignored (1) by the training, early-termination, split-precision and one-ray-per-wave kernels. */
    int32_t sample_split;
    /* Training only (round 5, appended): 0 = NS single_jitter=True (the reference's default, REF thermal_nerf_model.py:176): ONE
     * stratified draw per ray and level, tn_render_inputs.jitter = [3,R]; 1 = single_jitter=False: one draw per bin edge,
     * jitter = [R,P0+1] | [R,P1+1] | [R,S+1] back to back [NS SpacedSampler / PDFSampler.generate_ray_samples]. */
    int32_t per_sample_jitter;
    /* The last partial round of tiles of a whole-march call of the exact-fp32 lane = ray field kernel (eval; appended, 0 keeps
     * "the library decides").  A call of T tiles on 2 048 wave slots lasts ceil(T / 2048) tile-times: the 800 x 800 frame's
     * 10 000 tiles last five, the fifth with 1 808 of the slots busy.  Those T mod 2048 tiles can instead be evaluated as
     * (tile, segment) units that only RECORD (delta * density, r, g, b, thermal) per sample, and composited by a replay pass
     * that runs the serial march's own statements on the records: the same bits in every output, unlike sample_split.
     * 0 = by call shape (tn_render_tail_plan), 1 = never, k > 1 = k segments per tile (fewer where a segment would be shorter
     * than 12 samples; tn_render_tail_plan reports the value used).  Applies only to calls of at least one whole round with a
     * remainder, without early termination and not in the sample_split form; the records (5 x 4 B per ray and sample) live
     * behind the proposal scratch of the workspace (tn_render_workspace_bytes counts them; a workspace that ends before them
     * makes the call march whole tiles). */
    int32_t tail_balance;
    /* TEST HOOK for the above, 0 in production: the number of wave slots the lane = ray field kernel is launched on (a multiple of
     * 8: 16 = a grid of two blocks), so that a few thousand rays make whole rounds plus a remainder. */
    int32_t tail_slots;
} tn_render_config;

typedef struct tn_render_inputs {
    const float *origins;            /* [R,3] */
    const float *directions;         /* [R,3] */
    const float *nears;              /* [R]   (collider output) */
    const float *fars;               /* [R]   */
    const int32_t *camera_indices;   /* [R] or NULL (eval) */
    const float *lin_bins0;          /* [P0+1] torch.linspace(0,1,P0+1) */
    const float *u1;                 /* [P1+1] PDFSampler eval positions for level 1 */
    const float *u2;                 /* [S+1]  PDFSampler eval positions for the final level */
    const float *jitter;             /* training: [3,R] per-level single-jitter draws, or the per-edge draws of
                                      * tn_render_config.per_sample_jitter; NULL in eval */
} tn_render_inputs;

typedef struct tn_render_outputs {
    float *rgb;            /* [R,3] */
    float *accumulation;   /* [R]   */
    float *depth;          /* [R]   median */
    float *expected_depth; /* [R]   */
    float *prop_depth_0;   /* [R]   */
    float *prop_depth_1;   /* [R]   */
    float *thermal;        /* [R]   */
    /* optional (training / debugging): per-level weights and spacing/euclidean bins; NULL to skip */
    float *weights[3];       /* [R,P0], [R,P1], [R,S]       */
    float *spacing_bins[3];  /* [R,P0+1], [R,P1+1], [R,S+1] */
    float *eucl_bins[3];     /* same shapes                  */
} tn_render_outputs;

size_t tn_render_workspace_bytes(const tn_render_config *cfg, int64_t num_rays);

int tn_render_rays_fwd(const tn_density_field *prop0, const tn_density_field *prop1, const tn_thermal_field *field,
                       const tn_render_config *cfg, const tn_render_inputs *in, const tn_render_outputs *out,
                       int64_t num_rays, void *workspace, size_t workspace_bytes, void *stream);

/* The two halves of tn_render_rays_fwd, callable separately (tn_render_rays_fwd == both, in this order, sharing
 * `workspace`): NS ProposalNetworkSampler.generate_ray_samples [REF thermal_nerf_model.py:222-224] (+ prop_depth_i
 * [REF :267-270]) leaves the final S+1 bin edges in `workspace`; tn_field_render_fwd evaluates
 * ThermalNerfactoTField.forward on them and composites [REF :225-243,271-273].
 * PRECONDITION of tn_field_render_fwd: `workspace` was produced by tn_proposal_sample_fwd of the SAME call shape on the same
 * stream.  Besides the bin edges, that call resets the two words the expected-depth clip accumulates its call-global
 * [min, max] in (DepthRenderer "expected" clips to them): on a workspace that did not come from it, expected_depth is clipped
 * to stale bounds.  Every other output is independent of them. */
int tn_proposal_sample_fwd(const tn_density_field *prop0, const tn_density_field *prop1, const tn_render_config *cfg,
                           const tn_render_inputs *in, const tn_render_outputs *out, int64_t num_rays, void *workspace,
                           size_t workspace_bytes, void *stream);
int tn_field_render_fwd(const tn_thermal_field *field, const tn_render_config *cfg, const tn_render_inputs *in,
                        const tn_render_outputs *out, int64_t num_rays, void *workspace, size_t workspace_bytes,
                        void *stream);

/* One launch for SEVERAL of the reference's chunks, or for parts of them.  The one cross-ray quantity of the path is
 * DepthRenderer("expected")'s clip to the [min, max] of the sample mid-points of its call = of one eval_num_rays_per_chunk chunk of
 * the row-major frame [REF render/renderer.py:182-187 -> NS Model.get_outputs_for_camera_ray_bundle; REF config_thermal_nerf.py:30].
 * tn_field_render_chunked_fwd is tn_field_render_fwd for rays [first_ray, first_ray + num_rays) of such a frame: it keeps one
 * [min, max] pair per chunk the call touches (chunk = (first_ray + ray) / chunk_rays) and writes them to depth_bounds
 * [tn_depth_bound_slots(...), 2] (device floats; slot 0 = the call's first chunk).
 *   clip != 0: every ray's expected depth is clipped to its chunk's pair — a call that covers its chunks wholly (a whole frame in
 *              one launch pair) then equals the reference's chunk-by-chunk loop bit for bit at the throughput of one launch;
 *   clip == 0: expected_depth is left unclipped — the caller (ray sharding finer than the chunks, thermo_nerf_amd/distributed.py)
 *              reduces the pairs with the other parts' (min / max over the ranks sharing a chunk) and applies
 *              tn_expected_depth_clip_chunked with the reduced array.
 * first_ray and chunk_rays must be multiples of 64 (a 64-ray wavefront tile never straddles two chunks): TN_ERR_UNSUPPORTED
 * otherwise.  Same workspace precondition as tn_field_render_fwd. */
int64_t tn_depth_bound_slots(int64_t first_ray, int64_t num_rays, int64_t chunk_rays);

/* Which kernel form a call of num_rays rays takes under cfg->kernel_family (0 = by call size): 1 = lane = ray (a wavefront marches
 * 64 consecutive rays), 2 = one ray per wavefront.  pass 0: tn_proposal_sample_fwd (lane = ray from 24 576 rays; training calls: 65 536); pass 1:
 * tn_field_render_fwd / tn_field_render_chunked_fwd on `field`: lane = ray from 8 192 rays where the exact-fp32 kernel can march
 * its tiles in segments (sample_split != 1, no early termination, eval), from 40 960 with a split-precision blob (those kernels only
 * exist in form 1; a form-2 call with such a blob runs the exact-fp32 ray-per-wave kernel), from 57 344 otherwise or with field ==
 * NULL.  The two forms sum in different orders, so a caller that renders PART of a launch (ray shards of one frame,
 * thermo_nerf_amd/engine.py::render_shard) and wants the whole launch's bits asks for the whole launch's form here and passes it
 * as cfg->kernel_family.  No reference counterpart (the reference has one code path, REF render/renderer.py:182-187); 0 on a
 * NULL cfg. */
int32_t tn_render_kernel_form(const tn_thermal_field *field, const tn_render_config *cfg, int64_t num_rays, int32_t pass);
/* The number of sample segments per tile tn_field_render_fwd / _chunked_fwd use for a call of num_rays rays under
 * cfg->sample_split (see there).  Like the kernel form it is a property of the CALL: a caller that renders part of a launch and
 * wants the whole launch's bits passes the whole launch's value as cfg->sample_split. */
int32_t tn_render_sample_split(const tn_thermal_field *field, const tn_render_config *cfg, int64_t num_rays);
/* Segments per tile for the last partial round (tn_render_config.tail_balance) of `tiles` tiles on `slots` wave slots at
 * num_samples samples per ray; 1 = march whole tiles.  request 0: the k in 2..16 with segments of at least 12 samples that
 * minimises ceil(rem k / slots) / k, rem = tiles mod slots (the smallest such k), unless even that is above 0.95; request
 * k > 1: k, or fewer where the segments would be shorter than 12 samples.  Always 1 when tiles < slots (such calls belong to
 * sample_split) or rem == 0.  A pure function: (10 000, 2 048, 192) -> 9, 1 808 x 9 units = 7.95 rounds of one ninth. */
int32_t tn_render_tail_segments(int64_t tiles, int64_t slots, int32_t num_samples, int32_t request);
/* The same for a call of tn_field_render_fwd / _chunked_fwd under cfg (tail_balance, tail_slots, early termination, training,
 * kernel form, sample_split) on `field`; field == NULL: as for an exact-fp32 field (what tn_render_workspace_bytes assumes). */
int32_t tn_render_tail_plan(const tn_thermal_field *field, const tn_render_config *cfg, int64_t num_rays);
/* The bytes of records at the end of tn_render_workspace_bytes(cfg, num_rays): 0 where the plan is 1. */
size_t tn_render_tail_records_bytes(const tn_render_config *cfg, int64_t num_rays);
int tn_field_render_chunked_fwd(const tn_thermal_field *field, const tn_render_config *cfg, const tn_render_inputs *in,
                                const tn_render_outputs *out, int64_t num_rays, void *workspace, size_t workspace_bytes,
                                int64_t first_ray, int64_t chunk_rays, float *depth_bounds, int32_t clip, void *stream);
int tn_expected_depth_clip_chunked(float *expected_depth, int64_t num_rays, int64_t first_ray, int64_t chunk_rays,
                                   const float *depth_bounds, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Weight preparation (layout-only transforms, run once per weight update)
 * ---------------------------------------------------------------------------------------------------- */

/* dense re-layout of the coarse hash levels; fills grid_out->dense* fields (grid_out may alias grid_in). */
size_t tn_hashgrid_prepare_bytes(const tn_hashgrid *grid, int64_t max_bytes);
int tn_hashgrid_prepare(const tn_hashgrid *grid_in, tn_hashgrid *grid_out, void *dense_dev, size_t dense_bytes,
                        void *stream);

/* MFMA-fragment-ordered copy of the main field's MLP weights. */
size_t tn_field_prepare_bytes(const tn_thermal_field *field);
int tn_field_prepare(const tn_thermal_field *field, void *prepared_dev, size_t bytes, void *stream);

/* split-precision variants of the above (see tn_thermal_field.prepared_f16x3 / prepared_bf16x6). */
size_t tn_field_prepare_f16x3_bytes(const tn_thermal_field *field);
int tn_field_prepare_f16x3(const tn_thermal_field *field, void *prepared_dev, size_t bytes, void *stream);
size_t tn_field_prepare_bf16x6_bytes(const tn_thermal_field *field);
int tn_field_prepare_bf16x6(const tn_thermal_field *field, void *prepared_dev, size_t bytes, void *stream);

/* The operand split of mlp_precision = "bf16x6" on its own (test surface; no reference counterpart): per element i the three bf16
 * pieces of a[i] and b[i] — p1 = bf16(x), p2 = bf16(x - p1), p3 = bf16(x - p1 - p2), round to nearest even — written as floats to
 * pieces_a / pieces_b [n,3], and out[i] = the six piece products of order <= 2 accumulated in fp32 in the field kernel's order.
 * x = p1 + p2 + p3 exactly while p3 is representable (|x| >= 2^-110: its exponent is >= 2^-133, bf16's smallest sub-normal). */
int tn_bf16x6_split_product(const float *a, const float *b, int64_t n, float *pieces_a, float *pieces_b, float *out, void *stream);
/* One v_mfma_f32_32x32x16_bf16 with constant operands bf16(a_value), bf16(b_value): out[0] = 16 a b (fp32) — what the matrix core
 * does with sub-normal bf16 inputs (test surface). */
int tn_bf16_mfma_value_probe(float a_value, float b_value, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Training step: forward with a tape of per-sample activations, losses, backward.
 * The reference gets all of this from torch autograd over nerfstudio's modules
 * [REF thermal_nerf_model.py:210-326; nerfstudio model_components/losses.py]; here each differentiable stage
 * is one entry point on [N, width] fp32 row-major matrices (N = rays * samples of the level), the binding chains
 * them inside a torch.autograd.Function.  Gradient outputs marked (+=) are accumulated with atomics: zero them first.
 * ---------------------------------------------------------------------------------------------------- */

#define TN_ACT_NONE 0
#define TN_ACT_RELU 1
#define TN_ACT_SIGMOID 2

/* NS get_density position normalisation + HashEncoding.pytorch_fwd: positions [N,3] (world) ->
 * enc [N, 2*num_levels], selector [N] (0/1; the encoding is evaluated at p * selector like the reference). */
int tn_hash_encode_fwd(const tn_hashgrid *grid, const tn_space *space, const float *positions, int64_t n, float *enc,
                       float *selector, void *stream);
/* its backward w.r.t. the table: d_enc [N, 2*num_levels] -> d_table [num_levels << log2_hashmap_size, 2] (+=). */
int tn_hash_encode_bwd(const tn_hashgrid *grid, const tn_space *space, const float *positions, const float *d_enc,
                       int64_t n, float *d_table, void *stream);

/* tn_hash_encode_bwd restricted to the levels [level_begin, level_end) (d_enc keeps all num_levels columns). */
int tn_hash_encode_bwd_levels(const tn_hashgrid *grid, const tn_space *space, const float *positions, const float *d_enc,
                              int64_t n, float *d_table, int32_t level_begin, int32_t level_end, void *stream);
/* tn_hash_encode_bwd_levels with the COARSE levels (dense vertex grid of at most 48^3: scalings up to 46, the first four
 * levels of the reference grids) accumulated in 16 private dense copies of their vertex grids and summed into d_table by
 * a second launch: at those levels the samples of a trained scene hit the same few thousand entries, and same-address atomics
 * retire one at a time in the memory-side atomic unit.  Same sums (other order).  The workspace is cleared by the call;
 * levels outside the coarse set, or a call that does not start at level 0, run exactly as tn_hash_encode_bwd_levels. */
size_t tn_hash_encode_bwd_spread_workspace_bytes(const tn_hashgrid *grid);
int tn_hash_encode_bwd_spread(const tn_hashgrid *grid, const tn_space *space, const float *positions, const float *d_enc,
                              int64_t n, float *d_table, int32_t level_begin, int32_t level_end, void *workspace,
                              size_t workspace_bytes, void *stream);

/* The same adjoint without global atomics for the levels [level_begin, num_levels): contributions are written out as records
 * bucketed by the table slice (2^14 entries) that owns them and summed per slice in LDS, then added to d_table (+=) with plain
 * loads / stores.  Needs tn_hash_encode_bwd_sorted_workspace_bytes(grid, n, level_begin) bytes of 16-byte aligned device
 * scratch (a fixed region per (level, slice) bin sized 1.25 x an even spread: ~25 B per (sample, level, corner pair); a
 * record that does not fit its bin's region is added with global atomics instead); that function returns 0 — and tn_hash_encode_bwd_sorted
 * TN_ERR_UNSUPPORTED — for a geometry the bucketing does not cover (finest scaling + 2 >= 2^14 with more than one slice, or
 * >= 2^32 records).  tn_hash_encode_bwd_sorted_first_level: the level from which this form is the faster one on this part
 * (levels with a scaling >= 200, at least 128 (level, slice) bins), or -1: the caller runs tn_hash_encode_bwd_levels on the
 * levels below it and this on the rest. */
size_t tn_hash_encode_bwd_sorted_workspace_bytes(const tn_hashgrid *grid, int64_t n, int32_t level_begin);
int tn_hash_encode_bwd_sorted_first_level(const tn_hashgrid *grid, int64_t n);
int tn_hash_encode_bwd_sorted(const tn_hashgrid *grid, const tn_space *space, const float *positions, const float *d_enc,
                              int64_t n, float *d_table, int32_t level_begin, void *workspace, size_t workspace_bytes,
                              void *stream);

/* and w.r.t. the WORLD positions (camera-pose optimisation, NS CameraOptimizer applied at REF thermal_nerf_model.py:
 * 218-219): through the trilinear offsets, `p * selector`, (x + 2) / 4 and the L-inf contraction (or the AABB
 * normalisation): d_enc [N, 2*num_levels] -> d_positions [N,3] (=). */
int tn_hash_encode_bwd_input(const tn_hashgrid *grid, const tn_space *space, const float *positions, const float *d_enc,
                             int64_t n, float *d_positions, void *stream);
/* backward of tn_frustum_positions: d_positions [R,n,3] -> d_origins [R,3] (+=), d_directions [R,3] (+=). */
int tn_frustum_positions_bwd(const float *d_positions, const float *starts, const float *ends, int64_t num_rays, int32_t n,
                             float *d_origins, float *d_directions, void *stream);

/* torch.nn.Linear (+ activation): y[n, :out] = act(x[n, :in] W^T + b); x rows are ldx floats apart, y rows ldy.
 * in_dim, out_dim <= 256 (TN_ERR_SHAPE beyond).  Layers up to 64 wide — the reference's configs — keep a row's inputs in
 * registers; wider ones (config.hidden_dim / hidden_dim_color / hidden_dim_transient [REF thermal_nerf_model.py:96-114] above 64)
 * stage 64-row tiles of x in LDS, and their backward runs the 64-wide kernel once per 64 x 64 block of the weight matrix (it
 * needs the workspace: TN_ERR_WORKSPACE without one when weight gradients are asked for). */
int tn_linear_fwd(const float *x, int32_t ldx, const tn_linear *lin, int32_t act, int64_t n, float *y, int32_t ldy,
                  void *stream);
/* backward: g = dy * act'(y) (y = the forward OUTPUT, rows ldy apart like dy);  dx[n,:in] (= or += when
 * accumulate_dx) = g W;  d_weight [out,in] (+=) = g^T x;  d_bias [out] (+=) = sum_n g.  dx / d_weight / d_bias
 * may be NULL.  `workspace` (tn_linear_bwd_workspace_bytes(), reusable across calls on one stream) holds per-block
 * partial weight gradients summed by a second kernel; NULL falls back to one atomic per block and weight entry. */
size_t tn_linear_bwd_workspace_bytes(void);
int tn_linear_bwd(const float *x, int32_t ldx, const float *y, const float *dy, int32_t ldy, const tn_linear *lin,
                  int32_t act, int64_t n, float *dx, int32_t lddx, int32_t accumulate_dx, float *d_weight,
                  float *d_bias, void *workspace, size_t workspace_bytes, void *stream);

/* density = average_init_density * trunc_exp(raw) * selector (NS get_density); raw rows ld_raw floats apart.
 * backward: d_raw = d_density * average_init_density * exp(clamp(raw, trunc_exp_min, 15)) * selector (NS trunc_exp.backward:
 * trunc_exp_min = -15 is nerfstudio's / torch-ngp's two-sided clamp, -INFINITY clamps from above only), written to
 * column 0 of rows ld_d_raw apart; columns 1 .. clear_cols-1 of each row are set to zero (clear_cols <= 1: untouched) so that
 * the row can be the += target of the stages behind it without a separate fill. */
int tn_density_act_fwd(const float *raw, int32_t ld_raw, const float *selector, float average_init_density, int64_t n,
                       float *density, void *stream);
int tn_density_act_bwd(const float *raw, int32_t ld_raw, const float *selector, float average_init_density,
                       float trunc_exp_min, const float *d_density, int64_t n, float *d_raw, int32_t ld_d_raw,
                       int32_t clear_cols, void *stream);

/* backward of tn_weights_fwd: d_weights [R,n] -> d_densities [R,n]. */
int tn_weights_bwd(const float *deltas, const float *densities, const float *d_weights, int64_t num_rays, int32_t n,
                   float *d_densities, void *stream);

/* Backward of up to three CONSECUTIVE Linear(+activation) layers in one launch (an MLP's chain: mlp_head, mlp_thermal + head,
 * mlp_base).  layers[0] is the layer nearest the loss; layers[j].x = that layer's input rows (the ACTIVATED output of the
 * layer below, produced by activation act_x), so layers[j].lin.out_dim == layers[j-1].lin.in_dim.  dy [n, out_0] (rows lddy
 * apart) is the gradient w.r.t. layer 0's ACTIVATED output y_top (needed when act_top != none).  d_weight / d_bias (+=) per
 * layer, may be NULL; dx [n, in_last] (= or += when accumulate_dx) may be NULL.  Same arithmetic as num_layers calls of
 * tn_linear_bwd, with one [n, width] read per layer instead of three reads and a write. */
typedef struct tn_chain_layer {
    tn_linear lin;
    const float *x;
    int32_t ldx;
    int32_t act_x;   /* TN_ACT_* of the layer that produced x (unused for the last layer) */
    float *d_weight;
    float *d_bias;
} tn_chain_layer;
size_t tn_linear_chain_bwd_workspace_bytes(void);
int tn_linear_chain_bwd(const tn_chain_layer *layers, int32_t num_layers, const float *y_top, int32_t act_top, const float *dy,
                        int32_t lddy, int64_t n, float *dx, int32_t lddx, int32_t accumulate_dx, void *workspace,
                        size_t workspace_bytes, void *stream);

/* The final level's field forward of a training step in ONE launch [REF thermal_field.py:183-201 in train mode]: what the
 * chain tn_hash_encode_fwd -> tn_linear_fwd (mlp_base x2) -> tn_density_act_fwd -> tn_color_input_fwd -> tn_linear_fwd
 * (mlp_head x3, mlp_thermal x2, head) computes, with every activation the backward differentiates written to its tape
 * buffer in the same row-major layout: positions [N,3] (N = num_rays * n, ray-major), directions [R,3], camera_indices [R];
 * enc [N,32], selector [N], h1 [N,64] (ReLU applied), bo [N,16] (raw density | geo), density [N], c1, c2 [N,64] (ReLU),
 * rgb [N,3] (sigmoid), t1 [N,64] (ReLU), t2 [N,64] (sigmoid), thermal [N].  Needs field->prepared (tn_field_prepare on the
 * CURRENT weights); the reference geometry only (16 levels, geo 15, appearance 32). */
int tn_field_fwd_taped(const tn_thermal_field *field, const float *positions, const float *directions,
                       const int32_t *camera_indices, int64_t num_rays, int32_t n, float *enc, float *selector, float *h1,
                       float *bo, float *density, float *c1, float *c2, float *rgb, float *t1, float *t2, float *thermal,
                       void *stream);

/* The tape-free pair of the final level's training pass [REF thermal_field.py:108-201 differentiated; the modules
 * constructed at thermal_field.py:62-102].  tn_field_fwd_train is tn_field_fwd_taped keeping only what compositing, the
 * losses and the backward read: selector [N], density [N], rgb [N,3], thermal [N] and the hash features `enc`, the latter
 * in tiles of 64 consecutive samples, [ceil(N/64)][16 levels][64 samples][2] floats (the layout tn_field_bwd_fused reads;
 * allocate 32 * 64 * ceil(N/64) floats).  `ray_bias` [R,64] = mlp_head.0's
 * bias plus its SH(direction) and appearance-embedding columns applied to each ray's constants (tn_ray_head_fwd): the colour
 * layer sees them as a per-ray bias.  `base_out` (round 5; NULL to skip): mlp_base's 16 output rows [N,16] (raw density | geo
 * features) as well — 64 B per sample more — which tn_field_bwd_fused's split form then reads in its two head launches
 * instead of recomputing mlp_base there (pass the same pointer, or NULL to recompute).  `position_jacobian` (round 5; NULL to
 * skip; 96 * 64 * ceil(N/64) floats): d hash features / d normalised position, [ceil(N/64)][16 levels][3 axes][64 samples][2] —
 * the corner values are in registers in the forward; handed to tn_field_bwd_fused, its d_positions needs no table read.
 *
 * tn_field_bwd_fused recomputes the five hidden layers from `enc` in registers and runs their adjoints next to them (no
 * [N,64] activation ever touches HBM).  Inputs: enc / selector / rgb of the forward, ray_bias, the per-sample output
 * gradients d_rgb [N,3], d_thermal [N] (either may be NULL: that branch is skipped), d_density [N].  Outputs: d_enc [N,32]
 * (=), d_ray_sum [R,64] (+=, zero it first) = per-ray sums of mlp_head.0's pre-activation gradient — tn_ray_head_bwd then
 * yields mlp_head.0's bias gradient, its SH and appearance weight columns and the embedding / direction gradients — and the
 * gradients of every other Linear of the field (+=; NULL entries skipped; head0_w receives its geo columns 16..30 only).
 * d_positions [N,3] (=; NULL to skip; needs `positions` [N,3]): d loss / d sample position through the hash encoding — what
 * tn_hash_encode_bwd_input computes from d_enc — for camera-pose optimisation, produced by the mlp_base launch.
 * trunc_exp_min: lower clamp of trunc_exp's backward (g * exp(clamp(x, min, 15)); -15 = torch-ngp / nerfstudio's
 * two-sided clamp, -INFINITY = upper clamp only).  pass_thermal_gradients = 0 keeps the thermal branch from the geo
 * features [REF thermal_field.py:171-172].  split = 0: one launch for the whole field (one wave per SIMD: its ~210 gradient
 * accumulators); 1: the colour head and (thermal head + mlp_base) as two launches of two waves per SIMD each, the colour
 * head's adjoint of mlp_base's outputs passing through the workspace; 2 (round 5): the split form with the products whose K
 * is a multiple of 32 features — the 64 x 64 ones of the two head launches (second layer: recomputed forward and dx; with
 * base_out only) and mlp_base.0's forward and dx in the mlp_base launch — on v_mfma_f32_16x16x32_bf16 as six products of three
 * exact bf16 pieces per operand: fp32's rounding size per product (see tn_bf16x6_split_product).  The parameter gradients of
 * all launches leave through ONE slab reduction at the end.  The reference geometry only (16 levels, geo 15, appearance 32). */
/* One proposal level of a step on which the proposal networks take gradient, forward and backward in one launch each
 * [HashMLPDensityField built at REF thermal_nerf_model.py:127-149: 5 levels -> Linear(10,16)+ReLU -> Linear(16,1) -> trunc_exp]:
 * forward writes what tn_hash_encode_fwd + 2 x tn_linear_fwd + tn_density_act_fwd write (enc [n,10], selector, raw, density
 * [n]); backward takes d_density [n] to d_enc [n,10] (=) and the four parameter gradients (+=), the hidden layer recomputed
 * from enc.  The reference geometry only (5 levels, hidden 16): TN_ERR_UNSUPPORTED otherwise (use the stage entry points). */
int tn_density_fwd_train(const tn_density_field *f, const float *positions, int64_t n, float *enc, float *selector, float *raw,
                         float *density, void *stream);
int tn_density_bwd_train(const tn_density_field *f, const float *enc, const float *raw, const float *selector,
                         const float *d_density, int64_t n, float trunc_exp_min, float *d_enc, float *d_w0, float *d_b0,
                         float *d_w1, float *d_b1, void *stream);

/* mlp_head.0's ray-constant part [REF thermal_field.py:117-126,160-168]: ray_bias [R,64] = bias + W[:, 0:16] . SH(direction) +
 * W[:, 31:63] . embedding[camera] (training-mode appearance), and its adjoint on the per-ray sums d_ray_sum [R,64] of the layer's
 * pre-activation gradient: d_head0_weight (+=, the SH and appearance columns only), d_head0_bias (+=), d_appearance
 * [num_images, 32] (+=), and optionally d_ray_inputs [R,64] (=; columns 0..15 = gradient w.r.t. the SH basis values, which
 * tn_color_input_bwd with n = 1 carries on to the directions). */
int tn_ray_head_fwd(const tn_thermal_field *field, const float *directions, const int32_t *camera_indices, int64_t num_rays,
                    float *ray_bias, void *stream);
int tn_ray_head_bwd(const tn_thermal_field *field, const float *directions, const int32_t *camera_indices, int64_t num_rays,
                    const float *d_ray_sum, float *d_head0_weight, float *d_head0_bias, float *d_appearance, float *d_ray_inputs,
                    void *stream);
typedef struct tn_field_grads {
    float *base0_w, *base0_b, *base1_w, *base1_b;
    float *head0_w, *head1_w, *head1_b, *head2_w, *head2_b;
    float *th0_w, *th0_b, *th1_w, *th1_b, *thead_w, *thead_b;
} tn_field_grads;
int tn_field_fwd_train(const tn_thermal_field *field, const float *positions, const float *ray_bias, int64_t num_rays,
                       int32_t n, float *enc, float *selector, float *density, float *rgb, float *thermal, float *base_out,
                       float *position_jacobian, void *stream);
size_t tn_field_bwd_fused_workspace_bytes(int64_t num_rays, int32_t n);
int tn_field_bwd_fused(const tn_thermal_field *field, int64_t num_rays, int32_t n, const float *enc, const float *selector,
                       const float *base_out, const float *ray_bias, const float *rgb, const float *d_rgb, const float *d_thermal,
                       const float *d_density, int32_t pass_thermal_gradients, float trunc_exp_min, int32_t split,
                       float *d_enc, float *d_ray_sum, const float *positions, const float *position_jacobian,
                       float *d_positions, const tn_field_grads *grads, void *workspace, size_t workspace_bytes, void *stream);

/* NS scale_gradients_by_distance_squared [REF thermal_nerf_model.py:228-231, use_gradient_scaling]: the forward is the
 * identity; in the backward the gradient of EVERY field output of a sample (density [n], rgb [n,3], thermal [n]; any may
 * be NULL) is multiplied in place by clamp(((start + end) / 2)^2, 0, 1).  starts/ends [n]. */
int tn_gradient_scale_bwd(const float *starts, const float *ends, int64_t n, float *d_density, float *d_rgb,
                          float *d_thermal, void *stream);

/* NS CameraOptimizer(mode="SO3xR3").apply_to_raybundle — the first statement of the training forward
 * [REF thermal_nerf_model.py:218-219]: with M_c = exp_map_SO3xR3(pose_adjustment[c]) ([t | w] -> [R(w) | t], Rodrigues with
 * theta = sqrt(max(|w|^2, 1e-4))), out_origins = origins + t_c, out_directions = R(w_c) directions, c = camera_indices[ray]
 * (int64, as nerfstudio's ray bundles carry them; 0 <= c < num_cameras is the caller's contract).  pose_adjustment
 * [num_cameras, 6], origins / directions / outputs [R,3]; outputs may alias the inputs. */
int tn_camera_opt_fwd(const float *pose_adjustment, const int64_t *camera_indices, const float *origins,
                      const float *directions, int64_t num_rays, int32_t num_cameras, float *out_origins,
                      float *out_directions, void *stream);

/* its backward: d_out_origins / d_out_directions [R,3] (either may be NULL = zero), directions = the INPUT directions of the
 * forward -> d_pose_adjustment [num_cameras, 6] (+=, caller clears it; torch.clamp's sub-gradient: theta is a constant where
 * |w|^2 < 1e-4), optional d_directions [R,3] (=) = R^T d_out_directions.  d origins = d_out_origins (identity, not written). */
int tn_camera_opt_bwd(const float *pose_adjustment, const int64_t *camera_indices, const float *directions,
                      const float *d_out_origins, const float *d_out_directions, int64_t num_rays, int32_t num_cameras,
                      float *d_pose_adjustment, float *d_directions, void *stream);

/* backward of tn_composite_fwd in training mode (no nan_to_num / clamp): d_out [R,C], accumulation [R] ->
 * d_values [R,n,C] (=), d_weights [R,n] (+=). */
int tn_composite_bwd(const float *values, const float *weights, const float *accumulation, const float *d_out,
                     int64_t num_rays, int32_t n, int32_t channels, float *d_values, float *d_weights, void *stream);

/* input of mlp_head [REF thermal_field.py:160-167]: cin [R*n, 64] = [SH16(dir) | geo | appearance | 0];
 * geo rows ld_geo floats apart; training != 0: embedding[camera_indices[r]], else mean / zeros [REF :124-137]. */
int tn_color_input_fwd(const tn_thermal_field *field, const float *directions, const float *geo, int32_t ld_geo,
                       const int32_t *camera_indices, int32_t training, int64_t num_rays, int32_t n, float *cin,
                       void *stream);
/* backward: d_cin [R*n,64] -> d_geo (+=, rows ld_d_geo apart), d_appearance [num_images, app_dim] (+=; training),
 * d_directions [R,3] (+=; through the SH basis; NULL to skip, needs `directions`). */
int tn_color_input_bwd(const tn_thermal_field *field, const float *d_cin, const int32_t *camera_indices,
                       int32_t training, int64_t num_rays, int32_t n, float *d_geo, int32_t ld_d_geo,
                       float *d_appearance, const float *directions, float *d_directions, void *stream);

/* The final level's per-ray renderers of a training step in one launch, and their adjoints in one launch: weights =
 * RaySamples.get_weights(density) [REF thermal_nerf_model.py:233] [R,n], rgb [R,3] / thermal [R] = "last_sample" compositing
 * [REF :237, :271-273; thermal_renderer.py:55-79], accumulation [R] (what tn_weights_fwd + 2 x tn_composite_fwd compute).
 * Backward: d_rgb [R,3], d_thermal [R], d_accumulation [R], d_weights [R,n] (the regularisers' gradient) — each may be NULL
 * — to d_rgb_samples [R n,3], d_thermal_samples [R n], d_densities [R n] (=); starts / ends [R n] non-NULL apply
 * scale_gradients_by_distance_squared [REF :228-231] to the three.  n <= 1024. */
int tn_ray_render_fwd(const float *deltas, const float *densities, const float *rgb_samples, const float *thermal_samples,
                      int64_t num_rays, int32_t n, float *weights, float *rgb, float *thermal, float *accumulation, void *stream);
/* tn_ray_render_fwd + tn_depth_fwd(median, expected) of the same level in one pass [REF thermal_nerf_model.py:233-243]: the weights
 * are in registers when the depth renderers need them.  Bit-equal outputs to the two calls; the expected depth's call-global clip
 * [NS DepthRenderer("expected")] reduces per-block bounds instead of two atomically updated words: bounds_scratch holds
 * 2 * ceil(num_rays / 4) floats and needs no initialisation. */
int tn_ray_render_depth_fwd(const float *deltas, const float *densities, const float *rgb_samples, const float *thermal_samples,
                            const float *starts, const float *ends, int64_t num_rays, int32_t n, float *weights, float *rgb,
                            float *thermal, float *accumulation, float *median, float *expected, float *bounds_scratch, void *stream);
int tn_ray_render_bwd(const float *deltas, const float *densities, const float *rgb_samples, const float *thermal_samples,
                      const float *accumulation, const float *d_rgb, const float *d_thermal, const float *d_accumulation,
                      const float *d_weights, const float *starts, const float *ends, int64_t num_rays, int32_t n,
                      float *d_rgb_samples, float *d_thermal_samples, float *d_densities, void *stream);

/* The two image losses of get_loss_dict [REF thermal_nerf_model.py:294-295, 319-323: MSELoss means] and the PSNR of NS
 * get_metrics_dict in one launch: rgb / gt_rgb [R,3], thermal / gt_thermal [R] (thermal may be NULL) -> out[0] = rgb MSE,
 * out[1] = thermal MSE, out[2] = 10 log10(1 / out[0]); d_rgb [R,3] (=) and d_thermal [R] (=) = the gradients of the two means. */
int tn_image_losses(const float *rgb, const float *gt_rgb, const float *thermal, const float *gt_thermal, int64_t num_rays,
                    float *out, float *d_rgb, float *d_thermal, void *stream);

/* The step's total loss as nerfstudio's Trainer forms it — functools.reduce(torch.add, loss_dict.values()) [NS Trainer.train_iteration,
 * driven by REF thermo_nerf/thermal_nerf/config_thermal_nerf.py:17-30] — in one launch: out[0] = ((t0 + t1) + t2) + ...;
 * `terms` is a HOST array of `count` <= TN_SUM_MAX_TERMS device pointers to one float each. */
#define TN_SUM_MAX_TERMS 16
int tn_sum_scalars(const float *const *terms, int32_t count, float *out, void *stream);

/* NS losses.distortion_loss on one level: spacing bins [R,n+1], weights [R,n] -> loss_sum[0] (+=) = scale * sum over rays
 * of lossfun_distortion (scale = 1/R for nerfstudio's mean), d_weights [R,n] (=) = scale * d(sum)/dw.  O(n) per ray. */
int tn_distortion_loss(const float *spacing_bins, const float *weights, int64_t num_rays, int32_t n, float scale,
                       float *loss_sum, float *d_weights, void *stream);
/* the metric and the loss term NerfactoModel makes of it (metrics_dict["distortion"], then distortion_loss_mult * that
 * [REF thermal_nerf_model.py:301-304]) from the same launch: loss_pair[0] (+=) = scale * sum, loss_pair[1] (+=) = mult * scale *
 * sum, d_weights [R,n] (=) = the gradient of loss_pair[1]. */
int tn_distortion_loss_term(const float *spacing_bins, const float *weights, int64_t num_rays, int32_t n, float scale,
                            float mult, float *loss_pair, float *d_weights, void *stream);
/* NS losses.interlevel_loss, one proposal level: final bins c [R,n+1] / weights w [R,n] (constants), proposal bins
 * cp [R,p+1] / weights wp [R,p] -> loss_sum[0] (+=) = scale * sum over rays and samples of lossfun_outer (scale = 1/(R*n)),
 * d_wp [R,p] (=) = scale * d(sum)/dwp.  p <= 1024.  Several levels may add into the same loss_sum. */
int tn_interlevel_loss(const float *c, const float *w, const float *cp, const float *wp, int64_t num_rays, int32_t n,
                       int32_t p, float scale, float *loss_sum, float *d_wp, void *stream);
/* every proposal level of NS interlevel_loss in one launch (the levels are independent): cp / wp / d_wp are HOST arrays of
 * num_levels (<= 4) device pointers, p the levels' sample counts; same sums as num_levels calls of tn_interlevel_loss. */
int tn_interlevel_loss_levels(const float *c, const float *w, int64_t num_rays, int32_t n, int32_t num_levels,
                              const float *const *cp, const float *const *wp, const int32_t *p, float scale, float *loss_sum,
                              float *const *d_wp, void *stream);

/* ---- the training step's launch chains as two calls -------------------------------------------------------------------------
 * What ThermalNerfModel.get_outputs [REF thermal_nerf_model.py:210-275] queues in training mode on a step whose proposal networks
 * take no gradient (nerfstudio's ProposalNetworkSampler: 5 steps of 6 after warm-up), and the adjoint chain autograd runs for it —
 * the SAME entry points as above, in the same order and on the same streams as the per-call host path queues them (bit-identical
 * results), issued from C++: a step is ~20 launches whose Python cost (one ctypes call and ~2 output allocations each) decided the
 * step at the reference's default S = 48.  Every buffer is the caller's; the cross-stream order is made with events
 * created and destroyed inside the call (no state is kept).
 *
 * tn_train_step_fwd:  tn_field_prepare(field_raw -> field->prepared) | tn_proposal_sample_fwd (train-mode, untaped) |
 *   tn_frustum_from_edges | tn_ray_head_fwd | [wait for `wait_events`: a deferred table update of the previous step] |
 *   tn_field_fwd_train | tn_ray_render_depth_fwd | the two regularisers on `second` / `third` behind the level's weights (when their
 *   loss pointers are set: tn_distortion_loss_term, tn_interlevel_loss_levels).
 * tn_train_step_bwd:  tn_ray_render_bwd | tn_field_bwd_fused | the table scatter — tn_hash_encode_bwd_sorted on `second` beside
 *   tn_hash_encode_bwd_spread / _levels for the levels below `first_sorted_level` on `stream` (defer == 0: `stream` waits for
 *   `second` at the end) or on `third` (defer != 0: nobody waits — the caller joins, thermo_nerf_amd/_hip.py) | the ray-level
 *   adjoints on `stream`: tn_ray_head_bwd (+ tn_color_input_bwd with sh_direction_gradient), tn_frustum_positions_bwd. */
typedef struct tn_train_step {
    const tn_density_field *prop0, *prop1;
    const tn_thermal_field *field_raw;   /* the field as stored (what tn_field_prepare reads)                          */
    const tn_thermal_field *field;       /* the same with `prepared` -> a buffer of prepared_bytes this call (re)fills  */
    size_t prepared_bytes;
    const tn_render_config *cfg;         /* training = 1; sample counts, anneal, initial sampler, jitter form          */
    const tn_render_inputs *in;          /* rays, planes, camera indices (int32), jitter, bin tables                   */
    int64_t num_rays;
    /* kept for the backward (caller-allocated) */
    float *spacing[3], *eucl[3];         /* [R, n+1] per level                                                          */
    float *weights[3];                   /* [R, n]                                                                      */
    float *prop_depth[2];                /* [R]                                                                         */
    float *positions;                    /* [R S, 3]                                                                    */
    float *starts, *ends, *deltas;       /* [R, S]                                                                      */
    float *ray_bias;                     /* [R, 64]                                                                     */
    float *enc, *selector, *density, *rgb_samples, *thermal_samples, *base_out, *jacobian; /* tn_field_fwd_train's      */
    float *rgb, *thermal, *accumulation, *depth, *expected_depth, *depth_scratch; /* [R,3] [R] [R] [R] [R] [2 ceil(R/4)] */
    void *workspace;                     /* tn_render_workspace_bytes(cfg, num_rays)                                    */
    size_t workspace_bytes;
    void *zero_buffer;                   /* optional: cleared (hipMemsetAsync) on `second` at the start of the call — the  */
    size_t zero_bytes;                   /* backward's gradient arena, off the calling stream (tn_train_step_bwd waits);   */
                                         /* `second` first waits for everything queued on `stream` (the buffer's memory may */
                                         /* have been an earlier step's gradients, still read by kernels queued there)      */
    /* regularisers (optional: loss pointers NULL = not launched); losses are += accumulators the caller zeroed         */
    float distortion_mult, interlevel_mult;
    float *distortion_loss_pair, *distortion_grad;   /* [2], [R,S]                                                      */
    float *interlevel_loss, *interlevel_grad[2];     /* [1], [R,P0], [R,P1]                                             */
    /* streams; wait_events: hipEvent_t handles `stream` waits for right before the field's first table read            */
    void *stream, *second, *third;
    void *const *wait_events;
    int32_t num_wait_events;
} tn_train_step;
int tn_train_step_fwd(const tn_train_step *s);

typedef struct tn_train_step_bwd_args {
    const tn_thermal_field *field;       /* raw struct (no prepared blob needed)                                        */
    int64_t num_rays;
    int32_t n;                           /* samples per ray of the final level                                          */
    /* the forward's tensors */
    const float *positions, *starts, *ends, *deltas, *ray_bias, *enc, *selector, *density, *rgb_samples, *thermal_samples;
    const float *base_out, *jacobian, *accumulation, *directions;
    const int32_t *camera_indices;
    /* incoming gradients (any may be NULL) */
    const float *d_rgb, *d_thermal, *d_accumulation, *d_weights;
    int32_t use_gradient_scaling, pass_thermal_gradients, split_form, sh_direction_gradient;
    float trunc_exp_min;
    /* scratch the call fills: [R S,3] [R S] [R S] [R S,32] [R S,3 or NULL] [R,64 zeroed or NULL] [R,64 or NULL]        */
    float *d_rgb_samples, *d_thermal_samples, *d_density, *d_enc, *d_positions, *d_ray_sum, *d_ray_inputs;
    const tn_field_grads *grads;         /* zero-initialised parameter gradients (+=)                                   */
    float *d_table, *d_appearance, *d_head0_bias; /* zeroed (+=); mlp_head.0's bias gradient is the ray-level adjoint's         */
    float *d_origins, *d_directions;     /* [R,3] zeroed (+=) or NULL: no ray gradients                                 */
    void *fused_workspace; size_t fused_workspace_bytes;      /* tn_field_bwd_fused_workspace_bytes                     */
    int32_t first_sorted_level;          /* tn_hash_encode_bwd_sorted_first_level; < 0: every level with atomics        */
    void *sorted_workspace; size_t sorted_workspace_bytes;
    int32_t spread;                      /* config.spread_coarse_scatter                                                */
    void *spread_workspace; size_t spread_workspace_bytes;    /* of the stream the atomic levels run on                 */
    int32_t overlap, defer;              /* config.overlap_table_scatter / deferred_table_update                        */
    int32_t wait_second_first;           /* the gradients were cleared on `second` by tn_train_step_fwd (zero_buffer)   */
    void *stream, *second, *third;
} tn_train_step_bwd_args;
int tn_train_step_bwd(const tn_train_step_bwd_args *a);

/* ---- optimizer ------------------------------------------------------------------------------------------------------------
 * torch.optim.Adam as the reference's method config sets it for every parameter group — AdamOptimizerConfig(lr 1e-2,
 * eps 1e-15), nerfstudio's Optimizers.optimizer_step_all [REF thermo_nerf/thermal_nerf/config_thermal_nerf.py:31-44;
 * thermo_nerf/nerfacto_config/config_nerfacto.py:28-34 for camera_opt's weight decay] — over a LIST of tensors in ONE launch:
 *     g = grad + weight_decay * param ;  m += (1 - beta1) (g - m) ;  v = beta2 v + (1 - beta2) g g ;
 *     param -= step_size * m / (sqrt(v) / bias_correction2_sqrt + eps)
 * with the step-dependent scalars formed by the caller (step_size = lr / (1 - beta1^t), bias_correction2_sqrt =
 * sqrt(1 - beta2^t), t = the tensor's own step count): tensors of different groups and step counts share a launch.
 * `tensors` is a HOST array of `count` <= TN_ADAM_MAX_TENSORS descriptors (device pointers inside); param / exp_avg /
 * exp_avg_sq are updated in place, grad is read only; tensors with n = 0 are skipped (their pointers may be NULL).  The four
 * pointers need no alignment beyond a float's and may differ in it.
 * THE RESULT IS DEFINED: every output float is the following sequence of correctly rounded fp32 operations (round to nearest
 * even, no contraction) on the element's four inputs and the descriptor's seven scalars, one operation per line item:
 *     g' = grad + weight_decay * param                      product, sum          (skipped when weight_decay == 0: g' = grad)
 *     m' = exp_avg + (g' - exp_avg) * one_minus_beta1       difference, product, sum
 *     v' = beta2 * exp_avg_sq + (one_minus_beta2 * g') * g' product | product, product | sum
 *     den = sqrt(v') / bias_correction2_sqrt + eps          root, quotient, sum
 *     param' = param - step_size * (m' / den)               quotient, product, difference
 * exp_avg <- m', exp_avg_sq <- v', param <- param'.  Subnormal operands and results are kept, in every operation (v' of a
 * gradient of 1e-20 is one).  Where the sequence gives a NaN (an inf or NaN gradient; 0 / 0 with zero moments, zero gradient and
 * eps == 0) the output is a NaN whose sign and payload are not defined; no other element is affected.  Nothing outside
 * [0, n) of any array is read or written.  tests/adam_reference.py restates the sequence; tests/test_gpu_adam.py asserts it bit
 * for bit. */
#define TN_ADAM_MAX_TENSORS 32
typedef struct tn_adam_tensor {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int64_t n;
    float step_size;
    float bias_correction2_sqrt;
    float one_minus_beta1;
    float beta2;
    float one_minus_beta2;
    float eps;
    float weight_decay;
} tn_adam_tensor;
int tn_adam_step(const tn_adam_tensor *tensors, int32_t count, void *stream);

/* library identification: returns a static string "thermonerf_hip <version> gfx950". */
const char *tn_version(void);

#ifdef __cplusplus
}
#endif
#endif /* THERMONERF_HIP_H */
