"""ctypes binding of ``libthermonerf_hip.so`` (the C-ABI declared in ``include/thermonerf_hip.h``).

This is the only place the package touches the native library.  There is NO fallback: if the shared
object is missing or a symbol cannot be resolved, importing callers get a ``RuntimeError`` — the product
path never silently degrades to PyTorch/CPU arithmetic.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_LIB_NAME = "libthermonerf_hip.so"
# THERMONERF_HIP_LIB: load a differently-built copy of the same library (kernel A/B experiments only)
_LIB_PATH = os.environ.get("THERMONERF_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), _LIB_NAME)

TN_MAX_LEVELS = 16

TN_OK = 0
_ERRORS = {
    -1: "TN_ERR_NULL: a required pointer is NULL",
    -2: "TN_ERR_SHAPE: a dimension is out of the supported range",
    -3: "TN_ERR_UNSUPPORTED: configuration not implemented by the kernels",
    -4: "TN_ERR_WORKSPACE: workspace too small",
    -5: "TN_ERR_LAUNCH: HIP reported a launch error",
}

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)


class tn_hashgrid(C.Structure):
    _fields_ = [
        ("table", C.c_void_p),
        ("scalings", C.c_float * TN_MAX_LEVELS),
        ("num_levels", C.c_int32),
        ("log2_hashmap_size", C.c_int32),
        ("dense", C.c_void_p),
        ("dense_offset", C.c_int64 * TN_MAX_LEVELS),
        ("dense_res", C.c_int32 * TN_MAX_LEVELS),
        ("num_dense_levels", C.c_int32),
        ("_pad", C.c_int32),
    ]


class tn_linear(C.Structure):
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("in_dim", C.c_int32), ("out_dim", C.c_int32)]


class tn_chain_layer(C.Structure):
    _fields_ = [("lin", tn_linear), ("x", C.c_void_p), ("ldx", C.c_int32), ("act_x", C.c_int32), ("d_weight", C.c_void_p),
                ("d_bias", C.c_void_p)]


class tn_adam_tensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("n", C.c_int64),
                ("step_size", C.c_float), ("bias_correction2_sqrt", C.c_float), ("one_minus_beta1", C.c_float), ("beta2", C.c_float),
                ("one_minus_beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float)]


ADAM_MAX_TENSORS = 32  # TN_ADAM_MAX_TENSORS

class tn_field_grads(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("base0_w", "base0_b", "base1_w", "base1_b", "head0_w", "head1_w", "head1_b", "head2_w",
                                         "head2_b", "th0_w", "th0_b", "th1_w", "th1_b", "thead_w", "thead_b")]


class tn_space(C.Structure):
    _fields_ = [
        ("contraction", C.c_int32),
        ("aabb_min", C.c_float * 3),
        ("aabb_max", C.c_float * 3),
        ("_pad", C.c_int32),
    ]


class tn_pointcloud_params(C.Structure):
    _fields_ = [("min_accumulation", C.c_float), ("box_min", C.c_float * 3), ("box_max", C.c_float * 3), ("thermal_lo", C.c_float),
                ("thermal_hi", C.c_float), ("temperature_span", C.c_float), ("temperature_min", C.c_float),
                ("to_world", C.c_float * 12)]


class tn_voxel_params(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("voxel_size", C.c_float), ("dims", C.c_int32 * 3)]


class tn_mesh_region(C.Structure):
    _fields_ = [("area", C.c_double), ("label", C.c_int32), ("faces", C.c_int32), ("mean_temperature", C.c_float),
                ("min_temperature", C.c_float), ("max_temperature", C.c_float), ("centroid", C.c_float * 3), ("bounds", C.c_float * 6),
                ("coldest_vertex", C.c_int32), ("hottest_vertex", C.c_int32)]


class tn_raster_view(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("right", C.c_double * 3), ("down", C.c_double * 3), ("forward", C.c_double * 3),
                ("pixel_size", C.c_double), ("near", C.c_double), ("far", C.c_double), ("width", C.c_int32), ("height", C.c_int32),
                ("cull", C.c_int32), ("reserved", C.c_int32)]


class tn_raycast_params(C.Structure):
    _fields_ = [("t_min", C.c_double), ("t_max", C.c_double), ("cull", C.c_int32), ("mode", C.c_int32)]


TN_RAYCAST_CLOSEST, TN_RAYCAST_ANY = 0, 1


class tn_closest_params(C.Structure):
    _fields_ = [("max_distance", C.c_double), ("reserved", C.c_int32 * 2)]


class tn_project_camera(C.Structure):
    _fields_ = [("c2w", C.c_float * 12), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


class tn_project_params(C.Structure):
    _fields_ = [("t_lo", C.c_double), ("t_hi", C.c_double), ("min_cos", C.c_double), ("near", C.c_double), ("width", C.c_int32),
                ("height", C.c_int32), ("two_sided", C.c_int32), ("reserved", C.c_int32)]


class tn_register_params(C.Structure):
    _fields_ = [("max_distance", C.c_double), ("center", C.c_double * 3), ("length", C.c_double), ("damping", C.c_double),
                ("tolerance", C.c_double), ("iterations", C.c_int32), ("metric", C.c_int32), ("with_scale", C.c_int32),
                ("min_pairs", C.c_int32), ("reserved", C.c_int32 * 2)]


class tn_mesh_curve(C.Structure):
    _fields_ = [("length", C.c_double), ("level", C.c_int32), ("first_point", C.c_int32), ("points", C.c_int32), ("closed", C.c_int32),
                ("mean_temperature", C.c_float), ("min_temperature", C.c_float), ("max_temperature", C.c_float),
                ("first_face", C.c_int32)]


class tn_isoline_params(C.Structure):
    _fields_ = [("normal", C.c_double * 3), ("num_levels", C.c_int32), ("reserved", C.c_int32), ("levels", C.c_double * 256)]


class tn_mesh_patch(C.Structure):
    _fields_ = [("area", C.c_double), ("thermal_area", C.c_double), ("plane", C.c_double * 4), ("centroid", C.c_double * 3),
                ("flatness", C.c_float), ("rms_deviation", C.c_float), ("max_deviation", C.c_float), ("mean_temperature", C.c_float),
                ("min_temperature", C.c_float), ("max_temperature", C.c_float), ("bounds", C.c_float * 6), ("label", C.c_int32),
                ("faces", C.c_int32), ("thermal_faces", C.c_int32), ("reserved", C.c_int32)]


TN_REGISTER_POINT, TN_REGISTER_PLANE = 0, 1
TN_REGISTER_STATUS = ("converged", "iterations", "too_few", "degenerate")  # the words of result[0]


class tn_mesh_params(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("w2c", C.c_float * 12),
                ("truncation", C.c_float), ("inv_truncation", C.c_float), ("min_accumulation", C.c_float), ("lo", C.c_float * 3),
                ("step", C.c_float * 3), ("dims", C.c_int32 * 3), ("temperature_span", C.c_float), ("temperature_min", C.c_float),
                ("to_world", C.c_float * 12)]


class tn_density_field(C.Structure):
    _fields_ = [
        ("grid", tn_hashgrid),
        ("l0", tn_linear),
        ("l1", tn_linear),
        ("space", tn_space),
        ("average_init_density", C.c_float),
        ("_pad", C.c_int32),
    ]


class tn_thermal_field(C.Structure):
    _fields_ = [
        ("grid", tn_hashgrid),
        ("base0", tn_linear),
        ("base1", tn_linear),
        ("head0", tn_linear),
        ("head1", tn_linear),
        ("head2", tn_linear),
        ("th0", tn_linear),
        ("th1", tn_linear),
        ("thead", tn_linear),
        ("appearance", C.c_void_p),
        ("num_images", C.c_int32),
        ("app_dim", C.c_int32),
        ("geo_feat_dim", C.c_int32),
        ("use_average_appearance", C.c_int32),
        ("sh_shifted", C.c_int32),
        ("space", tn_space),
        ("average_init_density", C.c_float),
        ("prepared", C.c_void_p),
        ("prepared_f16x3", C.c_void_p),
        ("prepared_bf16x6", C.c_void_p),
    ]


class tn_render_config(C.Structure):
    _fields_ = [
        ("num_proposal_samples", C.c_int32 * 2),
        ("num_nerf_samples", C.c_int32),
        ("training", C.c_int32),
        ("pdf_anneal", C.c_float),
        ("early_stop_transmittance", C.c_float),
        ("kernel_family", C.c_int32),
        ("initial_sampler", C.c_int32),
        ("sample_split", C.c_int32),
        ("per_sample_jitter", C.c_int32),
        ("tail_balance", C.c_int32),
        ("tail_slots", C.c_int32),
    ]


class tn_render_inputs(C.Structure):
    _fields_ = [
        ("origins", C.c_void_p),
        ("directions", C.c_void_p),
        ("nears", C.c_void_p),
        ("fars", C.c_void_p),
        ("camera_indices", C.c_void_p),
        ("lin_bins0", C.c_void_p),
        ("u1", C.c_void_p),
        ("u2", C.c_void_p),
        ("jitter", C.c_void_p),
    ]


class tn_render_outputs(C.Structure):
    _fields_ = [
        ("rgb", C.c_void_p),
        ("accumulation", C.c_void_p),
        ("depth", C.c_void_p),
        ("expected_depth", C.c_void_p),
        ("prop_depth_0", C.c_void_p),
        ("prop_depth_1", C.c_void_p),
        ("thermal", C.c_void_p),
        ("weights", C.c_void_p * 3),
        ("spacing_bins", C.c_void_p * 3),
        ("eucl_bins", C.c_void_p * 3),
    ]


_fp = C.c_void_p  # a device pointer


class tn_train_step(C.Structure):
    _fields_ = [("prop0", C.POINTER(tn_density_field)), ("prop1", C.POINTER(tn_density_field)),
                ("field_raw", C.POINTER(tn_thermal_field)), ("field", C.POINTER(tn_thermal_field)), ("prepared_bytes", C.c_size_t),
                ("cfg", C.POINTER(tn_render_config)), ("inputs", C.POINTER(tn_render_inputs)), ("num_rays", C.c_int64),
                ("spacing", _fp * 3), ("eucl", _fp * 3), ("weights", _fp * 3), ("prop_depth", _fp * 2),
                ("positions", _fp), ("starts", _fp), ("ends", _fp), ("deltas", _fp), ("ray_bias", _fp),
                ("enc", _fp), ("selector", _fp), ("density", _fp), ("rgb_samples", _fp), ("thermal_samples", _fp), ("base_out", _fp),
                ("jacobian", _fp),
                ("rgb", _fp), ("thermal", _fp), ("accumulation", _fp), ("depth", _fp), ("expected_depth", _fp), ("depth_scratch", _fp),
                ("workspace", _fp), ("workspace_bytes", C.c_size_t), ("zero_buffer", _fp), ("zero_bytes", C.c_size_t),
                ("distortion_mult", C.c_float), ("interlevel_mult", C.c_float),
                ("distortion_loss_pair", _fp), ("distortion_grad", _fp), ("interlevel_loss", _fp), ("interlevel_grad", _fp * 2),
                ("stream", _fp), ("second", _fp), ("third", _fp), ("wait_events", C.POINTER(C.c_void_p)), ("num_wait_events", C.c_int32)]


class tn_train_step_bwd_args(C.Structure):
    _fields_ = [("field", C.POINTER(tn_thermal_field)), ("num_rays", C.c_int64), ("n", C.c_int32)] + [
        (k, _fp) for k in ("positions", "starts", "ends", "deltas", "ray_bias", "enc", "selector", "density", "rgb_samples",
                           "thermal_samples", "base_out", "jacobian", "accumulation", "directions", "camera_indices",
                           "d_rgb", "d_thermal", "d_accumulation", "d_weights")] + [
        ("use_gradient_scaling", C.c_int32), ("pass_thermal_gradients", C.c_int32), ("split_form", C.c_int32),
        ("sh_direction_gradient", C.c_int32), ("trunc_exp_min", C.c_float)] + [
        (k, _fp) for k in ("d_rgb_samples", "d_thermal_samples", "d_density", "d_enc", "d_positions", "d_ray_sum", "d_ray_inputs")] + [
        ("grads", C.POINTER(tn_field_grads)), ("d_table", _fp), ("d_appearance", _fp), ("d_head0_bias", _fp), ("d_origins", _fp),
        ("d_directions", _fp), ("fused_workspace", _fp), ("fused_workspace_bytes", C.c_size_t), ("first_sorted_level", C.c_int32),
        ("sorted_workspace", _fp), ("sorted_workspace_bytes", C.c_size_t), ("spread", C.c_int32), ("spread_workspace", _fp),
        ("spread_workspace_bytes", C.c_size_t), ("overlap", C.c_int32), ("defer", C.c_int32), ("wait_second_first", C.c_int32),
        ("stream", _fp), ("second", _fp), ("third", _fp)]


# name -> (restype, argtypes); every symbol declared in include/thermonerf_hip.h
_vp, _i64, _i32, _sz = C.c_void_p, C.c_int64, C.c_int32, C.c_size_t
SIGNATURES = {
    "tn_generate_rays": (C.c_int, [C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, C.c_float, _i32, _i32,
                                   C.POINTER(C.c_float), _i64, _i64, _vp, _vp, _vp, _vp]),
    "tn_frustum_positions": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp]),
    "tn_frustum_from_edges": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp]),
    "tn_density_fwd": (C.c_int, [C.POINTER(tn_density_field), _vp, _i64, _vp, _vp]),
    "tn_field_density_fwd": (C.c_int, [C.POINTER(tn_thermal_field), _vp, _i64, _vp, _vp, _vp]),
    "tn_field_heads_fwd": (C.c_int, [C.POINTER(tn_thermal_field), _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    "tn_camera_opt_fwd": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    "tn_camera_opt_bwd": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    "tn_sample_initial": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    "tn_weights_fwd": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "tn_sample_pdf": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    "tn_composite_fwd": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    "tn_depth_fwd": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp]),
    "tn_ssim_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "tn_ssim_fwd": (C.c_int, [_vp, _vp, _i32, _i32, _i32, C.c_float, _vp, _sz, _vp, _vp]),
    "tn_frame_to_rgb8": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "tn_otsu_thresholds": (C.c_int, [_vp, C.POINTER(C.c_int64), _i32, _vp, _vp, _vp]),
    "tn_pointcloud_tile_rays": (_i32, []),
    "tn_pointcloud_scan_width": (_i32, []),
    "tn_pointcloud_workspace_bytes": (_sz, [_i64]),
    "tn_pointcloud_append": (C.c_int, [_vp] * 6 + [_i64, _i64, C.POINTER(tn_pointcloud_params)] + [_vp] * 6 + [_i64, _vp, _vp, _sz, _vp]),
    "tn_knn_grid_resolution": (_i32, [_i64]),
    "tn_knn_workspace_bytes": (_sz, [_i64, _i32]),
    "tn_knn": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "tn_pointcloud_normals": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    "tn_sort_tile": (_i32, []),
    "tn_sort_pairs_workspace_bytes": (_sz, [_i64]),
    "tn_sort_pairs": (C.c_int, [_vp, _vp, _i64, C.c_int, _vp, _vp, _vp, _sz, _vp]),
    "tn_voxel_downsample_workspace_bytes": (_sz, [_i64]),
    "tn_voxel_downsample": (C.c_int, [_vp] * 5 + [_i64, C.POINTER(tn_voxel_params)] + [_vp] * 6 + [_i64, _vp, _vp, _sz, _vp]),
    "tn_mesh_simplify_workspace_bytes": (_sz, [_i64, _i64]),
    "tn_mesh_simplify": (C.c_int, [_vp] * 5 + [_i64, _i64, C.POINTER(tn_voxel_params)] + [_vp] * 5 + [_i64, _vp, _vp, _i64, _vp, _vp, _vp,
                                   _sz, _vp]),
    "tn_mesh_regions_workspace_bytes": (_sz, [_i64, _i64]),
    "tn_mesh_regions": (C.c_int, [_vp, _vp, _vp, _i64, _i64, C.c_float, C.c_float, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "tn_mesh_raster_small_box": (_i32, []),
    "tn_mesh_rasterize_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "tn_mesh_rasterize": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, C.POINTER(tn_raster_view), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "tn_mesh_bvh_depth_bound": (_i32, []),
    "tn_mesh_bvh_bytes": (_sz, [_i64]),
    "tn_mesh_bvh_workspace_bytes": (_sz, [_i64]),
    "tn_mesh_bvh_build": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _sz, _vp, _sz, _vp]),
    "tn_mesh_raycast": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _sz, _vp, _vp, _vp, _i64, C.POINTER(tn_raycast_params)] + [_vp] * 9),
    "tn_mesh_closest": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _sz, _vp, _vp, _i64, C.POINTER(tn_closest_params)] + [_vp] * 10),
    "tn_mesh_project": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _sz, _vp, _vp, _vp, _i64, _vp, _vp, _i64, C.POINTER(tn_project_params)]
                        + [_vp] * 8),
    "tn_mesh_register_workspace_bytes": (_sz, [_i64]),
    "tn_mesh_register": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _sz, _vp, _i64, C.POINTER(tn_register_params), _vp, _vp, _vp, _vp, _sz, _vp]),
    "tn_mesh_half_edges_workspace_bytes": (_sz, [_i64, _i64]),
    "tn_mesh_half_edges": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _sz, _vp]),
    "tn_mesh_isolines_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "tn_mesh_isolines": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, C.POINTER(tn_isoline_params)] + [_vp] * 5 + [_i64, _vp, _vp, _sz, _vp]),
    "tn_mesh_patches_workspace_bytes": (_sz, [_i64, _i64]),
    "tn_mesh_patches": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, C.c_double, _vp, _i64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "tn_mesh_tile": (_i32, []),
    "tn_mesh_scan_width": (_i32, []),
    "tn_mesh_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "tn_tsdf_integrate": (C.c_int, [_vp] * 4 + [_i32, _i32, C.POINTER(tn_mesh_params), _vp, _vp]),
    "tn_mesh_extract": (C.c_int, [_vp, C.POINTER(tn_mesh_params)] + [_vp] * 5 + [_i64, _vp, _i64, _vp, _vp, _sz, _vp]),
    "tn_mesh_components_workspace_bytes": (_sz, [_i64, _i64]),
    "tn_mesh_components": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "tn_mesh_filter_components": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _sz, _vp]),
    "tn_mesh_incidence_workspace_bytes": (_sz, [_i64, _i64]),
    "tn_mesh_incidence": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _sz, _vp]),
    "tn_mesh_vertex_normals": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "tn_mesh_smooth": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _i32, C.c_float, C.c_float, _vp, _vp, _vp]),
    "tn_mesh_scalar_smooth": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _i32, C.c_float, C.c_float, _i32, _vp, _vp, _vp]),
    "tn_mesh_scalar_gradient_workspace_bytes": (_sz, [_i64, _i64]),
    "tn_mesh_scalar_gradient": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "tn_mesh_peaks_workspace_bytes": (_sz, [_i64, _i64]),
    "tn_mesh_peaks": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _sz, _vp]),
    "tn_basin_persistence": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp]),
    "tn_mesh_spots_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "tn_mesh_spots": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp,
                                _sz, _vp]),
    "tn_mesh_geodesic_workspace_bytes": (_sz, [_i64, _i64]),
    "tn_mesh_geodesic": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _i64, C.c_double, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "tn_mesh_distance_bands_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "tn_mesh_distance_bands": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, C.c_double, _i64, _i32, _vp, _vp, _vp, _sz, _vp]),
    "tn_render_workspace_bytes": (_sz, [C.POINTER(tn_render_config), _i64]),
    "tn_render_rays_fwd": (
        C.c_int,
        [C.POINTER(tn_density_field), C.POINTER(tn_density_field), C.POINTER(tn_thermal_field),
         C.POINTER(tn_render_config), C.POINTER(tn_render_inputs), C.POINTER(tn_render_outputs), _i64, _vp, _sz, _vp],
    ),
    "tn_proposal_sample_fwd": (
        C.c_int,
        [C.POINTER(tn_density_field), C.POINTER(tn_density_field), C.POINTER(tn_render_config),
         C.POINTER(tn_render_inputs), C.POINTER(tn_render_outputs), _i64, _vp, _sz, _vp],
    ),
    "tn_field_render_fwd": (
        C.c_int,
        [C.POINTER(tn_thermal_field), C.POINTER(tn_render_config), C.POINTER(tn_render_inputs),
         C.POINTER(tn_render_outputs), _i64, _vp, _sz, _vp],
    ),
    "tn_bf16x6_split_product": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "tn_bf16_mfma_value_probe": (C.c_int, [C.c_float, C.c_float, _vp, _vp]),
    "tn_depth_bound_slots": (_i64, [_i64, _i64, _i64]),
    "tn_render_kernel_form": (C.c_int32, [C.POINTER(tn_thermal_field), C.POINTER(tn_render_config), _i64, C.c_int32]),
    "tn_render_sample_split": (C.c_int32, [C.POINTER(tn_thermal_field), C.POINTER(tn_render_config), _i64]),
    "tn_render_tail_segments": (C.c_int32, [_i64, _i64, C.c_int32, C.c_int32]),
    "tn_render_tail_plan": (C.c_int32, [C.POINTER(tn_thermal_field), C.POINTER(tn_render_config), _i64]),
    "tn_render_tail_records_bytes": (_sz, [C.POINTER(tn_render_config), _i64]),
    "tn_field_render_chunked_fwd": (
        C.c_int,
        [C.POINTER(tn_thermal_field), C.POINTER(tn_render_config), C.POINTER(tn_render_inputs),
         C.POINTER(tn_render_outputs), _i64, _vp, _sz, _i64, _i64, _vp, _i32, _vp],
    ),
    "tn_expected_depth_clip_chunked": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp]),
    "tn_hashgrid_prepare_bytes": (_sz, [C.POINTER(tn_hashgrid), _i64]),
    "tn_hashgrid_prepare": (C.c_int, [C.POINTER(tn_hashgrid), C.POINTER(tn_hashgrid), _vp, _sz, _vp]),
    "tn_field_prepare_bytes": (_sz, [C.POINTER(tn_thermal_field)]),
    "tn_field_prepare": (C.c_int, [C.POINTER(tn_thermal_field), _vp, _sz, _vp]),
    "tn_field_prepare_f16x3_bytes": (_sz, [C.POINTER(tn_thermal_field)]),
    "tn_field_prepare_f16x3": (C.c_int, [C.POINTER(tn_thermal_field), _vp, _sz, _vp]),
    "tn_field_prepare_bf16x6_bytes": (_sz, [C.POINTER(tn_thermal_field)]),
    "tn_field_prepare_bf16x6": (C.c_int, [C.POINTER(tn_thermal_field), _vp, _sz, _vp]),
    # training step
    "tn_hash_encode_fwd": (C.c_int, [C.POINTER(tn_hashgrid), C.POINTER(tn_space), _vp, _i64, _vp, _vp, _vp]),
    "tn_hash_encode_bwd": (C.c_int, [C.POINTER(tn_hashgrid), C.POINTER(tn_space), _vp, _vp, _i64, _vp, _vp]),
    "tn_hash_encode_bwd_levels": (C.c_int, [C.POINTER(tn_hashgrid), C.POINTER(tn_space), _vp, _vp, _i64, _vp, _i32, _i32, _vp]),
    "tn_hash_encode_bwd_spread_workspace_bytes": (_sz, [C.POINTER(tn_hashgrid)]),
    "tn_hash_encode_bwd_spread": (C.c_int, [C.POINTER(tn_hashgrid), C.POINTER(tn_space), _vp, _vp, _i64, _vp, _i32, _i32, _vp, _sz, _vp]),
    "tn_hash_encode_bwd_sorted_workspace_bytes": (_sz, [C.POINTER(tn_hashgrid), _i64, _i32]),
    "tn_hash_encode_bwd_sorted_first_level": (C.c_int, [C.POINTER(tn_hashgrid), _i64]),
    "tn_hash_encode_bwd_sorted": (C.c_int, [C.POINTER(tn_hashgrid), C.POINTER(tn_space), _vp, _vp, _i64, _vp, _i32, _vp, _sz, _vp]),
    "tn_linear_fwd": (C.c_int, [_vp, _i32, C.POINTER(tn_linear), _i32, _i64, _vp, _i32, _vp]),
    "tn_linear_bwd_workspace_bytes": (_sz, []),
    "tn_linear_bwd": (C.c_int, [_vp, _i32, _vp, _vp, _i32, C.POINTER(tn_linear), _i32, _i64, _vp, _i32, _i32, _vp, _vp, _vp,
                                _sz, _vp]),
    "tn_density_act_fwd": (C.c_int, [_vp, _i32, _vp, C.c_float, _i64, _vp, _vp]),
    "tn_density_act_bwd": (C.c_int, [_vp, _i32, _vp, C.c_float, C.c_float, _vp, _i64, _vp, _i32, _i32, _vp]),
    "tn_weights_bwd": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _vp]),
    "tn_gradient_scale_bwd": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "tn_linear_chain_bwd_workspace_bytes": (_sz, []),
    "tn_linear_chain_bwd": (C.c_int, [C.POINTER(tn_chain_layer), _i32, _vp, _i32, _vp, _i32, _i64, _vp, _i32, _i32, _vp, _sz, _vp]),
    "tn_field_fwd_taped": (C.c_int, [C.POINTER(tn_thermal_field), _vp, _vp, _vp, _i64, _i32] + [_vp] * 12),
    "tn_density_fwd_train": (C.c_int, [C.POINTER(tn_density_field), _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "tn_density_bwd_train": (C.c_int, [C.POINTER(tn_density_field), _vp, _vp, _vp, _vp, _i64, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tn_ray_head_fwd": (C.c_int, [C.POINTER(tn_thermal_field), _vp, _vp, _i64, _vp, _vp]),
    "tn_ray_head_bwd": (C.c_int, [C.POINTER(tn_thermal_field), _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tn_field_fwd_train": (C.c_int, [C.POINTER(tn_thermal_field), _vp, _vp, _i64, _i32] + [_vp] * 8),
    "tn_field_bwd_fused_workspace_bytes": (_sz, [_i64, _i32]),
    "tn_field_bwd_fused": (C.c_int, [C.POINTER(tn_thermal_field), _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, C.c_float,
                                     _i32, _vp, _vp, _vp, _vp, _vp, C.POINTER(tn_field_grads), _vp, _sz, _vp]),
    "tn_composite_bwd": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    "tn_color_input_fwd": (C.c_int, [C.POINTER(tn_thermal_field), _vp, _vp, _i32, _vp, _i32, _i64, _i32, _vp, _vp]),
    "tn_color_input_bwd": (C.c_int, [C.POINTER(tn_thermal_field), _vp, _vp, _i32, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "tn_hash_encode_bwd_input": (C.c_int, [C.POINTER(tn_hashgrid), C.POINTER(tn_space), _vp, _vp, _i64, _vp, _vp]),
    "tn_frustum_positions_bwd": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    "tn_ray_render_fwd": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp]),
    "tn_ray_render_bwd": (C.c_int, [_vp] * 11 + [_i64, _i32, _vp, _vp, _vp, _vp]),
    "tn_ray_render_depth_fwd": (C.c_int, [_vp] * 6 + [_i64, _i32] + [_vp] * 8),
    "tn_image_losses": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "tn_sum_scalars": (C.c_int, [C.POINTER(C.c_void_p), _i32, _vp, _vp]),
    "tn_distortion_loss": (C.c_int, [_vp, _vp, _i64, _i32, C.c_float, _vp, _vp, _vp]),
    "tn_distortion_loss_term": (C.c_int, [_vp, _vp, _i64, _i32, C.c_float, C.c_float, _vp, _vp, _vp]),
    "tn_interlevel_loss": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, C.c_float, _vp, _vp, _vp]),
    "tn_interlevel_loss_levels": (C.c_int, [_vp, _vp, _i64, _i32, _i32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_int32), C.c_float, _vp, C.POINTER(C.c_void_p), _vp]),
    "tn_adam_step": (C.c_int, [C.POINTER(tn_adam_tensor), _i32, _vp]),
    "tn_train_step_fwd": (C.c_int, [C.POINTER(tn_train_step)]),
    "tn_train_step_bwd": (C.c_int, [C.POINTER(tn_train_step_bwd_args)]),
    "tn_version": (C.c_char_p, []),
}

_lib: Optional[C.CDLL] = None


def lib_path() -> str:
    return _LIB_PATH


def load() -> C.CDLL:
    """Load the shared object and bind every declared symbol.  Raises RuntimeError (never falls back)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"{_LIB_NAME} not found at {_LIB_PATH}; build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C thermo_nerf_amd/csrc`). thermo_nerf_amd has no CPU/PyTorch fallback for its kernels."
        )
    try:
        lib = C.CDLL(_LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the box
        raise RuntimeError(f"failed to load {_LIB_PATH}: {e}") from e
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f"{_LIB_NAME} does not export {name}") from e
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(code: int, what: str) -> None:
    if code != TN_OK:
        raise RuntimeError(f"{what} failed: {_ERRORS.get(code, f'error code {code}')}")


def require_device_tensor(t: torch.Tensor, name: str, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The kernels read raw device pointers: insist on a contiguous ROCm tensor of the right dtype."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} is on {t.device}; thermo_nerf_amd runs only on a ROCm device (no CPU fallback exists)."
        )
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        t = t.contiguous()
    return t


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def current_stream() -> int:
    """raw handle of torch's current HIP stream on the current device.  torch.cuda.current_stream() walks
    _get_device_index -> is_available -> os.environ on every call (17 us; a training step asks ~23 times = 0.4 ms of host
    time); the raw accessor it ends in is called directly once the runtime is up."""
    try:
        return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
    except (AttributeError, RuntimeError):
        return torch.cuda.current_stream().cuda_stream  # also initialises the runtime on the first call


_CONCURRENT: dict = {}


SIDE_STREAM_PRIORITY = 0  # torch.cuda.Stream(priority=...) of the candidates below: 0 = default, -1 = high (tools/train_bench.py --side-priority)


def concurrent_streams(device, count: int, candidates: int = 12, with_main: bool = True) -> list:
    """``count`` HIP streams that run CONCURRENTLY with each other and — ``with_main`` — with torch's current stream on ``device``.
    ROCm maps streams onto four hardware queues, and two streams that share one execute their kernels one after the other:
    measured on MI355X (tools/stream_overlap_probe.py, profiles/micro/round5_stream_queues.txt) the default stream shares its
    queue with entries 6 and 10 of torch's 32-stream pool, entries 2 and 3 share one, ... — so `torch.cuda.Stream()` twice gives two
    streams that overlap, or do not, depending on how many streams the process handed out before (the training step read
    1.30 ... 1.54 ms at S=48 with the same kernels, VERDICT r4 Weak #3).  Here candidates are taken from the pool and kept only
    if a pair of short spin kernels (torch.cuda._sleep), one per stream, finishes in the time of one: a one-off calibration of a
    few ms per (device, current stream), which synchronises the device — call it from an initialisation path (``calibrate_streams``;
    the training step and the engine do so on first use); under an active stream capture nothing is probed (and nothing cached):
    the first pool streams are returned as they are.
    Four queues, one of them the current stream's: with ``with_main`` at most THREE streams can pass, without it (the engine's
    chunk streams: the caller's stream only waits for them) four.  If the probe finds fewer than ``count``, the rest is filled with
    the candidates that conflict with the fewest chosen ones — and never with the current stream while another is left."""
    import time

    dev = torch.device(device)
    main = torch.cuda.current_stream(dev)
    key = (dev, main.cuda_stream, count, bool(with_main))
    hit = _CONCURRENT.get(key)
    if hit is not None:
        return hit
    pool = [torch.cuda.Stream(device=dev, priority=SIDE_STREAM_PRIORITY) for _ in range(max(candidates, count))]
    try:
        if torch.cuda.is_current_stream_capturing():  # a synchronise would invalidate the capture
            return pool[:count]
    except (AttributeError, RuntimeError):  # pragma: no cover
        pass
    spin = 400_000  # cycles: ~0.17 ms per kernel

    def together(a, b) -> float:
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        with torch.cuda.stream(a):
            torch.cuda._sleep(spin)
        with torch.cuda.stream(b):
            torch.cuda._sleep(spin)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t

    chosen: list = []
    want = min(count, 3 if with_main else 4)  # the hardware's queues
    try:
        together(main, pool[0])  # first-use costs out of the way
        one = min(together(pool[0], pool[0]) for _ in range(3)) / 2

        def overlap(a, b) -> bool:
            return min(together(a, b), together(a, b)) < 1.5 * one

        for s in pool:
            if all(overlap(s, t) for t in ([main] if with_main else []) + chosen):
                chosen.append(s)
                if len(chosen) == want:
                    break
        if len(chosen) < count:  # more streams than queues (or a busy device skewed the probe): the least conflicting candidates
            rest = [s for s in pool if s not in chosen]
            score = {id(s): (0 if not with_main or overlap(s, main) else len(pool)) + sum(0 if overlap(s, t) else 1 for t in chosen)
                     for s in rest}
            rest.sort(key=lambda s: score[id(s)])
            chosen += rest[:count - len(chosen)]
    except (AttributeError, RuntimeError):  # pragma: no cover - no _sleep in this torch build: no calibration
        chosen = chosen + [s for s in pool if s not in chosen][:count - len(chosen)]
    _CONCURRENT[key] = chosen
    return chosen


def calibrate_streams(device, side_streams: int = 2, engine_streams: int = 2) -> None:
    """The explicit initialisation entry of ``concurrent_streams``: probe, once per (device, current stream), the side streams of the
    training step and the chunk streams of RayRenderEngine — outside any timed region or stream capture."""
    concurrent_streams(device, side_streams)
    concurrent_streams(device, engine_streams, with_main=False)


# ---- deferred table updates -----------------------------------------------------------------------------------------------------
# The training step's longest dependent chain is  field backward -> scatter of d(hash table) -> Adam on the table -> next field
# forward; everything else the step does after the field backward (ray-level adjoints, camera-pose backward, the small tensors'
# Adam, the NEXT step's ray gather / camera optimizer / proposal pass / level geometry / field_prepare) depends on neither the table
# nor its gradient.  With config.deferred_table_update the scatter's two halves and the table's Adam are queued on the step's side
# streams and NOT joined; the calling stream runs on, and whoever next reads the table or its gradient on another stream first calls
# join_pending — the training forward right before its field launch, the eval struct builders, Module.train()/state_dict(), the
# Trainer at the end of train().  Temporaries those side launches read (d_enc, positions, the record workspace, the gradient arena)
# are held here until the join: freed earlier, the caching allocator could hand them to the calling stream while a side kernel is
# still pending.
_PENDING: dict = {}


def defer(device, streams, keep=()) -> None:
    """register side-stream work on ``device`` that the current stream has NOT joined: the Stream objects it runs on and the
    tensors it reads or writes (kept alive until join_pending)"""
    e = _PENDING.setdefault(torch.device(device), {"streams": [], "keep": []})
    for s in streams:
        if all(s.cuda_stream != t.cuda_stream for t in e["streams"]):
            e["streams"].append(s)
    e["keep"].extend(keep)


def pending(device) -> Optional[dict]:
    return _PENDING.get(torch.device(device))


def take_pending(device) -> Optional[dict]:
    """remove and return the device's entry WITHOUT waiting: the caller orders its stream behind entry["streams"] itself (events
    handed to tn_train_step_fwd) and keeps entry["keep"] alive until that order is queued"""
    return _PENDING.pop(torch.device(device), None)


def join_pending(device=None) -> bool:
    """torch's current stream on ``device`` (default: every device with deferred work) waits for the deferred table updates; their
    temporaries are released.  Returns whether anything was pending.  A dictionary look-up when nothing is."""
    if not _PENDING:
        return False
    devs = list(_PENDING) if device is None else [torch.device(device)]
    hit = False
    for dev in devs:
        e = _PENDING.pop(dev, None)
        if e is None:
            continue
        cur = torch.cuda.current_stream(dev)
        for s in e["streams"]:
            if s.cuda_stream != cur.cuda_stream:
                cur.wait_stream(s)
        e["keep"].clear()
        hit = True
    return hit


_ZERO_BLOCKS: dict = {}
_ZERO_BLOCK_FLOATS = 1 << 20


def fresh_zeros(shape, device) -> torch.Tensor:
    """A zero-initialised float32 tensor nobody else holds, WITHOUT a fill launch per call: small accumulators (a loss scalar,
    the [num_cameras, 6] pose gradient) are handed out as successive, never reused slices of a 4 MiB block that one fill
    cleared (a new block when it is used up; a slice keeps its block alive).  Per (device, stream): the fill is ordered with
    that stream's kernels."""
    n = 1
    for k in shape:
        n *= int(k)
    n_al = (n + 63) // 64 * 64
    if n_al > _ZERO_BLOCK_FLOATS // 16:
        return torch.zeros(shape, dtype=torch.float32, device=device)
    key = (torch.device(device), current_stream())
    blk = _ZERO_BLOCKS.get(key)
    if blk is None or blk[1] + n_al > _ZERO_BLOCK_FLOATS:
        blk = _ZERO_BLOCKS[key] = [torch.zeros((_ZERO_BLOCK_FLOATS,), dtype=torch.float32, device=device), 0]
    out = blk[0][blk[1]:blk[1] + n].view(tuple(shape))
    blk[1] += n_al
    return out


def make_linear(layer: torch.nn.Linear) -> tn_linear:
    w = require_device_tensor(layer.weight.detach(), "Linear.weight")
    b = require_device_tensor(layer.bias.detach(), "Linear.bias")
    return tn_linear(w.data_ptr(), b.data_ptr(), layer.in_features, layer.out_features)


def host_values(owner, name: str) -> tuple:
    """Flat host copy of a small constant device buffer of module ``owner`` (scalings, aabb), cached ON the module per
    (storage, version): reading it back on every call would be a synchronising device-to-host copy in the middle of the
    launch stream.  (Not a global cache: device addresses are recycled between tensors.)"""
    t = getattr(owner, name)
    key = (t.data_ptr(), t._version, str(t.device))
    cache = owner.__dict__.setdefault("_host_copies", {})
    hit = cache.get(name)
    if hit is None or hit[0] != key:
        hit = (key, tuple(t.detach().float().reshape(-1).cpu().tolist()))
        cache[name] = hit
    return hit[1]


def make_space(contraction: bool, aabb: Optional[torch.Tensor], owner=None) -> tn_space:
    """``owner``: the module holding ``aabb`` as its attribute of that name (enables the cached host copy)."""
    s = tn_space()
    s.contraction = 1 if contraction else 0
    if aabb is not None:
        a = host_values(owner, "aabb") if owner is not None else tuple(aabb.detach().float().reshape(-1).cpu().tolist())
        for i in range(3):
            s.aabb_min[i] = a[i]
            s.aabb_max[i] = a[3 + i]
    return s
