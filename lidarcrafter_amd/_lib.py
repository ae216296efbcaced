"""ctypes binding of include/lidarcrafter_hip.h.  There is NO fallback: if the shared library is
missing the import of any compute op raises, so a GPU box can never silently run a CPU path."""
from __future__ import annotations

import ctypes as C
import os

from .build import LIB

i32, i64, f32, f64, vp = C.c_int, C.c_int64, C.c_float, C.c_double, C.c_void_p


class CmOperand(C.Structure):
    """struct lc_cm_operand: channel-major attention operand (pointer + batch/head/channel strides)."""
    _fields_ = [("p", vp), ("bs", i64), ("hs", i64), ("cs", i64)]


_op = C.POINTER(CmOperand)


class OctStats(C.Structure):
    """struct lc_oct_stats: producer-side GroupNorm statistics of one channel segment."""
    _fields_ = [("p", vp), ("channels", i32), ("slots", i32), ("unit", i32)]


_os = C.POINTER(OctStats)


class GnStatsInput(C.Structure):
    """struct lc_gn_stats_input: GroupNorm statistics + parameters for the conv's fused input norm."""
    _fields_ = [("partials", vp), ("G", i32), ("nch", i32), ("eps", f32), ("gamma", vp), ("beta", vp),
                ("scale", vp), ("shift", vp), ("ss_bs", i64), ("os0", _os), ("os1", _os)]


_gs = C.POINTER(GnStatsInput)


class RowSegment(C.Structure):
    """struct lc_row_segment: `width` columns of a gathered activation matrix (pointer, optional row index, row stride)."""
    _fields_ = [("p", vp), ("idx", vp), ("ld", i64), ("width", i32)]


_rs = C.POINTER(RowSegment)


class ConvRange(C.Structure):
    """struct lc_conv_range: device-resident pre-scale + running amax of one conv layer's input."""
    _fields_ = [("x_scale", f32), ("x_unscale", f32), ("amax_scaled", f32), ("reserved", f32)]


# name -> (restype, argtypes); mirrors include/lidarcrafter_hip.h one to one
SIGNATURES = {
    "lc_abi_version": (i32, []),
    "lc_device_arch": (i32, [C.c_char_p, i32]),
    "lc_load_code_objects": (i32, []),
    "lc_packed_conv_weight_elems": (i64, [i32, i32, i32]),
    "lc_pack_conv_weight": (i32, [vp, vp, i32, i32, i32, vp]),
    "lc_conv2d_ring_fwd": (i32, [vp, i64, vp, vp, vp, i64, vp, i64, i32, i32, i32, i32, i32, i32,
                                 f32, i32, vp]),
    "lc_packed_conv_weight_f16x2_elems": (i64, [i32, i32, i32]),
    "lc_pack_conv_weight_f16x2": (i32, [vp, vp, vp, i32, i32, i32, vp, vp]),
    "lc_pack_conv_weight_f16x2_dx": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "lc_pack_conv_weights_f16x2_multi": (i32, [vp, i32, i32, vp]),
    "lc_range_from_amax": (i32, [vp, i64, f32, vp, vp]),
    "lc_groupnorm_amax_partials": (i64, [i32, i32, i32, i32, i32, i32]),
    "lc_conv2d_ring_f16x2_fwd": (i32, [vp, i64, vp, vp, vp, vp, i64, vp, i64, i32, i32, i32, i32,
                                       i32, i32, f32, i32, vp, i32, i32, _gs, vp, i32, vp, vp, vp]),
    "lc_split_act_units": (i64, [i32, i32, i32, i32]),
    "lc_groupnorm_apply_split": (i32, [vp, i64, vp, vp, vp, vp, vp, i64, vp, i32, i32, i32, i32, i32,
                                       f32, i32, vp, vp]),
    "lc_groupnorm_apply_os_split": (i32, [vp, i64, _os, _os, vp, vp, vp, vp, i64, vp, i32, i32, i32,
                                          i32, i32, f32, i32, vp, vp]),
    "lc_conv1x1_f16x2_ps_fwd": (i32, [vp, vp, vp, vp, vp, i64, vp, i64, i32, i32, i32, i32, i32, f32, vp, vp, vp]),
    "lc_conv2d_ring_f16x2_ps_fwd": (i32, [vp, vp, vp, vp, vp, i64, vp, i64, i32, i32, i32, i32, i32,
                                          f32, i32, vp, i32, vp, i32, vp, vp, vp]),
    "lc_range_from_tensor": (i32, [vp, i64, i32, i64, vp, vp]),
    "lc_splitk_stats_slots": (i64, [i32, i32]),
    "lc_splitk_reduce": (i32, [vp, i32, vp, vp, i64, vp, i64, i32, i32, i32, i32, f32, vp, vp]),
    "lc_conv2d_ring_f16x2_stats_slots": (i64, [i32, i32, i32, i32, i32, i32, i32]),
    "lc_groupnorm_coeffs": (i32, [vp, i64, vp, vp, vp, vp, vp, i64, vp, i32, i32, i32, i32, i32,
                                  i32, f32, vp]),
    "lc_groupnorm_partials_elems": (i64, [i32, i32, i32, i32, i32]),
    "lc_groupnorm_stats": (i32, [vp, i64, vp, i32, i32, i32, i32, i32, vp]),
    "lc_groupnorm_apply": (i32, [vp, i64, vp, vp, vp, vp, vp, i64, vp, i64, i32, i32, i32, i32,
                                 i32, f32, i32, vp]),
    "lc_groupnorm_apply_train": (i32, [vp, i64, vp, vp, vp, vp, vp, i64, vp, i64, i32, i32, i32, i32,
                                       i32, f32, i32, vp, vp, vp]),
    "lc_groupnorm_apply_os": (i32, [vp, i64, _os, _os, vp, vp, vp, vp, i64, vp, i64, i32, i32, i32,
                                    i32, i32, f32, i32, vp]),
    "lc_conv2d_ring_wgrad_scratch_elems": (i64, [i32, i32, i32, i32, i32, i32]),
    "lc_conv2d_ring_wgrad": (i32, [vp, i64, vp, i64, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "lc_conv2d_ring_wgrad_f16x2": (i32, [vp, i64, vp, i64, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32,
                                         i32, i32, vp]),
    "lc_groupnorm_meanrstd": (i32, [vp, i64, vp, vp, i32, i32, i32, i32, i32, f32, vp]),
    "lc_groupnorm_bwd": (i32, [vp, i64, vp, i64, vp, vp, vp, vp, vp, i64, vp, vp, i64, i32, i32, i32,
                               i32, i32, i32, vp]),
    "lc_groupnorm_bwd_train": (i32, [vp, i64, vp, i64, vp, vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp,
                                     i32, i32, i32, i32, i32, i32, vp, vp]),
    "lc_conv2d_ring_wgrad_route": (i32, [i32, i32, i32, i32, i32, i32, i32, i64, i64, i32, i32, vp]),
    "lc_groupnorm_bwd_route": (i32, [i32, i32, i32, i32, i32, i64, i64, i64, i32, i32, i32, vp]),
    "lc_resample2x_fwd": (i32, [vp, i64, vp, i64, i32, i32, i32, i32, i32, vp]),
    "lc_resample2x_stats_slots": (i64, [i32, i32, i32]),
    "lc_resample2x_stats_fwd": (i32, [vp, i64, vp, i64, i32, i32, i32, i32, i32, vp, vp]),
    "lc_linear_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "lc_sinusoid_fwd": (i32, [vp, vp, i32, i32, f32, vp]),
    "lc_attention_fwd": (i32, [_op, _op, _op, _op, _op, _op, _op, _op, vp, i64, i64, i64,
                               i32, i32, i32, i32, i32, i32, i32, i32, f32, vp]),
    "lc_attention_f16x2_fwd": (i32, [_op, _op, _op, _op, _op, _op, _op, _op, vp, i64, i64, i64,
                                     i32, i32, i32, i32, i32, i32, i32, i32, f32, vp]),
    "lc_attention_route": (i32, [i32, i32, i32, i32, i32, i64, i32, i32]),
    "lc_attention_bwd_route": (i32, [i32, i32, i32, i64]),
    "lc_conv1x1_f16x2_ps_qkv_fwd": (i32, [vp, vp, vp, vp, vp, i64, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
    "lc_groupnorm_coeffs_os": (i32, [_os, _os, vp, vp, vp, vp, i64, vp, i32, i32, i32, i32, f32, vp]),
    "lc_resample2x_pair_fwd": (i32, [vp, i64, vp, i32, vp, i64, vp, i64, i32, i32, i32, i32, i32, vp]),
    "lc_split_act_fwd": (i32, [vp, i64, vp, i32, i32, i32, i32, vp, vp]),
    "lc_up2_combine9_stats_slots": (i64, [i32, i32]),
    "lc_up2_combine9_fwd": (i32, [vp, i64, vp, vp, i64, i32, i32, i32, i32, vp, vp]),
    "lc_up2_combine9_xup_fwd": (i32, [vp, i64, vp, vp, i64, vp, i64, vp, i64, i32, i32, i32, i32, vp, vp]),
    "lc_attention_units_elems": (i64, [i32, i32, i32, i32]),
    "lc_attention_pack_units": (i32, [_op, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "lc_attention_units_fwd": (i32, [_op, _op, vp, vp, i64, i64, i64, i32, i32, i32, i32, i32, i32, i32, i32, f32, vp]),
    "lc_qk_norm_cm_fwd": (i32, [vp, i64, i64, vp, i64, i64, vp, vp, i32, i32, i32, i32, vp]),
    "lc_flow_step_fwd": (i32, [vp, i64, vp, i64, vp, vp, i64, i32, i64, vp]),
    "lc_hdit_rmsnorm_fwd": (i32, [vp, i64, i64, vp, i64, i32, vp, i64, i64, i32, i32, i32, f32, vp]),
    "lc_hdit_geglu_fwd": (i32, [vp, i64, vp, i64, i32, i32, i32, vp]),
    "lc_hdit_qk_prep_fwd": (i32, [vp, i64, i64, vp, i64, i64, vp, vp, vp, i32, i32, i32, i32, vp]),
    "lc_hdit_na_fwd": (i32, [_op, _op, _op, vp, i64, i64, i64, i32, i32, i32, i32, i32, i32, i32, f32, vp]),
    "lc_hdit_space_to_depth_fwd": (i32, [vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, vp]),
    "lc_hdit_depth_to_space_fwd": (i32, [vp, i64, vp, i64, vp, i64, vp, i32, i32, i32, i32, i32, i32, vp]),
    "lc_hdit_tokenize_fwd": (i32, [vp, i64, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, vp]),
    "lc_hdit_fourier_fwd": (i32, [vp, vp, vp, i32, i32, vp]),
    "lc_hdit_na_train_fwd": (i32, [_op, _op, _op, vp, i64, i64, i64, vp, i32, i32, i32, i32, i32, i32, i32, f32, vp]),
    "lc_hdit_rmsnorm_bwd": (i32, [vp, i64, i64, vp, i64, i32, vp, i64, i64, vp, i64, i64, vp, vp, i64, i32, i32, i32,
                                  f32, vp]),
    "lc_hdit_geglu_bwd": (i32, [vp, i64, vp, i64, vp, i64, i32, i32, i32, vp]),
    "lc_hdit_qk_prep_bwd": (i32, [vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, i64, i64,
                                  vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "lc_hdit_na_bwd": (i32, [_op, _op, _op, _op, _op, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, vp]),
    "lc_hdit_lerp_bwd": (i32, [vp, i64, vp, i64, vp, i64, vp, vp, i64, vp, i64, vp, i32, i32, i32, i32, i32, i32, vp]),
    "lc_groupnorm_jvp_partials_elems": (i64, [i32, i32, i32, i32, i32]),
    "lc_groupnorm_jvp_stats": (i32, [vp, i64, vp, i64, vp, i32, i32, i32, i32, i32, vp]),
    "lc_groupnorm_jvp_apply_train": (i32, [vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, i64,
                                           i32, i32, i32, i32, i32, f32, i32, vp, vp, vp, vp]),
    "lc_qk_norm_cm_jvp": (i32, [vp, i64, i64, vp, i64, i64, vp, vp, i64, i64, vp, i64, i64, i32, i32, i32, i32, vp]),
    "lc_qk_norm_cm_bwd_partials": (i64, [i32, i32, i32]),
    "lc_qk_norm_cm_bwd": (i32, [vp, i64, i64, vp, i64, i64, vp, vp, i64, i64, vp, vp, i32, i32, i32, i32, vp]),
    "lc_attention_jvp_fwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp]),
    "lc_groupnorm_jvp_route": (i32, [i32, i32, i32, i32, i32, i64, i64, i32, i32, vp]),
    "lc_qk_norm_cm_route": (i32, [i32, i32, i32, i32, vp]),
    "lc_attention_jvp_route": (i32, [i32, i32, i32, i32, i32, vp]),
    "lc_attention_train_fwd": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp, vp]),
    "lc_attention_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp]),
    "lc_attention_bwd_f16x2": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp]),
    "lc_pstep_fwd": (i32, [vp, i64, vp, i64, vp, i64, vp, vp, i64, i32, i64, i32, i32, vp]),
    "lc_gate_bias_act": (i32, [vp, i64, vp, vp, i64, vp, i64, vp, i64, i32, i32, i32, i32, vp]),
    "lc_fir_down2_split_units": (i64, [i32, i32, i32, i32]),
    "lc_fir_down2_prefilter_split": (i32, [vp, i64, vp, i32, i32, i32, i32, vp, vp]),
    "lc_conv2d_ring_s2_stats_slots": (i64, [i32, i32]),
    "lc_conv2d_ring_s2_f16x2_ps_fwd": (i32, [vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, f32, vp, i32, vp, vp, vp]),
    "lc_calibrate_mfma_f16": (i64, [vp, i32, i32, vp, vp]),
    "lc_calibrate_stream_copy": (i32, [vp, vp, i64, vp]),
    "lc_copy_strided": (i32, [vp, i64, vp, i64, i32, i64, vp]),
    "lc_add_scale": (i32, [vp, i64, vp, i64, vp, i64, i32, i64, f32, vp]),
    "lc_project_points": (i32, [vp, i32, i32, i32, f64, f64, f32, f32, vp, vp, vp, vp, i32, vp]),
    "lc_project_workspace_init": (i32, [vp, i32, vp]),
    "lc_project_points_ws": (i32, [vp, i32, i32, i32, f64, f64, f32, f32, vp, vp, vp, vp, i32, vp]),
    "lc_project_points_f64": (i32, [vp, i32, i32, i32, f64, f64, f64, f64, vp, vp, vp, vp]),
    "lc_range_postprocess": (i32, [vp, i64, vp, vp, i32, i32, i32, i32, f32, f32, vp]),
    "lc_condition_preprocess": (i32, [vp, i64, vp, i64, i32, i32, i32, i32, i32, f32, f32, vp]),
    "lc_layout_scratch_bytes": (i64, [i32, i32]),
    "lc_layout_condition": (i32, [vp, i32, i32, vp, i32, i32, i32, i32, f64, f64, vp, vp, vp, vp, vp]),
    "lc_roiaware_pool3d_fwd": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp,
                                     vp, vp]),
    "lc_roiaware_pool3d_bwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "lc_points_in_boxes_mask": (i32, [vp, i32, vp, i32, f32, vp, vp]),
    "lc_points_in_boxes_mask4": (i32, [vp, i32, vp, i32, f32, vp, vp, vp]),
    "lc_transform_points": (i32, [vp, i32, C.POINTER(C.c_double), vp, vp]),
    "lc_transform_points_f64": (i32, [vp, i32, C.POINTER(C.c_double), i32, vp, vp]),
    "lc_image_to_points": (i32, [vp, i64, vp, vp, i32, i32, f32, f32, f32, vp, vp, vp]),
    "lc_bev_occupancy_accumulate": (i32, [vp, i32, i32, f32, f32, f32, f32, f32, i32, i32, i32, i32,
                                          i32, vp, vp, vp]),
    "lc_sparse_quantize_scratch_bytes": (i64, [i32, i32]),
    "lc_sparse_quantize": (i32, [vp, i32, i32, f64, f64, f64, vp, vp, vp, vp, vp, vp]),
    "lc_bev_histogram": (i32, [vp, i32, i32, vp, i32, f32, f32, vp, vp, vp]),
    "lc_rbf_partials_elems": (i64, [i32, i32]),
    "lc_rbf_kernel_sum": (i32, [vp, vp, i32, i32, i32, f32, vp, vp]),
    "lc_chamfer3d_fwd": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
    "lc_chamfer2d_fwd": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
    "lc_chamfer_bwd_scratch_bytes": (i64, [i32, i32, i32]),
    "lc_chamfer3d_bwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]),
    "lc_chamfer2d_bwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]),
    "lc_bev_grid_supported": (i32, [i32, i32]),
    "lc_bev_occupancy_bits": (i32, [vp, i32, vp, i32, i64, f32, f32, f32, f32, f32, i32, i32, i32, i32, vp, vp, vp]),
    "lc_bev_cell_lists": (i32, [vp, i32, i32, i32, vp, vp, vp]),
    "lc_bev_distance_transform": (i32, [vp, i32, i32, i32, vp, vp, i32, vp]),
    "lc_bev_pair_sums": (i32, [vp, vp, i32, vp, i32, i32, vp, vp]),
    "lc_bev_chamfer_combine": (i32, [vp, vp, vp, vp, i32, i32, i64, i32, i32, i32, vp, vp, vp, i64, vp]),
    "lc_emd_scratch_bytes": (i64, [i32, i32]),
    "lc_emd_fwd": (i32, [vp, vp, i32, i32, f32, i32, i32, vp, vp, vp, vp]),
    "lc_compact_scratch_elems": (i64, [i32]),
    "lc_compact_points": (i32, [vp, vp, i32, i32, vp, vp, vp, vp, vp]),
    "lc_points_in_boxes_index": (i32, [vp, vp, i32, i32, i32, f32, vp, vp]),
    "lc_skinny_parts": (i64, [i32, i32, i32]),
    "lc_skinny_gemm_fwd": (i32, [_rs, i32, vp, vp, i32, i32, i32, i32, vp]),
    "lc_skinny_combine_fwd": (i32, [vp, i32, vp, i32, vp, i64, vp, vp, i64, vp, i64, i32, i32, vp]),
    "lc_rowprep_fwd": (i32, [_rs, i32, vp, i64, i32, i32, i32, f32, vp, vp, i32, vp]),
    "lc_graph_pool_fwd": (i32, [vp, i64, i32, i32, vp, vp, vp, i64, i32, i32, vp]),
    "lc_time_embed_fwd": (i32, [vp, vp, vp, i32, i32, vp]),
    "lc_pointnet_trunk_scratch_elems": (i64, [i32, i32]),
    "lc_pointnet_trunk_fwd": (i32, [vp, i64, vp, vp, vp, vp, vp, vp, vp, i32, vp, i64, i32, i32, vp, vp]),
    "lc_spconv_hash_bytes": (i64, [i32]),
    "lc_spconv_hash_build": (i32, [vp, i32, i32, i32, vp, i64, vp]),
    "lc_spconv_map": (i32, [vp, i32, i32, i32, vp, i32, vp, vp]),
    "lc_spconv_fwd": (i32, [vp, i64, vp, i32, vp, vp, vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, vp]),
    "lc_spconv_sector_means": (i32, [vp, i64, vp, vp, i32, i32, vp, f32, vp, vp]),
    "lc_spvox_query": (i32, [vp, i32, i32, vp, i32, vp, vp, vp]),
    "lc_spvox_devoxelize": (i32, [vp, i64, i32, vp, vp, vp, i64, vp, i64, i32, i32, vp]),
    "lc_spvox_voxelize": (i32, [vp, i64, i32, vp, i32, vp, i32, vp, i64, i32, vp]),
    "lc_rangenet_tile_extent": (i32, [i32]),
    "lc_rangenet_packed_weight_elems": (i64, [i32, i32, i32]),
    "lc_rangenet_pack_weight": (i32, [vp, i32, i32, i32, vp]),
    "lc_rangenet_conv_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "lc_rangenet_reduce_fwd": (i32, [vp, vp, i32, i32, i32, i32, i32, vp]),
    "lc_pointmlp_limit": (i32, [i32]),
    "lc_fps_fwd": (i32, [vp, vp, i32, i32, i32, vp]),
    "lc_fps_stack_fwd": (i32, [vp, vp, i32, i32, i32, vp]),
    "lc_knn_fwd": (i32, [vp, vp, vp, i32, i32, i32, i32, vp]),
    "lc_pointmlp_group_scratch_elems": (i64, [i32, i32, i32]),
    "lc_pointmlp_group_fwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "lc_pointmlp_packed_weight_elems": (i64, [i32, i32]),
    "lc_pointmlp_pack_weight": (i32, [vp, i32, i32, vp]),
    "lc_pointmlp_conv_fwd": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "lc_pointmlp_groupmax_fwd": (i32, [vp, vp, i32, i32, i32, i32, i64, i64, i64, vp]),
    "lc_nn_grid_bytes": (i64, [i32, i64]),
    "lc_nn_grid_build": (i32, [vp, vp, i32, i64, i32, f64, vp, vp]),
    "lc_nn_radius": (i32, [vp, vp, i32, i64, vp, vp, vp, i32, i32, f64, vp, vp, vp]),
    "lc_icp_scratch_bytes": (i64, [i32, i32]),
    "lc_icp_run": (i32, [vp, vp, i32, i64, vp, vp, i32, i32, f64, i32, f64, f64, vp, vp, vp, vp, vp, vp]),
    "lc_segment_center_fwd": (i32, [vp, vp, i32, i64, f64, f64, f64, vp, vp, vp]),
    "lc_glenet_trunk_fwd": (i32, [vp, i64, vp, vp, i32, i32, i64] + [vp] * 12 + [vp, vp, vp]),
    "lc_rbox_inter_fwd": (i32, [vp, vp, i32, vp, vp, vp, vp]),
    "lc_riou3d_paired_fwd": (i32, [vp, i32, vp, i32, i32, vp, vp]),
    "lc_glenet_score_fwd": (i32, [vp, vp, i32, i32, f64, f32, f32, f32, vp, vp, vp, vp, vp]),
    "lc_boxes_iou_pairwise_fwd": (i32, [vp, i32, vp, i32, i32, vp, vp]),
    "lc_boxes_iou_aligned_fwd": (i32, [vp, vp, i32, i32, vp, vp]),
    "lc_nms_mask_fwd": (i32, [vp, i32, f32, i32, vp, vp]),
    "lc_nms_select_fwd": (i32, [vp, i32, vp, vp, vp]),
    "lc_boxes_iou_bev_host": (i32, [vp, i32, vp, i32, vp]),
    "lc_boxes_overlap_bev_host": (i32, [vp, i32, vp, i32, vp, vp]),
    "lc_pn2_limit": (i32, [i32]),
    "lc_pn2_scratch_elems": (i64, [i32, i32]),
    "lc_pn2_ball_query_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, vp]),
    "lc_pn2_group_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "lc_pn2_three_nn_fwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "lc_pn2_three_interpolate_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, vp]),
    "lc_pn2_three_interpolate_bwd": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "lc_pn2_voxel_query_fwd": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, i32, i32, i32, vp]),
    "lc_pn2_sa_first_fwd": (i32, [vp] * 10 + [i32] * 7 + [vp]),
    "lc_stats_limit": (i32, [i32]),
    "lc_stats_jacobi_pair": (i32, [i32, i32, i32, C.POINTER(C.c_int)]),
    "lc_stats_gemm_f64": (i32, [vp, i64, i64, vp, i64, i64, vp, i64, i32, i32, i32, vp]),
    "lc_stats_mmd_partials": (i64, [i32, i32]),
    "lc_stats_mmd_f64": (i32, [vp, i32, vp, i32, i32, vp, i32, i32, vp, vp, vp]),
    "lc_stats_center_f64": (i32, [vp, i32, i32, vp, vp, vp]),
    "lc_stats_reduce_f64": (i32, [vp, i64, vp, i64, i64, i32, vp, vp, vp]),
    "lc_stats_scale_rows_f64": (i32, [vp, vp, i32, f64, vp, vp]),
    "lc_stats_jacobi_init": (i32, [vp, i32, vp]),
    "lc_stats_jacobi_sweep": (i32, [vp, vp, i32, f64, f64, vp, vp, vp]),
    "lc_stats_jacobi_values": (i32, [vp, i32, vp, vp]),
    "lc_range_batch_fwd": (i32, [vp, i32, vp, i32, i32, i32, i32, f64, f64, f32, f32, f64, f64, vp, vp, vp, vp]),
    "lc_voxel_batch_key_bits": (i32, [i32, f64, f64, C.POINTER(C.c_int32)]),
    "lc_voxel_batch_scratch_bytes": (i64, [i32, i32]),
    "lc_voxel_batch_fwd": (i32, [vp, i32, vp, i32, i32, f64, f64, f64, vp, vp, vp, vp, vp]),
}

_lib = None
ABI_VERSION = 6   # include/lidarcrafter_hip.h lc_abi_version: bumped with every change of an exported signature


class HipLibraryMissing(RuntimeError):
    pass


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        path = os.environ.get("LC_HIP_LIB", LIB)   # developer override: A/B a differently built library
        if not os.path.exists(path):
            raise HipLibraryMissing(
                f"{path} not found: run `python -m lidarcrafter_amd.build` "
                "(or __graft_entry__.build()). There is no CPU fallback for the hot path.")
        handle = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        if handle.lc_abi_version() != ABI_VERSION:
            raise HipLibraryMissing("ABI version mismatch, rebuild the library")
        _lib = handle
    return _lib


_lib_p1 = None


def lib_p1() -> C.CDLL:
    """The single-product build of the convolution kernels (liblidarcrafter_hip_p1.so, -DLC_F16X2_TERMS=1):
    same entry points and arguments as the product library, used only through ops.conv_products() == 1."""
    global _lib_p1
    if _lib_p1 is None:
        path = os.path.join(os.path.dirname(LIB), "liblidarcrafter_hip_p1.so")
        if not os.path.exists(path):
            raise HipLibraryMissing(f"{path} not found: run `python -m lidarcrafter_amd.build`")
        handle = C.CDLL(path)
        for name in ("lc_conv2d_ring_f16x2_fwd", "lc_conv2d_ring_f16x2_ps_fwd", "lc_conv1x1_f16x2_ps_fwd",
                     "lc_conv1x1_f16x2_ps_qkv_fwd"):
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = SIGNATURES[name]
        _lib_p1 = handle
    return _lib_p1


class HipError(RuntimeError):
    pass


def check(code: int, what: str) -> None:
    if code != 0:
        kind = {-1: "invalid argument", -2: "unsupported shape"}.get(code, f"hipError {code}")
        raise HipError(f"{what}: {kind}")
