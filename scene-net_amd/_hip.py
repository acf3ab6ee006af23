"""ctypes binding of the C-ABI HIP library (include/scenenet_hip.h).

There is NO CPU fallback: if the library is missing or a tensor is not on a HIP
device, the call raises.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import contextlib
import ctypes
import functools
import os
from ctypes import c_char_p, c_int, c_void_p
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# SN_HIP_LIB: another build of the same library (A/B timing of kernel variants); default: the in-tree build
LIB_PATH = os.environ.get("SN_HIP_LIB") or os.path.join(_HERE, "lib", "libscenenet_hip.so")

SN_F32, SN_F64, SN_U8, SN_OCC8, SN_BF16, SN_I32 = 0, 1, 2, 3, 4, 5
SN_GENEO_CY, SN_GENEO_CONE, SN_GENEO_NEG = 0, 1, 2
SN_GENEO_CY_V1, SN_GENEO_CONE_V1, SN_GENEO_NEG_V1 = 3, 4, 5
SN_P_RADIUS, SN_P_SIGMA, SN_P_APEX, SN_P_CONE_RADIUS, SN_P_CONE_INC, SN_P_NEG_FACTOR = 0, 1, 2, 3, 4, 5
SN_NPARAM = 8

# every symbol include/scenenet_hip.h declares: (restype, argtypes)
_P, _I = c_void_p, c_int
SYMBOLS = {
    "sn_version": (c_int, []),
    "sn_prepare_device": (c_int, []),
    "sn_device_status": (c_int, [_P, _P]),
    "sn_device_status_clear": (c_int, []),
    "sn_last_error": (c_char_p, []),
    "sn_device_count": (c_int, []),
    "sn_conv_i8_path_counts": (c_int, [_P]),
    "sn_set_option": (c_int, [c_char_p, _I]),
    "sn_get_option": (c_int, [c_char_p]),
    "sn_geneo_bank": (c_int, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "sn_effective_lambdas": (c_int, [_P, _P, _I, _I, _P, _P]),
    "sn_conv_bank": (c_int, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P]),
    "sn_conv_bank_plan": (c_int, [_I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "sn_geneo_bank_prep": (c_int, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P]),
    "sn_conv_bank_prep": (c_int, [_P, _I, _I, _I, _I, _P, _P]),
    "sn_conv_bank_prepared": (c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P]),
    "sn_conv_bank_prepared_served": (c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P]),
    "sn_conv_bank_prepared_rows": (c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _I, _P, _P]),
    "sn_conv_prep_verdict_offset": (c_int, []),
    "sn_conv_i8_spin_timeouts": (c_int, [_P]),
    "sn_conv_i8z_round_counts": (c_int, [_P]),
    "sn_conv_i8z_plane_counts": (c_int, [_P]),
    "sn_voxel_onepass_giveups": (c_int, [_P]),
    "sn_launch_timing_events": (c_int, [_P, _P]),
    "sn_conv_fused": (c_int, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P]),
    "sn_conv_fused_supported": (c_int, [_I, _I, _I, _I, _I, _I, _I]),
    "sn_conv_fused_plan": (c_int, [_I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "sn_forward_auto": (c_int, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P]),
    "sn_voxel_bbox": (c_int, [_P, _P, _I, _P, _P]),
    "sn_voxel_desc": (c_int, [_P, _I, _I, _I, _I, _I, _P, _P]),
    "sn_voxel_desc_from_bounds": (c_int, [_P, _I, _I, _I, _I, _P, _P]),
    "sn_voxel_desc_sized": (c_int, [_P, _I, _P, _I, _I, _I, _P, _P, _P, _P]),
    "sn_voxel_finalize_sized": (c_int, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "sn_voxel_scatter": (c_int, [_P, _P, _P, _I, _P, _I, _I, _I, _P, _P, _P, _I, _P, _P]),
    "sn_voxel_finalize": (c_int, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "sn_voxel_occupancy": (c_int, [_P, _P, _P, _I, _P, _I, _I, _I, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "sn_voxel_occupancy_fused": (c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P,
                                         _P]),
    "sn_voxel_occupancy_fused_rows": (c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P,
                                              _P, _P, _P]),
    "sn_voxel_occupancy_fused_bank_rows": (c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P,
                                                   _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "sn_voxel_occupancy_plan": (c_int, [_I] * 11 + [_P]),
    "sn_voxel_occupancy_fused_bank": (c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P,
                                              _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P]),
    "sn_voxel_occupancy_sized": (c_int, [_P, _P, _P, _I, _P, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P,
                                         _P, _P, _P]),
    "sn_voxel_occupancy_sized_bank": (c_int, [_P, _P, _P, _I, _P, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P,
                                              _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P]),
    "sn_voxel_prepare": (c_int, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "sn_gather_points": (c_int, [_P, _I, _I, _P, _P, _I, _P, _I, _I, _I, ctypes.c_double, _P, _P]),
    "sn_grid_to_points": (c_int, [_P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "sn_conv_corr": (c_int, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "sn_conv_corr_t": (c_int, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "sn_conv_corr_blocks": (c_int, [_I, _I, _I, _I]),
    "sn_conv_corr_ws_bytes": (ctypes.c_size_t, [_I, _I, _I, _I, _I, _I, _I, _I]),
    "sn_conv_corr_ws": (c_int, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, ctypes.c_size_t, _P, _P]),
    "sn_conv_corr_plan": (c_int, [_I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "sn_geneo_bank_lambdas": (c_int, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P]),
    "sn_geneo_bank_bwd": (c_int, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "sn_geneo_backward": (c_int, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P]),
    "sn_loss_forward": (c_int, [_P, _I, _P, _I, _I, ctypes.c_int64, _P, _P, _I, _I] + [ctypes.c_double] * 6
                        + [_P, _P, _P, _P, _P]),
    "sn_param_penalty": (c_int, [_P, _P, _I, ctypes.c_float, _I, _P, _P, _P]),
    "sn_loss_backward": (c_int, [_P, _I, _P, _I, _I, ctypes.c_int64, _P, _I, _P, _P, _P, _P]),
    "sn_conv_fused_prep_bytes": (ctypes.c_size_t, [_I, _I, _I]),
    "sn_conv_fused_prep": (c_int, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "sn_conv_fused_prepared": (c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _I, _P]),
    "sn_conv_fused_v": (c_int, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _I, _P]),
    "sn_loss_forward_m": (c_int, [_P, _I, _P, _I, _I, ctypes.c_int64, _P, _P, _I, _I] + [ctypes.c_double] * 6
                          + [_P, _P, _P, _P, _P, _P]),
    "sn_loss_backward_u": (c_int, [_P, _I, _P, _I, _I, ctypes.c_int64, _P, _I, _P, _P, _I, _P, _P]),
    "sn_criterion_forward": (c_int, [_P, _I, _P, _I, _I, ctypes.c_int64, _P, _P, _I, _I] + [ctypes.c_double] * 6
                             + [_P, _P, _P, _P, _P, _P, _P, _I, ctypes.c_float, _I, _P, _P, _P, _P]),
    "sn_criterion_backward": (c_int, [_P, _I, _P, _I, _I, ctypes.c_int64, _P, _I, _P, _P, _I, _P, _P, _I, _P, _P]),
    "sn_binary_stats": (c_int, [_P, _I, _P, _I, ctypes.c_int64, ctypes.c_double, ctypes.c_double, _P, _P, _P, _P, _P]),
    "sn_binary_curve_ws_bytes": (ctypes.c_size_t, [ctypes.c_int64, _I, _I]),
    "sn_binary_curve": (c_int, [_P, _I, _P, _I, ctypes.c_int64, _I, _P, _I, _P, ctypes.c_size_t, _P, _P, _P]),
    "sn_tiles_unpack": (c_int, [_P, _I, _I, ctypes.c_int64, _P, _I, _P, _P, _P, _P]),
    "sn_towers_stencil": (c_int, [ctypes.c_double, _P, _P, _I, _P]),
    "sn_towers_ws_bytes": (ctypes.c_size_t, [_I, _I, _I, _I]),
    "sn_tower_proposals": (c_int, [_P, _I, _I, _I, _I, _I, ctypes.c_double, ctypes.c_double, _P, _I, _I, _P,
                                   ctypes.c_size_t, _P, _P, _P, _P]),
    "sn_tower_proposals_launches": (c_int, [_P, _I, _I, _I, _I, _I, ctypes.c_double, ctypes.c_double, _P, _I, _I, _P,
                                            ctypes.c_size_t, _P, _P, _P, _I, _I, _P]),
    "sn_crops_ws_bytes": (ctypes.c_size_t, [ctypes.c_int64, _I]),
    "sn_crops_chunk_points": (c_int, []),
    "sn_crop_count": (c_int, [_P, ctypes.c_int64, _P, _P, _I, _P, ctypes.c_size_t, _P, _P]),
    "sn_crop_scatter": (c_int, [_P, _P, ctypes.c_int64, _P, _P, _I, _P, ctypes.c_size_t, _P, ctypes.c_int64, _P, _P, _P,
                                _P]),
    "sn_crop_census_ws_bytes": (ctypes.c_size_t, [ctypes.c_int64, _I, _I]),
    "sn_census_chunk_points": (c_int, []),
    "sn_crop_census": (c_int, [_P, _P, ctypes.c_int64, _P, _P, _I, _P, _I, _P, ctypes.c_size_t, _P, _P, _P]),
    "sn_points_select_chunk_points": (c_int, []),
    "sn_dbscan_chunk_points": (c_int, []),
    "sn_points_select_ws_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "sn_points_select": (c_int, [_P, _P, ctypes.c_int64, _P, _I, ctypes.c_int64, _P, ctypes.c_size_t, _P, _P, _P, _P]),
    "sn_dbscan_cell_grid": (c_int, [_P, ctypes.c_double, ctypes.c_int64, _P, _P]),
    "sn_dbscan_ws_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64]),
    "sn_dbscan_points": (c_int, [_P, ctypes.c_int64, _P, _P, ctypes.c_int64, _P, ctypes.c_double, _I, ctypes.c_int64, _I, _P,
                                 ctypes.c_size_t, _P, _P, _P, _P, _P]),
    "sn_dbscan_points_launches": (c_int, [_P, ctypes.c_int64, _P, _P, ctypes.c_int64, _P, ctypes.c_double, _I, ctypes.c_int64,
                                          _I, _P, ctypes.c_size_t, _P, _P, _P, _P, _I, _I, _P]),
    "sn_tower_centroids": (c_int, [_P, _P, _I, _I, _I, _P, _P, _I, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                   ctypes.c_double, _P, _P, _P, _P, _P, _P]),
    "sn_las_chunk_records": (c_int, []),
    "sn_las_decode": (c_int, [_P, ctypes.c_int64, _I, _I, _P, _P, _P, _P, _P, _P]),
    "sn_tower_match": (c_int, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _P, ctypes.c_double, _P, _P, _P, _P, _P, _P]),
    "sn_kitti_chunk_points": (c_int, []),
    "sn_kitti_decode": (c_int, [_P, _P, ctypes.c_int64, _P, _I, _P, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P]),
    "sn_las_encode_chunk_records": (c_int, []),
    "sn_las_encode": (c_int, [_P, _P, _P, _P, _P, ctypes.c_int64, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "sn_voxel_cloud_chunk_cells": (c_int, []),
    "sn_voxel_cloud_ws_bytes": (ctypes.c_size_t, [_I, ctypes.c_int64]),
    "sn_voxel_cloud_count": (c_int, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P, ctypes.c_size_t, _P, _P, _P]),
    "sn_voxel_cloud_scatter": (c_int, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, ctypes.c_size_t, _P, ctypes.c_int64, _P, _P,
                                       _P, _P]),
    "sn_thin_ws_bytes": (ctypes.c_size_t, [ctypes.c_int64, _I]),
    "sn_thin_chunk_points": (c_int, []),
    "sn_thin_count": (c_int, [_P, _P, ctypes.c_int64, _I, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P, ctypes.c_size_t, _P, _P, _P,
                              _P]),
    "sn_thin_scatter": (c_int, [_P, _P, _P, ctypes.c_int64, _I, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P, ctypes.c_size_t,
                                ctypes.c_int64, _P, _P, _P, _P, _P]),
    "sn_voxel_classes_chunk_points": (c_int, []),
    "sn_class_chunk_points": (c_int, []),
    "sn_voxel_classes": (c_int, [_P, _P, _P, ctypes.c_int64, _I, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "sn_class_census": (c_int, [_P, _P, ctypes.c_int64, _I, _P, _P, _P]),
    "sn_class_paint": (c_int, [_P, _P, ctypes.c_int64, _I, _P, _P, _I, _P, _P, _P, _I, _P, _P, _P]),
    "sn_scan_merge": (c_int, [_P, _I, _I, _I, _I, _I, _I, _P, _P, ctypes.c_int64, _P, _P, _P, _I, _I, ctypes.c_double, _P, _P,
                              _P]),
    "sn_quantile_forward": (c_int, [_P, _I, _P, _I, _I, _I, ctypes.c_int64, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
    "sn_quantile_backward": (c_int, [_P, _I, _P, _I, _I, _I, ctypes.c_int64, _P, _P, _I, _P, _P, _I, _P, _P]),
    "sn_knn_chunk_points": (c_int, []),
    "sn_knn_ws_bytes": (ctypes.c_size_t, [ctypes.c_int64, _I, ctypes.c_int64]),
    "sn_knn_points": (c_int, [_P, _P, ctypes.c_int64, _I, ctypes.c_double, _I, _I, _P, _I, _I, _I, ctypes.c_int64, _P,
                              ctypes.c_size_t, _P, _P, _P, _P, _P]),
    "sn_knn_points_launches": (c_int, [_P, _P, ctypes.c_int64, _I, ctypes.c_double, _I, _I, _P, _I, _I, _I, ctypes.c_int64, _P,
                                       ctypes.c_size_t, _P, _P, _P, _P, _I, _I, _P]),
    "sn_knn_tile_stats": (c_int, [_P, _P, _P, ctypes.c_int64, _I, _I, _P, ctypes.c_size_t, _P, _P]),
    "sn_shape_chunk_points": (c_int, []),
    "sn_shape_ws_bytes": (ctypes.c_size_t, [ctypes.c_int64, _I, ctypes.c_int64]),
    "sn_shape_points": (c_int, [_P, _P, ctypes.c_int64, _I, ctypes.c_double, _I, _I, _P, _I, _I, _I, ctypes.c_int64, _P,
                                ctypes.c_size_t, _P, _P, _P, _P, _P, _P, _P]),
    "sn_shape_points_launches": (c_int, [_P, _P, ctypes.c_int64, _I, ctypes.c_double, _I, _I, _P, _I, _I, _I, ctypes.c_int64,
                                         _P, ctypes.c_size_t, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "sn_render_chunk_points": (c_int, []),
    "sn_render_splat": (c_int, [_P, _P, ctypes.c_int64, _I, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "sn_render_resolve": (c_int, [_P, _I, _I, _I, _P, _I, _P, _P, _I, ctypes.c_uint32, ctypes.c_double, _P, _P, _P, _P]),
    "sn_voxel_pool_chunk_points": (c_int, []),
    "sn_voxel_pool_ws_bytes": (ctypes.c_int64, [_I, _I, _I, _I, _I]),
    "sn_voxel_pool": (c_int, [_P, _P, _I, _P, ctypes.c_int64, _I, _P, _I, _I, _I, _P, _P, _I, _P, ctypes.c_double, _I, _P, _P,
                              _P, _P, _P, _P]),
}
SN_CONV_PREP_BYTES = 16384
SN_LOSS_WMSE, SN_LOSS_FOCAL_TVERSKY, SN_LOSS_DICE, SN_LOSS_WBCE = 1, 2, 4, 8
SN_LOSS_MAX_BINS = 16
SN_QUANTILE_MAX_Q = 8
SN_OCC_PARTS = 16
SN_BBOX_PARTS = 32
SN_METRIC_NCOUNT, SN_METRIC_NVALUE, SN_METRIC_MAX_PARTS = 6, 5, 1024
SN_METRIC_WS_BYTES = SN_METRIC_MAX_PARTS * SN_METRIC_NCOUNT * 8
SN_CURVE_MAX_THRESHOLDS = 255
SN_TOWER_NSTAT, SN_TOWER_LAUNCHES, SN_TOWER_MAX_RADIUS = 12, 6, 10
SN_TSCORE_MAX_ROWS, SN_TSCORE_NTOTAL = 1024, 8
SN_CROP_DISC, SN_CROP_BOX = 0, 1
SN_CENSUS_MAX_WATCH = 16
SN_DBSCAN_NSTAT, SN_DBSCAN_LAUNCHES = 3, 8
SN_KITTI_MAX_LUT, SN_KITTI_MAX_HIST = 65536, 1024
SN_CLOUD_DENSITY, SN_CLOUD_RANGES, SN_CLOUD_MAX_R = 0, 1, 32
SN_THIN_GROUP_NONE, SN_THIN_GROUP_Z, SN_THIN_GROUP_VOXEL = 0, 1, 2
SN_CLASS_WORDS, SN_VOXEL_CLASSES_NO_SKIP = 2048, 1
SN_MERGE_MAX, SN_MERGE_MEAN, SN_MERGE_INTERIOR = 0, 1, 2
SN_KNN_MAX_K, SN_KNN_NSTAT, SN_KNN_LAUNCHES, SN_KNN_EXCLUDE_ZERO = 16, 5, 4, 1
SN_SHAPE_SWEEPS, SN_SHAPE_NFEAT, SN_SHAPE_LAUNCHES = 4, 6, 5
SN_RENDER_MAX_VIEWS, SN_RENDER_MAX_SPLAT = 64, 9
SN_RENDER_ACCUMULATE, SN_RENDER_NO_LOOK, SN_RENDER_LOOK_ALWAYS = 1, 2, 4
SN_RENDER_RGB16, SN_RENDER_DEPTH = 0, 1
SN_POOL_MEAN, SN_POOL_MIN, SN_POOL_MAX = 0, 1, 2
SN_POOL_MAX_PLANES, SN_POOL_MAX_COLUMNS, SN_VOXEL_POOL_NO_LOOK = 8, 5, 1
OCC_MAX_WORDS = 16 * 1024


class HipLibraryError(RuntimeError):
    pass


_lib = None


def load() -> ctypes.CDLL:
    """Loads libscenenet_hip.so (built by `make` / __graft_entry__.build()).  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f"{LIB_PATH} not found: the HIP extension is not built (run `make` or __graft_entry__.build()). "
            "There is no CPU fallback for this path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().sn_last_error()
        raise HipLibraryError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def device_status() -> Tuple[int, int, int]:
    """(code, workgroup, detail) of the current device's sticky status (sn_device_status): code 0 = healthy; 1 a dependency
    spin of the z-walk gave up, 2 a launch made with `assume_served` was declined by its bank's guard, 3 a tile kernel's
    hand-over spin gave up.  While a code is latched every launching entry of the library raises.  A host memory read: no
    synchronisation -- a kernel that is still running may latch later."""
    code = ctypes.c_int(0)
    detail = (ctypes.c_int * 2)(0, 0)
    _check_plain(load().sn_device_status(ctypes.byref(code), detail), "sn_device_status")
    return int(code.value), int(detail[0]), int(detail[1])


def device_status_clear() -> None:
    """Synchronises the device and re-arms its sticky status (sn_device_status_clear)."""
    _check_plain(load().sn_device_status_clear(), "sn_device_status_clear")


def _check_plain(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().sn_last_error()
        raise HipLibraryError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def set_option(name: str, value: int) -> None:
    """Process-wide library option (include/scenenet_hip.h: sn_set_option)."""
    _check(load().sn_set_option(name.encode(), int(value)), "sn_set_option")


def get_option(name: str) -> int:
    return int(load().sn_get_option(name.encode()))


@contextlib.contextmanager
def options(**values: int):
    """`with options(conv_i8_legacy=1): ...` sets library options for the block and then puts back the values it found, in
    reverse order, on an exception as well.  An unknown name raises before anything is changed."""
    found = []
    for name in values:
        old = get_option(name)
        if old == -1:
            raise HipLibraryError(f"sn_get_option: unknown option '{name}'")
        found.append((name, old))
    try:
        for name, value in values.items():
            set_option(name, value)
        yield
    finally:
        for name, old in reversed(found):
            set_option(name, old)


def conv_i8_path_counts() -> Tuple[int, int, int]:
    """(served by the folded int8 kernel, declined by it: bank not symmetric, sent to the fp32 kernel by its guard) --
    launches of this process on the current device; synchronises (sn_conv_i8_path_counts)."""
    buf = (ctypes.c_ulonglong * 3)()
    _check(load().sn_conv_i8_path_counts(ctypes.cast(buf, ctypes.c_void_p)), "sn_conv_i8_path_counts")
    return int(buf[0]), int(buf[1]), int(buf[2])


def conv_i8_spin_timeouts() -> int:
    """Waves of the int8 kernels that ever gave up a bounded LDS hand-over spin (must be 0); synchronises."""
    buf = (ctypes.c_ulonglong * 1)()
    _check(load().sn_conv_i8_spin_timeouts(ctypes.cast(buf, ctypes.c_void_p)), "sn_conv_i8_spin_timeouts")
    return int(buf[0])


def conv_i8z_round_counts() -> Tuple[int, int]:
    """(rounds run, rounds skipped) by the z-walk contraction since the library was loaded, on the current device: a round
    whose operand window holds no set voxel is skipped unless option conv_i8z_dense is 1, and so is every round of a z segment
    that a workgroup filled without walking it (option conv_i8z_segments); synchronises (sn_conv_i8z_round_counts)."""
    buf = (ctypes.c_ulonglong * 2)()
    _check(load().sn_conv_i8z_round_counts(ctypes.cast(buf, ctypes.c_void_p)), "sn_conv_i8z_round_counts")
    return int(buf[0]), int(buf[1])


def conv_i8z_plane_counts() -> Tuple[int, int]:
    """(planes streamed, planes trimmed away) by the head-only z-walk since the library was loaded, on the current device: where
    the balanced deal stands a live z segment streams only its live output planes' range (option conv_i8z_trim), and the planes
    it leaves out are counted in the second figure; synchronises (sn_conv_i8z_plane_counts)."""
    buf = (ctypes.c_ulonglong * 2)()
    _check(load().sn_conv_i8z_plane_counts(ctypes.cast(buf, ctypes.c_void_p)), "sn_conv_i8z_plane_counts")
    return int(buf[0]), int(buf[1])


def voxel_onepass_giveups() -> int:
    """Workgroups of the one-pass voxelisation kernel that ever gave up the box exchange's bounded wait and took their tile's
    box from the points alone (same bits; 0 in normal use, every workgroup with voxel_onepass_spin = 0); synchronises."""
    buf = (ctypes.c_ulonglong * 1)()
    _check(load().sn_voxel_onepass_giveups(ctypes.cast(buf, ctypes.c_void_p)), "sn_voxel_onepass_giveups")
    return int(buf[0])


def launch_timing_events(start: "torch.cuda.Event", stop: "torch.cuda.Event") -> None:
    """sn_launch_timing_events: the next z-walk launch of this thread writes its own start / stop timestamps into the two
    events (both created with enable_timing=True and RECORDED ONCE before -- torch creates the hipEvent_t at the first
    record, and elapsed_time() wants both marked as recorded)."""
    a, b = int(start.cuda_event), int(stop.cuda_event)
    if not a or not b:
        raise HipLibraryError("launch_timing_events: record each event once first (torch creates the handle lazily)")
    _check_plain(load().sn_launch_timing_events(ctypes.c_void_p(a), ctypes.c_void_p(b)), "sn_launch_timing_events")


def _ptr(t: Optional[torch.Tensor], dtype: Optional[torch.dtype] = None, name: str = "tensor") -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise HipLibraryError(f"{name} must live on a HIP device (got {t.device}); there is no CPU path")
    if not t.is_contiguous():
        raise HipLibraryError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise HipLibraryError(f"{name} must be {dtype} (got {t.dtype})")
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """HIP stream handle of torch's current stream on the current device (what every launch of the C ABI goes to).
    The raw accessor costs ~0.3 us; torch.cuda.current_stream() builds a Stream object (~12 us per call measured on
    the GPU box, six calls per step: the fused forward step is 0.11 ms of GPU work)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _common_device(tensors) -> Optional[torch.device]:
    """The one HIP device every tensor argument of a C-ABI call lives on (None when there is no device tensor).
    Raises on a mix: the library takes raw pointers and ONE stream, so operands on different devices would be
    dereferenced from the wrong device."""
    dev = None
    for t in tensors:
        if t is None or not getattr(t, "is_cuda", False):
            continue   # CPU tensors are rejected with their own message by _ptr
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise HipLibraryError(f"tensor arguments live on different devices ({dev} and {t.device}); "
                                  "a call of the C ABI runs on one device and one stream")
    return dev


_get_device = getattr(torch._C, "_cuda_getDevice", None)


def _on_tensor_device(fn):
    """Runs a wrapper with the HIP device of its tensor arguments current, so `_stream()` (torch's current stream on
    the CURRENT device) and the launch itself match the pointers -- `model.to('cuda:1')` while cuda:0 is current would
    otherwise launch on device 0 with device-1 pointers.  Tensors on different devices are refused (_common_device).
    Cheap on the common path (the eager forward step is host bound at ~0.1 ms): one `get_device()` per tensor argument,
    no objects built."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        idx = -1
        for a in args:
            if isinstance(a, torch.Tensor):
                d = a.get_device()
                if d >= 0:
                    if idx < 0:
                        idx = d
                    elif d != idx:
                        _common_device([t for t in args if isinstance(t, torch.Tensor)])   # raises with the message
        if kwargs:
            for a in kwargs.values():
                if isinstance(a, torch.Tensor):
                    d = a.get_device()
                    if d >= 0:
                        if idx < 0:
                            idx = d
                        elif d != idx:
                            _common_device([t for t in list(args) + list(kwargs.values()) if isinstance(t, torch.Tensor)])
        if idx < 0 or idx == (_get_device() if _get_device is not None else torch.cuda.current_device()):
            return fn(*args, **kwargs)
        with torch.cuda.device(idx):
            return fn(*args, **kwargs)
    return wrapper


# torch.bool (one byte, 0/1) is the binary-occupancy dtype: sn_conv_bank takes it on the int8 matrix cores
# torch.bfloat16: STORAGE of activations and their gradients in the training path (sn_conv_fused out, sn_loss_* pred /
# grad, sn_conv_corr_t gradients); never an input grid
_DT = {torch.float32: SN_F32, torch.float64: SN_F64, torch.uint8: SN_U8, torch.bool: SN_OCC8, torch.bfloat16: SN_BF16}
_DT_OUT = {torch.float32: SN_F32, torch.float64: SN_F64, torch.uint8: SN_U8, torch.bool: SN_U8,
           torch.bfloat16: SN_BF16}


# --------------------------------------------------------------------------- #
@_on_tensor_device
def geneo_bank(params: torch.Tensor, kinds: torch.Tensor, kernel_size: Sequence[int],
               status: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """params [G, SN_NPARAM] f32, kinds [G] i32 -> bank [G, kz, kx, ky] f32 (sn_geneo_bank)."""
    G = params.shape[0]
    kz, kx, ky = (int(k) for k in kernel_size)
    if out is None:
        out = torch.empty((G, kz, kx, ky), dtype=torch.float32, device=params.device)
    rc = load().sn_geneo_bank(_ptr(params, torch.float32, "params"), _ptr(kinds, torch.int32, "kinds"), G, kz, kx, ky,
                              _ptr(out, torch.float32, "bank"), _ptr(status, torch.int32, "status"), _stream())
    _check(rc, "sn_geneo_bank")
    return out


@_on_tensor_device
def geneo_bank_lambdas(params: torch.Tensor, kinds: torch.Tensor, kernel_size: Sequence[int], lambdas: torch.Tensor,
                       order: torch.Tensor, last: int):
    """sn_geneo_bank_lambdas: (bank [G,kz,kx,ky], effective coefficients [G]) in one launch; `lambdas[last]` is
    refreshed in place like sn_effective_lambdas does."""
    G = params.shape[0]
    kz, kx, ky = (int(k) for k in kernel_size)
    bank = torch.empty((G, kz, kx, ky), dtype=torch.float32, device=params.device)
    lam = torch.empty((G,), dtype=torch.float32, device=params.device)
    rc = load().sn_geneo_bank_lambdas(_ptr(params, torch.float32, "params"), _ptr(kinds, torch.int32, "kinds"), G, kz,
                                      kx, ky, _ptr(bank), None, _ptr(lambdas, torch.float32, "lambdas"),
                                      _ptr(order, torch.int32, "order"), int(last), _ptr(lam), _stream())
    _check(rc, "sn_geneo_bank_lambdas")
    return bank, lam


@_on_tensor_device
def geneo_bank_prep(params: torch.Tensor, kinds: torch.Tensor, lambdas: Optional[torch.Tensor] = None,
                    order: Optional[torch.Tensor] = None, last: int = 0, bank: Optional[torch.Tensor] = None,
                    lam_out: Optional[torch.Tensor] = None, prep: Optional[torch.Tensor] = None):
    """sn_geneo_bank_prep: the 9 x 9 x 9 bank, (optionally) the effective coefficients, and the int8 contraction's
    preparation blob in ONE launch -> (bank [G,9,9,9] f32, lam [G] f32 | None, prep uint8).  `bank`, `lam_out`, `prep`:
    caller-owned outputs to write into (persistent buffers: nothing is allocated on the step)."""
    G = params.shape[0]
    if bank is None:
        bank = torch.empty((G, 9, 9, 9), dtype=torch.float32, device=params.device)
    nbytes = SN_CONV_PREP_BYTES * ((G + 15) // 16)
    if prep is None:
        prep = torch.empty(nbytes, dtype=torch.uint8, device=params.device)
    if lambdas is not None and lam_out is None:
        lam_out = torch.empty(G, dtype=torch.float32, device=params.device)
    rc = load().sn_geneo_bank_prep(_ptr(params, torch.float32, "params"), _ptr(kinds, torch.int32, "kinds"), G, 9, 9, 9,
                                   _ptr(bank, torch.float32, "bank"), None, _ptr(lambdas, torch.float32, "lambdas"),
                                   _ptr(order, torch.int32, "order"), int(last), _ptr(lam_out, torch.float32, "lam_out"),
                                   _ptr(prep, torch.uint8, "prep"), _stream())
    _check(rc, "sn_geneo_bank_prep")
    return bank, (lam_out if lambdas is not None else None), prep


def prep_verdicts(prep: torch.Tensor) -> torch.Tensor:
    """view of the walk's verdict words (int32, one per group of 16 kernels) inside a preparation blob"""
    off = int(load().sn_conv_prep_verdict_offset())
    return prep.view(-1, SN_CONV_PREP_BYTES)[:, off:off + 4].view(torch.int32).reshape(-1)


class PreparedVerdict:
    """Learns, WITHOUT synchronising, whether the launches of one (weights, coefficients, tolerance, outputs) combination
    are served by the z-walk, so that later launches of the same combination can leave the fallback launch out
    (sn_conv_bank_prepared_served).  After a launch made with the fallback in place, `note(prep, key)` enqueues a 4-byte
    copy of the verdict words into pinned host memory and records an event; `served(key)` is True once that copy has
    completed and read 0 -- until then (and for every new key: an optimiser step changes it) the caller keeps the fallback.
    The words start every preparation at -1 (conv_prep.h): a 0 can only have been written by a walk that ran on THIS bank,
    and a -1 that comes back (the noted call was not the walk's) teaches nothing.  A caller whose knowledge is stale anyway
    -- the one thing the key cannot see is a raw-pointer write -- gets NaN outputs and the sticky device status from the
    launch itself (sn_conv_bank_prepared_served), never an unwritten buffer."""

    def __init__(self):
        self._key = None
        self._state = 0          # 0 nothing known, 1 read-back in flight, 2 served, 3 not served
        self._host = None
        self._event = None

    def __reduce__(self):
        # copied / pickled with a module: a fresh object that knows nothing (the event and the pinned buffer stay behind)
        return (PreparedVerdict, ())

    def served(self, key) -> bool:
        if torch.cuda.is_current_stream_capturing():
            return False   # a captured graph outlives these parameters: it keeps the fallback launch
        if key != self._key:
            self._key, self._state = key, 0
            return False
        if self._state == 1 and self._event.query():
            # -1: the preparation's sentinel -- no walk has written a verdict for this bank (the call that was noted went to
            # other kernels: a shape the walk does not serve): nothing learnt, the next call is noted again
            if int(self._host.min()) < 0:
                self._state = 0
            else:
                self._state = 2 if int(self._host.max()) == 0 else 3
        return self._state == 2

    def note(self, prep: torch.Tensor, key) -> None:
        self.note_words(prep_verdicts(prep), key)

    def note_words(self, words: torch.Tensor, key) -> None:
        """`words`: int32 device tensor of verdict words (all 0 = served) written by the launch just enqueued"""
        if key != self._key or self._state != 0 or torch.cuda.is_current_stream_capturing():
            return
        if self._host is None or self._host.numel() != words.numel():
            self._host = torch.empty(words.numel(), dtype=torch.int32, pin_memory=True)
        self._host.copy_(words, non_blocking=True)
        self._event = torch.cuda.Event()
        self._event.record()
        self._state = 1


@_on_tensor_device
def conv_bank_prep(bank: torch.Tensor, prep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The per-bank work of the int8 contraction, once (sn_conv_bank_prep): symmetry verdict, 24-bit fixed-point weights,
    error bounds and digit table of `bank` [G,kz,kx,ky] f32 into a caller-owned blob (uint8, SN_CONV_PREP_BYTES per group
    of 16 kernels), which conv_bank(..., prep=) then uses.  One blob serves the launches of one stream at a time."""
    G, kz, kx, ky = bank.shape
    nbytes = SN_CONV_PREP_BYTES * ((G + 15) // 16)
    if prep is None:
        prep = torch.empty(nbytes, dtype=torch.uint8, device=bank.device)
    elif prep.dtype != torch.uint8 or prep.numel() < nbytes:
        raise HipLibraryError(f"prep must be uint8 with at least {nbytes} bytes")
    rc = load().sn_conv_bank_prep(_ptr(bank, torch.float32, "bank"), G, kz, kx, ky, _ptr(prep, torch.uint8, "prep"),
                                  _stream())
    _check(rc, "sn_conv_bank_prep")
    return prep


ROWS_ATTR = "_sn_row_bits"


def row_bits_of(occ: torch.Tensor) -> torch.Tensor:
    """The row bits of an occupancy [B,1,Z,X,Y] (any dtype; set = non-zero) in plain torch ops: int32 [B, Z, ceil(X / 32)],
    bit x % 32 of word x / 32 set iff occ[b, 0, z, x, :] holds a set voxel (include/scenenet_hip.h,
    sn_conv_bank_prepared_rows).  No synchronisation; usable inside a graph capture."""
    B, _, Z, X, _ = occ.shape
    wx = (X + 31) // 32
    any_y = (occ[:, 0] != 0).any(dim=-1)                                        # [B, Z, X]
    if wx * 32 != X:
        any_y = torch.nn.functional.pad(any_y, (0, wx * 32 - X))
    shifts = torch.arange(32, dtype=torch.int64, device=occ.device)            # (made on the device: no copy, no sync)
    v = (any_y.reshape(B, Z, wx, 32).to(torch.int64) << shifts).sum(dim=-1)
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32).contiguous()


def attach_rows(occ: torch.Tensor, rows: torch.Tensor) -> None:
    """The voxel stage's note on the occupancy tensor it returns: the bits, and what `occ` was when they were made"""
    setattr(occ, ROWS_ATTR, (rows, occ._version, occ.data_ptr(), tuple(occ.shape)))


def rows_for(x: torch.Tensor) -> Optional[torch.Tensor]:
    """The row bits attached to THIS tensor object, if it has not been written since (same version counter, storage and
    shape) and they live on its device; else None -- a missing bit would be a silently wrong result, a missing tensor of
    bits only costs time."""
    note = getattr(x, ROWS_ATTR, None)
    if note is None:
        return None
    rows, version, ptr, shape = note
    if x._version != version or x.data_ptr() != ptr or tuple(x.shape) != shape or rows.device != x.device:
        return None
    return rows


@_on_tensor_device
def conv_bank(x: torch.Tensor, bank: torch.Tensor, lambdas: Optional[torch.Tensor], want_act: bool = False,
              want_out: bool = True, out_dtype: Optional[torch.dtype] = None, prep: Optional[torch.Tensor] = None,
              assume_served: bool = False, row_bits: Optional[torch.Tensor] = None,
              plan_out: Optional[torch.Tensor] = None):
    """x [B,1,Z,X,Y] (f32|f64|u8|bool), bank [G,kz,kx,ky] f32, lambdas [G] f32 (effective) ->
    (act [B,G,Z,X,Y] | None, out [B,1,Z,X,Y] | None) of out_dtype (sn_conv_bank; with `prep` = conv_bank_prep(bank):
    sn_conv_bank_prepared -- same results bit for bit, the per-bank work not repeated; `assume_served`: the caller has
    read the blob's verdict as 0 for these weights / coefficients / tolerance / outputs: sn_conv_bank_prepared_served, no
    fallback launch -- see PreparedVerdict).  With `prep`, the occupancy's row bits travel to the z-walk's balanced deal
    (sn_conv_bank_prepared_rows): `row_bits` as given (the caller vouches that they describe x: row_bits_of), else the ones
    the voxel stage left on this very tensor -- taken only while x is still what they were made for (rows_for).  plan_out:
    int32 [compute units, 65], receives the deal (diagnostics)."""
    if x.dim() != 5 or x.shape[1] != 1:
        raise HipLibraryError(f"x must be [B,1,Z,X,Y] (got {tuple(x.shape)})")
    if x.dtype not in _DT or x.dtype == torch.bfloat16:
        raise HipLibraryError(f"x dtype {x.dtype} unsupported (f32, f64, u8, bool)")
    B, _, Z, X, Y = x.shape
    G, kz, kx, ky = bank.shape
    if out_dtype is None:
        out_dtype = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32
    act = torch.empty((B, G, Z, X, Y), dtype=out_dtype, device=x.device) if want_act else None
    out = torch.empty((B, 1, Z, X, Y), dtype=out_dtype, device=x.device) if want_out else None
    if prep is not None:
        if prep.dtype != torch.uint8 or prep.numel() < SN_CONV_PREP_BYTES * ((G + 15) // 16):
            raise HipLibraryError("prep: not a blob of conv_bank_prep for this bank")
        rows = row_bits if row_bits is not None else rows_for(x)
        if rows is not None and (rows.dtype != torch.int32 or rows.device != x.device or not rows.is_contiguous()
                                 or tuple(rows.shape) != (B, Z, (X + 31) // 32)):
            raise HipLibraryError("row_bits: int32 [B, Z, ceil(X / 32)] on x's device")
        if plan_out is not None:   # (the launch writes row blockIdx.x of [compute units][65])
            cus = torch.cuda.get_device_properties(x.device).multi_processor_count
            if plan_out.dtype != torch.int32 or plan_out.device != x.device or plan_out.numel() < 65 * cus:
                raise HipLibraryError(f"plan_out: int32 on x's device with at least {cus} x 65 words")
        rc = load().sn_conv_bank_prepared_rows(
            _ptr(x, None, "x"), _DT[x.dtype], _ptr(bank, torch.float32, "bank"),
            _ptr(lambdas, torch.float32, "lambdas"), _ptr(prep, torch.uint8, "prep"),
            B, Z, X, Y, G, kz, kx, ky, _ptr(act, None, "act"), _ptr(out, None, "out"),
            _DT_OUT[out_dtype], _stream(), int(bool(assume_served)), _ptr(rows, torch.int32, "row_bits"),
            _ptr(plan_out, torch.int32, "plan_out"))
        _check(rc, "sn_conv_bank_prepared_rows")
        return act, out
    rc = load().sn_conv_bank(_ptr(x, None, "x"), _DT[x.dtype], _ptr(bank, torch.float32, "bank"),
                             _ptr(lambdas, torch.float32, "lambdas"), B, Z, X, Y, G, kz, kx, ky,
                             _ptr(act, None, "act"), _ptr(out, None, "out"), _DT_OUT[out_dtype], _stream())
    _check(rc, "sn_conv_bank")
    return act, out


class ConvPlan(NamedTuple):
    """sn_conv_bank_plan's eight words (include/scenenet_hip.h)."""
    kernel: str          # "fp32" | "four_copy" | "stride4" | "folded"
    tz: int
    tx: int
    ntiles: int
    double_buffered: bool
    staged: bool         # halo staged by LDS-DMA
    row_stride: int      # bytes of a halo row in LDS
    cus: int             # compute units the tile ladder counted

    @property
    def rung(self) -> Tuple[int, int]:
        return (self.tz, self.tx)


CONV_PLAN_KERNELS = ("fp32", "four_copy", "stride4", "folded")


def conv_bank_plan(x, bank_shape: Sequence[int]) -> ConvPlan:
    """What conv_bank(x, bank) would launch under the options in force (sn_conv_bank_plan: host only, no launch, no device
    needed).  x: a [B,1,Z,X,Y] tensor on any device, or (dtype, shape); bank_shape: (G, kz, kx, ky)."""
    dtype, shape = (x.dtype, tuple(x.shape)) if isinstance(x, torch.Tensor) else (x[0], tuple(x[1]))
    if len(shape) != 5 or shape[1] != 1:
        raise HipLibraryError(f"x must be [B,1,Z,X,Y] (got {shape})")
    if dtype not in _DT or dtype == torch.bfloat16:
        raise HipLibraryError(f"x dtype {dtype} unsupported (f32, f64, u8, bool)")
    B, _, Z, X, Y = (int(v) for v in shape)
    G, kz, kx, ky = (int(v) for v in bank_shape)
    p = (ctypes.c_int32 * 8)()
    _check(load().sn_conv_bank_plan(_DT[dtype], B, Z, X, Y, G, kz, kx, ky, ctypes.cast(p, c_void_p)), "sn_conv_bank_plan")
    return ConvPlan(CONV_PLAN_KERNELS[p[0]], int(p[1]), int(p[2]), int(p[3]), bool(p[4] & 1), bool(p[4] & 2), int(p[5]),
                    int(p[6]))


def conv_fused_supported(x: torch.Tensor, kernel_size: Sequence[int]) -> bool:
    """Shapes sn_conv_fused serves: binary occupancy [B,1,Z,X,Y], and whatever the library's own plan accepts
    (sn_conv_fused_supported: Y % 4 == 0, a 16-y strip's window within 32 bytes, tables + halo in LDS)."""
    if x.dtype != torch.bool or x.dim() != 5:
        return False
    kz, kx, ky = (int(k) for k in kernel_size)
    B, _, Z, X, Y = x.shape
    return bool(load().sn_conv_fused_supported(int(B), int(Z), int(X), int(Y), kz, kx, ky))


class ConvFusedPlan(NamedTuple):
    """sn_conv_fused_plan's eight words (include/scenenet_hip.h)."""
    w24: bool            # kernel rows packed at 24 bytes of K (else 32)
    nsteps: int          # MFMA steps per tile
    deferred: bool       # a tile's outputs are finished between the MFMAs of the workgroup's next tile
    halo_passes: int     # > 16: the synchronous remainder pass runs
    ntiles: int
    workgroups: int
    lds_bytes: int
    cus: int

    @property
    def tiles_per_workgroup_min(self) -> int:
        return self.ntiles // self.workgroups

    @property
    def tiles_per_workgroup_max(self) -> int:
        return -(-self.ntiles // self.workgroups)


def conv_fused_plan(x_or_shape, kernel_size: Sequence[int], G: int = 1) -> ConvFusedPlan:
    """What conv_fused(x, bank, lambdas) would launch under the options in force (sn_conv_fused_plan: host only, no launch,
    no device needed).  x_or_shape: a [B,1,Z,X,Y] tensor on any device, or that shape; kernel_size: (kz, kx, ky)."""
    shape = tuple(x_or_shape.shape) if isinstance(x_or_shape, torch.Tensor) else tuple(x_or_shape)
    if len(shape) != 5 or shape[1] != 1:
        raise HipLibraryError(f"x must be [B,1,Z,X,Y] (got {shape})")
    B, _, Z, X, Y = (int(v) for v in shape)
    kz, kx, ky = (int(k) for k in kernel_size)
    p = (ctypes.c_int32 * 8)()
    _check(load().sn_conv_fused_plan(B, Z, X, Y, int(G), kz, kx, ky, ctypes.cast(p, c_void_p)), "sn_conv_fused_plan")
    return ConvFusedPlan(bool(p[0]), int(p[1]), bool(p[2]), int(p[3]), int(p[4]), int(p[5]), int(p[6]), int(p[7]))


@_on_tensor_device
def conv_fused(x: torch.Tensor, bank: torch.Tensor, lambdas: torch.Tensor,
               out_dtype: torch.dtype = torch.float32, verdict: Optional[torch.Tensor] = None,
               assume_served: bool = False, prep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """relu(tanh(conv3d(x, sum_g lambda_g K_g))) [B,1,Z,X,Y] (sn_conv_fused): the forward output through linearity.
    verdict: a caller-owned int32 [1] device tensor that receives the guard's verdict (sn_conv_fused_v); assume_served:
    the caller has read it as 0 for these weights / coefficients / tolerance -- the gated fp32 launches are left out."""
    B, _, Z, X, Y = x.shape
    G, kz, kx, ky = bank.shape
    out = torch.empty((B, 1, Z, X, Y), dtype=out_dtype, device=x.device)
    if prep is not None:   # the tables come from a blob (conv_fused_prep): same bits
        rc = load().sn_conv_fused_prepared(_ptr(x, None, "x"), _DT[x.dtype], _ptr(bank, torch.float32, "bank"),
                                           _ptr(lambdas, torch.float32, "lambdas"), _ptr(prep, torch.uint8, "prep"), B, Z,
                                           X, Y, G, kz, kx, ky, _ptr(out), _DT_OUT[out_dtype], int(bool(assume_served)),
                                           _stream())
        _check(rc, "sn_conv_fused_prepared")
        return out
    if verdict is None:
        rc = load().sn_conv_fused(_ptr(x, None, "x"), _DT[x.dtype], _ptr(bank, torch.float32, "bank"),
                                  _ptr(lambdas, torch.float32, "lambdas"), B, Z, X, Y, G, kz, kx, ky, _ptr(out),
                                  _DT_OUT[out_dtype], _stream())
    else:
        rc = load().sn_conv_fused_v(_ptr(x, None, "x"), _DT[x.dtype], _ptr(bank, torch.float32, "bank"),
                                    _ptr(lambdas, torch.float32, "lambdas"), B, Z, X, Y, G, kz, kx, ky, _ptr(out),
                                    _DT_OUT[out_dtype], _ptr(verdict, torch.int32, "verdict"), int(bool(assume_served)),
                                    _stream())
    _check(rc, "sn_conv_fused")
    return out


def conv_fused_prep_bytes(kernel_size: Sequence[int]) -> int:
    kz, kx, ky = (int(k) for k in kernel_size)
    return int(load().sn_conv_fused_prep_bytes(kz, kx, ky))


@_on_tensor_device
def conv_fused_prep(bank: torch.Tensor, lambdas: torch.Tensor, blob: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sn_conv_fused_prep: the fused forward's per-(bank, coefficients) tables into a blob (uint8) conv_fused(prep=) uses."""
    G, kz, kx, ky = bank.shape
    nbytes = conv_fused_prep_bytes((kz, kx, ky))
    if nbytes == 0:
        raise HipLibraryError(f"sn_conv_fused_prep: kernel {kz}x{kx}x{ky} is outside the combined kernel")
    if blob is None:
        blob = torch.empty(nbytes, dtype=torch.uint8, device=bank.device)
    elif blob.dtype != torch.uint8 or blob.numel() < nbytes:
        raise HipLibraryError(f"blob must be uint8 with at least {nbytes} bytes")
    _check(load().sn_conv_fused_prep(_ptr(bank, torch.float32, "bank"), _ptr(lambdas, torch.float32, "lambdas"), G, kz, kx,
                                     ky, _ptr(blob, torch.uint8, "blob"), _stream()), "sn_conv_fused_prep")
    return blob


def conv_fused_prep_verdict(blob: torch.Tensor, kernel_size: Sequence[int]) -> torch.Tensor:
    """view of the guard's verdict word (int32 [1]) inside a fused-forward blob"""
    n = conv_fused_prep_bytes(kernel_size)
    return blob[n - 12:n - 8].view(torch.int32)


@_on_tensor_device
def forward_auto(x: torch.Tensor, bank: torch.Tensor, lambdas: torch.Tensor, out_dtype: Optional[torch.dtype] = None):
    """sn_forward_auto: the forward output for a float grid; binary grids (the reference's f64 {0,1} input) take the
    int8 path, anything else the fp32 contraction, decided on the device.  Returns (out, not_binary flag [1] i32).
    out_dtype: float32 | float64 (sn_conv_bank's output contract; default x's own)."""
    if x.dim() != 5 or x.shape[1] != 1:
        raise HipLibraryError(f"x must be [B,1,Z,X,Y] (got {tuple(x.shape)})")
    if x.dtype not in (torch.float32, torch.float64):
        raise HipLibraryError(f"x dtype {x.dtype} unsupported (f32, f64; byte grids: conv_fused / conv_bank)")
    B, _, Z, X, Y = x.shape
    G, kz, kx, ky = bank.shape
    out_dtype = x.dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise HipLibraryError(f"out_dtype {out_dtype} unsupported (f32, f64)")
    if x.data_ptr() % 16:   # a sliced view (x[1:] of an odd-sized grid): the binary check reads 16-byte vectors
        x = x.clone()
    out = torch.empty((B, 1, Z, X, Y), dtype=out_dtype, device=x.device)
    occ = torch.empty((x.numel(),), dtype=torch.uint8, device=x.device)
    flag = torch.empty((1,), dtype=torch.int32, device=x.device)
    rc = load().sn_forward_auto(_ptr(x, None, "x"), _DT[x.dtype], _ptr(bank, torch.float32, "bank"),
                                _ptr(lambdas, torch.float32, "lambdas"), B, Z, X, Y, G, kz, kx, ky, _ptr(occ), _ptr(flag),
                                _ptr(out), _DT_OUT[out_dtype], _stream())
    _check(rc, "sn_forward_auto")
    return out, flag


def desc_len(nx: int, ny: int, nz: int) -> int:
    return 6 + nx + ny + nz + 3


@_on_tensor_device
def voxel_bbox(pts: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    B = offsets.numel() - 1
    bbox = torch.empty((B, 6), dtype=torch.float64, device=pts.device)
    rc = load().sn_voxel_bbox(_ptr(pts, torch.float64, "pts"), _ptr(offsets, torch.int64, "offsets"), B,
                              _ptr(bbox), _stream())
    _check(rc, "sn_voxel_bbox")
    return bbox


@_on_tensor_device
def voxel_prepare(pts: torch.Tensor, offsets: torch.Tensor, n_xyz: Sequence[int], regular: bool = True,
                  want_bbox: bool = False):
    """bbox + cube + linspace edge tables in two launches (sn_voxel_prepare): returns (desc, bbox | None)."""
    B = offsets.numel() - 1
    nx, ny, nz = (int(v) for v in n_xyz)
    dev = pts.device
    partial = torch.empty((B, SN_BBOX_PARTS, 6), dtype=torch.float64, device=dev)
    desc = torch.empty((B, desc_len(nx, ny, nz)), dtype=torch.float64, device=dev)
    bbox = torch.empty((B, 6), dtype=torch.float64, device=dev) if want_bbox else None
    rc = load().sn_voxel_prepare(_ptr(pts, torch.float64, "pts"), _ptr(offsets, torch.int64, "offsets"), B, nx, ny, nz,
                                 int(regular), _ptr(partial), _ptr(bbox), _ptr(desc), _stream())
    _check(rc, "sn_voxel_prepare")
    return desc, bbox


@_on_tensor_device
def voxel_desc(bbox: torch.Tensor, n_xyz: Sequence[int], regular: bool = True, from_bounds: bool = False):
    B = bbox.shape[0]
    nx, ny, nz = (int(v) for v in n_xyz)
    desc = torch.empty((B, desc_len(nx, ny, nz)), dtype=torch.float64, device=bbox.device)
    if from_bounds:
        rc = load().sn_voxel_desc_from_bounds(_ptr(bbox, torch.float64, "bounds"), B, nx, ny, nz, _ptr(desc),
                                              _stream())
    else:
        rc = load().sn_voxel_desc(_ptr(bbox, torch.float64, "bbox"), B, nx, ny, nz, int(regular), _ptr(desc),
                                  _stream())
    _check(rc, "sn_voxel_desc")
    return desc


@_on_tensor_device
def voxel_desc_sized(bbox: torch.Tensor, voxel_dims: Sequence[float], max_n_xyz: Sequence[int]):
    """sn_voxel_desc_sized: size-mode descriptors of a batch on the device.  Returns (desc [B, desc_len(max)], dims
    [B,3] i32 = (n_x, n_y, n_z) per tile, status [B] i32 = 1 where a tile needs more than the maximum)."""
    B = bbox.shape[0]
    nx, ny, nz = (int(v) for v in max_n_xyz)
    dev = bbox.device
    desc = torch.empty((B, desc_len(nx, ny, nz)), dtype=torch.float64, device=dev)
    dims = torch.empty((B, 3), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    if len(voxel_dims) != 3:
        raise HipLibraryError("voxel_dims must have 3 entries (size_x, size_y, size_z)")
    sz = (ctypes.c_double * 3)(*[float(v) for v in voxel_dims])
    rc = load().sn_voxel_desc_sized(_ptr(bbox, torch.float64, "bbox"), B, ctypes.cast(sz, c_void_p), nx, ny, nz,
                                    _ptr(desc), _ptr(dims), _ptr(status), _stream())
    _check(rc, "sn_voxel_desc_sized")
    return desc, dims, status


@_on_tensor_device
def voxel_finalize_sized(counts, towers, desc, want_density=False, want_gt=False, want_occ=True, want_gt_occ=False):
    """sn_voxel_finalize_sized: voxel_finalize over each tile's own part of the padded grids."""
    B, nz, nx, ny = counts.shape
    dev = counts.device
    shape = (B, 1, nz, nx, ny)
    colstats = torch.empty((B, 2, ny), dtype=torch.int32, device=dev) if (want_density or want_occ) else None
    density = torch.empty(shape, dtype=torch.float64, device=dev) if want_density else None
    gt = torch.empty(shape, dtype=torch.float64, device=dev) if want_gt else None
    occ = torch.empty(shape, dtype=torch.float32, device=dev) if want_occ else None
    gt_occ = torch.empty(shape, dtype=torch.float32, device=dev) if want_gt_occ else None
    rc = load().sn_voxel_finalize_sized(_ptr(counts, torch.int32, "counts"), _ptr(towers, torch.int32, "towers"), B, nx,
                                        ny, nz, _ptr(desc, torch.float64, "desc"), _ptr(colstats), _ptr(density),
                                        _ptr(gt), _ptr(occ), _ptr(gt_occ), _stream())
    _check(rc, "sn_voxel_finalize_sized")
    return density, gt, occ, gt_occ


@_on_tensor_device
def voxel_scatter(pts, labels, offsets, desc, n_xyz, keep_labels: Sequence[float] = (), want_towers: bool = False,
                  counts=None, towers=None, dropped=None):
    B = offsets.numel() - 1
    nx, ny, nz = (int(v) for v in n_xyz)
    dev = pts.device
    if counts is None:
        counts = torch.empty((B, nz, nx, ny), dtype=torch.int32, device=dev)
    if want_towers and towers is None:
        towers = torch.empty((B, nz, nx, ny), dtype=torch.int32, device=dev)
    if dropped is None:
        dropped = torch.empty((B,), dtype=torch.int32, device=dev)
    keep = (ctypes.c_double * max(1, len(keep_labels)))(*[float(k) for k in keep_labels])
    rc = load().sn_voxel_scatter(_ptr(pts, torch.float64, "pts"), _ptr(labels, torch.float64, "labels"),
                                 _ptr(offsets, torch.int64, "offsets"), B, _ptr(desc, torch.float64, "desc"),
                                 nx, ny, nz, _ptr(counts, torch.int32, "counts"),
                                 _ptr(towers, torch.int32, "towers") if want_towers else None,
                                 ctypes.cast(keep, c_void_p), len(keep_labels), _ptr(dropped), _stream())
    _check(rc, "sn_voxel_scatter")
    return counts, (towers if want_towers else None), dropped


@_on_tensor_device
def voxel_finalize(counts, towers, want_density=False, want_gt=False, want_occ=True, want_gt_occ=False):
    B, nz, nx, ny = counts.shape
    dev = counts.device
    shape = (B, 1, nz, nx, ny)
    colstats = torch.empty((B, 2, ny), dtype=torch.int32, device=dev) if (want_density or want_occ) else None
    density = torch.empty(shape, dtype=torch.float64, device=dev) if want_density else None
    gt = torch.empty(shape, dtype=torch.float64, device=dev) if want_gt else None
    occ = torch.empty(shape, dtype=torch.float32, device=dev) if want_occ else None
    gt_occ = torch.empty(shape, dtype=torch.float32, device=dev) if want_gt_occ else None
    rc = load().sn_voxel_finalize(_ptr(counts, torch.int32, "counts"), _ptr(towers, torch.int32, "towers"), B, nx, ny,
                                  nz, _ptr(colstats), _ptr(density), _ptr(gt), _ptr(occ), _ptr(gt_occ), _stream())
    _check(rc, "sn_voxel_finalize")
    return density, gt, occ, gt_occ


def occupancy_supported(n_xyz: Sequence[int], planes: int) -> bool:
    """mirrors sn_voxel_occupancy's z-slab rule: some power-of-two slab count <= SN_OCC_PARTS fits the LDS bitmap."""
    nx, ny, nz = (int(v) for v in n_xyz)
    V = nx * ny * nz
    if V % 32:
        return False
    sl = 1
    while sl <= SN_OCC_PARTS:
        if nz % sl == 0 and (V // 32) % sl == 0 and ((nz // sl) * nx * ny) % 32 == 0 \
                and (V // 32 // sl) * planes <= OCC_MAX_WORDS:
            return True
        sl *= 2
    return False


class OccupancyPlan(NamedTuple):
    """sn_voxel_occupancy_plan's eight words (include/scenenet_hip.h)."""
    one_pass: int        # 1: the one-pass kernel, 0: the two-kernel form
    slabs: int           # z-slabs of the LDS bitmap
    parts: int           # partial bitmaps per tile
    proof: int           # 0 none, 1 on the merged words, 2 a second pass over the rows
    vec4: int            # the finalize kernel takes four words per thread
    wpr: int             # ny // 32
    finalize_blocks: int
    lds_bytes: int       # dynamic LDS of the binning launch


def voxel_occupancy_plan(n_xyz: Sequence[int], planes: int = 1, B: int = 1, fused: bool = False, sized: bool = False,
                         pts_aligned16: bool = True, labels_aligned16: bool = True, ws_aligned16: bool = True,
                         want_flags: bool = True) -> Optional[OccupancyPlan]:
    """What the bitmap entries would launch under the options in force (sn_voxel_occupancy_plan: host only, no launch, no
    device needed); None where they return SN_ERR_UNSUPPORTED (no z-slab count fits: the counting kernels serve the grid)."""
    nx, ny, nz = (int(v) for v in n_xyz)
    p = (ctypes.c_int32 * 8)()
    rc = load().sn_voxel_occupancy_plan(nx, ny, nz, int(planes), int(B), int(fused), int(sized), int(pts_aligned16),
                                        int(labels_aligned16), int(ws_aligned16), int(want_flags), ctypes.cast(p, c_void_p))
    if rc == -2:
        return None
    _check(rc, "sn_voxel_occupancy_plan")
    return OccupancyPlan(*(int(v) for v in p))


@_on_tensor_device
def voxel_occupancy(pts, labels, offsets, desc, n_xyz, keep_labels: Sequence[float] = (), want_gt_occ: bool = False,
                    out_dtype: torch.dtype = torch.uint8, exact_fallback: bool = True):
    """LDS-bitmap occupancy (sn_voxel_occupancy): returns (occ, gt_occ | None, flags, dropped), grids [B,1,nz,nx,ny]."""
    B = offsets.numel() - 1
    nx, ny, nz = (int(v) for v in n_xyz)
    V = nx * ny * nz
    dev = pts.device
    planes = 2 if want_gt_occ else 1
    bits = torch.empty((B * SN_OCC_PARTS * (planes * (V // 32) + 1),), dtype=torch.int32, device=dev)
    occ = torch.empty((B, 1, nz, nx, ny), dtype=out_dtype, device=dev)
    gt_occ = torch.empty((B, 1, nz, nx, ny), dtype=out_dtype, device=dev) if want_gt_occ else None
    flags = torch.empty((B,), dtype=torch.int32, device=dev)
    dropped = torch.empty((B,), dtype=torch.int32, device=dev)
    counts = towers = None
    if exact_fallback:  # scratch for tiles whose flag is raised (gated launch: untouched otherwise)
        counts = torch.empty((B, V), dtype=torch.int32, device=dev)
        towers = torch.empty((B, V), dtype=torch.int32, device=dev) if want_gt_occ else None
    keep = (ctypes.c_double * max(1, len(keep_labels)))(*[float(k) for k in keep_labels])
    rc = load().sn_voxel_occupancy(_ptr(pts, torch.float64, "pts"),
                                   _ptr(labels, torch.float64, "labels") if want_gt_occ else None,
                                   _ptr(offsets, torch.int64, "offsets"), B, _ptr(desc, torch.float64, "desc"),
                                   nx, ny, nz, ctypes.cast(keep, c_void_p), len(keep_labels) if want_gt_occ else 0,
                                   _ptr(bits), _ptr(occ), _ptr(gt_occ), _DT_OUT[out_dtype], _ptr(flags), _ptr(dropped),
                                   _ptr(counts), _ptr(towers), _stream())
    _check(rc, "sn_voxel_occupancy")
    return occ, gt_occ, flags, dropped


@_on_tensor_device
def voxel_occupancy_fused(pts, labels, offsets, n_xyz, regular: bool = True, keep_labels: Sequence[float] = (),
                          want_gt_occ: bool = False, out_dtype: torch.dtype = torch.uint8, exact_fallback: bool = True,
                          want_bbox: bool = False, bank_rider=None, want_rows: bool = False):
    """sn_voxel_occupancy_fused: bbox + descriptor + LDS-bitmap occupancy in four launches.  Returns
    (occ, gt_occ | None, flags, dropped, desc, bbox | None).  bank_rider = (params [G, SN_NPARAM] f32, kinds [G] i32,
    bank [G,9,9,9] f32 out, prep uint8 out): K2 and the int8 contraction's preparation ride in the first launch
    (sn_voxel_occupancy_fused_bank) -- the two output buffers hold what sn_geneo_bank_prep would have written."""
    B = offsets.numel() - 1
    nx, ny, nz = (int(v) for v in n_xyz)
    V = nx * ny * nz
    dev = pts.device
    planes = 2 if want_gt_occ else 1
    partial = torch.empty((B, SN_BBOX_PARTS, 6), dtype=torch.float64, device=dev)
    desc = torch.empty((B, desc_len(nx, ny, nz)), dtype=torch.float64, device=dev)
    bbox = torch.empty((B, 6), dtype=torch.float64, device=dev) if want_bbox else None
    bits = torch.empty((B * SN_OCC_PARTS * (planes * (V // 32) + 1),), dtype=torch.int32, device=dev)
    occ = torch.empty((B, 1, nz, nx, ny), dtype=out_dtype, device=dev)
    gt_occ = torch.empty((B, 1, nz, nx, ny), dtype=out_dtype, device=dev) if want_gt_occ else None
    flags = torch.empty((B,), dtype=torch.int32, device=dev)
    dropped = torch.empty((B,), dtype=torch.int32, device=dev)
    counts = towers = None
    if exact_fallback:
        counts = torch.empty((B, V), dtype=torch.int32, device=dev)
        towers = torch.empty((B, V), dtype=torch.int32, device=dev) if want_gt_occ else None
    keep = (ctypes.c_double * max(1, len(keep_labels)))(*[float(k) for k in keep_labels])
    common = (_ptr(pts, torch.float64, "pts"), _ptr(labels, torch.float64, "labels") if want_gt_occ else None,
              _ptr(offsets, torch.int64, "offsets"), B, nx, ny, nz, int(regular), ctypes.cast(keep, c_void_p),
              len(keep_labels) if want_gt_occ else 0, _ptr(partial), _ptr(bbox), _ptr(desc), _ptr(bits), _ptr(occ),
              _ptr(gt_occ), _DT_OUT[out_dtype], _ptr(flags), _ptr(dropped), _ptr(counts), _ptr(towers))
    rows = torch.empty((B, nz, (nx + 31) // 32), dtype=torch.int32, device=dev) if want_rows else None
    if bank_rider is None:
        rc = load().sn_voxel_occupancy_fused_rows(*common, _stream(), _ptr(rows))
        _check(rc, "sn_voxel_occupancy_fused")
    else:
        _check(load().sn_voxel_occupancy_fused_bank_rows(*common, *_rider_args(bank_rider), _stream(), _ptr(rows)),
               "sn_voxel_occupancy_fused_bank")
    if want_rows:   # (want_rows: the occupancy's row bits int32 [B, nz, ceil(nx / 32)] ride on `occ`: attach_rows)
        attach_rows(occ, rows)
    return occ, gt_occ, flags, dropped, desc, bbox


def _rider_args(bank_rider):
    """bank_rider = (params [G, SN_NPARAM] f32, kinds [G] i32, bank [G,9,9,9] f32 out, prep uint8 out) or, with the effective
    coefficients riding too, (params, kinds, bank, prep, lambdas [G] f32 (refreshed in place), order [G] i32, last, lam_out [G]
    f32 out) -> the C argument tail of the sn_voxel_occupancy_*_bank entries"""
    params, kinds, bank, prep = bank_rider[:4]
    lambdas, order, last, lam_out = bank_rider[4:] if len(bank_rider) > 4 else (None, None, 0, None)
    G = params.shape[0]
    if tuple(bank.shape) != (G, 9, 9, 9) or prep.numel() < SN_CONV_PREP_BYTES * ((G + 15) // 16):
        raise HipLibraryError("bank_rider: bank must be [G,9,9,9] f32 and prep SN_CONV_PREP_BYTES x ceil(G / 16) bytes")
    return (_ptr(params, torch.float32, "params"), _ptr(kinds, torch.int32, "kinds"), G, 9, 9, 9,
            _ptr(bank, torch.float32, "bank"), None, _ptr(lambdas, torch.float32, "lambdas"),
            _ptr(order, torch.int32, "order"), int(last), _ptr(lam_out, torch.float32, "lam_out"),
            _ptr(prep, torch.uint8, "prep"))


@_on_tensor_device
def voxel_occupancy_sized(pts, labels, offsets, size_xyz: Sequence[float], n_xyz_max, keep_labels: Sequence[float] = (),
                          want_gt_occ: bool = False, out_dtype: torch.dtype = torch.uint8, exact_fallback: bool = True,
                          bank_rider=None):
    """sn_voxel_occupancy_sized: voxel-size mode on the LDS-bitmap kernels.  Returns
    (occ, gt_occ | None, flags, dropped, desc, dims [B,3], status [B], bbox [B,6])."""
    B = offsets.numel() - 1
    nx, ny, nz = (int(v) for v in n_xyz_max)
    V = nx * ny * nz
    dev = pts.device
    planes = 2 if want_gt_occ else 1
    partial = torch.empty((B, SN_BBOX_PARTS, 6), dtype=torch.float64, device=dev)
    desc = torch.empty((B, desc_len(nx, ny, nz)), dtype=torch.float64, device=dev)
    bbox = torch.empty((B, 6), dtype=torch.float64, device=dev)
    dims = torch.empty((B, 3), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    bits = torch.empty((B * SN_OCC_PARTS * (planes * (V // 32) + 1),), dtype=torch.int32, device=dev)
    occ = torch.empty((B, 1, nz, nx, ny), dtype=out_dtype, device=dev)
    gt_occ = torch.empty((B, 1, nz, nx, ny), dtype=out_dtype, device=dev) if want_gt_occ else None
    flags = torch.empty((B,), dtype=torch.int32, device=dev)
    dropped = torch.empty((B,), dtype=torch.int32, device=dev)
    counts = towers = None
    if exact_fallback:
        counts = torch.empty((B, V), dtype=torch.int32, device=dev)
        towers = torch.empty((B, V), dtype=torch.int32, device=dev) if want_gt_occ else None
    keep = (ctypes.c_double * max(1, len(keep_labels)))(*[float(k) for k in keep_labels])
    size = (ctypes.c_double * 3)(*[float(v) for v in size_xyz])
    common = (_ptr(pts, torch.float64, "pts"), _ptr(labels, torch.float64, "labels") if want_gt_occ else None,
              _ptr(offsets, torch.int64, "offsets"), B, ctypes.cast(size, c_void_p), nx, ny, nz,
              ctypes.cast(keep, c_void_p), len(keep_labels) if want_gt_occ else 0, _ptr(partial), _ptr(bbox), _ptr(desc),
              _ptr(dims), _ptr(status), _ptr(bits), _ptr(occ), _ptr(gt_occ), _DT_OUT[out_dtype], _ptr(flags),
              _ptr(dropped), _ptr(counts), _ptr(towers))
    if bank_rider is None:
        _check(load().sn_voxel_occupancy_sized(*common, _stream()), "sn_voxel_occupancy_sized")
    else:   # (as voxel_occupancy_fused: K2 + the preparation ride in the first launch)
        _check(load().sn_voxel_occupancy_sized_bank(*common, *_rider_args(bank_rider), _stream()),
               "sn_voxel_occupancy_sized_bank")
    return occ, gt_occ, flags, dropped, desc, dims, status, bbox


@_on_tensor_device
def gather_points(grid: torch.Tensor, pts: torch.Tensor, offsets: torch.Tensor, desc: torch.Tensor,
                  fill: float = 0.0) -> torch.Tensor:
    """grid [B,C,nz,nx,ny] (f32|f64) -> per-point values [C, total] via the scatter's binning (sn_gather_points).
    pts must hold exactly the batch's offsets[B] points: the kernel strides the channels of `out` by offsets[B] (a device
    value), this wrapper allocates them pts.shape[0] apart."""
    if grid.dim() != 5 or grid.dtype not in (torch.float32, torch.float64):
        raise HipLibraryError("grid must be [B,C,nz,nx,ny] float32/float64")
    B, C, nz, nx, ny = grid.shape
    # host-side shape checks, no synchronisation: the kernel reads desc[b * desc_len + ..] and offsets[0..B] unchecked
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise HipLibraryError(f"pts must be [N,3] (got {tuple(pts.shape)})")
    if offsets.numel() != B + 1:
        raise HipLibraryError(f"offsets must have B + 1 = {B + 1} entries for a grid of {B} tiles (got {offsets.numel()})")
    if tuple(desc.shape) != (B, desc_len(nx, ny, nz)):
        raise HipLibraryError(f"desc must be [B, desc_len(nx, ny, nz)] = [{B}, {desc_len(nx, ny, nz)}] "
                              f"(got {tuple(desc.shape)})")
    out = torch.empty((C, pts.shape[0]), dtype=grid.dtype, device=grid.device)
    rc = load().sn_gather_points(_ptr(grid, None, "grid"), _DT[grid.dtype], C, _ptr(pts, torch.float64, "pts"),
                                 _ptr(offsets, torch.int64, "offsets"), B, _ptr(desc, torch.float64, "desc"),
                                 nx, ny, nz, float(fill), _ptr(out), _stream())
    _check(rc, "sn_gather_points")
    return out


@_on_tensor_device
def grid_to_points(grid: torch.Tensor, origin=None, voxel_size=None) -> torch.Tensor:
    """grid [n0,n1,n2] (f32|f64|u8|bool) -> rows [n0*n1*n2, 4] f64 = (origin + index * voxel_size, value), C order of
    the indices (sn_grid_to_points; utils/voxelization.py:328-360)."""
    if grid.dim() != 3 or grid.dtype not in _DT:
        raise HipLibraryError("grid must be [n0,n1,n2] float32/float64/uint8/bool")
    n0, n1, n2 = grid.shape

    def host3(v, name):
        if v is None:
            return None, None
        a = (ctypes.c_double * 3)(*[float(t) for t in v])
        if len(v) != 3:
            raise HipLibraryError(f"{name} must have 3 entries")
        return a, ctypes.cast(a, ctypes.c_void_p)

    o_keep, o_ptr = host3(origin, "origin")
    s_keep, s_ptr = host3(voxel_size, "voxel_size")
    out = torch.empty((n0 * n1 * n2, 4), dtype=torch.float64, device=grid.device)
    rc = load().sn_grid_to_points(_ptr(grid, None, "grid"), _DT[grid.dtype], n0, n1, n2, o_ptr, s_ptr, _ptr(out),
                                  _stream())
    _check(rc, "sn_grid_to_points")
    return out


@_on_tensor_device
def conv_corr(x: torch.Tensor, gout: torch.Tensor, out: Optional[torch.Tensor], kernel_size: Sequence[int]):
    """C [kz,kx,ky] f32 = sum_{b,v} delta[b,v] x[b, v+t-p]  (sn_conv_corr_ws: bool input as the gather over the set
    voxels, anything else as the GEMM); gout/out [B,1,Z,X,Y] both f32 or both bf16 (bf16 activation storage: the products
    are formed and summed in fp32 either way)."""
    B, _, Z, X, Y = x.shape
    kz, kx, ky = (int(k) for k in kernel_size)
    if gout.dtype not in (torch.float32, torch.bfloat16):
        raise HipLibraryError(f"gout must be float32 or bfloat16 (got {gout.dtype})")
    if out is not None and out.dtype != gout.dtype:
        raise HipLibraryError(f"out ({out.dtype}) and gout ({gout.dtype}) must have the same dtype")
    nbytes = int(load().sn_conv_corr_ws_bytes(_DT[x.dtype], B, Z, X, Y, kz, kx, ky))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)   # (torch's allocator: 512-byte aligned)
    C = torch.empty((kz, kx, ky), dtype=torch.float32, device=x.device)
    rc = load().sn_conv_corr_ws(_ptr(x, None, "x"), _DT[x.dtype], _ptr(gout, None, "gout"), _ptr(out, None, "out"),
                                _DT[gout.dtype], B, Z, X, Y, kz, kx, ky, _ptr(ws), nbytes, _ptr(C), _stream())
    _check(rc, "sn_conv_corr_ws")
    return C


class CorrPlan(NamedTuple):
    """sn_conv_corr_plan's eight words (include/scenenet_hip.h)."""
    kernel: str          # "taps" (thread per tap) | "gemm" (K4) | "gather" (K4s)
    rows: int            # input rows per job
    row_tiles: int       # row tiles per plane
    jobs: int
    workgroups: int
    kzmax: int           # 9 | 16 (0: thread per tap)
    lds_bytes: int
    vec: bool            # Y admits the four-element staging loads
    list_vec: bool       # the list kernel's 8-byte loads
    every_step: bool     # K4 runs every K step of a non-empty row
    multi_group: bool    # the gather has more than one group


CORR_PLAN_KERNELS = ("taps", "gemm", "gather")


def conv_corr_plan(x, kernel_size: Sequence[int], g_dtype: torch.dtype = torch.float32) -> CorrPlan:
    """What conv_corr(x, gout, out, kernel_size) would launch under the options in force (sn_conv_corr_plan: host only, no
    launch, no device needed).  x: a [B,1,Z,X,Y] tensor on any device, or (dtype, shape); g_dtype: float32 | bfloat16."""
    dtype, shape = (x.dtype, tuple(x.shape)) if isinstance(x, torch.Tensor) else (x[0], tuple(x[1]))
    if len(shape) != 5 or shape[1] != 1:
        raise HipLibraryError(f"x must be [B,1,Z,X,Y] (got {shape})")
    if dtype not in _DT or dtype == torch.bfloat16:
        raise HipLibraryError(f"x dtype {dtype} unsupported (f32, f64, u8, bool)")
    if g_dtype not in (torch.float32, torch.bfloat16):
        raise HipLibraryError(f"g_dtype must be float32 or bfloat16 (got {g_dtype})")
    B, _, Z, X, Y = (int(v) for v in shape)
    kz, kx, ky = (int(k) for k in kernel_size)
    p = (ctypes.c_int32 * 8)()
    _check(load().sn_conv_corr_plan(_DT[dtype], _DT[g_dtype], B, Z, X, Y, kz, kx, ky, ctypes.cast(p, c_void_p)),
           "sn_conv_corr_plan")
    return CorrPlan(CORR_PLAN_KERNELS[p[0]], int(p[1]), int(p[2]), int(p[3]), int(p[4]), int(p[5]), int(p[6]),
                    bool(p[7] & 1), bool(p[7] & 2), bool(p[7] & 4), bool(p[7] & 8))


@_on_tensor_device
def geneo_bank_bwd(params: torch.Tensor, kinds: torch.Tensor, kernel_size: Sequence[int], dW: torch.Tensor):
    """dparams [G, SN_NPARAM] f32 from dW [G,kz,kx,ky] f32 (sn_geneo_bank_bwd)."""
    G = params.shape[0]
    kz, kx, ky = (int(k) for k in kernel_size)
    dparams = torch.empty((G, SN_NPARAM), dtype=torch.float32, device=params.device)
    rc = load().sn_geneo_bank_bwd(_ptr(params, torch.float32, "params"), _ptr(kinds, torch.int32, "kinds"), G, kz, kx,
                                  ky, _ptr(dW, torch.float32, "dW"), _ptr(dparams), _stream())
    _check(rc, "sn_geneo_bank_bwd")
    return dparams


@_on_tensor_device
def geneo_backward(params: torch.Tensor, kinds: torch.Tensor, kernel_size: Sequence[int], bank: torch.Tensor,
                   lambdas: torch.Tensor, corr: torch.Tensor, last: int, out: torch.Tensor) -> torch.Tensor:
    """sn_geneo_backward: writes out[: G*SN_NPARAM] (dparams) and out[G*SN_NPARAM :] (dlambdas) of the packed gradient
    vector in one launch, from the correlation `corr` [kz,kx,ky]."""
    G = params.shape[0]
    kz, kx, ky = (int(k) for k in kernel_size)
    n = G * SN_NPARAM
    if out.numel() != n + G or out.dtype != torch.float32:
        raise HipLibraryError("packed gradient must be f32 [G*SN_NPARAM + G]")
    base = _ptr(out, torch.float32, "out")
    rc = load().sn_geneo_backward(_ptr(params, torch.float32, "params"), _ptr(kinds, torch.int32, "kinds"), G, kz, kx,
                                  ky, _ptr(bank, torch.float32, "bank"), _ptr(lambdas, torch.float32, "lambdas"),
                                  _ptr(corr, torch.float32, "corr"), int(last), base, base + 4 * n, _stream())
    _check(rc, "sn_geneo_backward")
    return out


@_on_tensor_device
def effective_lambdas(lambdas: torch.Tensor, order: torch.Tensor, last: int) -> torch.Tensor:
    """sn_effective_lambdas: [G] f32 effective coefficients; `lambdas[last]` is refreshed in place."""
    G = int(lambdas.numel())
    out = torch.empty((G,), dtype=torch.float32, device=lambdas.device)
    rc = load().sn_effective_lambdas(_ptr(lambdas, torch.float32, "lambdas"), _ptr(order, torch.int32, "order"), G,
                                     int(last), _ptr(out), _stream())
    _check(rc, "sn_effective_lambdas")
    return out


# --------------------------------------------------------------------------- #
def loss_parts(n_per: int) -> int:
    """SN_LOSS_PARTS of include/scenenet_hip.h."""
    return 1 if n_per <= 16384 else min(256, (n_per + 16383) // 16384)


@_on_tensor_device
def loss_forward(pred: torch.Tensor, gt: torch.Tensor, ranges: torch.Tensor, bin_w: torch.Tensor, terms: int,
                 mse_weight: float = 1.0, tversky_alpha: float = 0.5, tversky_beta: float = 1.0,
                 focal_gamma: float = 1.0, tversky_smooth: float = 1.0, dice_smooth: float = 1.0):
    """sn_loss_forward_m on pred/gt [B, ...] (same shape).  Returns (loss [5] f64 = {total, wmse, focal tversky, dice,
    weighted bce}, stats [B, 3H+5] f64, coef f64 for loss_backward, loss32 [5] f32 = the same five rounded once)."""
    if pred.shape != gt.shape:
        raise HipLibraryError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must have the same shape")
    B = int(pred.shape[0])
    n_per = pred.numel() // max(B, 1)
    H = int(ranges.numel())
    dev = pred.device
    ws = torch.empty((B * loss_parts(n_per) * (3 * H + 5),), dtype=torch.float64, device=dev)
    stats = torch.empty((B, 3 * H + 5), dtype=torch.float64, device=dev)
    loss = torch.empty((5,), dtype=torch.float64, device=dev)
    loss32 = torch.empty((5,), dtype=torch.float32, device=dev)
    coef = torch.empty((2 * SN_LOSS_MAX_BINS + 3 * B,), dtype=torch.float64, device=dev)
    rc = load().sn_loss_forward_m(_ptr(pred, None, "pred"), _DT[pred.dtype], _ptr(gt, None, "gt"), _DT[gt.dtype], B,
                                  n_per, _ptr(ranges, torch.float32, "ranges"), _ptr(bin_w, torch.float32, "bin_w"), H,
                                  int(terms), float(mse_weight), float(tversky_alpha), float(tversky_beta),
                                  float(focal_gamma), float(tversky_smooth), float(dice_smooth), _ptr(ws), _ptr(stats),
                                  _ptr(loss), _ptr(loss32), _ptr(coef), _stream())
    _check(rc, "sn_loss_forward")
    return loss, stats, coef, loss32


@_on_tensor_device
def criterion_forward(pred: torch.Tensor, gt: torch.Tensor, ranges: torch.Tensor, bin_w: torch.Tensor, terms: int,
                      P: torch.Tensor, mask: torch.Tensor, weight: float, with_sum: bool, mse_weight: float = 1.0,
                      tversky_alpha: float = 0.5, tversky_beta: float = 1.0, focal_gamma: float = 1.0,
                      tversky_smooth: float = 1.0, dice_smooth: float = 1.0):
    """sn_criterion_forward: the dense terms of loss_forward and the penalties of param_penalty over the packed parameters
    P in the dense loss's two launches.  Returns (total [1] f32 = float(dense) + penalty, stats, coef, pen_grad [N] f32)."""
    if pred.shape != gt.shape:
        raise HipLibraryError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must have the same shape")
    B = int(pred.shape[0])
    n_per = pred.numel() // max(B, 1)
    H = int(ranges.numel())
    N = int(P.numel())
    dev = pred.device
    ws = torch.empty((B * loss_parts(n_per) * (3 * H + 5),), dtype=torch.float64, device=dev)
    stats = torch.empty((B, 3 * H + 5), dtype=torch.float64, device=dev)
    loss = torch.empty((5,), dtype=torch.float64, device=dev)
    coef = torch.empty((2 * SN_LOSS_MAX_BINS + 3 * B,), dtype=torch.float64, device=dev)
    f32 = torch.empty((7 + N,), dtype=torch.float32, device=dev)   # loss32 [5] | total [1] | penalty [1] | its gradient [N]
    base = f32.data_ptr()
    rc = load().sn_criterion_forward(_ptr(pred, None, "pred"), _DT[pred.dtype], _ptr(gt, None, "gt"), _DT[gt.dtype], B,
                                     n_per, _ptr(ranges, torch.float32, "ranges"), _ptr(bin_w, torch.float32, "bin_w"),
                                     H, int(terms), float(mse_weight), float(tversky_alpha), float(tversky_beta),
                                     float(focal_gamma), float(tversky_smooth), float(dice_smooth), _ptr(ws), _ptr(stats),
                                     _ptr(loss), base, _ptr(coef), _ptr(P, torch.float32, "P"),
                                     _ptr(mask, torch.int8, "mask"), N, float(weight), int(bool(with_sum)), base + 24,
                                     base + 28, base + 20, _stream())
    _check(rc, "sn_criterion_forward")
    return f32[5:6], stats, coef, f32[7:]


@_on_tensor_device
def criterion_backward(pred: torch.Tensor, gt: torch.Tensor, ranges: torch.Tensor, coef: torch.Tensor,
                       upstream: torch.Tensor, pen_grad: torch.Tensor):
    """sn_criterion_backward: (dL/dpred, penalty gradient x upstream [N] f32) in the gradient pass's one launch."""
    B = int(pred.shape[0])
    n_per = pred.numel() // max(B, 1)
    grad = torch.empty_like(pred)
    N = int(pen_grad.numel())
    pen_out = torch.empty((N,), dtype=torch.float32, device=pred.device)
    if upstream.dtype not in (torch.float64, torch.float32):
        upstream = upstream.to(torch.float64)
    rc = load().sn_criterion_backward(_ptr(pred, None, "pred"), _DT[pred.dtype], _ptr(gt, None, "gt"), _DT[gt.dtype], B,
                                      n_per, _ptr(ranges, torch.float32, "ranges"), int(ranges.numel()),
                                      _ptr(coef, torch.float64, "coef"), _ptr(upstream, None, "upstream"),
                                      _DT[upstream.dtype], _ptr(grad), _ptr(pen_grad, torch.float32, "pen_grad"), N,
                                      _ptr(pen_out), _stream())
    _check(rc, "sn_criterion_backward")
    return grad, pen_out


@_on_tensor_device
def loss_backward(pred: torch.Tensor, gt: torch.Tensor, ranges: torch.Tensor, coef: torch.Tensor,
                  upstream: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dL/dpred (pred's dtype and shape) from the coefficients of loss_forward (sn_loss_backward_u); upstream: a
    one-element f64 or f32 tensor (or None = 1); out: a contiguous tensor like pred to write into (default: a new one)."""
    B = int(pred.shape[0])
    n_per = pred.numel() // max(B, 1)
    if out is None:
        grad = torch.empty_like(pred)
    else:
        if out.shape != pred.shape or out.dtype != pred.dtype or out.device != pred.device or not out.is_contiguous():
            raise HipLibraryError("loss_backward: out must be contiguous with pred's shape, dtype and device")
        grad = out
    if upstream is not None and upstream.dtype not in (torch.float64, torch.float32):
        upstream = upstream.to(torch.float64)
    up_dt = _DT[upstream.dtype] if upstream is not None else SN_F64
    rc = load().sn_loss_backward_u(_ptr(pred, None, "pred"), _DT[pred.dtype], _ptr(gt, None, "gt"), _DT[gt.dtype], B,
                                   n_per, _ptr(ranges, torch.float32, "ranges"), int(ranges.numel()),
                                   _ptr(coef, torch.float64, "coef"), _ptr(upstream, None, "upstream"), up_dt,
                                   _ptr(grad), _stream())
    _check(rc, "sn_loss_backward")
    return grad


@_on_tensor_device
def param_penalty(P: torch.Tensor, mask: torch.Tensor, weight: float, with_sum: bool):
    """sn_param_penalty: (value [1] f32, grad [N] f32) of the GENEO_Loss penalties over the packed parameters."""
    N = int(P.numel())
    value = torch.empty((1,), dtype=torch.float32, device=P.device)
    grad = torch.empty((N,), dtype=torch.float32, device=P.device)
    rc = load().sn_param_penalty(_ptr(P, torch.float32, "P"), _ptr(mask, torch.int8, "mask"), N, float(weight),
                                 int(bool(with_sum)), _ptr(value), _ptr(grad), _stream())
    _check(rc, "sn_param_penalty")
    return value, grad


# --------------------------------------------------------------------------- #
def quantile_parts(n_per: int) -> Tuple[int, int]:
    """(SN_QUANTILE_PARTS, SN_QUANTILE_BWD_PARTS) of include/scenenet_hip.h."""
    fwd = 1 if n_per <= 16384 else min(256, (n_per + 16383) // 16384)
    bwd = 1 if n_per <= 8192 else min(512, (n_per + 8191) // 8192)
    return fwd, bwd


def _quantile_head(pred, gt, qs):
    if pred.dim() < 2:
        raise HipLibraryError(f"pred {tuple(pred.shape)} must be [B, Q, ...]")
    B, Q = int(pred.shape[0]), int(pred.shape[1])
    n_per = pred.numel() // max(B * Q, 1)
    if gt.numel() != B * n_per or int(gt.shape[0]) != B:
        raise HipLibraryError(f"gt {tuple(gt.shape)} must hold one value per voxel of pred {tuple(pred.shape)}: [B, ...]")
    if len(qs) != Q:
        raise HipLibraryError(f"pred has {Q} channels for {len(qs)} quantiles")
    return B, Q, n_per, (ctypes.c_float * max(Q, 1))(*[float(q) for q in qs])


@_on_tensor_device
def quantile_forward(pred: torch.Tensor, gt: torch.Tensor, qs: Sequence[float], ranges: torch.Tensor, bin_w: torch.Tensor):
    """sn_quantile_forward on pred [B, Q, ...] and gt [B, ...] (one value per voxel).  Returns (loss [1 + Q] f64 = {total,
    each quantile's share}, loss32 [1 + Q] f32 = the same rounded once, stats [B, Q + H] f64, coef [H] f64)."""
    B, Q, n_per, qs_c = _quantile_head(pred, gt, qs)
    H = int(ranges.numel())
    dev = pred.device
    ws = torch.empty((B * quantile_parts(n_per)[0] * (Q + H),), dtype=torch.float64, device=dev)
    stats = torch.empty((B, Q + H), dtype=torch.float64, device=dev)
    loss = torch.empty((1 + Q,), dtype=torch.float64, device=dev)
    loss32 = torch.empty((1 + Q,), dtype=torch.float32, device=dev)
    coef = torch.empty((H,), dtype=torch.float64, device=dev)
    rc = load().sn_quantile_forward(_ptr(pred, None, "pred"), _DT[pred.dtype], _ptr(gt, None, "gt"), _DT[gt.dtype], B, Q,
                                    n_per, ctypes.cast(qs_c, c_void_p), _ptr(ranges, torch.float32, "ranges"),
                                    _ptr(bin_w, torch.float32, "bin_w"), H, _ptr(ws), _ptr(stats), _ptr(loss),
                                    _ptr(loss32), _ptr(coef), _stream())
    _check(rc, "sn_quantile_forward")
    return loss, loss32, stats, coef


@_on_tensor_device
def quantile_backward(pred: torch.Tensor, gt: torch.Tensor, qs: Sequence[float], ranges: torch.Tensor, coef: torch.Tensor,
                      upstream: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dL/dpred (pred's dtype and shape) from the coefficients of quantile_forward (sn_quantile_backward); upstream: a
    one-element f64 or f32 tensor (or None = 1)."""
    B, Q, n_per, qs_c = _quantile_head(pred, gt, qs)
    grad = torch.empty_like(pred)
    if upstream is not None and upstream.dtype not in (torch.float64, torch.float32):
        upstream = upstream.to(torch.float64)
    up_dt = _DT[upstream.dtype] if upstream is not None else SN_F64
    rc = load().sn_quantile_backward(_ptr(pred, None, "pred"), _DT[pred.dtype], _ptr(gt, None, "gt"), _DT[gt.dtype], B, Q,
                                     n_per, ctypes.cast(qs_c, c_void_p), _ptr(ranges, torch.float32, "ranges"),
                                     int(ranges.numel()), _ptr(coef, torch.float64, "coef"),
                                     _ptr(upstream, None, "upstream"), up_dt, _ptr(grad), _stream())
    _check(rc, "sn_quantile_backward")
    return grad


# --------------------------------------------------------------------------- #
# sn_binary_stats only: int32 labels (`y.to(torch.int)` at the reference's call site) are a target dtype of this entry and
# of no other, so the mapping lives here and not in _DT (every other wrapper keeps refusing int32 in Python)
_METRIC_PRED_DT = {torch.float32: SN_F32, torch.bfloat16: SN_BF16, torch.float64: SN_F64}
_METRIC_TGT_DT = {torch.float32: SN_F32, torch.float64: SN_F64, torch.bfloat16: SN_BF16, torch.uint8: SN_U8,
                  torch.bool: SN_OCC8, torch.int32: SN_I32}


@_on_tensor_device
def binary_stats(pred: torch.Tensor, target: torch.Tensor, tau: float, beta: float, ws: torch.Tensor,
                 state: torch.Tensor, batch: Optional[torch.Tensor] = None,
                 values: Optional[torch.Tensor] = None) -> None:
    """sn_binary_stats over pred / target flattened (same numel): adds this call's (tp, fp, fn, tn, bad_pred, bad_target)
    to `state` [6] int64; `batch` [6] int64 (optional) receives them; `values` [10] f32 (optional) receives this call's
    (JaccardIndex, Precision, Recall, F1Score, FBetaScore), then the accumulated state's.  ws: int64 scratch of
    SN_METRIC_WS_BYTES.  Two launches on the current stream, no synchronisation."""
    if pred.numel() != target.numel():
        raise ValueError(f"pred ({pred.numel()} elements) and target ({target.numel()} elements) must have the same size")
    if pred.dtype not in _METRIC_PRED_DT:
        raise HipLibraryError(f"pred must be float32, bfloat16 or float64 (got {pred.dtype})")
    if target.dtype not in _METRIC_TGT_DT:
        raise HipLibraryError(f"target must be float32, float64, bfloat16, uint8, bool or int32 (got {target.dtype})")
    if ws.numel() * ws.element_size() < SN_METRIC_WS_BYTES:
        raise HipLibraryError(f"ws must hold {SN_METRIC_WS_BYTES} bytes")
    rc = load().sn_binary_stats(_ptr(pred, None, "pred"), _METRIC_PRED_DT[pred.dtype], _ptr(target, None, "target"),
                                _METRIC_TGT_DT[target.dtype], int(pred.numel()), float(tau), float(beta), _ptr(ws, None, "ws"),
                                _ptr(state, torch.int64, "state"), _ptr(batch, torch.int64, "batch"),
                                _ptr(values, torch.float32, "values"), _stream())
    _check(rc, "sn_binary_stats")


def curve_record(T: int) -> int:
    """SN_CURVE_RECORD(T): int64 words of one segment's record -- hist[2][T + 1], bad_pred, bad_target."""
    return 2 * (int(T) + 1) + 2


def curve_ws_bytes(n: int, segments: int, T: int) -> int:
    """sn_binary_curve_ws_bytes: scratch bytes of one binary_curve call over `segments` x `n` elements (host only)."""
    need = int(load().sn_binary_curve_ws_bytes(int(n), int(segments), int(T)))
    if need == 0:
        raise HipLibraryError(f"sn_binary_curve serves no call of {segments} segment(s) x {n} elements at {T} thresholds "
                              f"(n > 0, 1 <= segments <= 2^20, segments * n <= 2^40, 1 <= T <= {SN_CURVE_MAX_THRESHOLDS})")
    return need


@_on_tensor_device
def binary_curve(pred: torch.Tensor, target: torch.Tensor, thresholds, ws: torch.Tensor, state: torch.Tensor,
                 segments: int = 1, batch: Optional[torch.Tensor] = None) -> None:
    """sn_binary_curve over pred / target flattened (same numel, `segments` equal parts): adds each segment's record --
    hist[2][T + 1] (bin = number of thresholds the prediction clears; target negative, then positive), bad_pred,
    bad_target -- to `state` [segments, curve_record(T)] int64; `batch` (optional, same shape) receives this call's.
    thresholds: T floats, or a ctypes array of c_double built once.  ws: scratch of curve_ws_bytes(n, segments, T).
    Two launches on the current stream, no synchronisation."""
    if pred.numel() != target.numel():
        raise ValueError(f"pred ({pred.numel()} elements) and target ({target.numel()} elements) must have the same size")
    segments = int(segments)
    if segments < 1 or pred.numel() % segments:
        raise ValueError(f"{pred.numel()} elements do not split into {segments} equal segments")
    if pred.dtype not in _METRIC_PRED_DT:
        raise HipLibraryError(f"pred must be float32, bfloat16 or float64 (got {pred.dtype})")
    if target.dtype not in _METRIC_TGT_DT:
        raise HipLibraryError(f"target must be float32, float64, bfloat16, uint8, bool or int32 (got {target.dtype})")
    thr = thresholds if isinstance(thresholds, ctypes.Array) else (ctypes.c_double * len(thresholds))(
        *[float(v) for v in thresholds])
    T = len(thr)
    words = segments * curve_record(T)
    if state.numel() != words or (batch is not None and batch.numel() != words):
        raise HipLibraryError(f"state / batch must hold {segments} x {curve_record(T)} int64 words")
    rc = load().sn_binary_curve(_ptr(pred, None, "pred"), _METRIC_PRED_DT[pred.dtype], _ptr(target, None, "target"),
                                _METRIC_TGT_DT[target.dtype], pred.numel() // segments, segments, thr, T,
                                _ptr(ws, None, "ws"), ws.numel() * ws.element_size(), _ptr(state, torch.int64, "state"),
                                _ptr(batch, torch.int64, "batch"), _stream())
    _check(rc, "sn_binary_curve")


# --------------------------------------------------------------------------- #
@_on_tensor_device
def tiles_unpack(rows: torch.Tensor, pts: torch.Tensor, labels: Optional[torch.Tensor] = None,
                 offsets: Optional[torch.Tensor] = None, bad: Optional[torch.Tensor] = None) -> None:
    """sn_tiles_unpack: rows [total, cols] (f64 | f32, the raw rows of the batch's tiles, concatenated) -> pts[:total]
    (columns 0..2) and labels[:total] (the last column), both f64 and written in place: pts holds at least total x 3
    and labels at least total elements, and nothing beyond `total` is touched.  bad [B] i32 (with offsets [B+1] i64) is
    overwritten with every tile's count of points that carry a non-finite value in a column that is read.  Allocates
    nothing and does not synchronise."""
    if rows.dim() != 2:
        raise HipLibraryError(f"rows must be [total, cols] (got {tuple(rows.shape)})")
    if rows.dtype not in (torch.float64, torch.float32):
        raise HipLibraryError(f"rows must be float64 or float32 (got {rows.dtype})")
    total, cols = int(rows.shape[0]), int(rows.shape[1])
    if pts.numel() < 3 * total or (labels is not None and labels.numel() < total):
        raise HipLibraryError("pts / labels are smaller than the rows they are to hold")
    B = 1
    if offsets is not None:
        B = int(offsets.numel()) - 1
        if bad is not None and bad.numel() < B:
            raise HipLibraryError("bad must hold one count per tile")
    rc = load().sn_tiles_unpack(_ptr(rows, None, "rows"), _DT[rows.dtype], cols, total,
                                _ptr(offsets, torch.int64, "offsets"), B, _ptr(pts, torch.float64, "pts"),
                                _ptr(labels, torch.float64, "labels"), _ptr(bad, torch.int32, "bad"), _stream())
    _check(rc, "sn_tiles_unpack")


# --------------------------------------------------------------------------- #
_TOWER_DT = {torch.float32: SN_F32, torch.bfloat16: SN_BF16, torch.float64: SN_F64, torch.uint8: SN_U8, torch.bool: SN_OCC8}


def _voxel_size_c(voxel_size):
    if voxel_size is None:
        return None
    vs = [float(v) for v in voxel_size]
    if len(vs) != 3:
        raise ValueError("voxel_size must have 3 entries, one per grid axis")
    return (ctypes.c_double * 3)(*vs)


def towers_stencil(eps: float, voxel_size=None):
    """sn_towers_stencil (host only): (rows [R, 3] int32 = d0, d1, half-width along axis 2; number of offsets)."""
    vs = _voxel_size_c(voxel_size)
    cap = (2 * SN_TOWER_MAX_RADIUS + 1) ** 2
    rows = (ctypes.c_int32 * (3 * cap))()
    n = ctypes.c_int64(0)
    rc = load().sn_towers_stencil(float(eps), ctypes.cast(vs, c_void_p) if vs is not None else None,
                                  ctypes.cast(rows, c_void_p), cap, ctypes.cast(ctypes.pointer(n), c_void_p))
    if rc < 0:
        _check(rc, "sn_towers_stencil")
    return torch.tensor(list(rows[:3 * rc]), dtype=torch.int32).reshape(rc, 3), int(n.value)


def towers_ws_bytes(B: int, n0: int, n1: int, n2: int) -> int:
    """sn_towers_ws_bytes: scratch bytes of one tower_proposals call (host only)."""
    need = int(load().sn_towers_ws_bytes(int(B), int(n0), int(n1), int(n2)))
    if need == 0:
        raise HipLibraryError(f"sn_tower_proposals serves no grid of {B} x ({n0}, {n1}, {n2}) (positive extents, at most "
                              "2^24 voxels per tile with rows padded to 64)")
    return need


@_on_tensor_device
def tower_proposals(grid: torch.Tensor, tau: float, eps: float, min_points: int, max_towers: int, ws: torch.Tensor,
                    labels: torch.Tensor, n_towers: torch.Tensor, stats: Optional[torch.Tensor], voxel_size=None,
                    launches: Optional[Tuple[int, int]] = None) -> None:
    """sn_tower_proposals over grid [B, n0, n1, n2] (f32 | bf16 | f64 | u8 | bool): labels [B, n0, n1, n2] i32, n_towers
    [B] i32, stats [B, max_towers, SN_TOWER_NSTAT] i64, all caller-owned like the scratch `ws`
    (towers_ws_bytes).  voxel_size: 3 floats or a ctypes array built once.  launches = (first, last): only those of the
    SN_TOWER_LAUNCHES launches (sn_tower_proposals_launches: timing).  No allocation, no synchronisation."""
    if grid.dim() != 4:
        raise HipLibraryError(f"grid must be [B, n0, n1, n2] (got {tuple(grid.shape)})")
    if grid.dtype not in _TOWER_DT:
        raise HipLibraryError(f"grid must be float32, bfloat16, float64, uint8 or bool (got {grid.dtype})")
    B, n0, n1, n2 = (int(v) for v in grid.shape)
    max_towers = int(max_towers)
    if labels.numel() != grid.numel() or n_towers.numel() != B or \
            (stats is not None and stats.numel() != B * max_towers * SN_TOWER_NSTAT):
        raise HipLibraryError("labels / n_towers / stats do not have the sizes of this grid and max_towers")
    vs = voxel_size if isinstance(voxel_size, ctypes.Array) else _voxel_size_c(voxel_size)
    head = (_ptr(grid, None, "grid"), _TOWER_DT[grid.dtype], B, n0, n1, n2, float(tau), float(eps),
            ctypes.cast(vs, c_void_p) if vs is not None else None, int(min_points), max_towers, _ptr(ws, None, "ws"),
            ws.numel() * ws.element_size(), _ptr(labels, torch.int32, "labels"), _ptr(n_towers, torch.int32, "n_towers"),
            _ptr(stats, torch.int64, "stats"))
    if launches is None:
        rc = load().sn_tower_proposals(*head, _stream())
    else:
        rc = load().sn_tower_proposals_launches(*head, int(launches[0]), int(launches[1]), _stream())
    _check(rc, "sn_tower_proposals")


def _double3_c(v, name):
    if v is None or isinstance(v, ctypes.Array):
        return v
    vals = [float(x) for x in v]
    if len(vals) != 3:
        raise ValueError(f"{name} must have 3 entries, one per grid axis")
    return (ctypes.c_double * 3)(*vals)


@_on_tensor_device
def tower_centroids(stats: torch.Tensor, n_towers: torch.Tensor, height_axis: int, center, apply_filter: bool,
                    threshold: float, tower_height: float, rim_sq: float, min_euc: float, keep: torch.Tensor,
                    planar: Optional[torch.Tensor], agg: torch.Tensor, n_agg: torch.Tensor, status: torch.Tensor,
                    voxel_size=None) -> None:
    """sn_tower_centroids over stats [B, K, SN_TOWER_NSTAT] i64 and n_towers [B] i32: keep [B, K] u8, planar [B, K, 2] f64
    (or None), agg [B, K, 2] f64, n_agg [B] i32, status [B] i32, all caller-owned.  center / voxel_size: 3 floats or a
    ctypes array built once (center may be None without the filter).  No allocation, no synchronisation."""
    if stats.dim() != 3 or stats.shape[2] != SN_TOWER_NSTAT:
        raise HipLibraryError(f"stats must be [B, K, {SN_TOWER_NSTAT}] (got {tuple(stats.shape)})")
    B, K = int(stats.shape[0]), int(stats.shape[1])
    if n_towers.numel() != B or keep.numel() != B * K or agg.numel() != 2 * B * K or n_agg.numel() != B or \
            status.numel() != B or (planar is not None and planar.numel() != 2 * B * K):
        raise HipLibraryError("n_towers / keep / planar / agg / n_agg / status do not have the sizes of these stats")
    vs, ctr = _double3_c(voxel_size, "voxel_size"), _double3_c(center, "center")
    rc = load().sn_tower_centroids(
        _ptr(stats, torch.int64, "stats"), _ptr(n_towers, torch.int32, "n_towers"), B, K, int(height_axis),
        ctypes.cast(vs, c_void_p) if vs is not None else None, ctypes.cast(ctr, c_void_p) if ctr is not None else None,
        1 if apply_filter else 0, float(threshold), float(tower_height), float(rim_sq), float(min_euc),
        _ptr(keep, torch.uint8, "keep"), _ptr(planar, torch.float64, "planar"), _ptr(agg, torch.float64, "agg"),
        _ptr(n_agg, torch.int32, "n_agg"), _ptr(status, torch.int32, "status"), _stream())
    _check(rc, "sn_tower_centroids")


@_on_tensor_device
def tower_match(agg: torch.Tensor, n_agg: torch.Tensor, status_pred: torch.Tensor, gt_stats: torch.Tensor,
                gt_n_towers: torch.Tensor, height_axis: int, hit_dist: float, match: torch.Tensor, dist: torch.Tensor,
                gt_planar: Optional[torch.Tensor] = None, totals: Optional[torch.Tensor] = None,
                dist_total: Optional[torch.Tensor] = None, voxel_size=None) -> None:
    """sn_tower_match: agg [B, Kp, 2] f64, n_agg / status_pred [B] i32 of tower_centroids against gt_stats [B, Kg,
    SN_TOWER_NSTAT] i64, gt_n_towers [B] i32 -> match [B, Kg] i32, dist [B, Kg] f64, gt_planar [B, Kg, 2] f64 (or None);
    totals i64[SN_TSCORE_NTOTAL] and dist_total f64[1] (both or neither) are accumulated into.  No allocation, no
    synchronisation."""
    if agg.dim() != 3 or agg.shape[2] != 2:
        raise HipLibraryError(f"agg must be [B, K, 2] (got {tuple(agg.shape)})")
    if gt_stats.dim() != 3 or gt_stats.shape[2] != SN_TOWER_NSTAT or gt_stats.shape[0] != agg.shape[0]:
        raise HipLibraryError(f"gt_stats must be [{agg.shape[0]}, Kg, {SN_TOWER_NSTAT}] (got {tuple(gt_stats.shape)})")
    B, Kp, Kg = int(agg.shape[0]), int(agg.shape[1]), int(gt_stats.shape[1])
    if n_agg.numel() != B or status_pred.numel() != B or gt_n_towers.numel() != B or match.numel() != B * Kg or \
            dist.numel() != B * Kg or (gt_planar is not None and gt_planar.numel() != 2 * B * Kg) or \
            (totals is not None and totals.numel() != SN_TSCORE_NTOTAL) or (dist_total is not None and dist_total.numel() != 1):
        raise HipLibraryError("n_agg / status_pred / gt_n_towers / match / dist / gt_planar / totals / dist_total do not have "
                              "the sizes of agg and gt_stats")
    vs = _double3_c(voxel_size, "voxel_size")
    rc = load().sn_tower_match(
        _ptr(agg, torch.float64, "agg"), _ptr(n_agg, torch.int32, "n_agg"), _ptr(status_pred, torch.int32, "status_pred"),
        Kp, _ptr(gt_stats, torch.int64, "gt_stats"), _ptr(gt_n_towers, torch.int32, "gt_n_towers"), Kg, B, int(height_axis),
        ctypes.cast(vs, c_void_p) if vs is not None else None, float(hit_dist), _ptr(match, torch.int32, "match"),
        _ptr(dist, torch.float64, "dist"), _ptr(gt_planar, torch.float64, "gt_planar"), _ptr(totals, torch.int64, "totals"),
        _ptr(dist_total, torch.float64, "dist_total"), _stream())
    _check(rc, "sn_tower_match")


# --------------------------------------------------------------------------- #
def crops_chunk_points() -> int:
    """sn_crops_chunk_points: points per workgroup of the crop kernels (host only)."""
    return int(load().sn_crops_chunk_points())


def crops_ws_bytes(n: int, K: int) -> int:
    """sn_crops_ws_bytes: scratch bytes of crop_count / crop_scatter over n points and K regions (host only)."""
    need = int(load().sn_crops_ws_bytes(int(n), int(K)))
    if need == 0:
        raise HipLibraryError(f"sn_crop_count serves no scan of {n} points with {K} regions (1 <= n <= 2^36, "
                              "1 <= K <= 65536)")
    return need


def _crop_head(pts, regions, kinds):
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise HipLibraryError(f"pts must be [n, 3] (got {tuple(pts.shape)})")
    if regions.dim() != 2 or regions.shape[1] != 4:
        raise HipLibraryError(f"regions must be [K, 4] (got {tuple(regions.shape)})")
    n, K = int(pts.shape[0]), int(regions.shape[0])
    if kinds is not None and kinds.numel() != K:
        raise HipLibraryError("kinds must hold one entry per region")
    return n, K


@_on_tensor_device
def crop_count(pts: torch.Tensor, regions: torch.Tensor, kinds: Optional[torch.Tensor], ws: torch.Tensor,
               offsets: torch.Tensor) -> None:
    """sn_crop_count: pts [n,3] f64, regions [K,4] f64, kinds [K] i32 | None -> offsets [K+1] i64 and the per-workgroup
    prefixes in `ws` (crops_ws_bytes), both caller-owned.  Three launches, no allocation, no synchronisation."""
    n, K = _crop_head(pts, regions, kinds)
    if offsets.numel() != K + 1:
        raise HipLibraryError("offsets must hold K + 1 entries")
    rc = load().sn_crop_count(_ptr(pts, torch.float64, "pts"), n, _ptr(regions, torch.float64, "regions"),
                              _ptr(kinds, torch.int32, "kinds"), K, _ptr(ws, None, "ws"), ws.numel() * ws.element_size(),
                              _ptr(offsets, torch.int64, "offsets"), _stream())
    _check(rc, "sn_crop_count")


@_on_tensor_device
def crop_scatter(pts: torch.Tensor, labels: Optional[torch.Tensor], regions: torch.Tensor, kinds: Optional[torch.Tensor],
                 ws: torch.Tensor, offsets: torch.Tensor, out_pts: torch.Tensor, out_labels: Optional[torch.Tensor],
                 out_src: Optional[torch.Tensor], capacity: Optional[int] = None) -> None:
    """sn_crop_scatter behind crop_count on the same arguments: fills out_pts [rows,3] f64, out_labels [rows] f64 (iff
    labels) and out_src [rows] i64 (optional); rows at or beyond the capacity -- out_pts' row count, or a smaller
    `capacity` -- and beyond offsets[K] are left as they are.  One launch, no allocation, no synchronisation."""
    n, K = _crop_head(pts, regions, kinds)
    if out_pts.dim() != 2 or out_pts.shape[1] != 3:
        raise HipLibraryError(f"out_pts must be [capacity, 3] (got {tuple(out_pts.shape)})")
    capacity = int(out_pts.shape[0]) if capacity is None else int(capacity)
    if capacity > out_pts.shape[0]:
        raise HipLibraryError("capacity exceeds the rows of out_pts")
    if labels is not None and labels.numel() != n:
        raise HipLibraryError("labels and pts disagree in length")
    if (out_labels is not None and out_labels.numel() < capacity) or (out_src is not None and out_src.numel() < capacity):
        raise HipLibraryError("out_labels / out_src are shorter than out_pts")
    rc = load().sn_crop_scatter(_ptr(pts, torch.float64, "pts"), _ptr(labels, torch.float64, "labels"), n,
                                _ptr(regions, torch.float64, "regions"), _ptr(kinds, torch.int32, "kinds"), K,
                                _ptr(ws, None, "ws"), ws.numel() * ws.element_size(), _ptr(offsets, torch.int64, "offsets"),
                                capacity, _ptr(out_pts, torch.float64, "out_pts"),
                                _ptr(out_labels, torch.float64, "out_labels"), _ptr(out_src, torch.int64, "out_src"),
                                _stream())
    _check(rc, "sn_crop_scatter")


# --------------------------------------------------------------------------- #
def census_chunk_points() -> int:
    """sn_census_chunk_points: points per workgroup of the census kernel (host only)."""
    return int(load().sn_census_chunk_points())


def crop_census_ws_bytes(n: int, K: int, C: int) -> int:
    """sn_crop_census_ws_bytes: scratch bytes of crop_census over n points, K regions and C watch ranges (host only)."""
    need = int(load().sn_crop_census_ws_bytes(int(n), int(K), int(C)))
    if need == 0:
        raise HipLibraryError(f"sn_crop_census serves no scan of {n} points with {K} regions and {C} watch ranges "
                              f"(1 <= n <= 2^36, 1 <= K <= 65536, 0 <= C <= {SN_CENSUS_MAX_WATCH})")
    return need


@_on_tensor_device
def crop_census(pts: torch.Tensor, labels: Optional[torch.Tensor], regions: torch.Tensor, kinds: Optional[torch.Tensor],
                watch: Optional[torch.Tensor], ws: torch.Tensor, counts: torch.Tensor,
                label_range: Optional[torch.Tensor]) -> None:
    """sn_crop_census: pts [n,3] f64, labels [n] f64 | None, regions [K,4] f64, kinds [K] i32 | None, watch [C,2] f64 | None
    (C = 0) -> counts [K, 2 + C] i64 and label_range [K,2] f64 (iff labels), with `ws` (crop_census_ws_bytes) all
    caller-owned.  One memset node and two launches, no allocation, no synchronisation."""
    n, K = _crop_head(pts, regions, kinds)
    C = 0 if watch is None else int(watch.shape[0])
    if watch is not None and (watch.dim() != 2 or watch.shape[1] != 2 or C == 0):
        raise HipLibraryError(f"watch must be [C, 2] with C >= 1, or None (got {tuple(watch.shape)})")
    if labels is not None and labels.numel() != n:
        raise HipLibraryError("labels and pts disagree in length")
    if counts.numel() != K * (2 + C):
        raise HipLibraryError("counts must hold K * (2 + C) entries")
    if label_range is not None and label_range.numel() != 2 * K:
        raise HipLibraryError("label_range must hold 2 * K entries")
    rc = load().sn_crop_census(_ptr(pts, torch.float64, "pts"), _ptr(labels, torch.float64, "labels"), n,
                               _ptr(regions, torch.float64, "regions"), _ptr(kinds, torch.int32, "kinds"), K,
                               _ptr(watch, torch.float64, "watch"), C, _ptr(ws, None, "ws"),
                               ws.numel() * ws.element_size(), _ptr(counts, torch.int64, "counts"),
                               _ptr(label_range, torch.float64, "label_range"), _stream())
    _check(rc, "sn_crop_census")


# --------------------------------------------------------------------------- #
def points_select_chunk_points() -> int:
    """sn_points_select_chunk_points: scan points per workgroup of the select kernels (host only)."""
    return int(load().sn_points_select_chunk_points())


def dbscan_chunk_points() -> int:
    """sn_dbscan_chunk_points: positions per workgroup of the clustering kernels (host only)."""
    return int(load().sn_dbscan_chunk_points())


def points_select_ws_bytes(n: int) -> int:
    """sn_points_select_ws_bytes: scratch bytes of points_select over n points (host only)."""
    need = int(load().sn_points_select_ws_bytes(int(n)))
    if need == 0:
        raise HipLibraryError(f"sn_points_select serves no scan of {n} points (1 <= n <= 2^33)")
    return need


def _bounds_c(bounds):
    if isinstance(bounds, ctypes.Array):
        return bounds
    vals = [float(v) for v in bounds]
    if len(vals) != 6:
        raise ValueError("bounds must have 6 entries: xmin, ymin, zmin, xmax, ymax, zmax")
    return (ctypes.c_double * 6)(*vals)


def dbscan_cell_grid(bounds, eps: float, max_cells: int) -> Tuple[Tuple[int, int, int], float]:
    """sn_dbscan_cell_grid (host only): ((dims per axis), cell side) of the search grid over bounds = (xmin, ymin, zmin,
    xmax, ymax, zmax)."""
    dims = (ctypes.c_int32 * 3)()
    side = ctypes.c_double(0.0)
    b = _bounds_c(bounds)
    _check(load().sn_dbscan_cell_grid(ctypes.cast(b, c_void_p), float(eps), int(max_cells), ctypes.cast(dims, c_void_p),
                                      ctypes.cast(ctypes.pointer(side), c_void_p)), "sn_dbscan_cell_grid")
    return (int(dims[0]), int(dims[1]), int(dims[2])), float(side.value)


def dbscan_ws_bytes(capacity: int, cells: int) -> int:
    """sn_dbscan_ws_bytes: scratch bytes of dbscan_points for `capacity` positions and `cells` grid cells (host only)."""
    need = int(load().sn_dbscan_ws_bytes(int(capacity), int(cells)))
    if need == 0:
        raise HipLibraryError(f"sn_dbscan_points serves no {capacity} positions on {cells} cells (1 <= capacity < 2^31, "
                              "1 <= cells <= 2^22)")
    return need


@_on_tensor_device
def points_select(pts: torch.Tensor, labels: Optional[torch.Tensor], keep: Optional[torch.Tensor], ws: torch.Tensor,
                  sel: Optional[torch.Tensor], n_sel: torch.Tensor, bbox: torch.Tensor,
                  capacity: Optional[int] = None) -> None:
    """sn_points_select: pts [n,3] f64, labels [n] f64 | None, keep [n_keep] f64 (device) -> sel [capacity] i64, n_sel [1]
    i64 (the true count), bbox [6] f64, all caller-owned like the scratch `ws` (points_select_ws_bytes).  Three launches,
    no allocation, no synchronisation."""
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise HipLibraryError(f"pts must be [n, 3] (got {tuple(pts.shape)})")
    n = int(pts.shape[0])
    if labels is not None and labels.numel() != n:
        raise HipLibraryError("labels and pts disagree in length")
    rows = 0 if sel is None else int(sel.numel())
    capacity = rows if capacity is None else int(capacity)
    if capacity > rows:
        raise HipLibraryError("capacity exceeds the rows of sel")
    if n_sel.numel() != 1 or bbox.numel() != 6:
        raise HipLibraryError("n_sel must hold 1 entry and bbox 6")
    rc = load().sn_points_select(_ptr(pts, torch.float64, "pts"), _ptr(labels, torch.float64, "labels"), n,
                                 _ptr(keep, torch.float64, "keep"), 0 if keep is None else int(keep.numel()), capacity,
                                 _ptr(ws, None, "ws"), ws.numel() * ws.element_size(),
                                 _ptr(sel, torch.int64, "sel") if capacity > 0 else None, _ptr(n_sel, torch.int64, "n_sel"),
                                 _ptr(bbox, torch.float64, "bbox"), _stream())
    _check(rc, "sn_points_select")


@_on_tensor_device
def dbscan_points(pts: torch.Tensor, sel: Optional[torch.Tensor], n_sel: Optional[torch.Tensor], bounds, eps: float,
                  min_points: int, max_cells: int, max_clusters: int, ws: torch.Tensor, cluster: torch.Tensor,
                  n_clusters: torch.Tensor, stats: Optional[torch.Tensor], status: torch.Tensor,
                  capacity: Optional[int] = None, launches: Optional[Tuple[int, int]] = None) -> None:
    """sn_dbscan_points over the positions sel [>= capacity] i64 (None: the scan's own rows) of pts [n,3] f64: cluster
    [capacity] i32, n_clusters [1] i32, stats [max_clusters, SN_DBSCAN_NSTAT] i64, status [1] i32, all caller-owned like
    the scratch `ws` (dbscan_ws_bytes).  bounds: 6 floats or a ctypes array built once.  launches = (first, last): only
    those of the SN_DBSCAN_LAUNCHES launches (sn_dbscan_points_launches: timing).  No allocation, no synchronisation."""
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise HipLibraryError(f"pts must be [n, 3] (got {tuple(pts.shape)})")
    n = int(pts.shape[0])
    capacity = int(cluster.numel()) if capacity is None else int(capacity)
    max_clusters = int(max_clusters)
    if capacity > cluster.numel() or (sel is not None and sel.numel() < capacity):
        raise HipLibraryError("capacity exceeds the rows of cluster / sel")
    if n_clusters.numel() != 1 or status.numel() != 1 or (n_sel is not None and n_sel.numel() != 1) or \
            (stats is not None and stats.numel() != max_clusters * SN_DBSCAN_NSTAT):
        raise HipLibraryError("n_clusters / status / n_sel / stats do not have the sizes of this call")
    b = _bounds_c(bounds)
    head = (_ptr(pts, torch.float64, "pts"), n, _ptr(sel, torch.int64, "sel"), _ptr(n_sel, torch.int64, "n_sel"), capacity,
            ctypes.cast(b, c_void_p), float(eps), int(min_points), int(max_cells), max_clusters, _ptr(ws, None, "ws"),
            ws.numel() * ws.element_size(), _ptr(cluster, torch.int32, "cluster"), _ptr(n_clusters, torch.int32, "n_clusters"),
            _ptr(stats, torch.int64, "stats"), _ptr(status, torch.int32, "status"))
    if launches is None:
        rc = load().sn_dbscan_points(*head, _stream())
    else:
        rc = load().sn_dbscan_points_launches(*head, int(launches[0]), int(launches[1]), _stream())
    _check(rc, "sn_dbscan_points")


# --------------------------------------------------------------------------- #
def las_chunk_records() -> int:
    """sn_las_chunk_records: records per workgroup and pass of the LAS decode kernel (host only)."""
    return int(load().sn_las_chunk_records())


@_on_tensor_device
def las_decode(records: torch.Tensor, n: int, point_format: int, record_length: int, scale: Sequence[float],
               offset: Sequence[float], pts: torch.Tensor, classes: Optional[torch.Tensor] = None,
               hist: Optional[torch.Tensor] = None) -> None:
    """sn_las_decode: records, a uint8 tensor at ANY byte address that holds n records of record_length bytes -> pts [n,3]
    f64, classes [n] f64 | None, hist [256] i64 | None (ACCUMULATED: the caller zeroes it), all caller-owned and written in
    place; pts / classes may be larger, nothing beyond point n - 1 is touched.  One launch, no allocation, no
    synchronisation."""
    n, record_length = int(n), int(record_length)
    if records.dtype != torch.uint8 or records.dim() != 1:
        raise HipLibraryError("records must be a one-dimensional uint8 tensor (the file's bytes as they are)")
    if n > 0 and records.numel() < n * record_length:
        raise HipLibraryError(f"records holds {records.numel()} bytes, {n} records of {record_length} need more")
    if n > 0 and (pts.numel() < 3 * n or (classes is not None and classes.numel() < n)):
        raise HipLibraryError("pts / classes are smaller than the records they are to hold")
    if hist is not None and hist.numel() != 256:
        raise HipLibraryError("hist must hold 256 counts")
    if len(scale) != 3 or len(offset) != 3:
        raise HipLibraryError("scale and offset have 3 entries each")
    sc = (ctypes.c_double * 3)(*[float(v) for v in scale])
    of = (ctypes.c_double * 3)(*[float(v) for v in offset])
    rc = load().sn_las_decode(_ptr(records, torch.uint8, "records"), n, int(point_format), record_length,
                              ctypes.cast(sc, c_void_p), ctypes.cast(of, c_void_p), _ptr(pts, torch.float64, "pts"),
                              _ptr(classes, torch.float64, "classes"), _ptr(hist, torch.int64, "hist"), _stream())
    _check(rc, "sn_las_decode")


# --------------------------------------------------------------------------- #
def las_encode_chunk_records() -> int:
    """sn_las_encode_chunk_records: records per workgroup and pass of the LAS encode kernel (host only)."""
    return int(load().sn_las_encode_chunk_records())


def _u16_ptr(t: Optional[torch.Tensor], name: str) -> Optional[int]:
    """pointer of a tensor of 16-bit words: uint16, or int16 taken as the same bits"""
    if t is not None and t.dtype == torch.int16:
        return _ptr(t, torch.int16, name)
    return _ptr(t, torch.uint16, name)


@_on_tensor_device
def las_encode(pts: torch.Tensor, n: int, point_format: int, record_length: int, scale: Sequence[float],
               offset: Sequence[float], records: torch.Tensor, classes: Optional[torch.Tensor] = None,
               intensity: Optional[torch.Tensor] = None, gps_time: Optional[torch.Tensor] = None,
               rgb: Optional[torch.Tensor] = None, box: Optional[torch.Tensor] = None, hist: Optional[torch.Tensor] = None,
               bad: Optional[torch.Tensor] = None) -> None:
    """sn_las_encode: pts [n,3] f64, classes [n] f64 | None, intensity [n] u16 | None, gps_time [n] f64 | None, rgb [n,3] u16
    | None -> n records of record_length bytes at the start of `records`, a 16-byte aligned uint8 tensor; box [6] i32 | None
    (UPDATED by min / max: the caller sets INT32_MAX / INT32_MIN pairs), hist [256] i64 | None and bad [2] i64 | None
    (ACCUMULATED: the caller zeroes them).  The inputs may be larger than n; nothing beyond byte n * record_length - 1 of
    records is touched.  One launch, no allocation, no synchronisation."""
    n, record_length = int(n), int(record_length)
    if records.dtype != torch.uint8 or records.dim() != 1:
        raise HipLibraryError("records must be a one-dimensional uint8 tensor (the file's bytes as they will be)")
    if n > 0 and records.numel() < n * record_length:
        raise HipLibraryError(f"records holds {records.numel()} bytes, {n} records of {record_length} need more")
    for name, t, per in (("pts", pts, 3), ("classes", classes, 1), ("intensity", intensity, 1), ("gps_time", gps_time, 1),
                         ("rgb", rgb, 3)):
        if t is not None and n > 0 and t.numel() < per * n:
            raise HipLibraryError(f"{name} holds {t.numel()} elements, {n} points need {per * n}")
    if box is not None and box.numel() != 6:
        raise HipLibraryError("box must hold 6 integers")
    if hist is not None and hist.numel() != 256:
        raise HipLibraryError("hist must hold 256 counts")
    if bad is not None and bad.numel() != 2:
        raise HipLibraryError("bad must hold 2 counts")
    if len(scale) != 3 or len(offset) != 3:
        raise HipLibraryError("scale and offset have 3 entries each")
    sc = (ctypes.c_double * 3)(*[float(v) for v in scale])
    of = (ctypes.c_double * 3)(*[float(v) for v in offset])
    rc = load().sn_las_encode(_ptr(pts, torch.float64, "pts"), _ptr(classes, torch.float64, "classes"),
                              _u16_ptr(intensity, "intensity"), _ptr(gps_time, torch.float64, "gps_time"),
                              _u16_ptr(rgb, "rgb"), n, int(point_format), record_length, ctypes.cast(sc, c_void_p),
                              ctypes.cast(of, c_void_p), _ptr(records, torch.uint8, "records"),
                              _ptr(box, torch.int32, "box"), _ptr(hist, torch.int64, "hist"), _ptr(bad, torch.int64, "bad"),
                              _stream())
    _check(rc, "sn_las_encode")


# --------------------------------------------------------------------------- #
def kitti_chunk_points() -> int:
    """sn_kitti_chunk_points: points per workgroup and pass of the SemanticKITTI decode kernel (host only)."""
    return int(load().sn_kitti_chunk_points())


def _raw4(t: Optional[torch.Tensor], nbytes: int, name: str) -> Optional[int]:
    """pointer of a tensor that is taken as raw bytes (uint8, int32 or float32) and holds `nbytes` at least"""
    if t is None:
        return None
    if t.dtype not in (torch.uint8, torch.int32, torch.float32):
        raise HipLibraryError(f"{name} must be uint8, int32 or float32: the file's bytes as they are (got {t.dtype})")
    if t.numel() * t.element_size() < nbytes:
        raise HipLibraryError(f"{name} holds {t.numel() * t.element_size()} bytes, {nbytes} are needed")
    return _ptr(t, None, name)


@_on_tensor_device
def kitti_decode(scans: torch.Tensor, label_words: Optional[torch.Tensor], total: int, offsets: torch.Tensor,
                 pts: torch.Tensor, labels: Optional[torch.Tensor] = None, lut: Optional[torch.Tensor] = None,
                 remission: Optional[torch.Tensor] = None, instance: Optional[torch.Tensor] = None,
                 hist: Optional[torch.Tensor] = None, bad: Optional[torch.Tensor] = None,
                 unmapped: Optional[torch.Tensor] = None) -> None:
    """sn_kitti_decode: scans, the .bin bytes of B scans concatenated (16 * total bytes at any 4-byte address), and
    label_words, their .label bytes (4 * total; None: points only) -> pts [total,3] f64, labels [total] f64, remission
    [total] f32, instance [total] i32, hist [B, n_hist] i64 (ACCUMULATED: the caller zeroes it), bad [B] i32 and unmapped
    [B] i32 (both written), all caller-owned and written in place; offsets [B+1] i64 is the CSR of the scans, lut [n_lut]
    i32 the optional class remap.  The outputs may be larger: nothing beyond point total - 1 is touched.  One launch, no
    allocation, no synchronisation."""
    total = int(total)
    B = int(offsets.numel()) - 1
    if total > 0:
        if pts.numel() < 3 * total or (labels is not None and labels.numel() < total):
            raise HipLibraryError("pts / labels are smaller than the points they are to hold")
        if (remission is not None and remission.numel() < total) or (instance is not None and instance.numel() < total):
            raise HipLibraryError("remission / instance are smaller than the points they are to hold")
    n_hist = 0
    if hist is not None:
        if hist.dim() != 2 or hist.shape[0] != B:
            raise HipLibraryError(f"hist must be [B, n_hist] with B = {B} (got {tuple(hist.shape)})")
        n_hist = int(hist.shape[1])
    for name, t in (("bad", bad), ("unmapped", unmapped)):
        if t is not None and t.numel() < B:
            raise HipLibraryError(f"{name} must hold one count per scan")
    rc = load().sn_kitti_decode(_raw4(scans, 16 * max(total, 0), "scans"), _raw4(label_words, 4 * max(total, 0), "label_words"),
                                total, _ptr(offsets, torch.int64, "offsets"), B, _ptr(lut, torch.int32, "lut"),
                                0 if lut is None else int(lut.numel()), _ptr(pts, torch.float64, "pts"),
                                _ptr(labels, torch.float64, "labels"), _ptr(remission, torch.float32, "remission"),
                                _ptr(instance, torch.int32, "instance"), _ptr(hist, torch.int64, "hist"), n_hist,
                                _ptr(bad, torch.int32, "bad"), _ptr(unmapped, torch.int32, "unmapped"), _stream())
    _check(rc, "sn_kitti_decode")


# --------------------------------------------------------------------------- #
def voxel_cloud_chunk_cells() -> int:
    """sn_voxel_cloud_chunk_cells: cells per workgroup of the voxel-cloud kernels (host only)."""
    return int(load().sn_voxel_cloud_chunk_cells())


def voxel_cloud_ws_bytes(B: int, V: int) -> int:
    """sn_voxel_cloud_ws_bytes: scratch bytes of voxel_cloud_count / voxel_cloud_scatter over B tiles of V cells (host only)."""
    need = int(load().sn_voxel_cloud_ws_bytes(int(B), int(V)))
    if need == 0:
        raise HipLibraryError(f"sn_voxel_cloud_count serves no batch of {B} grids with {V} cells each (1 <= B <= 65535, "
                              "1 <= cells < 2^31)")
    return need


def _cloud_head(grids, desc):
    if grids.dim() != 4 or grids.dtype not in _DT or grids.dtype == torch.bfloat16:
        raise HipLibraryError("grids must be [B,n0,n1,n2] float32/float64/uint8/bool")
    B, n0, n1, n2 = (int(v) for v in grids.shape)
    if desc is not None and tuple(desc.shape) != (B, desc_len(n1, n2, n0)):
        raise HipLibraryError(f"desc must be [B, desc_len(nx, ny, nz)] = [{B}, {desc_len(n1, n2, n0)}] "
                              f"(got {tuple(desc.shape)})")
    return B, n0, n1, n2


@_on_tensor_device
def voxel_cloud_count(grids: torch.Tensor, mode: int, r: int, desc: Optional[torch.Tensor], ws: torch.Tensor,
                      offsets: torch.Tensor, bad: torch.Tensor) -> None:
    """sn_voxel_cloud_count: grids [B,n0,n1,n2] -> offsets [B+1] i64, bad [B,2] i64 and the per-workgroup prefixes in `ws`
    (voxel_cloud_ws_bytes), all caller-owned.  Three launches, no allocation, no synchronisation."""
    B, n0, n1, n2 = _cloud_head(grids, desc)
    if offsets.numel() != B + 1 or bad.numel() != 2 * B:
        raise HipLibraryError("offsets must hold B + 1 entries and bad 2 * B")
    rc = load().sn_voxel_cloud_count(_ptr(grids, None, "grids"), _DT[grids.dtype], B, n0, n1, n2, int(mode), int(r),
                                     _ptr(desc, torch.float64, "desc"), _ptr(ws, None, "ws"),
                                     ws.numel() * ws.element_size(), _ptr(offsets, torch.int64, "offsets"),
                                     _ptr(bad, torch.int64, "bad"), _stream())
    _check(rc, "sn_voxel_cloud_count")


@_on_tensor_device
def voxel_cloud_scatter(grids: torch.Tensor, mode: int, r: int, table, desc: Optional[torch.Tensor], ws: torch.Tensor,
                        offsets: torch.Tensor, rows: Optional[torch.Tensor], xyz: Optional[torch.Tensor] = None,
                        rgb16: Optional[torch.Tensor] = None, capacity: Optional[int] = None) -> None:
    """sn_voxel_cloud_scatter behind voxel_cloud_count on the same arguments: fills rows [cap,6] f64 and / or xyz [cap,3] f64
    and rgb16 [cap,3] (u)int16; `table`: [r,3] doubles on the host (None in the density mode).  Rows at or beyond the
    capacity -- the outputs' row count, or a smaller `capacity` -- and beyond offsets[B] are left as they are.  One launch,
    no allocation, no synchronisation."""
    B, n0, n1, n2 = _cloud_head(grids, desc)
    have = [t for t in (rows, xyz, rgb16) if t is not None]
    if rows is None and xyz is None:
        raise HipLibraryError("one of rows and xyz must be given")
    for t, cols, name in ((rows, 6, "rows"), (xyz, 3, "xyz"), (rgb16, 3, "rgb16")):
        if t is not None and (t.dim() != 2 or t.shape[1] != cols):
            raise HipLibraryError(f"{name} must be [capacity, {cols}] (got {tuple(t.shape)})")
    least = min(int(t.shape[0]) for t in have)
    capacity = least if capacity is None else int(capacity)
    if capacity > least:
        raise HipLibraryError("capacity exceeds the rows of an output")
    if rgb16 is not None and rgb16.dtype not in (torch.uint16, torch.int16):
        raise HipLibraryError(f"rgb16 must be uint16 (got {rgb16.dtype})")
    t_keep, t_ptr = None, None
    if table is not None:
        flat = [float(v) for row in table for v in row]
        if len(flat) != 3 * int(r):
            raise HipLibraryError(f"the colour table must be [r, 3] = [{int(r)}, 3]")
        t_keep = (ctypes.c_double * len(flat))(*flat)
        t_ptr = ctypes.cast(t_keep, c_void_p)
    rc = load().sn_voxel_cloud_scatter(_ptr(grids, None, "grids"), _DT[grids.dtype], B, n0, n1, n2, int(mode), int(r), t_ptr,
                                       _ptr(desc, torch.float64, "desc"), _ptr(ws, None, "ws"),
                                       ws.numel() * ws.element_size(), _ptr(offsets, torch.int64, "offsets"), capacity,
                                       _ptr(rows, torch.float64, "rows"), _ptr(xyz, torch.float64, "xyz"),
                                       _ptr(rgb16, None, "rgb16"), _stream())
    _check(rc, "sn_voxel_cloud_scatter")


# --------------------------------------------------------------------------- #
def thin_chunk_points() -> int:
    """sn_thin_chunk_points: rows per workgroup of the thinning kernels (host only)."""
    return int(load().sn_thin_chunk_points())


def thin_ws_bytes(total: int, B: int) -> int:
    """sn_thin_ws_bytes: scratch bytes of thin_count / thin_scatter over a batch of `total` rows in B tiles (host only)."""
    need = int(load().sn_thin_ws_bytes(int(total), int(B)))
    if need == 0:
        raise HipLibraryError(f"sn_thin_count serves no batch of {total} rows in {B} tiles (1 <= total <= 2^33, "
                              "1 <= B <= 65536)")
    return need


def thin_groups(group: int, n_xyz: Sequence[int]) -> int:
    """G of a rule: thresholds per tile (1, nz or nx * ny * nz)."""
    nx, ny, nz = (int(v) for v in n_xyz)
    return {SN_THIN_GROUP_NONE: 1, SN_THIN_GROUP_Z: nz, SN_THIN_GROUP_VOXEL: nx * ny * nz}[int(group)]


def _thin_head(pts, offsets, group, desc, n_xyz, thr, u, seed, tile_ids):
    """The checks and the leading arguments sn_thin_count and sn_thin_scatter share."""
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise HipLibraryError(f"pts must be [total, 3] (got {tuple(pts.shape)})")
    total, B = int(pts.shape[0]), int(offsets.numel()) - 1
    nx, ny, nz = (int(v) for v in n_xyz)
    G = thin_groups(group, (nx, ny, nz))
    if thr.numel() != B * G:
        raise HipLibraryError(f"thr must be [B, G] = [{B}, {G}] (got {tuple(thr.shape)})")
    if int(group) != SN_THIN_GROUP_NONE and (desc is None or tuple(desc.shape) != (B, desc_len(nx, ny, nz))):
        raise HipLibraryError(f"desc must be [B, desc_len(nx, ny, nz)] = [{B}, {desc_len(nx, ny, nz)}]")
    if u is not None and u.numel() != total:
        raise HipLibraryError("u must hold one entry per row of pts")
    if seed is not None and seed.numel() != 1:
        raise HipLibraryError("seed must hold one 64-bit word")
    if tile_ids is not None and tile_ids.numel() != B:
        raise HipLibraryError("tile_ids must hold one entry per tile")
    return total, B, G, (_ptr(offsets, torch.int64, "offsets"), total, B, int(group), _ptr(desc, torch.float64, "desc"),
                         nx, ny, nz, _ptr(thr, torch.float64, "thr"), _ptr(u, torch.float64, "u"),
                         _ptr(seed, torch.int64, "seed"), _ptr(tile_ids, torch.int64, "tile_ids"))


@_on_tensor_device
def thin_count(pts: torch.Tensor, offsets: torch.Tensor, group: int, desc: Optional[torch.Tensor], n_xyz: Sequence[int],
               thr: torch.Tensor, u: Optional[torch.Tensor], seed: Optional[torch.Tensor], tile_ids: Optional[torch.Tensor],
               ws: torch.Tensor, offsets_out: torch.Tensor, unbinned: torch.Tensor,
               first: Optional[torch.Tensor] = None) -> None:
    """sn_thin_count: pts [total,3] f64, offsets [B+1] i64, thr [B,G] f64, u [total] f64 or seed [1] i64 (the u64's bits),
    tile_ids [B] i64 | None -> offsets_out [B+1] i64, unbinned [B] i64, first [B,G] i64 | None (all ones = -1: an empty
    group) and the decisions in `ws` (thin_ws_bytes), all caller-owned.  No allocation, no synchronisation."""
    total, B, G, head = _thin_head(pts, offsets, group, desc, n_xyz, thr, u, seed, tile_ids)
    if offsets_out.numel() != B + 1 or unbinned.numel() != B:
        raise HipLibraryError("offsets_out must hold B + 1 entries and unbinned B")
    if first is not None and first.numel() != B * G:
        raise HipLibraryError(f"first must be [B, G] = [{B}, {G}]")
    rc = load().sn_thin_count(_ptr(pts, torch.float64, "pts"), *head, _ptr(ws, None, "ws"), ws.numel() * ws.element_size(),
                              _ptr(offsets_out, torch.int64, "offsets_out"), _ptr(unbinned, torch.int64, "unbinned"),
                              _ptr(first, torch.int64, "first"), _stream())
    _check(rc, "sn_thin_count")


@_on_tensor_device
def thin_scatter(pts: torch.Tensor, labels: Optional[torch.Tensor], offsets: torch.Tensor, group: int,
                 desc: Optional[torch.Tensor], n_xyz: Sequence[int], thr: torch.Tensor, u: Optional[torch.Tensor],
                 seed: Optional[torch.Tensor], tile_ids: Optional[torch.Tensor], ws: torch.Tensor, out_pts: torch.Tensor,
                 out_labels: Optional[torch.Tensor], out_src: Optional[torch.Tensor], out_key: Optional[torch.Tensor] = None,
                 capacity: Optional[int] = None) -> None:
    """sn_thin_scatter behind thin_count on the same arguments: fills out_pts [rows,3] f64, out_labels [rows] f64 (iff
    labels), out_src [rows] i64 and out_key [rows] i32 (both optional); rows at or beyond the capacity -- out_pts' row
    count, or a smaller `capacity` -- and beyond offsets_out[B] are left as they are.  One launch, no allocation, no
    synchronisation."""
    total, B, G, head = _thin_head(pts, offsets, group, desc, n_xyz, thr, u, seed, tile_ids)
    if out_pts.dim() != 2 or out_pts.shape[1] != 3:
        raise HipLibraryError(f"out_pts must be [capacity, 3] (got {tuple(out_pts.shape)})")
    capacity = int(out_pts.shape[0]) if capacity is None else int(capacity)
    if capacity > out_pts.shape[0]:
        raise HipLibraryError("capacity exceeds the rows of out_pts")
    if labels is not None and labels.numel() != total:
        raise HipLibraryError("labels and pts disagree in length")
    if any(t is not None and t.numel() < capacity for t in (out_labels, out_src, out_key)):
        raise HipLibraryError("out_labels / out_src / out_key are shorter than out_pts")
    rc = load().sn_thin_scatter(_ptr(pts, torch.float64, "pts"), _ptr(labels, torch.float64, "labels"), *head,
                                _ptr(ws, None, "ws"), ws.numel() * ws.element_size(), capacity,
                                _ptr(out_pts, torch.float64, "out_pts"), _ptr(out_labels, torch.float64, "out_labels"),
                                _ptr(out_src, torch.int64, "out_src"), _ptr(out_key, torch.int32, "out_key"), _stream())
    _check(rc, "sn_thin_scatter")


# --------------------------------------------------------------------------- #
def voxel_classes_chunk_points() -> int:
    """sn_voxel_classes_chunk_points: rows per workgroup of the class-grid kernel (host only)."""
    return int(load().sn_voxel_classes_chunk_points())


def class_chunk_points() -> int:
    """sn_class_chunk_points: rows per workgroup of the class census and paint kernels (host only)."""
    return int(load().sn_class_chunk_points())


@_on_tensor_device
def voxel_classes(pts: torch.Tensor, labels: torch.Tensor, offsets: torch.Tensor, desc: torch.Tensor, n_xyz: Sequence[int],
                  grid: torch.Tensor, unbinned: torch.Tensor, nan_labels: torch.Tensor, skip: bool = True) -> None:
    """sn_voxel_classes: pts [total,3] f64, labels [total] f64, offsets [B+1] i64, desc [B, desc_len] -> grid [B,nz,nx,ny] f64
    (any shape of B * nz * nx * ny elements), unbinned [B] i64, nan_labels [B] i64, all caller-owned.  skip=False sends
    every row's atomic (same result; for timing).  No allocation, no synchronisation."""
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise HipLibraryError(f"pts must be [total, 3] (got {tuple(pts.shape)})")
    total, B = int(pts.shape[0]), int(offsets.numel()) - 1
    nx, ny, nz = (int(v) for v in n_xyz)
    if labels.numel() != total:
        raise HipLibraryError("labels and pts disagree in length")
    if tuple(desc.shape) != (B, desc_len(nx, ny, nz)):
        raise HipLibraryError(f"desc must be [B, desc_len(nx, ny, nz)] = [{B}, {desc_len(nx, ny, nz)}] "
                              f"(got {tuple(desc.shape)})")
    if grid.numel() != B * nx * ny * nz or unbinned.numel() != B or nan_labels.numel() != B:
        raise HipLibraryError("grid must hold B * nz * nx * ny cells, unbinned and nan_labels B entries")
    rc = load().sn_voxel_classes(_ptr(pts, torch.float64, "pts"), _ptr(labels, torch.float64, "labels"),
                                 _ptr(offsets, torch.int64, "offsets"), total, B, _ptr(desc, torch.float64, "desc"), nx, ny,
                                 nz, 0 if skip else SN_VOXEL_CLASSES_NO_SKIP, _ptr(grid, torch.float64, "grid"),
                                 _ptr(unbinned, torch.int64, "unbinned"), _ptr(nan_labels, torch.int64, "nan_labels"),
                                 _stream())
    _check(rc, "sn_voxel_classes")


@_on_tensor_device
def class_census(classes: torch.Tensor, offsets: torch.Tensor, present: torch.Tensor, bad: torch.Tensor) -> None:
    """sn_class_census: classes [total] f64, offsets [B+1] i64 -> present [B, SN_CLASS_WORDS] i32 (the u32 words' bits), bad
    [B] i64, caller-owned.  No allocation, no synchronisation."""
    total, B = int(classes.numel()), int(offsets.numel()) - 1
    if present.numel() != B * SN_CLASS_WORDS or bad.numel() != B:
        raise HipLibraryError(f"present must be [B, {SN_CLASS_WORDS}] and bad [B] for B = {B}")
    rc = load().sn_class_census(_ptr(classes, torch.float64, "classes"), _ptr(offsets, torch.int64, "offsets"), total, B,
                                _ptr(present, torch.int32, "present"), _ptr(bad, torch.int64, "bad"), _stream())
    _check(rc, "sn_class_census")


@_on_tensor_device
def class_paint(classes: torch.Tensor, offsets: torch.Tensor, present: torch.Tensor, table: torch.Tensor,
                colors: Optional[torch.Tensor], rgb: Optional[torch.Tensor], unique: Optional[torch.Tensor],
                n_unique: torch.Tensor, short_table: torch.Tensor) -> None:
    """sn_class_paint behind class_census: table [T,3] f64 on the device -> colors [total,3] f64 and / or rgb [total,3]
    u16 (int16 storage serves), unique [B, U_max] f64 | None, n_unique [B] i64, short_table [B] i64, caller-owned; the
    outputs may be longer than the batch, rows beyond it are left as they are.  No allocation, no synchronisation."""
    total, B = int(classes.numel()), int(offsets.numel()) - 1
    if table.dim() != 2 or table.shape[1] != 3 or table.shape[0] < 1:
        raise HipLibraryError(f"table must be [T, 3] with T >= 1 (got {tuple(table.shape)})")
    if present.numel() != B * SN_CLASS_WORDS or n_unique.numel() != B or short_table.numel() != B:
        raise HipLibraryError(f"present must be [B, {SN_CLASS_WORDS}], n_unique and short_table [B] for B = {B}")
    if colors is None and rgb is None:
        raise HipLibraryError("one of colors and rgb is needed")
    if any(t is not None and t.numel() < 3 * total for t in (colors, rgb)):
        raise HipLibraryError("colors / rgb hold fewer than total rows")
    U_max = 0
    if unique is not None:
        if unique.dim() != 2 or unique.shape[0] != B or unique.shape[1] < 1:
            raise HipLibraryError(f"unique must be [B, U_max] with U_max >= 1 (got {tuple(unique.shape)})")
        U_max = int(unique.shape[1])
    rc = load().sn_class_paint(_ptr(classes, torch.float64, "classes"), _ptr(offsets, torch.int64, "offsets"), total, B,
                               _ptr(present, torch.int32, "present"), _ptr(table, torch.float64, "table"),
                               int(table.shape[0]), _ptr(colors, torch.float64, "colors"), _u16_ptr(rgb, "rgb"),
                               _ptr(unique, torch.float64, "unique"), U_max, _ptr(n_unique, torch.int64, "n_unique"),
                               _ptr(short_table, torch.int64, "short_table"), _stream())
    _check(rc, "sn_class_paint")


# --------------------------------------------------------------------------- #
@_on_tensor_device
def scan_merge(grid: torch.Tensor, desc: torch.Tensor, pts: torch.Tensor, regions: torch.Tensor,
               kinds: Optional[torch.Tensor], tile_of: Optional[torch.Tensor], rule: int, fill: float, out: torch.Tensor,
               cover: Optional[torch.Tensor]) -> None:
    """sn_scan_merge: grid [B,C,nz,nx,ny] (f32|f64), desc [B, desc_len], pts [n,3] f64, regions [K,4] f64, kinds [K] i32 |
    None, tile_of [K] i32 | None (then B == K) -> out [C, n] of the grid's dtype and cover [n] i32 | None, caller-owned.
    One launch, no allocation, no synchronisation."""
    if grid.dim() != 5 or grid.dtype not in (torch.float32, torch.float64):
        raise HipLibraryError("grid must be [B,C,nz,nx,ny] float32/float64")
    B, C, nz, nx, ny = grid.shape
    n, K = _crop_head(pts, regions, kinds)
    # host-side shape checks, no synchronisation: the kernel reads desc[b * desc_len + ..] and tile_of[0..K) unchecked
    if tuple(desc.shape) != (B, desc_len(nx, ny, nz)):
        raise HipLibraryError(f"desc must be [B, desc_len(nx, ny, nz)] = [{B}, {desc_len(nx, ny, nz)}] "
                              f"(got {tuple(desc.shape)})")
    if tile_of is not None and tile_of.numel() != K:
        raise HipLibraryError("tile_of must hold one entry per region")
    if out.dtype != grid.dtype or out.numel() < C * n:
        raise HipLibraryError("out must hold channels * n values of the grid's dtype")
    if cover is not None and cover.numel() < n:
        raise HipLibraryError("cover must hold n entries")
    rc = load().sn_scan_merge(_ptr(grid, None, "grid"), _DT[grid.dtype], C, B, nx, ny, nz, _ptr(desc, torch.float64, "desc"),
                              _ptr(pts, torch.float64, "pts"), n, _ptr(regions, torch.float64, "regions"),
                              _ptr(kinds, torch.int32, "kinds"), _ptr(tile_of, torch.int32, "tile_of"), K, int(rule),
                              float(fill), _ptr(out, None, "out"), _ptr(cover, torch.int32, "cover"), _stream())
    _check(rc, "sn_scan_merge")


# --------------------------------------------------------------------------- #
def knn_chunk_points() -> int:
    """sn_knn_chunk_points: rows per workgroup of the neighbour kernels and per partial of their statistics (host only)."""
    return int(load().sn_knn_chunk_points())


def knn_ws_bytes(total: int, B: int, cells_per_tile: int) -> int:
    """sn_knn_ws_bytes: scratch bytes of knn_points / knn_tile_stats over `total` rows in B tiles (host only)."""
    need = int(load().sn_knn_ws_bytes(int(total), int(B), int(cells_per_tile)))
    if need == 0:
        raise HipLibraryError(f"sn_knn_points serves no batch of {total} rows in {B} tiles on {cells_per_tile} cells per tile "
                              "(1 <= total < 2^31, B * cells <= 2^22)")
    return need


@_on_tensor_device
def knn_points(pts: torch.Tensor, offsets: torch.Tensor, radius: float, k: int, lo: torch.Tensor, dims: Sequence[int], mult: int,
               ws: torch.Tensor, d2: torch.Tensor, found: torch.Tensor, mean_dist: Optional[torch.Tensor] = None,
               index: Optional[torch.Tensor] = None, exclude_zero: bool = False,
               launches: Optional[Tuple[int, int]] = None) -> None:
    """sn_knn_points: pts [total,3] f64, offsets [B+1] i64, lo [B,3] f64 -> d2 [total,k] f64, found [total] i32, mean_dist
    [total] f64 | None, index [total,k] i64 | None, all caller-owned like the scratch `ws` (knn_ws_bytes).  dims, mult: the
    grid (dbscan_cell_grid).  launches = (first, last): only those of the SN_KNN_LAUNCHES launches
    (sn_knn_points_launches: timing).  No allocation, no synchronisation."""
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise HipLibraryError(f"pts must be [n, 3] (got {tuple(pts.shape)})")
    total, B, k = int(pts.shape[0]), int(offsets.numel()) - 1, int(k)
    if lo.numel() != 3 * B or d2.numel() != total * k or found.numel() != total or \
            (mean_dist is not None and mean_dist.numel() != total) or (index is not None and index.numel() != total * k):
        raise HipLibraryError("lo / d2 / found / mean_dist / index do not have the sizes of this call")
    head = (_ptr(pts, torch.float64, "pts"), _ptr(offsets, torch.int64, "offsets"), total, B, float(radius), k,
            SN_KNN_EXCLUDE_ZERO if exclude_zero else 0, _ptr(lo, torch.float64, "lo"), int(dims[0]), int(dims[1]), int(dims[2]),
            int(mult), _ptr(ws, None, "ws"), ws.numel() * ws.element_size(), _ptr(d2, torch.float64, "d2"),
            _ptr(found, torch.int32, "found"), _ptr(mean_dist, torch.float64, "mean_dist"), _ptr(index, torch.int64, "index"))
    if launches is None:
        rc = load().sn_knn_points(*head, _stream())
    else:
        rc = load().sn_knn_points_launches(*head, int(launches[0]), int(launches[1]), _stream())
    _check(rc, "sn_knn_points")


@_on_tensor_device
def knn_tile_stats(mean_dist: torch.Tensor, found: torch.Tensor, offsets: torch.Tensor, k: int, ws: torch.Tensor,
                   stats: torch.Tensor) -> None:
    """sn_knn_tile_stats: mean_dist [total] f64 and found [total] i32 of knn_points -> stats [B, SN_KNN_NSTAT] f64 (n_valid,
    n_full, sum, sum_sq, max per tile) in a fixed order.  No allocation, no synchronisation."""
    total, B = int(found.numel()), int(offsets.numel()) - 1
    if mean_dist.numel() != total or stats.numel() != B * SN_KNN_NSTAT:
        raise HipLibraryError("mean_dist / stats do not have the sizes of this call")
    rc = load().sn_knn_tile_stats(_ptr(mean_dist, torch.float64, "mean_dist"), _ptr(found, torch.int32, "found"),
                                  _ptr(offsets, torch.int64, "offsets"), total, B, int(k), _ptr(ws, None, "ws"),
                                  ws.numel() * ws.element_size(), _ptr(stats, torch.float64, "stats"), _stream())
    _check(rc, "sn_knn_tile_stats")


# --------------------------------------------------------------------------- #
def shape_chunk_points() -> int:
    """sn_shape_chunk_points: rows per workgroup of the shape kernels (host only)."""
    return int(load().sn_shape_chunk_points())


def shape_ws_bytes(total: int, B: int, cells_per_tile: int) -> int:
    """sn_shape_ws_bytes: scratch bytes of shape_points over `total` rows in B tiles (host only)."""
    need = int(load().sn_shape_ws_bytes(int(total), int(B), int(cells_per_tile)))
    if need == 0:
        raise HipLibraryError(f"sn_shape_points serves no batch of {total} rows in {B} tiles on {cells_per_tile} cells per "
                              "tile (1 <= total <= 2^30, B * cells <= 2^22)")
    return need


@_on_tensor_device
def shape_points(pts: torch.Tensor, offsets: torch.Tensor, radius: float, min_points: int, lo: torch.Tensor,
                 dims: Sequence[int], mult: int, ws: torch.Tensor, count: torch.Tensor,
                 moments: Optional[torch.Tensor] = None, eig: Optional[torch.Tensor] = None,
                 normal: Optional[torch.Tensor] = None, axis: Optional[torch.Tensor] = None,
                 feat: Optional[torch.Tensor] = None, launches: Optional[Tuple[int, int]] = None) -> None:
    """sn_shape_points: pts [total,3] f64, offsets [B+1] i64, lo [B,3] f64 -> count [total] i32 and, each or None, moments
    [total,9] i64, eig / normal / axis [total,3] f64, feat [total,SN_SHAPE_NFEAT] f64, all caller-owned like the scratch
    `ws` (shape_ws_bytes).  dims, mult: the grid (dbscan_cell_grid).  launches = (first, last): only those of the
    SN_SHAPE_LAUNCHES launches (sn_shape_points_launches: timing).  No allocation, no synchronisation."""
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise HipLibraryError(f"pts must be [n, 3] (got {tuple(pts.shape)})")
    total, B = int(pts.shape[0]), int(offsets.numel()) - 1
    sizes = ((count, total), (moments, total * 9), (eig, total * 3), (normal, total * 3), (axis, total * 3),
             (feat, total * SN_SHAPE_NFEAT))
    if lo.numel() != 3 * B or any(t is not None and t.numel() != n for t, n in sizes):
        raise HipLibraryError("lo / count / moments / eig / normal / axis / feat do not have the sizes of this call")
    head = (_ptr(pts, torch.float64, "pts"), _ptr(offsets, torch.int64, "offsets"), total, B, float(radius), int(min_points), 0,
            _ptr(lo, torch.float64, "lo"), int(dims[0]), int(dims[1]), int(dims[2]), int(mult), _ptr(ws, None, "ws"),
            ws.numel() * ws.element_size(), _ptr(count, torch.int32, "count"), _ptr(moments, torch.int64, "moments"),
            _ptr(eig, torch.float64, "eig"), _ptr(normal, torch.float64, "normal"), _ptr(axis, torch.float64, "axis"),
            _ptr(feat, torch.float64, "feat"))
    if launches is None:
        rc = load().sn_shape_points(*head, _stream())
    else:
        rc = load().sn_shape_points_launches(*head, int(launches[0]), int(launches[1]), _stream())
    _check(rc, "sn_shape_points")


# --------------------------------------------------------------------------- #
def render_chunk_points() -> int:
    """sn_render_chunk_points: rows per workgroup of the splat kernel (host only)."""
    return int(load().sn_render_chunk_points())


@_on_tensor_device
def render_splat(pts: torch.Tensor, offsets: torch.Tensor, cam: torch.Tensor, view_tile: torch.Tensor, size: Sequence[int],
                 keys: torch.Tensor, count: Optional[torch.Tensor], bad_views: torch.Tensor, accumulate: bool = False,
                 look: Optional[bool] = None) -> None:
    """sn_render_splat: pts [total,3] f64, offsets [B+1] i64, cam [K,16] f64, view_tile [K] i32, size (H, W) -> keys [K,H,W]
    (int64 storage of the u64 keys), count [K,H,W] i32 | None (the u32 counts), bad_views [K] i32, all caller-owned.
    accumulate: composite onto what they hold.  look: None looks at a pixel before the atomic where the point size is >= 2,
    True at every size, False at none (same result; for timing).  No allocation, no synchronisation."""
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise HipLibraryError(f"pts must be [total, 3] (got {tuple(pts.shape)})")
    total, B = int(pts.shape[0]), int(offsets.numel()) - 1
    H, W = (int(v) for v in size)
    if cam.dim() != 2 or cam.shape[1] != 16:
        raise HipLibraryError(f"cam must be [K, 16] (got {tuple(cam.shape)})")
    K = int(cam.shape[0])
    if view_tile.numel() != K or bad_views.numel() != K:
        raise HipLibraryError(f"view_tile and bad_views must hold K = {K} entries")
    if keys.numel() != K * H * W or (count is not None and count.numel() != K * H * W):
        raise HipLibraryError(f"keys and count must hold K * H * W = {K * H * W} pixels")
    flags = (SN_RENDER_ACCUMULATE if accumulate else 0) | (0 if look is None else SN_RENDER_LOOK_ALWAYS if look else SN_RENDER_NO_LOOK)
    rc = load().sn_render_splat(_ptr(pts, torch.float64, "pts"), _ptr(offsets, torch.int64, "offsets"), total, B,
                                _ptr(cam, torch.float64, "cam"), _ptr(view_tile, torch.int32, "view_tile"), K, H, W, flags,
                                _ptr(keys, torch.int64, "keys"), _ptr(count, torch.int32, "count"),
                                _ptr(bad_views, torch.int32, "bad_views"), _stream())
    _check(rc, "sn_render_splat")


@_on_tensor_device
def render_resolve(keys: torch.Tensor, size: Sequence[int], offsets: torch.Tensor, view_tile: torch.Tensor,
                   rgb16: Optional[torch.Tensor], mode: int, background: Sequence[int], edl: float, rgba: torch.Tensor,
                   index: Optional[torch.Tensor] = None, depth_q: Optional[torch.Tensor] = None) -> None:
    """sn_render_resolve on the keys sn_render_splat left: -> rgba [K,H,W,4] u8, index [K,H,W] i64 | None, depth_q [K,H,W]
    i32 | None (the u32 quanta), caller-owned.  rgb16 [total,3] u16 (int16 storage serves; None in SN_RENDER_DEPTH mode);
    background (r, g, b, a) bytes.  No allocation, no synchronisation."""
    H, W = (int(v) for v in size)
    K, B = int(view_tile.numel()), int(offsets.numel()) - 1
    if keys.numel() != K * H * W or rgba.numel() != 4 * K * H * W:
        raise HipLibraryError(f"keys must hold K * H * W = {K * H * W} pixels and rgba four bytes for each")
    if any(t is not None and t.numel() != K * H * W for t in (index, depth_q)):
        raise HipLibraryError(f"index and depth_q must hold K * H * W = {K * H * W} pixels")
    bg = [int(v) for v in background]
    if len(bg) != 4 or any(v < 0 or v > 255 for v in bg):
        raise HipLibraryError(f"background must be four bytes (r, g, b, a) (got {tuple(background)})")
    rc = load().sn_render_resolve(_ptr(keys, torch.int64, "keys"), K, H, W, _ptr(offsets, torch.int64, "offsets"), B,
                                  _ptr(view_tile, torch.int32, "view_tile"), _u16_ptr(rgb16, "rgb16"), int(mode),
                                  bg[0] | (bg[1] << 8) | (bg[2] << 16) | (bg[3] << 24), float(edl),
                                  _ptr(rgba, torch.uint8, "rgba"), _ptr(index, torch.int64, "index"),
                                  _ptr(depth_q, torch.int32, "depth_q"), _stream())
    _check(rc, "sn_render_resolve")


# --------------------------------------------------------------------------- #
def voxel_pool_chunk_points() -> int:
    """sn_voxel_pool_chunk_points: rows per workgroup of the pooling kernel (host only)."""
    return int(load().sn_voxel_pool_chunk_points())


def voxel_pool_ws_bytes(B: int, n_xyz: Sequence[int], P: int) -> int:
    """sn_voxel_pool_ws_bytes: workspace bytes of voxel_pool (host only): 0, the call accumulates in its outputs."""
    nx, ny, nz = (int(v) for v in n_xyz)
    return int(load().sn_voxel_pool_ws_bytes(int(B), nx, ny, nz, int(P)))


@_on_tensor_device
def voxel_pool(pts: torch.Tensor, values: Optional[torch.Tensor], offsets: torch.Tensor, desc: torch.Tensor,
               n_xyz: Sequence[int], sources: Sequence[int], ops: Sequence[int],
               value_ranges: Optional[Sequence[Sequence[float]]], fill: float, out: torch.Tensor, counts: torch.Tensor,
               unbinned: torch.Tensor, nan_rows: torch.Tensor, look: bool = True) -> None:
    """sn_voxel_pool: pts [total,3] f64, values [total,C] f64 | None, offsets [B+1] i64, desc [B, desc_len]; plane p reduces
    source sources[p] (0, 1, 2: x, y, z; 3 + c: column c) with ops[p] (SN_POOL_MEAN / MIN / MAX); value_ranges [C] pairs (lo,
    hi) on the host, read for the columns a MEAN plane reads -> out [B,P,nz,nx,ny] f64, counts [B,nz,nx,ny] i32, unbinned [B]
    i64, nan_rows [B] i64, all caller-owned; the accumulators live in out and counts themselves.  look=False sends every min /
    max atomic (same result; for timing).  No allocation, no synchronisation."""
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise HipLibraryError(f"pts must be [total, 3] (got {tuple(pts.shape)})")
    total, B = int(pts.shape[0]), int(offsets.numel()) - 1
    nx, ny, nz = (int(v) for v in n_xyz)
    P = len(sources)
    if len(ops) != P:
        raise HipLibraryError("sources and ops disagree in length")
    C = 0
    if values is not None:
        if values.dim() != 2 or int(values.shape[0]) != total:
            raise HipLibraryError(f"values must be [total, C] = [{total}, C] (got {tuple(values.shape)})")
        C = int(values.shape[1])
    if tuple(desc.shape) != (B, desc_len(nx, ny, nz)):
        raise HipLibraryError(f"desc must be [B, desc_len(nx, ny, nz)] = [{B}, {desc_len(nx, ny, nz)}] "
                              f"(got {tuple(desc.shape)})")
    V = nx * ny * nz
    if out.numel() != B * P * V or counts.numel() != B * V or unbinned.numel() != B or nan_rows.numel() != B:
        raise HipLibraryError("out must hold B * P * nz * nx * ny cells, counts B * nz * nx * ny, unbinned and nan_rows B")
    src = (ctypes.c_int32 * max(P, 1))(*[int(v) for v in sources])
    op = (ctypes.c_int32 * max(P, 1))(*[int(v) for v in ops])
    rng = None
    if value_ranges is not None:
        flat = [float(v) for pair in value_ranges for v in pair]
        if len(flat) != 2 * C:
            raise HipLibraryError(f"value_ranges must hold C = {C} pairs (lo, hi)")
        rng = (ctypes.c_double * max(len(flat), 1))(*flat)
    rc = load().sn_voxel_pool(_ptr(pts, torch.float64, "pts"), _ptr(values, torch.float64, "values"), C,
                              _ptr(offsets, torch.int64, "offsets"), total, B, _ptr(desc, torch.float64, "desc"), nx, ny, nz,
                              ctypes.cast(src, c_void_p), ctypes.cast(op, c_void_p), P,
                              None if rng is None else ctypes.cast(rng, c_void_p), float(fill),
                              0 if look else SN_VOXEL_POOL_NO_LOOK, None, _ptr(out, torch.float64, "out"),
                              _ptr(counts, torch.int32, "counts"), _ptr(unbinned, torch.int64, "unbinned"),
                              _ptr(nan_rows, torch.int64, "nan_rows"), _stream())
    _check(rc, "sn_voxel_pool")
