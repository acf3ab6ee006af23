"""scene-net_amd -- MI355X-native SCENE-Net GENEO forward path (voxelise -> GENEO bank -> 3D conv -> head).

Only what the hot path needs: `csrc/` (hand-written HIP for gfx950 behind the C ABI of
include/scenenet_hip.h) and the host-side mirror of the reference's operator interface.
Import as `scene_net_amd` (shim package at the repo root).
"""
from . import _hip
from ._hip import HipLibraryError, LIB_PATH
from .geneos import (GENEO_kernel_torch, arrow, cone_kernel, cylinder_kernel, cylinderv2, neg_sphere_kernel,
                     negSpherev2)
from .scene_net import GENEO_Layer, SCENE_Net, SCENE_Net_Class, SCENENetQuantile, SceneNet
from .transforms import ToFullDense, ToTensor, Voxelization, xyz_ToFullDense, xyz_Voxelization
from .voxelization import (PointBatch, VoxelGrids, hist_on_voxel, prob_to_label, reg_on_voxel, voxelize_batch,
                           vxg_to_xyz)
from .pipeline import CapturedPipeline, ScenePipeline, shard_range
from .tiles import TS40KTiles, batch_to_device, pack_csr, point_predictions, split_tile
from .stream import TileRing, TileStream, scan_tiles
from .training import CapturedTrainingStep, allreduce_flat_grads
from .metrics import BinarySegmentationCurve, BinarySegmentationMetrics, init_metrics
from .towers import TowerProposals, aggregate_centroids, filter_towers, tower_proposals
from .tower_score import (TowerCentroids, TowerDetectionMetrics, TowerMatches, compute_euc_dists, get_tower_proposals,
                          tower_centroids, tower_detection_values)
from .crops import (ScanCrops, crop_at_locations, crop_regions, crop_tower_radius, crop_tower_samples, crop_two_towers,
                    lattice_regions, merge_to_scan)
from .scan_merge import ScanSegmentation, classify_las, scan_predictions, segment_scan
from .clusters import PointClusters, cluster_points, crop_two_towers_samples, extract_towers, select_object
from .census import (RegionCensus, accept_kinds, crop_accepted, crop_ground_samples, crop_pole_slabs, pole_radius_samples,
                     region_census, scan_has_class, slab_regions, watch_equal, watch_trunc)
from .las import (LasHeader, LasReader, LasScan, build_data_samples, las_to_numpy, plan_chunks, read_las, read_las_header,
                  split_slices)
from .las_write import LasWriter, LasWritten, las_header_bytes, reclassify_las, write_las
from .kitti import (KittiReader, KittiScans, build_pole_radius_samples, build_pole_samples, kitti_scan_lists, lut_array,
                    read_kitti_scan, semKITTI)
from .voxel_cloud import (VoxelCloud, jet_ranges, plot_quantile_uncertainty, plot_voxelgrid, voxel_cloud,
                          write_voxel_cloud_las)
from .thin import (ThinnedPoints, ThinPoints, downsampling, downsampling_relative_height, height_thresholds,
                   philox_uniforms, thin_points, uniform_thresholds)
from .voxel_classes import (ClassColors, VoxelClasses, class_colors, classes_on_voxel, color_pointcloud,
                            random_class_colors, voxel_classes)
from .neighbours import (PointNeighbours, avg_dist_points, k_distance_curve, knn_distances, point_spacing,
                         remove_outliers)
from .shapes import PointShapes, estimate_normals, select_by_shape, shape_colors, shape_features
from .render import (RenderedViews, default_class_table, ortho_camera, perspective_camera, png_bytes, render_points,
                     render_pred_vs_gt, render_scan, render_voxelgrid, write_png)
from .voxel_pool import (VoxelPool, centroid_hist_on_voxel, centroid_reg_on_voxel, voxel_centroids, voxel_downsample,
                         voxel_pool)
from .criterions import (BinaryDiceLoss, BinaryDiceLoss_BCE, FocalLoss, FocalTverskyLoss, GENEO_Dice_BCE, GENEO_Dice_Loss,
                         GENEO_Loss, GENEO_Tversky_Loss, IoULoss, QuantileGENEOLoss, QuantileLoss, TverskyLoss, WeightedMSE)

__all__ = ["SceneNet", "SCENE_Net", "SCENENetQuantile", "SCENE_Net_Class", "cylinder_kernel", "cone_kernel",
           "neg_sphere_kernel", "GENEO_Layer", "GENEO_kernel_torch", "cylinderv2", "arrow", "negSpherev2", "Voxelization",
           "ToTensor", "ToFullDense", "hist_on_voxel", "reg_on_voxel", "prob_to_label", "vxg_to_xyz", "voxelize_batch",
           "PointBatch", "VoxelGrids", "ScenePipeline", "CapturedPipeline", "CapturedTrainingStep", "allreduce_flat_grads", "shard_range", "TS40KTiles", "batch_to_device", "pack_csr",
           "point_predictions", "split_tile", "TileStream", "TileRing", "scan_tiles", "BinarySegmentationMetrics", "BinarySegmentationCurve", "init_metrics", "TowerProposals", "tower_proposals", "filter_towers", "aggregate_centroids", "TowerCentroids", "TowerMatches", "TowerDetectionMetrics",
           "tower_centroids", "get_tower_proposals", "compute_euc_dists", "tower_detection_values", "ScanCrops", "crop_regions", "crop_at_locations",
           "crop_tower_radius", "crop_two_towers", "crop_tower_samples", "lattice_regions", "merge_to_scan", "ScanSegmentation", "scan_predictions", "segment_scan", "classify_las", "PointClusters", "cluster_points", "select_object", "extract_towers",
           "crop_two_towers_samples", "RegionCensus", "region_census", "watch_equal", "watch_trunc", "accept_kinds", "crop_accepted",
           "slab_regions", "crop_ground_samples", "crop_pole_slabs", "pole_radius_samples", "scan_has_class", "LasHeader", "LasReader", "LasScan",
           "read_las_header", "read_las", "las_to_numpy", "build_data_samples", "plan_chunks", "split_slices", "LasWriter", "LasWritten",
           "las_header_bytes", "write_las", "reclassify_las", "KittiReader", "KittiScans",
           "VoxelCloud", "voxel_cloud", "plot_voxelgrid", "plot_quantile_uncertainty", "jet_ranges", "write_voxel_cloud_las",
           "ThinnedPoints", "ThinPoints", "thin_points", "downsampling", "downsampling_relative_height", "height_thresholds",
           "uniform_thresholds", "philox_uniforms",
           "VoxelClasses", "ClassColors", "voxel_classes", "classes_on_voxel", "class_colors", "color_pointcloud",
           "random_class_colors", "PointNeighbours", "knn_distances", "point_spacing", "k_distance_curve", "remove_outliers",
           "avg_dist_points", "PointShapes", "shape_features", "estimate_normals", "select_by_shape", "shape_colors",
           "RenderedViews", "ortho_camera", "perspective_camera", "render_points", "render_scan", "render_voxelgrid",
           "render_pred_vs_gt", "png_bytes", "write_png", "default_class_table",
           "VoxelPool", "voxel_pool", "voxel_centroids", "centroid_hist_on_voxel", "centroid_reg_on_voxel", "voxel_downsample",
           "xyz_Voxelization", "xyz_ToFullDense",
           "read_kitti_scan", "kitti_scan_lists", "semKITTI", "build_pole_samples", "build_pole_radius_samples", "lut_array", "HipLibraryError", "LIB_PATH", "WeightedMSE", "GENEO_Loss",
           "GENEO_Tversky_Loss", "GENEO_Dice_Loss", "GENEO_Dice_BCE", "TverskyLoss", "FocalTverskyLoss", "BinaryDiceLoss",
           "BinaryDiceLoss_BCE", "QuantileLoss", "QuantileGENEOLoss", "FocalLoss", "IoULoss"]
