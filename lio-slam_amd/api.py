"""ctypes binding of include/liogpu.h -- one Python method per C entry point.

Method names follow the reference's member functions where one exists
(mapOptimization::scan2MapOptimization MO:1839, transformUpdate MO:1867,
ImageProjection::projectPointCloud IP:577, FeatureExtraction::calculateSmoothness
FE:81) so the parity tests read like tests of the reference's own classes.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIO_MAX_ITERS = 32
STATUS_NAMES = {0: "OK", 1: "TOO_FEW_POINTS", 2: "TOO_FEW_CORR", -1: "ERR_ARG", -2: "ERR_HIP",
                -3: "ERR_CAPACITY", -4: "ERR_NO_MAP", -5: "ERR_NO_DEVICE"}


class LioError(RuntimeError):
    pass


class S2MConfig(C.Structure):
    _fields_ = [
        ("k", C.c_int32), ("max_sq_dist", C.c_float),
        ("plane_tol", C.c_double), ("weight", C.c_double), ("min_s", C.c_double),
        ("min_corr", C.c_int32), ("max_iters", C.c_int32), ("eig_thresh", C.c_float),
        ("conv_deg", C.c_double), ("conv_cm", C.c_double),
        ("min_scan_pts", C.c_int32), ("jacobian_mode", C.c_int32), ("force_all_iters", C.c_int32),
        ("device_id", C.c_int32), ("cell_size", C.c_float), ("max_batch", C.c_int32),
        ("max_scan_pts", C.c_int32), ("record_corr_iter", C.c_int32), ("kernel_variant", C.c_int32),
        ("profile", C.c_int32), ("lookahead", C.c_int32), ("use_lds", C.c_int32), ("sort_scan", C.c_int32),
        ("cell_div", C.c_int32), ("xcd_remap", C.c_int32), ("tile_size", C.c_float),
        ("use_graph", C.c_int32), ("graph_iters", C.c_int32), ("sort_batch", C.c_int32), ("nn_cache", C.c_int32),
        ("pipeline", C.c_int32), ("n_devices", C.c_int32), ("device_ids", C.c_int32 * 8), ("x_sub", C.c_int32), ("tight_rows", C.c_int32),
    ]


class GridPlanInfo(C.Structure):
    _fields_ = [
        ("origin", C.c_float * 3), ("inv_cell", C.c_float),
        ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("n_cells", C.c_int32), ("k", C.c_int32), ("xs", C.c_int32), ("nxf", C.c_int32),
        ("inv_cell_x", C.c_float),
        ("tb_row0", C.c_int32 * 3), ("tb_ny", C.c_int32 * 3), ("tb_nz", C.c_int32 * 3),
        ("tb_oy", C.c_float * 3), ("tb_oz", C.c_float * 3), ("tb_inv_cell", C.c_float * 3), ("tb_reach", C.c_float * 3),
        ("tb_try", C.c_int32), ("tb_try_b2", C.c_float * 3),
        ("cell", C.c_float), ("n_tb", C.c_int32), ("grow_steps", C.c_int32), ("want_occupancy", C.c_int32),
        ("pts_per_cell", C.c_float), ("buckets", C.c_int64),
    ]


class S2MResult(C.Structure):
    _fields_ = [
        ("status", C.c_int32), ("iters", C.c_int32), ("converged", C.c_int32),
        ("is_degenerate", C.c_int32), ("n_corr_last", C.c_int32),
        ("n_corr_iter", C.c_int32 * LIO_MAX_ITERS),
        ("matP", C.c_float * 36), ("AtA", C.c_float * 36), ("AtB", C.c_float * 6),
        ("pose_iter", (C.c_float * 6) * LIO_MAX_ITERS),
    ]


class S2MProfile(C.Structure):
    _fields_ = [
        ("map_build_ms", C.c_float), ("map_upload_ms", C.c_float), ("n_launches", C.c_int32),
        ("n_units", C.c_int32), ("unit_iters", C.c_int32),
        ("launch_ms", C.c_float * LIO_MAX_ITERS), ("launch_active", C.c_int32 * LIO_MAX_ITERS),
        ("point_iters", C.c_int64),
        ("n_map", C.c_int64), ("n_cells", C.c_int64),
        ("pipeline", C.c_int32), ("multi_iterations", C.c_int32), ("multi_stream_syncs", C.c_int32),
        ("multi_event_waits", C.c_int32), ("multi_exchange", C.c_int32), ("persist_fallbacks", C.c_int32),
        ("map_x_sub", C.c_int32), ("map_tight_tables", C.c_int32), ("map_first_try", C.c_int32), ("map_pts_per_cell", C.c_float),
    ]


class DeskewConfig(C.Structure):
    _fields_ = [
        ("N_SCAN", C.c_int32), ("downsampleRate", C.c_int32), ("point_filter_num", C.c_int32),
        ("lidarMinFront", C.c_float), ("lidarMinBack", C.c_float),
        ("lidarMinLeft", C.c_float), ("lidarMinRight", C.c_float),
        ("lidarMaxRange", C.c_float), ("lidarMaxIntensity", C.c_float),
        ("deskew_flag", C.c_int32), ("device_id", C.c_int32),
    ]


class RangeImageConfig(C.Structure):
    _fields_ = [("N_SCAN", C.c_int32), ("Horizon_SCAN", C.c_int32), ("downsampleRate", C.c_int32),
                ("lidarMinRange", C.c_float), ("lidarMaxRange", C.c_float), ("deskew_flag", C.c_int32),
                ("device_id", C.c_int32)]


class PC2Layout(C.Structure):
    """Field layout of a sensor_msgs/PointCloud2 (include/liogpu.h lio_pc2_layout)."""
    _fields_ = [("point_step", C.c_uint32), ("off_x", C.c_uint32), ("off_intensity", C.c_int32), ("off_ring", C.c_int32),
                ("ring_type", C.c_int32), ("off_time", C.c_int32), ("time_type", C.c_int32), ("pin_host", C.c_int32)]


PC2_UINT8, PC2_UINT16, PC2_INT32 = 2, 4, 5
PC2_TIME_F32_SECONDS, PC2_TIME_U32_NS, PC2_TIME_U32_RAW, PC2_TIME_F64_STAMP = 0, 1, 2, 3


class NearbyConfig(C.Structure):
    """extractNearby's parameters (include/liogpu.h lio_nearby_config)."""
    _fields_ = [("search_radius", C.c_float), ("pose_density", C.c_float), ("recent_window_s", C.c_double)]


class FeatureConfig(C.Structure):
    _fields_ = [("N_SCAN", C.c_int32), ("edgeThreshold", C.c_float), ("surfThreshold", C.c_float),
                ("surfLeafSize", C.c_float), ("device_id", C.c_int32)]


class IcpConfig(C.Structure):
    """pcl::IterativeClosestPoint as MO:1110-1116 sets it up (include/liogpu.h lio_icp_config)."""
    _fields_ = [("max_corr_dist", C.c_double), ("transform_eps", C.c_double), ("fitness_eps", C.c_double),
                ("rel_mse_eps", C.c_double), ("rotation_threshold", C.c_double), ("fitness_max", C.c_double),
                ("max_iters", C.c_int32), ("min_corr", C.c_int32), ("max_similar", C.c_int32),
                ("min_source_points", C.c_int32), ("min_target_points", C.c_int32), ("lookahead", C.c_int32)]


class IcpResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("converged", C.c_int32), ("state", C.c_int32), ("iters", C.c_int32),
                ("n_corr_last", C.c_int32), ("accepted", C.c_int32), ("n_source", C.c_int32), ("n_target", C.c_int32),
                ("n_launches", C.c_int32), ("pad", C.c_int32), ("fitness", C.c_double), ("T", C.c_float * 16),
                ("pose_corrected", C.c_float * 6)]


class IcpGridInfo(C.Structure):
    """The search grid of an alignment's target (include/liogpu.h lio_icp_grid_info)."""
    _fields_ = [("origin", C.c_float * 3), ("edge", C.c_float), ("inv_cell", C.c_float), ("nx", C.c_int32), ("ny", C.c_int32),
                ("nz", C.c_int32), ("n_cells", C.c_int32), ("occupied", C.c_int32), ("any", C.c_int32)]


class IcpClouds(C.Structure):
    _fields_ = [("source", C.c_void_p), ("target", C.c_void_p), ("closed", C.c_void_p),
                ("cap_source", C.c_size_t), ("cap_target", C.c_size_t), ("cap_closed", C.c_size_t),
                ("n_source", C.c_size_t), ("n_target", C.c_size_t), ("n_closed", C.c_size_t), ("stride", C.c_size_t)]


SC_MAX_CANDIDATES = 16


class ScConfig(C.Structure):
    """SCManager's constants, Scancontext.h:80-99 (include/liogpu.h lio_sc_config)."""
    _fields_ = [("max_radius", C.c_double), ("lidar_height", C.c_double), ("search_ratio", C.c_double), ("dist_thres", C.c_double),
                ("num_rings", C.c_int32), ("num_sectors", C.c_int32), ("num_exclude_recent", C.c_int32),
                ("num_candidates", C.c_int32), ("tree_period", C.c_int32), ("pad", C.c_int32)]


class ScResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("loop_id", C.c_int32), ("align", C.c_int32), ("nn_idx", C.c_int32),
                ("n_searched", C.c_int32), ("n_candidates", C.c_int32), ("yaw_diff_rad", C.c_float), ("pad", C.c_int32),
                ("min_dist", C.c_double), ("cand_idx", C.c_int32 * SC_MAX_CANDIDATES), ("cand_ring_d2", C.c_float * SC_MAX_CANDIDATES),
                ("cand_dist", C.c_double * SC_MAX_CANDIDATES), ("cand_align", C.c_int32 * SC_MAX_CANDIDATES)]


class LocalMapConfig(C.Structure):
    """publishLocalMap's parameters, UT:219-229 (include/liogpu.h lio_local_map_config)."""
    _fields_ = [("n_keyframes", C.c_int32), ("front", C.c_float), ("left", C.c_float), ("back", C.c_float), ("right", C.c_float),
                ("remove_outliers", C.c_int32), ("mean_k", C.c_int32), ("stddev_mul", C.c_float), ("downsample", C.c_int32),
                ("leaf", C.c_float)]


class LocalMapInfo(C.Structure):
    _fields_ = [("first_keyframe", C.c_int32), ("n_keyframes", C.c_int32), ("n_summed", C.c_int32), ("n_cropped", C.c_int32),
                ("n_inliers", C.c_int32), ("n_out", C.c_int32), ("voxel_passthrough", C.c_int32), ("pad", C.c_int32),
                ("sor_mean", C.c_double), ("sor_stddev", C.c_double), ("sor_threshold", C.c_double)]


class HeightMapConfig(C.Structure):
    """grid_map_pcl's config/parameters.yaml and the node's roll / pitch (include/liogpu.h lio_height_map_config)."""
    _fields_ = [("roll", C.c_float), ("pitch", C.c_float), ("level_and_ego_filter", C.c_int32), ("remove_outliers", C.c_int32),
                ("mean_k", C.c_int32), ("stddev_mul", C.c_float), ("downsample", C.c_int32), ("voxel", C.c_float * 3),
                ("resolution", C.c_double), ("min_points_per_cell", C.c_int32), ("max_points_per_cell", C.c_int32),
                ("use_cluster", C.c_int32), ("cluster_tolerance", C.c_float), ("cluster_min_points", C.c_int32),
                ("cluster_max_points", C.c_int32), ("use_max_height", C.c_int32), ("fill_holes", C.c_int32)]


class HeightMapInfo(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("length", C.c_double * 2), ("position", C.c_double * 2),
                ("n_in", C.c_int32), ("n_inliers", C.c_int32), ("n_filtered", C.c_int32), ("n_binned", C.c_int32),
                ("n_valid_cells", C.c_int32), ("n_filled_cells", C.c_int32), ("voxel_passthrough", C.c_int32), ("pad", C.c_int32)]


TERRAIN_LAYERS = ("smooth", "normal_x", "normal_y", "normal_z", "slope", "roughness", "edges", "traversability")   # LIO_TERRAIN_*


class TerrainConfig(C.Structure):
    """grid_map_demos' filters_demo_filter_chain.yaml behind elevation_inpainted (include/liogpu.h lio_terrain_config)."""
    _fields_ = [("normal_method", C.c_int32), ("normal_axis", C.c_int32), ("normal_radius", C.c_double), ("smooth_radius", C.c_double),
                ("edge_window_size", C.c_int32), ("edge_window_length", C.c_double), ("slope_critical", C.c_float),
                ("roughness_critical", C.c_float), ("slope_weight", C.c_float), ("roughness_weight", C.c_float), ("layers", C.c_uint32)]


class TerrainInfo(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("n_valid_cells", C.c_int32), ("normal_method_used", C.c_int32),
                ("n_normal_cells", C.c_int32), ("n_few_points", C.c_int32), ("n_degenerate", C.c_int32), ("edge_window_size", C.c_int32)]


class GlobalMapConfig(C.Structure):
    """publishGlobalMap's parameters, globalMapVisualization* of the yaml files (include/liogpu.h lio_global_map_config)."""
    _fields_ = [("search_radius", C.c_float), ("pose_density", C.c_float), ("leaf", C.c_float)]


class GlobalMapInfo(C.Structure):
    _fields_ = [("n_keyframes", C.c_int32), ("n_summed", C.c_int32), ("n_out", C.c_int32), ("voxel_passthrough", C.c_int32)]


class ExportConfig(C.Structure):
    """saveMapService's resolution and the transfer chunk (include/liogpu.h lio_export_config)."""
    _fields_ = [("resolution", C.c_float), ("chunk_points", C.c_int32)]


class OgmConfig(C.Structure):
    """The parameters of the fork's draft ogmGeneration.cpp (include/liogpu.h lio_ogm_config)."""
    _fields_ = [("z_min", C.c_float), ("z_max", C.c_float), ("z_negative", C.c_int32), ("remove_outliers", C.c_int32),
                ("radius", C.c_float), ("min_neighbors", C.c_int32), ("resolution", C.c_double), ("whole_box", C.c_int32)]


class OgmInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("origin", C.c_double * 2), ("n_in", C.c_int32), ("n_slice", C.c_int32),
                ("n_inliers", C.c_int32), ("n_binned", C.c_int32), ("n_occupied", C.c_int32), ("pad", C.c_int32)]


class SdfConfig(C.Structure):
    """grid_map_sdf's band and what to do with a non-finite cell (include/liogpu.h lio_sdf_config)."""
    _fields_ = [("min_height", C.c_double), ("max_height", C.c_double), ("nan_policy", C.c_int32), ("pad", C.c_int32)]


class SdfInfo(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("layers", C.c_int32), ("n_nan", C.c_int32), ("origin", C.c_double * 3),
                ("resolution", C.c_double), ("layer_min", C.c_float), ("layer_max", C.c_float), ("n_all_obstacle", C.c_int32),
                ("n_all_free", C.c_int32), ("n_mixed", C.c_int32), ("pad", C.c_int32)]


class MedianFillConfig(C.Structure):
    """grid_map_filters' MedianFillFilter parameters (include/liogpu.h lio_median_fill_config)."""
    _fields_ = [("fill_hole_radius", C.c_double), ("existing_value_radius", C.c_double), ("filter_existing_values", C.c_int32),
                ("num_erode_dilation_iterations", C.c_int32)]


class MedianFillInfo(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("fill_radius_cells", C.c_int32), ("existing_radius_cells", C.c_int32),
                ("n_nan_in", C.c_int32), ("n_mask", C.c_int32), ("n_filled", C.c_int32), ("n_filtered", C.c_int32),
                ("n_nan_out", C.c_int32), ("pad", C.c_int32)]


class PlanningMapBuffers(C.Structure):
    """the host buffers of lio_kf_store_planning_map, each with its capacity in floats (lio_planning_map_buffers)"""
    _fields_ = [("grid", C.c_void_p), ("grid_cap", C.c_size_t), ("filled", C.c_void_p), ("filled_cap", C.c_size_t),
                ("fill_mask", C.c_void_p), ("fill_mask_cap", C.c_size_t), ("layers", C.c_void_p), ("layers_cap", C.c_size_t)]


class GridSampleConfig(C.Structure):
    """GridMap::atPosition's interpolation method and the border mode (include/liogpu.h lio_grid_sample_config)."""
    _fields_ = [("method", C.c_int32), ("border_mode", C.c_int32)]


class GridSampleInfo(C.Structure):
    _fields_ = [("n_outside", C.c_int64), ("n_method", C.c_int64 * 4)]


class GridInfo(C.Structure):
    """what lio_grid_info reports (include/liogpu.h lio_grid_desc)"""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("resolution", C.c_double), ("length", C.c_double * 2), ("position", C.c_double * 2),
                ("layer_mask", C.c_uint32), ("pad", C.c_int32)]


class GridRegion(C.Structure):
    """one region of lio_grid_region_reduce / lio_grid_region_cells (include/liogpu.h lio_grid_region)"""
    _fields_ = [("kind", C.c_int32), ("n_vertices", C.c_int32), ("first_vertex", C.c_int64), ("p", C.c_double * 5)]


class GridRegionConfig(C.Structure):
    _fields_ = [("threshold", C.c_float), ("pad", C.c_int32)]


class GridRegionStat(C.Structure):
    _fields_ = [("sum", C.c_double), ("min", C.c_float), ("max", C.c_float), ("n_finite", C.c_int32), ("n_below", C.c_int32)]


class GridRegionInfo(C.Structure):
    _fields_ = [("n_ok", C.c_int64), ("n_empty", C.c_int64), ("n_invalid", C.c_int64), ("n_cells", C.c_int64)]


GRID_REGION_DTYPE = np.dtype({"names": ["kind", "n_vertices", "first_vertex", "p"], "formats": [np.int32, np.int32, np.int64, (np.float64, 5)],
                              "offsets": [0, 4, 8, 16], "itemsize": 56})
GRID_REGION_STAT_DTYPE = np.dtype([("sum", np.float64), ("min", np.float32), ("max", np.float32), ("n_finite", np.int32), ("n_below", np.int32)])
# lio_grid_transform_info and lio_grid_occupancy_desc of include/liogpu.h, one record each (tests/test_grid_transform_capi.py
# holds the layouts to gcc's)
GRID_TRANSFORM_INFO_DTYPE = np.dtype({"names": ["rows", "cols", "length", "position", "n_source_cells", "n_samples_outside", "n_cells_written"],
                                      "formats": [np.int32, np.int32, (np.float64, 2), (np.float64, 2), np.int64, np.int64, np.int64],
                                      "offsets": [0, 4, 8, 24, 40, 48, 56], "itemsize": 64})
GRID_OCCUPANCY_DESC_DTYPE = np.dtype({"names": ["width", "height", "resolution", "pad", "origin"],
                                      "formats": [np.uint32, np.uint32, np.float32, np.int32, (np.float64, 2)],
                                      "offsets": [0, 4, 8, 12, 16], "itemsize": 32})
GRID_TRANSFORM_MAX_SOURCE_CELLS = 429496729
# lio_grid_submap_info, lio_grid_move_info, lio_grid_extend_info and lio_grid_add_info (tests/test_grid_geom_capi.py holds the
# layouts to gcc's)
GRID_SUBMAP_INFO_DTYPE = np.dtype({"names": ["success", "rows", "cols", "pad", "length", "position", "top_left", "requested_index"],
                                   "formats": [np.int32, np.int32, np.int32, np.int32, (np.float64, 2), (np.float64, 2), (np.int32, 2), (np.int32, 2)],
                                   "offsets": [0, 4, 8, 12, 16, 32, 48, 56], "itemsize": 64})
GRID_MOVE_INFO_DTYPE = np.dtype({"names": ["moved", "pad", "index_shift", "position", "n_cells_cleared"],
                                 "formats": [np.int32, np.int32, (np.int32, 2), (np.float64, 2), np.int64], "offsets": [0, 4, 8, 16, 32], "itemsize": 40})
GRID_EXTEND_INFO_DTYPE = np.dtype({"names": ["resized", "rows", "cols", "pad", "length", "position", "n_cells_kept", "n_index_outside"],
                                   "formats": [np.int32, np.int32, np.int32, np.int32, (np.float64, 2), (np.float64, 2), np.int64, np.int64],
                                   "offsets": [0, 4, 8, 12, 16, 32, 48, 56], "itemsize": 64})
GRID_ADD_INFO_DTYPE = np.dtype({"names": ["resized", "rows", "cols", "pad", "length", "position", "n_cells_skipped_valid", "n_cells_outside_other",
                                          "n_index_outside", "n_values_copied"],
                                "formats": [np.int32, np.int32, np.int32, np.int32, (np.float64, 2), (np.float64, 2), np.int64, np.int64, np.int64, np.int64],
                                "offsets": [0, 4, 8, 12, 16, 32, 48, 56, 64, 72], "itemsize": 80})
# lio_grid_image_info, lio_grid_from_image_info and lio_grid_from_occupancy_info (tests/test_grid_convert_capi.py holds the
# layouts to gcc's)
GRID_IMAGE_INFO_DTYPE = np.dtype({"names": ["rows", "cols", "lower", "upper", "n_pixels", "n_clamped_low", "n_clamped_high", "n_nonfinite"],
                                  "formats": [np.int32, np.int32, np.float32, np.float32, np.int64, np.int64, np.int64, np.int64],
                                  "offsets": [0, 4, 8, 12, 16, 24, 32, 40], "itemsize": 48})
GRID_FROM_IMAGE_INFO_DTYPE = np.dtype({"names": ["rows", "cols", "geometry_set", "pad", "n_cells_set", "n_cells_transparent"],
                                       "formats": [np.int32, np.int32, np.int32, np.int32, np.int64, np.int64], "offsets": [0, 4, 8, 12, 16, 24], "itemsize": 32})
GRID_FROM_OCCUPANCY_INFO_DTYPE = np.dtype({"names": ["rows", "cols", "geometry_replaced", "pad", "length", "position", "n_unknown"],
                                           "formats": [np.int32, np.int32, np.int32, np.int32, (np.float64, 2), (np.float64, 2), np.int64],
                                           "offsets": [0, 4, 8, 12, 16, 32, 48], "itemsize": 56})
# lio_grid_filter_info (tests/test_grid_filter_capi.py holds the layout to gcc's)
GRID_FILTER_INFO_DTYPE = np.dtype({"names": ["rows", "cols", "window_size", "pad", "n_visited", "n_written", "n_changed"],
                                   "formats": [np.int32, np.int32, np.int32, np.int32, np.int64, np.int64, np.int64], "offsets": [0, 4, 8, 12, 16, 24, 32],
                                   "itemsize": 40})
# lio_grid_expression_info (tests/test_grid_expression_capi.py holds the layout to gcc's)
GRID_EXPRESSION_INFO_DTYPE = np.dtype({"names": ["rows", "cols", "n_ops", "n_passes", "layers_read", "stack_depth", "n_finite"],
                                       "formats": [np.int32, np.int32, np.int32, np.int32, np.uint32, np.int32, np.int64],
                                       "offsets": [0, 4, 8, 12, 16, 20, 24], "itemsize": 32})
GF_MIN, GF_MEAN = 0, 1
GW_INSIDE, GW_CROP, GW_EMPTY, GW_EDGE_MEAN = 0, 1, 2, 3
GW_SUM, GW_MEAN_OF_FINITES, GW_MIN_OF_FINITES, GW_MAX_OF_FINITES, GW_NUMBER_OF_FINITES, GW_STDDEV, GW_WEIGHTED_SUM = range(7)
IMAGE_8U, IMAGE_16U, IMAGE_32F = 0, 1, 2
IMAGE_DTYPES = {IMAGE_8U: np.uint8, IMAGE_16U: np.uint16, IMAGE_32F: np.float32}
REGION_LINE, REGION_CIRCLE, REGION_ELLIPSE, REGION_POLYGON = 0, 1, 2, 3
REGION_OK, REGION_EMPTY, REGION_INVALID = 0, 1, 2
REGION_MAX_VERTICES, REGION_MAX_WALK = 64, 4096
GRID_MAX_LAYERS = 16
GRID_NEAREST, GRID_LINEAR, GRID_CUBIC_CONVOLUTION, GRID_CUBIC, GRID_OUTSIDE = 0, 1, 2, 3, 255
GRID_LAYER_ELEVATION, GRID_LAYER_FILLED, GRID_LAYER_TERRAIN = 0, 1, 2
SDF_NODE_LIMIT = 1 << 25
STAGED_DS, STAGED_RAW = 0, 1

ICP_STATES = {0: "NOT_CONVERGED", 1: "ITERATIONS", 2: "TRANSFORM", 3: "ABS_MSE", 4: "REL_MSE", 5: "NO_CORRESPONDENCES"}


def lib_path():
    # LIOGPU_LIB: A/B-test another build of the same library (kernel experiments); default = the in-tree build
    return os.environ.get("LIOGPU_LIB") or os.path.join(_HERE, "libliogpu.so")


def build_library(verbose=False):
    """hipcc cross-compiles for gfx950 without a GPU (seconds)."""
    out = subprocess.run(["make", "-j8", "-C", os.path.join(_HERE, "csrc")], capture_output=True, text=True)
    if out.returncode != 0:
        raise LioError("building libliogpu.so failed:\n" + out.stdout + out.stderr)
    if verbose:
        print(out.stdout)
    return lib_path()


# The C ABI: one line per symbol of include/liogpu.h, in the header's order.  name -> argtypes, or (restype, argtypes) where the
# function does not return int.  load_library() binds from this table, EXPORTS is its names, and tests/test_capi_signatures.py
# holds every line to the header's prototype.  A new entry point takes one line here.
vp, i32, f32, f64, sz, u64, P = C.c_void_p, C.c_int32, C.c_float, C.c_double, C.c_size_t, C.c_uint64, C.POINTER
pvp, pi, pf, pd, psz = P(vp), P(i32), P(f32), P(f64), P(sz)
_PLANNING = [vp, P(LocalMapConfig), pf, P(HeightMapConfig), P(MedianFillConfig), P(TerrainConfig), vp, P(SdfConfig), P(PlanningMapBuffers),
             P(LocalMapInfo), P(HeightMapInfo), P(MedianFillInfo), P(TerrainInfo), P(SdfInfo)]      # lio_kf_store_planning_map's
CAPI = {
    "lio_version": [],
    "lio_s2m_default_config": (None, [P(S2MConfig)]),
    "lio_last_error": (C.c_char_p, []),
    "lio_s2m_create": [P(S2MConfig), pvp],
    "lio_s2m_destroy": (None, [vp]),
    "lio_s2m_set_map": [vp, vp, sz, sz],
    "lio_s2m_register": [vp, vp, sz, sz, pf, P(S2MResult)],
    "lio_s2m_batch_upload": [vp, i32, pvp, psz, sz],
    "lio_s2m_batch_set_poses": [vp, pf],
    "lio_s2m_batch_run": [vp],
    "lio_s2m_batch_sync": [vp],
    "lio_s2m_batch_results": [vp, pf, P(S2MResult)],
    "lio_s2m_share_map": [vp, vp],
    "lio_s2m_batch_upload_async": [vp, i32, pvp, psz, sz],
    "lio_host_alloc": (vp, [sz]),
    "lio_host_free": (None, [vp]),
    "lio_host_register": [vp, sz],
    "lio_host_unregister": [vp],
    "lio_device_alloc": (vp, [i32, sz]),
    "lio_device_free": (None, [i32, vp]),
    "lio_device_upload": [i32, vp, vp, sz],
    "lio_s2m_set_degeneracy": [vp, i32, pf, i32],
    "lio_s2m_get_correspondences": [vp, i32, vp, vp, vp],
    "lio_s2m_set_corner_map": [vp, vp, sz, sz],
    "lio_s2m_batch_upload_corners": [vp, i32, pvp, psz, sz],
    "lio_s2m_register_cs": [vp, vp, sz, vp, sz, sz, pf, P(S2MResult)],
    "lio_s2m_get_corner_correspondences": [vp, i32, vp, vp, vp],
    "lio_s2m_get_profile": [vp, P(S2MProfile)],
    "lio_s2m_kernel_variant": [vp],
    "lio_s2m_launch_forms": [vp, pi, pi],
    "lio_s2m_debug_persist_spin": [vp, i32, i32],
    "lio_debug_plane_fit": [i32, vp, sz, f64, vp],
    "lio_debug_gn_step": [i32, P(S2MConfig), sz, vp, vp, vp, vp, vp, i32, i32, i32, vp],
    "lio_debug_corner_fit": [i32, vp, vp, sz, f64, f64, vp],
    "lio_debug_fast_f32_ops": [i32, i32, i32, vp, u64, u64, vp, P(u64), vp, pi],
    "lio_debug_threshold_f32": (f32, [f64]),
    "lio_debug_grid_plan": [P(S2MConfig), pf, pf, sz, i32, i32, P(GridPlanInfo)],
    "lio_s2m_debug_stamps": [vp, vp, sz],
    "lio_s2m_debug_scan_order": [vp, vp, vp, sz, pi],
    "lio_debug_scan_tile_plan": [pf, pf, f32, i32, pi, pf],
    "lio_s2m_set_stream": [vp, vp],
    "lio_s2m_set_global_grid": [vp, pf, pi],
    "lio_s2m_set_shard": [vp, i32, i32, i32],
    "lio_s2m_set_shard_plan": [vp, i32, i32, i32, pi, i32],
    "lio_s2m_set_scan_shard": [vp, i32, i32],
    "lio_s2m_batch_begin": [vp],
    "lio_s2m_batch_iter_partial": [vp, vp],
    "lio_s2m_batch_iter_apply": [vp, vp],
    "lio_s2m_batch_n_active": [vp, pi],
    "lio_s2m_batch_poll_active": [vp, i32, pi],
    "lio_transform_update": (None, [pf, i32, i32, f32, f32, f32, f32, f32]),
    "lio_deskew_default_config": (None, [P(DeskewConfig)]),
    "lio_imu_deskew_info": [pd, pd, pd, pd, i32, f64, f64, pd, pd, pd, pd],
    "lio_deskew": [P(DeskewConfig), vp, sz, sz, f64, pd, pd, pd, pd, i32, vp, sz, psz],
    "lio_s2m_register_pc2": [vp, vp, sz, P(PC2Layout), pf, P(S2MResult)],
    "lio_s2m_register_raw": [vp, vp, sz, P(PC2Layout), f32, pf, P(S2MResult), vp, sz, psz],
    "lio_deskew_pc2": [P(DeskewConfig), vp, sz, P(PC2Layout), f64, pd, pd, pd, pd, i32, vp, sz, psz],
    "lio_range_image_default_config": (None, [P(RangeImageConfig)]),
    "lio_range_image": [P(RangeImageConfig), vp, sz, sz, f64, pd, pd, pd, pd, i32, vp, sz, psz, vp, vp, vp, vp],
    "lio_curvature": [i32, vp, sz, vp, vp, vp],
    "lio_feature_default_config": (None, [P(FeatureConfig)]),
    "lio_extract_features": [P(FeatureConfig), vp, sz, sz, vp, vp, vp, vp, vp, psz, vp, psz, sz, vp, vp, vp],
    "lio_voxel_grid": [i32, vp, sz, sz, f32, vp, sz, psz],
    "lio_assemble_map": [vp, i32, i32, pvp, psz, sz, pf, f32, vp, sz, psz],
    "lio_kf_store_create": [i32, pvp],
    "lio_kf_store_destroy": (None, [vp]),
    "lio_kf_store_add": [vp, vp, sz, sz, pi],
    "lio_kf_store_count": [vp],
    "lio_kf_store_points": (sz, [vp, i32]),
    "lio_kf_store_add_device": [vp, vp, sz, sz, pi],
    "lio_kf_store_add_from_handle": [vp, vp, i32, pi],
    "lio_assemble_map_resident": [vp, vp, i32, pi, pf, f32, vp, sz, psz],
    "lio_nearby_default_config": (None, [P(NearbyConfig)]),
    "lio_kf_store_set_poses": [vp, i32, i32, pf, pd],
    "lio_assemble_map_nearby": [vp, vp, P(NearbyConfig), f64, f32, pi, i32, pi, vp, sz, sz, psz],
    "lio_icp_default_config": (None, [P(IcpConfig)]),
    "lio_icp_align": [i32, vp, sz, sz, vp, sz, sz, P(IcpConfig), pf, P(IcpResult)],
    "lio_kf_store_loop_icp": [vp, i32, i32, i32, i32, f32, P(IcpConfig), P(IcpResult), P(IcpClouds)],
    "lio_kf_store_detect_loop": [vp, f32, f64, f64, pi, pi],
    "lio_icp_debug_trace": [i32, vp, sz, sz, vp, sz, sz, P(IcpConfig), pf, i32, P(IcpResult), vp, vp, vp, vp, pi],
    "lio_icp_debug_grid": [i32, vp, sz, sz, P(IcpGridInfo)],
    "lio_sc_default_config": (None, [P(ScConfig)]),
    "lio_sc_make": [i32, vp, sz, sz, P(ScConfig), vp, vp, vp],
    "lio_kf_store_sc_add": [vp, vp, sz, sz, P(ScConfig), pi],
    "lio_kf_store_sc_add_device": [vp, vp, sz, sz, P(ScConfig), pi],
    "lio_kf_store_sc_add_from_handle": [vp, vp, P(ScConfig), pi],
    "lio_kf_store_sc_count": [vp],
    "lio_kf_store_sc_geometry": [vp, pi, pi],
    "lio_kf_store_sc_get": [vp, i32, vp, vp, vp],
    "lio_kf_store_sc_detect": [vp, P(ScConfig), P(ScResult)],
    "lio_sc_distance": [i32, vp, vp, P(ScConfig), pd, pi],
    "lio_sor_filter": [i32, vp, sz, sz, i32, f32, vp, sz, psz, vp, pd],
    "lio_sor_debug_grid": [i32, vp, sz, sz, i32, P(IcpGridInfo)],
    "lio_local_map_default_config": (None, [P(LocalMapConfig)]),
    "lio_kf_store_local_map": [vp, P(LocalMapConfig), pf, vp, sz, sz, psz, P(LocalMapInfo)],
    "lio_height_map_default_config": (None, [P(HeightMapConfig)]),
    "lio_height_map": [i32, vp, sz, sz, P(HeightMapConfig), vp, sz, P(HeightMapInfo)],
    "lio_kf_store_height_map": [vp, P(LocalMapConfig), pf, P(HeightMapConfig), vp, sz, P(LocalMapInfo), P(HeightMapInfo)],
    "lio_terrain_default_config": (None, [P(TerrainConfig)]),
    "lio_terrain_layers": [i32, vp, i32, i32, f64, pd, pd, P(TerrainConfig), vp, sz, P(TerrainInfo)],
    "lio_kf_store_terrain_map": [vp, P(LocalMapConfig), pf, P(HeightMapConfig), P(TerrainConfig), vp, sz, vp, sz, P(LocalMapInfo), P(HeightMapInfo),
                                 P(TerrainInfo)],
    "lio_global_map_default_config": (None, [P(GlobalMapConfig)]),
    "lio_kf_store_global_map": [vp, P(GlobalMapConfig), pi, i32, pi, vp, sz, sz, psz, P(GlobalMapInfo)],
    "lio_kf_store_export_map": [vp, P(ExportConfig), vp, sz, sz, psz, vp, sz, sz, psz, pi],
    "lio_kf_store_get_keyframe": [vp, i32, pf, vp, sz, sz, psz],
    "lio_s2m_registered_cloud": [vp, i32, pf, vp, sz, sz, psz],
    "lio_radius_filter": [i32, vp, sz, sz, f32, i32, vp, sz, psz, vp],
    "lio_ogm_default_config": (None, [P(OgmConfig)]),
    "lio_occupancy_grid": [i32, vp, sz, sz, P(OgmConfig), vp, sz, P(OgmInfo)],
    "lio_kf_store_occupancy_grid": [vp, f32, P(OgmConfig), vp, sz, psz, P(OgmInfo)],
    "lio_ogm_debug_stage_ms": [i32, pf],
    "lio_sdf_default_config": (None, [P(SdfConfig)]),
    "lio_sdf_create": [i32, pvp],
    "lio_sdf_destroy": (None, [vp]),
    "lio_sdf_build": [vp, vp, i32, i32, f64, pd, pd, P(SdfConfig), P(SdfInfo)],
    "lio_kf_store_sdf": [vp, P(LocalMapConfig), pf, P(HeightMapConfig), P(SdfConfig), vp, sz, vp, P(LocalMapInfo), P(HeightMapInfo), P(SdfInfo)],
    "lio_sdf_nodes": [vp, vp, sz],
    "lio_sdf_query": [vp, vp, sz, vp, vp],
    "lio_occupancy_sdf": [i32, vp, i32, i32, f32, i32, vp],
    "lio_sdf_memory": [vp, psz, psz],
    "lio_sdf_debug_stage_ms": [i32, pf],
    "lio_median_fill_default_config": (None, [P(MedianFillConfig)]),
    "lio_median_fill": [i32, vp, i32, i32, f64, P(MedianFillConfig), vp, vp, vp, vp, P(MedianFillInfo)],
    "lio_kf_store_planning_map": _PLANNING,
    "lio_grid_sample_default_config": (None, [P(GridSampleConfig)]),
    "lio_grid_create": [i32, pvp],
    "lio_grid_destroy": (None, [vp]),
    "lio_grid_set_layers": [vp, vp, i32, i32, i32, f64, pd, pd],
    "lio_grid_get_layer": [vp, i32, vp, sz],
    "lio_grid_info": [vp, P(GridInfo)],
    "lio_grid_memory": [vp, psz],
    "lio_grid_sample": [vp, pi, i32, P(GridSampleConfig), vp, sz, vp, vp, P(GridSampleInfo)],
    "lio_kf_store_planning_grid": _PLANNING + [vp],
    "lio_grid_debug_stage_ms": [i32, pf],
    "lio_grid_region_default_config": (None, [P(GridRegionConfig)]),
    "lio_grid_region_reduce": [vp, pi, i32, P(GridRegionConfig), vp, sz, vp, sz, vp, vp, vp, P(GridRegionInfo)],
    "lio_grid_region_cells": [vp, vp, sz, vp, sz, vp, vp, sz, vp, P(GridRegionInfo)],
    "lio_grid_region_debug_stage_ms": [i32, pf],
    "lio_grid_transform": [vp, pd, i32, f64, vp, vp],
    "lio_grid_to_occupancy": [vp, i32, f32, f32, vp, sz, vp],
    "lio_grid_transform_debug_stage_ms": [i32, pf],
    "lio_grid_submap": [vp, pd, pd, vp, vp],
    "lio_grid_move": [vp, pd, vp],
    "lio_grid_extend_to_include": [vp, vp, vp],
    "lio_grid_add_data_from": [vp, vp, i32, i32, pi, i32, C.c_uint32, vp],
    "lio_grid_geom_debug_kernel_ms": [i32, pf],
    "lio_grid_to_image": [vp, i32, i32, i32, f32, f32, vp, sz, vp],
    "lio_grid_add_layer_from_image": [vp, i32, vp, i32, i32, i32, i32, f32, f32, f64, f64, pd, vp],
    "lio_grid_add_color_layer_from_image": [vp, i32, vp, i32, i32, i32, i32, f64, pd, vp],
    "lio_grid_from_occupancy": [vp, i32, vp, sz, C.c_uint32, C.c_uint32, f32, pd, vp],
    "lio_grid_to_point_cloud": [vp, i32, pi, i32, C.c_uint32, vp, sz, psz, pi],
    "lio_grid_to_grid_cells": [vp, i32, f32, f32, vp, sz, psz],
    "lio_sdf_to_point_cloud": [vp, i32, f32, f32, vp, sz, psz],
    "lio_grid_convert_debug_stage_ms": [i32, i32, pf],
    "lio_grid_filter_radius": [vp, i32, i32, i32, f64, vp],
    "lio_grid_filter_window": [vp, i32, i32, i32, i32, i32, f64, pf, vp],
    "lio_grid_filter_curvature": [vp, i32, i32, vp],
    "lio_grid_filter_threshold": [vp, i32, i32, i32, f64, f64, vp],
    "lio_grid_duplicate_layer": [vp, i32, i32],
    "lio_grid_delete_layers": [vp, pi, i32],
    "lio_grid_filter_debug_kernel_ms": [i32, pf],
    "lio_grid_expression_check": [C.c_char_p, P(C.c_char_p), pi, i32, vp],
    "lio_grid_filter_expression": [vp, C.c_char_p, P(C.c_char_p), pi, i32, i32, vp],
    "lio_debug_grid_expression_host": [C.c_char_p, P(C.c_char_p), i32, pf, i32, i32, pf],
    "lio_grid_expression_debug_kernel_ms": [i32, pf],
}
CAPI = {name: sig if isinstance(sig, tuple) else (C.c_int, sig) for name, sig in CAPI.items()}     # -> (restype, argtypes), all of them
EXPORTS = list(CAPI)
_LIB = None


def _bind(L):
    """Gives every symbol of CAPI its types on the library L.  One that L lacks is skipped (A/B runs load older builds through
    LIOGPU_LIB); calling it later raises ctypes' own AttributeError."""
    for name, (restype, argtypes) in CAPI.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return L


def load_library():
    """Loads lio-slam_amd/libliogpu.so; raises LioError when it is missing (no fallback)."""
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise LioError(f"{p} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950). "
                           "There is no CPU fallback.")
        _LIB = _bind(C.CDLL(p))
    return _LIB


def _check(rc, what):
    if rc < 0:
        msg = load_library().lio_last_error()
        raise LioError(f"{what} failed: {STATUS_NAMES.get(rc, rc)}: {msg.decode() if msg else ''}")
    return rc


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _as_points(a):
    """Accepts [n,3] float32 (stride 12) or any C-contiguous [n,k>=3] float32 (stride 4k)."""
    a = np.ascontiguousarray(a, np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("points must be [n, >=3] float32")
    return a, a.shape[1] * 4


def _default_config(struct_cls, entry_name, overrides, convert=None):
    """A struct_cls as the library's entry_name fills it, then the overrides: a key that is no field raises AttributeError,
    convert = {field: function} turns that field's value into what the struct takes."""
    cfg = struct_cls()
    getattr(load_library(), entry_name)(C.byref(cfg))
    for k, v in overrides.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, convert[k](v) if convert and k in convert else v)
    return cfg


def s2m_config(**overrides):
    """The scan-to-map configuration: the library's defaults, then the overrides; device_ids sets the leading elements."""
    ids = overrides.pop("device_ids", ())
    cfg = _default_config(S2MConfig, "lio_s2m_default_config", overrides)
    for i, d in enumerate(ids):
        cfg.device_ids[i] = int(d)
    return cfg


class _Owner:
    """close() and __del__ of an object that owns one resource of the library, under the attribute `_owned` names: a handle
    (c_void_p) or an address (int).  A subclass supplies _release().  It runs once: not again on a second close(), and not at
    all when __init__ raised before the resource existed.  close() leaves the attribute empty (c_void_p() or 0)."""
    _owned = "h"

    def close(self):
        r = getattr(self, self._owned, None)
        if r:
            self._release()
            setattr(self, self._owned, type(r)())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ScanToMap(_Owner):
    """Device-resident replacement of mapOptimization's scan-to-map block (MO:1839-1865)."""

    def __init__(self, **cfg_overrides):
        self.lib = load_library()
        self.cfg = s2m_config(**cfg_overrides)
        self.h = C.c_void_p()
        _check(self.lib.lio_s2m_create(C.byref(self.cfg), C.byref(self.h)), "lio_s2m_create")
        self._n_scans = 0
        self._npts = []

    def _release(self):
        self.lib.lio_s2m_destroy(self.h)

    # kdtreeSurfFromMap->setInputCloud(laserCloudSurfFromMapDS), MO:1846
    def set_map(self, map_pts):
        a, stride = _as_points(map_pts)
        _check(self.lib.lio_s2m_set_map(self.h, a.ctypes.data, len(a), stride), "lio_s2m_set_map")

    # scan2MapOptimization, MO:1839-1865 (loop MO:1848-1859)
    def scan2MapOptimization(self, scan_pts, pose):
        a, stride = _as_points(scan_pts)
        p = np.array(pose, np.float32).copy()
        res = S2MResult()
        rc = _check(self.lib.lio_s2m_register(self.h, a.ctypes.data, len(a), stride, _f32p(p), C.byref(res)),
                    "lio_s2m_register")
        self._n_scans, self._npts = 1, [len(a)]
        return p, res, rc

    # pcl::fromROSMsg(msgIn->cloud_deskewed, ...) MO:440 + scan2MapOptimization on the PointCloud2 blob itself
    def scan2MapOptimizationPC2(self, blob, n_points, layout, pose):
        b = np.ascontiguousarray(blob).view(np.uint8).reshape(-1)
        p = np.array(pose, np.float32).copy()
        res = S2MResult()
        rc = _check(self.lib.lio_s2m_register_pc2(self.h, b.ctypes.data, n_points, C.byref(layout), _f32p(p), C.byref(res)),
                    "lio_s2m_register_pc2")
        self._n_scans, self._npts = 1, [n_points]
        return p, res, rc

    # downsampleCurrentScan MO:1605-1611 + scan2MapOptimization MO:1839-1865 on the blob of cloud_info.cloud_deskewed,
    # one H2D copy, no host round trip between the voxel filter and the registration
    def downsampleAndScan2MapOptimization(self, blob, n_points, layout, leaf, pose, want_ds=False, device_ptr=None):
        p = np.array(pose, np.float32).copy()
        res = S2MResult()
        if device_ptr is None:
            b = np.ascontiguousarray(blob).view(np.uint8).reshape(-1)
            ptr = b.ctypes.data
        else:
            ptr = int(device_ptr)
        out = np.zeros((n_points, 8), np.float32) if want_ds else None
        n_ds = C.c_size_t(0)
        rc = _check(self.lib.lio_s2m_register_raw(self.h, ptr, n_points, C.byref(layout), float(leaf), _f32p(p), C.byref(res),
                                                  out.ctypes.data if want_ds else None, 32, C.byref(n_ds)), "lio_s2m_register_raw")
        self._n_scans, self._npts = 1, [int(n_ds.value)]
        if want_ds:
            o = out[:n_ds.value]
            return p, res, rc, np.concatenate([o[:, :3], o[:, 4:5]], 1)
        return p, res, rc, int(n_ds.value)

    # publishFrames MO:2330-2345: the staged scan (STAGED_DS) or the whole staged cloud (STAGED_RAW) under the final pose
    def registered_cloud(self, which, pose):
        """-> [n,4] (x, y, z, intensity) in the frame of `pose`."""
        p = np.ascontiguousarray(pose, np.float32).reshape(6)
        n = C.c_size_t()
        _check(self.lib.lio_s2m_registered_cloud(self.h, which, _f32p(p), None, 32, 0, C.byref(n)), "lio_s2m_registered_cloud")
        out = np.zeros((max(n.value, 1), 8), np.float32)
        _check(self.lib.lio_s2m_registered_cloud(self.h, which, _f32p(p), out.ctypes.data, 32, len(out), C.byref(n)),
               "lio_s2m_registered_cloud")
        return _from_records(out, n.value)

    # batched form
    def batch_upload(self, scans):
        arrs = [_as_points(s) for s in scans]
        strides = {s for _, s in arrs}
        if len(strides) != 1:
            raise ValueError("all scans of a batch must share one stride")
        n = len(arrs)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a, _ in arrs])
        npts = (C.c_size_t * n)(*[len(a) for a, _ in arrs])
        _check(self.lib.lio_s2m_batch_upload(self.h, n, ptrs, npts, strides.pop()), "lio_s2m_batch_upload")
        self._n_scans, self._npts = n, [len(a) for a, _ in arrs]

    def share_map(self, owner):
        """This handle searches `owner`'s resident map (double-buffered streaming, see include/liogpu.h)."""
        _check(self.lib.lio_s2m_share_map(self.h, owner.h if owner is not None else None), "lio_s2m_share_map")
        self._map_owner = owner          # keep it alive

    def batch_upload_raw(self, base_ptr, n_pts, stride, asynchronous=True):
        """Scans laid out back to back at `base_ptr` (pinned host or device memory): n_pts[s] records of `stride` bytes."""
        n = len(n_pts)
        offs = np.concatenate([[0], np.cumsum(np.asarray(n_pts, np.int64) * stride)])
        ptrs = (C.c_void_p * n)(*[int(base_ptr) + int(o) for o in offs[:-1]])
        npts = (C.c_size_t * n)(*[int(v) for v in n_pts])
        fn = self.lib.lio_s2m_batch_upload_async if asynchronous else self.lib.lio_s2m_batch_upload
        _check(fn(self.h, n, ptrs, npts, stride), "lio_s2m_batch_upload(_async)")
        self._n_scans, self._npts = n, [int(v) for v in n_pts]

    def batch_set_poses(self, poses):
        p = np.ascontiguousarray(poses, np.float32).reshape(self._n_scans, 6)
        _check(self.lib.lio_s2m_batch_set_poses(self.h, _f32p(p)), "lio_s2m_batch_set_poses")

    def batch_run(self):
        _check(self.lib.lio_s2m_batch_run(self.h), "lio_s2m_batch_run")

    def batch_sync(self):
        _check(self.lib.lio_s2m_batch_sync(self.h), "lio_s2m_batch_sync")

    def batch_results(self, with_results=True):
        poses = np.zeros((self._n_scans, 6), np.float32)
        res = (S2MResult * self._n_scans)() if with_results else None
        _check(self.lib.lio_s2m_batch_results(self.h, _f32p(poses), res), "lio_s2m_batch_results")
        return poses, res

    def set_degeneracy(self, scan, matP, is_degenerate):
        m = np.ascontiguousarray(matP, np.float32).reshape(36)
        _check(self.lib.lio_s2m_set_degeneracy(self.h, scan, _f32p(m), int(is_degenerate)), "lio_s2m_set_degeneracy")

    def get_correspondences(self, scan=0):
        n = self._npts[scan]
        flag = np.zeros(n, np.uint8)
        coeff = np.zeros((n, 4), np.float32)
        nn = np.full((n, 5), -1, np.int32)
        _check(self.lib.lio_s2m_get_correspondences(self.h, scan, flag.ctypes.data, coeff.ctypes.data,
                                                    nn.ctypes.data), "lio_s2m_get_correspondences")
        return flag, coeff, nn

    # ---- extension beyond this reference: point-to-line residuals (upstream LIO-SAM cornerOptimization) ----
    def set_corner_map(self, map_pts):
        a, stride = _as_points(np.asarray(map_pts, np.float32).reshape(-1, 3) if len(map_pts) == 0 else map_pts)
        _check(self.lib.lio_s2m_set_corner_map(self.h, a.ctypes.data, len(a), stride), "lio_s2m_set_corner_map")

    def batch_upload_corners(self, scans):
        arrs = [_as_points(np.zeros((0, 3), np.float32) if len(s) == 0 else s) for s in scans]
        n = len(arrs)
        stride = {s for a, s in arrs if len(a)} or {12}
        if len(stride) != 1:
            raise ValueError("all scans of a batch must share one stride")
        ptrs = (C.c_void_p * n)(*[a.ctypes.data if len(a) else None for a, _ in arrs])
        npts = (C.c_size_t * n)(*[len(a) for a, _ in arrs])
        _check(self.lib.lio_s2m_batch_upload_corners(self.h, n, ptrs, npts, stride.pop()), "lio_s2m_batch_upload_corners")
        self._ncorner = [len(a) for a, _ in arrs]

    def scan2MapOptimizationCS(self, corner_pts, surf_pts, pose):
        cpts, cstride = _as_points(corner_pts)
        a, stride = _as_points(surf_pts)
        if cstride != stride:
            raise ValueError("corner and surf clouds must share one stride")
        p = np.array(pose, np.float32).copy()
        res = S2MResult()
        rc = _check(self.lib.lio_s2m_register_cs(self.h, cpts.ctypes.data, len(cpts), a.ctypes.data, len(a), stride,
                                                 _f32p(p), C.byref(res)), "lio_s2m_register_cs")
        self._n_scans, self._npts, self._ncorner = 1, [len(a)], [len(cpts)]
        return p, res, rc

    def get_corner_correspondences(self, scan=0):
        n = self._ncorner[scan]
        flag = np.zeros(n, np.uint8)
        coeff = np.zeros((n, 4), np.float32)
        nn = np.full((n, 5), -1, np.int32)
        _check(self.lib.lio_s2m_get_corner_correspondences(self.h, scan, flag.ctypes.data, coeff.ctypes.data,
                                                           nn.ctypes.data), "lio_s2m_get_corner_correspondences")
        return flag, coeff, nn

    def profile(self):
        p = S2MProfile()
        _check(self.lib.lio_s2m_get_profile(self.h, C.byref(p)), "lio_s2m_get_profile")
        return p

    def kernel_variant(self):
        """(plain, waves): whether the last run's surface launches used the plain k_s2m_iterate, and its occupancy target."""
        v = self.lib.lio_s2m_kernel_variant(self.h)
        _check(min(v, 0), "lio_s2m_kernel_variant")
        return bool(v & 1), v >> 8

    def launch_forms(self):
        """(full, looped): surface launches of the last run with one workgroup per block, and with the looped form of the plain
        kernel (LIO_TAIL_FROM / LIO_TAIL_WGS in the environment when the handle was created; include/liogpu.h)."""
        full, looped = C.c_int32(0), C.c_int32(0)
        _check(self.lib.lio_s2m_launch_forms(self.h, C.byref(full), C.byref(looped)), "lio_s2m_launch_forms")
        return full.value, looped.value

    def debug_persist_spin(self, spin_max=0, withhold_wg=-1):
        """Test hook of the one-launch loop: poll bound and a workgroup that never arrives (include/liogpu.h)."""
        _check(self.lib.lio_s2m_debug_persist_spin(self.h, int(spin_max), int(withhold_wg)), "lio_s2m_debug_persist_spin")

    def debug_stamps(self):
        nb = self.lib.lio_s2m_debug_stamps(self.h, None, 0)
        out = np.zeros((max(nb, 0), 4, 8), np.int64)
        if nb > 0:
            self.lib.lio_s2m_debug_stamps(self.h, out.ctypes.data, out.size)
        return out

    def debug_scan_order(self):
        """Test hook of the upload-time tile sort (include/liogpu.h) -> (sorted, perm, xyz): perm[j] = the caller's batch-wide
        index of the record at sorted position j (None when the batch was not sorted), xyz [n, 3] = the SoA as uploaded."""
        srt = C.c_int32(0)
        n = _check(self.lib.lio_s2m_debug_scan_order(self.h, None, None, 0, C.byref(srt)), "lio_s2m_debug_scan_order")
        perm = np.full(n, -1, np.int32)
        soa = np.zeros((3, n), np.float32)
        _check(self.lib.lio_s2m_debug_scan_order(self.h, perm.ctypes.data, soa.ctypes.data, n, C.byref(srt)), "lio_s2m_debug_scan_order")
        return bool(srt.value), (perm if srt.value else None), np.ascontiguousarray(soa.T)

    # multi-GPU hooks
    def set_stream(self, hip_stream):
        _check(self.lib.lio_s2m_set_stream(self.h, C.c_void_p(hip_stream)), "lio_s2m_set_stream")

    def set_global_grid(self, origin, dims):
        o = (C.c_float * 3)(*origin)
        d = (C.c_int32 * 3)(*dims)
        _check(self.lib.lio_s2m_set_global_grid(self.h, o, d), "lio_s2m_set_global_grid")

    def set_shard(self, axis, lo, hi):
        _check(self.lib.lio_s2m_set_shard(self.h, axis, lo, hi), "lio_s2m_set_shard")

    def set_shard_plan(self, axis, rank, bounds, halo_cells):
        b = (C.c_int32 * len(bounds))(*[int(v) for v in bounds])
        _check(self.lib.lio_s2m_set_shard_plan(self.h, axis, len(bounds) - 1, rank, b, halo_cells), "lio_s2m_set_shard_plan")

    def set_scan_shard(self, rank, world):
        _check(self.lib.lio_s2m_set_scan_shard(self.h, rank, world), "lio_s2m_set_scan_shard")

    def batch_begin(self):
        _check(self.lib.lio_s2m_batch_begin(self.h), "lio_s2m_batch_begin")

    def batch_iter_partial(self, d_sums_ptr):
        _check(self.lib.lio_s2m_batch_iter_partial(self.h, C.c_void_p(d_sums_ptr)), "lio_s2m_batch_iter_partial")

    def batch_iter_apply(self, d_sums_ptr):
        _check(self.lib.lio_s2m_batch_iter_apply(self.h, C.c_void_p(d_sums_ptr)), "lio_s2m_batch_iter_apply")

    def batch_poll_active(self, iteration):
        v = C.c_int32()
        _check(self.lib.lio_s2m_batch_poll_active(self.h, iteration, C.byref(v)), "lio_s2m_batch_poll_active")
        return v.value

    def batch_n_active(self):
        v = C.c_int32()
        _check(self.lib.lio_s2m_batch_n_active(self.h, C.byref(v)), "lio_s2m_batch_n_active")
        return v.value


class DeviceBuffer(_Owner):
    """hipMalloc'ed bytes on `device_id` holding a copy of a numpy array (a cloud that already lives in HBM)."""
    _owned = "ptr"

    def __init__(self, array, device_id=0):
        self.lib = load_library()
        self.device_id = int(device_id)
        a = np.ascontiguousarray(array)
        self.nbytes = a.nbytes
        self.ptr = self.lib.lio_device_alloc(self.device_id, self.nbytes)
        if not self.ptr:
            raise LioError("lio_device_alloc failed")
        _check(self.lib.lio_device_upload(self.device_id, self.ptr, a.ctypes.data, self.nbytes), "lio_device_upload")

    def _release(self):
        self.lib.lio_device_free(self.device_id, self.ptr)


class PinnedBuffer(_Owner):
    """hipHostMalloc'ed bytes as a numpy array (true-DMA source for batch_upload_raw)."""
    _owned = "ptr"

    def __init__(self, nbytes):
        self.lib = load_library()
        self.nbytes = int(nbytes)
        self.ptr = self.lib.lio_host_alloc(self.nbytes)
        if not self.ptr:
            raise LioError("lio_host_alloc failed")
        self.array = np.ctypeslib.as_array((C.c_uint8 * self.nbytes).from_address(self.ptr))

    def _release(self):
        self.array = None                  # the view goes before the bytes under it
        self.lib.lio_host_free(self.ptr)


# transformUpdate, MO:1867-1907
def transform_update(pose, imu_available=0, imu_type=0, imu_roll_init=0.0, imu_pitch_init=0.0,
                     imu_rpy_weight=0.01, rotation_tollerance=1000.0, z_tollerance=1000.0):
    p = np.array(pose, np.float32).copy()
    load_library().lio_transform_update(_f32p(p), imu_available, imu_type, imu_roll_init, imu_pitch_init,
                                        imu_rpy_weight, rotation_tollerance, z_tollerance)
    return p


# imuDeskewInfo, IP:359-418
def imu_deskew_info(stamp, gyro, t_cur, t_end):
    stamp = np.ascontiguousarray(stamp, np.float64)
    g = np.ascontiguousarray(gyro, np.float64)
    gx, gy, gz = (np.ascontiguousarray(g[:, k]) for k in range(3))
    T, RX, RY, RZ = (np.zeros(2000) for _ in range(4))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    cur = load_library().lio_imu_deskew_info(dp(stamp), dp(gx), dp(gy), dp(gz), len(stamp), t_cur, t_end,
                                             dp(T), dp(RX), dp(RY), dp(RZ))
    return cur, T, RX, RY, RZ


_XYZIRT = np.dtype({"names": ["x", "y", "z", "intensity", "ring", "time"],
                    "formats": ["<f4", "<f4", "<f4", "<f4", "<u2", "<f4"],
                    "offsets": [0, 4, 8, 16, 20, 24], "itemsize": 32})


def pack_xyzirt(xyz, intensity, ring, time):
    """VelodynePointXYZIRT records (IP:4-15): 32-byte stride."""
    rec = np.zeros(len(xyz), _XYZIRT)
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    rec["intensity"], rec["ring"], rec["time"] = intensity, ring, time
    return rec


# projectPointCloud + deskewPoint, IP:545-615
_SCRATCH = {}


def _scratch(name, shape, dtype=np.float32):
    """Re-used host output buffer (like a node's member clouds).  A fresh np.zeros per call hands the HIP
    runtime never-touched pages to pin for the D2H copy, which costs milliseconds and says nothing about
    the library; results are copied out of the scratch before they are returned."""
    need = int(np.prod(shape))
    buf = _SCRATCH.get((name, np.dtype(dtype).str))
    if buf is None or buf.size < need:
        buf = np.zeros(max(need, 1), dtype)
        _SCRATCH[(name, np.dtype(dtype).str)] = buf
    return buf[:need].reshape(shape)


def deskew(dcfg, records, t_cur, imu):
    cur, T, RX, RY, RZ = imu
    L = load_library()
    n = len(records)
    out = _scratch("deskew", (n, 8))       # pcl::PointXYZI, 32-byte stride
    n_out = C.c_size_t()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rec = np.ascontiguousarray(records)
    _check(L.lio_deskew(C.byref(dcfg), rec.ctypes.data, n, rec.dtype.itemsize, t_cur,
                        dp(T), dp(RX), dp(RY), dp(RZ), cur, out.ctypes.data, 32, C.byref(n_out)), "lio_deskew")
    o = out[:n_out.value]
    return np.concatenate([o[:, :3], o[:, 4:5]], axis=1).copy()


def deskew_pc2(dcfg, blob, n_points, layout, t_cur, imu):
    """projectPointCloud on the raw PointCloud2 `data` blob (any of the four sensor layouts of IP:226-285)."""
    cur, T, RX, RY, RZ = imu
    L = load_library()
    b = np.ascontiguousarray(blob).view(np.uint8).reshape(-1)
    out = _scratch("deskew", (max(n_points, 1), 8))
    n_out = C.c_size_t()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    _check(L.lio_deskew_pc2(C.byref(dcfg), b.ctypes.data, n_points, C.byref(layout), t_cur,
                            dp(T), dp(RX), dp(RY), dp(RZ), cur, out.ctypes.data, 32, C.byref(n_out)), "lio_deskew_pc2")
    o = out[:n_out.value]
    return np.concatenate([o[:, :3], o[:, 4:5]], axis=1).copy()


def deskew_default_config(**overrides):
    return _default_config(DeskewConfig, "lio_deskew_default_config", overrides)


# calculateSmoothness, FE:81-101
def curvature(rng, device_id=0):
    r = np.ascontiguousarray(rng, np.float32)
    curv = np.zeros(len(r), np.float32)
    picked = np.full(len(r), -1, np.int32)
    label = np.full(len(r), -1, np.int32)
    _check(load_library().lio_curvature(device_id, r.ctypes.data, len(r), curv.ctypes.data,
                                        picked.ctypes.data, label.ctypes.data), "lio_curvature")
    return curv, picked, label


# test hook: the device plane fit of the association on (n, 5, 3) neighbour sets -> (n, 8) uint32: the bits of X0[0..2],
# pa, pb, pc, pd, then planeValid (include/liogpu.h)
def debug_plane_fit(sets, plane_tol=0.2, device_id=0):
    a = np.ascontiguousarray(sets, np.float32).reshape(-1, 15)
    out = np.zeros((len(a), 8), np.uint32)
    _check(load_library().lio_debug_plane_fit(device_id, a.ctypes.data, len(a), float(plane_tol), out.ctypes.data), "lio_debug_plane_fit")
    return out


# the packed record of lio_debug_gn_step (include/liogpu.h): 109 words of 4 bytes, no padding
class DebugGnRecord(C.Structure):
    _fields_ = [
        ("pose", C.c_float * 6), ("matP", C.c_float * 36), ("AtA", C.c_float * 36), ("AtB", C.c_float * 6),
        ("T", C.c_float * 12), ("trig", C.c_float * 6),
        ("iter", C.c_int32), ("done", C.c_int32), ("status", C.c_int32), ("converged", C.c_int32),
        ("is_degenerate", C.c_int32), ("n_corr_last", C.c_int32), ("ret", C.c_int32),
    ]


DEBUG_GN_RECORD_DTYPE = np.dtype([
    ("pose", np.float32, 6), ("matP", np.float32, 36), ("AtA", np.float32, 36), ("AtB", np.float32, 6),
    ("T", np.float32, 12), ("trig", np.float32, 6),
    ("iter", np.int32), ("done", np.int32), ("status", np.int32), ("converged", np.int32),
    ("is_degenerate", np.int32), ("n_corr_last", np.int32), ("ret", np.int32)])
assert DEBUG_GN_RECORD_DTYPE.itemsize == C.sizeof(DebugGnRecord) == 436


# test hook: the serial Gauss-Newton step (lio_gn_step) on n independent cases, one wave each.  sums (n, 28) float64: the 21
# upper-triangle JtJ entries, the 6 of Jtr, the correspondence count; pose (n, 6); it, is_degenerate (n,); matP (n, 36);
# the three speculation arguments hold for the whole call; cfg_overrides: fields of the scan-to-map configuration.
# Returns a structured array of DEBUG_GN_RECORD_DTYPE.  Non-finite sums or poses are refused (include/liogpu.h)
def debug_gn_step(sums, pose, it, is_degenerate, matP, deg_override=-1, skip_eigen=False, hold_if_done=False, device_id=0,
                  **cfg_overrides):
    cfg = s2m_config(**cfg_overrides)
    sums = np.ascontiguousarray(sums, np.float64).reshape(-1, 28)
    n = len(sums)
    pose = np.ascontiguousarray(pose, np.float32).reshape(n, 6)
    it = np.ascontiguousarray(it, np.int32).reshape(n)
    deg = np.ascontiguousarray(is_degenerate, np.int32).reshape(n)
    matP = np.ascontiguousarray(matP, np.float32).reshape(n, 36)
    out = np.zeros(n, DEBUG_GN_RECORD_DTYPE)
    _check(load_library().lio_debug_gn_step(device_id, C.byref(cfg) if cfg_overrides else None, n, sums.ctypes.data, pose.ctypes.data,
                                            it.ctypes.data, deg.ctypes.data, matP.ctypes.data, int(deg_override), 1 if skip_eigen else 0,
                                            1 if hold_if_done else 0, out.ctypes.data), "lio_debug_gn_step")
    return out


# test hook: the line fit of the corner association (lio_corner_assoc) on (n, 5, 3) neighbour sets in the caller's order and
# (n, 3) transformed points -> (n, 5) uint32: the bits of the four coefficients, then the accept flag (include/liogpu.h)
def debug_corner_fit(sets, pts, weight=0.9, min_s=0.1, device_id=0):
    a = np.ascontiguousarray(sets, np.float32).reshape(-1, 15)
    q = np.ascontiguousarray(pts, np.float32).reshape(len(a), 3)
    out = np.zeros((len(a), 5), np.uint32)
    _check(load_library().lio_debug_corner_fit(device_id, a.ctypes.data, q.ctypes.data, len(a), float(weight), float(min_s), out.ctypes.data),
           "lio_debug_corner_fit")
    return out


# test hook: the association's fast fp32 square root (op 0), x / 5 (op 1) or fourth root of the range of the scan point (x, 0, 0) (op 2) against the device's plain operator on the bit patterns
# `patterns` (array) or first .. first + count; raw: the fast sequence without its guard.  Returns (number of differing results,
# up to eight differing patterns, result bits or None) (include/liogpu.h)
def debug_fast_f32_ops(op, raw=False, patterns=None, first=0, count=0, want_values=False, device_id=0):
    pat = None
    if patterns is not None:
        pat = np.ascontiguousarray(patterns, np.uint32)
        count = len(pat)
    vals = np.zeros(count, np.uint32) if want_values else None
    n_diff, n_first = C.c_uint64(0), C.c_int32(0)
    firsts = np.zeros(8, np.uint32)
    _check(load_library().lio_debug_fast_f32_ops(device_id, int(op), 1 if raw else 0, pat.ctypes.data if pat is not None else None, int(first),
                                                 int(count), vals.ctypes.data if vals is not None else None, C.byref(n_diff),
                                                 firsts.ctypes.data, C.byref(n_first)), "lio_debug_fast_f32_ops")
    return int(n_diff.value), firsts[:n_first.value].copy(), vals


# test hook (host only): the largest float32 not above the double t, as the library converts plane_tol and min_s
def debug_threshold_f32(t):
    return np.float32(load_library().lio_debug_threshold_f32(float(t)))


# test hook (host only): the search grid set_map would lay out over n map points in the box [mn, mx] under ScanToMap settings
# `cfg_overrides` (and LIO_X_SUB / LIO_TIGHT / LIO_TRY in the environment); occupied = grid cells holding a point (negative:
# not counted), caller_box: the box came from the caller, as for a map assembled on the device (include/liogpu.h)
def debug_grid_plan(mn, mx, n, occupied=-1, caller_box=False, **cfg_overrides):
    cfg = s2m_config(**cfg_overrides)
    lo, hi = np.ascontiguousarray(mn, np.float32).reshape(3), np.ascontiguousarray(mx, np.float32).reshape(3)
    out = GridPlanInfo()
    _check(load_library().lio_debug_grid_plan(C.byref(cfg), _f32p(lo), _f32p(hi), int(n), int(occupied), 1 if caller_box else 0, C.byref(out)),
           "lio_debug_grid_plan")
    return out


# test hook (host only): the scan-local tile grid of the upload-time sort over the box [mn, mx] (include/liogpu.h)
def debug_scan_tile_plan(mn, mx, tile, shard_axis=-1):
    lo, hi = np.ascontiguousarray(mn, np.float32).reshape(3), np.ascontiguousarray(mx, np.float32).reshape(3)
    oi, of = np.zeros(6, np.int32), np.zeros(4, np.float32)
    _check(load_library().lio_debug_scan_tile_plan(_f32p(lo), _f32p(hi), float(tile), int(shard_axis),
                                                   oi.ctypes.data_as(C.POINTER(C.c_int32)), _f32p(of)), "lio_debug_scan_tile_plan")
    return dict(ntx=int(oi[0]), nty=int(oi[1]), ntz=int(oi[2]), mx=int(oi[3]), my=int(oi[4]), mz=int(oi[5]),
                ox=of[0], oy=of[1], oz=of[2], inv_tile=of[3])


# extension (row A4): projectPointCloud + cloudExtraction of upstream LIO-SAM -> the cloud_info arrays FE consumes
def range_image(records, t_cur, imu, device_id=0, **cfg_overrides):
    """PointXYZIRT records -> dict(cloud [n,4], start_ring, end_ring, col, range) like synth.organize_scan."""
    L = load_library()
    cfg = _default_config(RangeImageConfig, "lio_range_image_default_config", {"device_id": device_id, **cfg_overrides})
    cur, T, RX, RY, RZ = imu
    rec = np.ascontiguousarray(records)
    cells = int(cfg.N_SCAN) * int(cfg.Horizon_SCAN)
    out = _scratch("ri_cloud", (max(cells, 1), 8))
    col = _scratch("ri_col", (max(cells, 1),), np.int32)
    rng = _scratch("ri_range", (max(cells, 1),))
    start = np.zeros(cfg.N_SCAN, np.int32)
    end = np.zeros(cfg.N_SCAN, np.int32)
    n_out = C.c_size_t()
    dpp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    _check(L.lio_range_image(C.byref(cfg), rec.ctypes.data, len(rec), rec.dtype.itemsize, t_cur, dpp(T), dpp(RX), dpp(RY), dpp(RZ),
                             cur, out.ctypes.data, 32, C.byref(n_out), start.ctypes.data, end.ctypes.data, col.ctypes.data,
                             rng.ctypes.data), "lio_range_image")
    n = n_out.value
    return {"cloud": _from_records(out, n), "start_ring": start, "end_ring": end, "col": col[:n].copy(), "range": rng[:n].copy()}


# markOccludedPoints + extractFeatures, FE:103-238 (with calculateSmoothness: the whole handler FE:67-77)
def extract_features(cloud_xyzi, start_ring, end_ring, point_col, point_range, device_id=0, **cfg_overrides):
    """cloud_xyzi [n,4] -> dict(corner [n_c,4], surface [n_s,4], curvature, picked, label)."""
    L = load_library()
    cfg = _default_config(FeatureConfig, "lio_feature_default_config", {"N_SCAN": len(start_ring), "device_id": device_id, **cfg_overrides})
    rec = _as_xyzi_records(np.asarray(cloud_xyzi, np.float32).reshape(-1, 4))
    n = len(rec)
    sr = np.ascontiguousarray(start_ring, np.int32)
    er = np.ascontiguousarray(end_ring, np.int32)
    col = np.ascontiguousarray(point_col, np.int32)
    rng = np.ascontiguousarray(point_range, np.float32)
    corner = _scratch("fe_corner", (120 * max(cfg.N_SCAN, 1), 8))
    surf = _scratch("fe_surf", (max(n, 1), 8))
    curv = np.zeros(max(n, 1), np.float32)
    picked = np.zeros(max(n, 1), np.int32)
    label = np.zeros(max(n, 1), np.int32)
    nc, ns = C.c_size_t(0), C.c_size_t(0)
    _check(L.lio_extract_features(C.byref(cfg), rec.ctypes.data, n, 32, sr.ctypes.data, er.ctypes.data,
                                  col.ctypes.data, rng.ctypes.data, corner.ctypes.data, C.byref(nc),
                                  surf.ctypes.data, C.byref(ns), 32, curv.ctypes.data, picked.ctypes.data,
                                  label.ctypes.data), "lio_extract_features")
    return {"corner": _from_records(corner, nc.value), "surface": _from_records(surf, ns.value),
            "curvature": curv[:n], "picked": picked[:n], "label": label[:n]}


def _as_xyzi_records(a):
    """[n,4] (x,y,z,intensity) float32 -> pcl::PointXYZI records [n,8] (32-byte stride)."""
    a = np.ascontiguousarray(a, np.float32)
    rec = np.zeros((len(a), 8), np.float32)
    rec[:, :3] = a[:, :3]
    rec[:, 3] = 1.0
    rec[:, 4] = a[:, 3]
    return rec


def _from_records(rec, n):
    return np.concatenate([rec[:n, :3], rec[:n, 4:5]], axis=1).copy()


# downsampleCurrentScan, MO:1605-1611 (pcl::VoxelGrid)
def voxel_grid(xyzi, leaf, device_id=0):
    rec = _as_xyzi_records(xyzi)
    out = _scratch("voxel", rec.shape)
    n_out = C.c_size_t()
    rc = _check(load_library().lio_voxel_grid(device_id, rec.ctypes.data, len(rec), 32, leaf, out.ctypes.data, 32,
                                              C.byref(n_out)), "lio_voxel_grid")
    return _from_records(out, n_out.value), rc


def nearby_default_config(**overrides):
    return _default_config(NearbyConfig, "lio_nearby_default_config", overrides)


def icp_default_config(**overrides):
    return _default_config(IcpConfig, "lio_icp_default_config", overrides)


def _guess_ptr(guess):
    if guess is None:
        return None, None
    g = np.ascontiguousarray(guess, np.float32).reshape(16)
    return g, _f32p(g)


# icp.align + icp.getFitnessScore, MO:1119-1124
def icp_align(source, target, cfg=None, guess=None, device_id=0):
    """-> (IcpResult, rc).  source / target: [n, >=3] float32."""
    src, ss = _as_points(source)
    tgt, ts = _as_points(target)
    cfg = cfg or icp_default_config()
    g, gp = _guess_ptr(guess)
    res = IcpResult()
    rc = _check(load_library().lio_icp_align(device_id, src.ctypes.data, len(src), ss, tgt.ctypes.data, len(tgt), ts, C.byref(cfg), gp,
                                             C.byref(res)), "lio_icp_align")
    return res, rc


def icp_debug_trace(source, target, cfg=None, guess=None, rec_iter=-1, device_id=0):
    """Test hook -> (IcpResult, steps [k,4,4], n_corr [k], mse [k], corr [n_source] of iteration rec_iter)."""
    src, ss = _as_points(source)
    tgt, ts = _as_points(target)
    cfg = cfg or icp_default_config()
    g, gp = _guess_ptr(guess)
    res = IcpResult()
    steps = np.zeros((cfg.max_iters, 16), np.float32)
    n_corr = np.zeros(cfg.max_iters, np.int32)
    mse = np.zeros(cfg.max_iters, np.float64)
    corr = np.full(max(len(src), 1), -1, np.int32)
    nt = C.c_int32()
    _check(load_library().lio_icp_debug_trace(device_id, src.ctypes.data, len(src), ss, tgt.ctypes.data, len(tgt), ts, C.byref(cfg), gp,
                                              rec_iter, C.byref(res), steps.ctypes.data, n_corr.ctypes.data, mse.ctypes.data,
                                              corr.ctypes.data, C.byref(nt)), "lio_icp_debug_trace")
    k = nt.value
    return res, steps[:k].reshape(k, 4, 4).copy(), n_corr[:k].copy(), mse[:k].copy(), corr[:len(src)].copy()


def icp_debug_grid(target, device_id=0):
    """Test hook, read-only -> IcpGridInfo: the grid lio_icp_align lays over `target`, by the alignment's own code."""
    tgt, ts = _as_points(target)
    out = IcpGridInfo()
    _check(load_library().lio_icp_debug_grid(device_id, tgt.ctypes.data, len(tgt), ts, C.byref(out)), "lio_icp_debug_grid")
    return out


def sc_default_config(**overrides):
    return _default_config(ScConfig, "lio_sc_default_config", overrides)


# scManager.makeAndSaveScancontextAndKeys without the store, SC:236-246
def sc_make(cloud, cfg=None, device_id=0):
    """-> (desc [rings, sectors] float32, ring_key [rings] float32, sector_key [sectors] float64).  cloud: [n, >=3] float32."""
    pts, stride = _as_points(cloud)
    cfg = cfg or sc_default_config()
    R, S = max(cfg.num_rings, 1), max(cfg.num_sectors, 1)
    desc, rk, sk = np.zeros((R, S), np.float32), np.zeros(R, np.float32), np.zeros(S, np.float64)
    _check(load_library().lio_sc_make(device_id, pts.ctypes.data, len(pts), stride, C.byref(cfg), desc.ctypes.data, rk.ctypes.data,
                                      sk.ctypes.data), "lio_sc_make")
    return desc, rk, sk


def sc_distance(desc_a, desc_b, cfg=None, device_id=0):
    """Test hook: distanceBtnScanContext SC:116-148 -> (dist, align)."""
    cfg = cfg or sc_default_config()
    a = np.ascontiguousarray(desc_a, np.float32).reshape(cfg.num_rings, cfg.num_sectors)
    b = np.ascontiguousarray(desc_b, np.float32).reshape(cfg.num_rings, cfg.num_sectors)
    d, al = C.c_double(), C.c_int32()
    _check(load_library().lio_sc_distance(device_id, a.ctypes.data, b.ctypes.data, C.byref(cfg), C.byref(d), C.byref(al)), "lio_sc_distance")
    return d.value, al.value


# sor.filter, MO:2513-2514 (pcl::StatisticalOutlierRemoval)
def sor_filter(xyzi, mean_k=10, stddev_mul=1.0, device_id=0):
    """-> (inliers [m,4], mean_dist [n] with NaN for a skipped point, stats (mean, stddev, threshold), rc); rc 1 = passed
    through (at most mean_k finite points).  xyzi: [n,4] float32 (x, y, z, intensity)."""
    rec = _as_xyzi_records(np.asarray(xyzi, np.float32).reshape(-1, 4))
    n = len(rec)
    out = np.zeros((max(n, 1), 8), np.float32)
    dist = np.zeros(max(n, 1), np.float32)
    stats = (C.c_double * 3)()
    n_out = C.c_size_t()
    rc = _check(load_library().lio_sor_filter(device_id, rec.ctypes.data, n, 32, int(mean_k), float(stddev_mul), out.ctypes.data, 32,
                                              C.byref(n_out), dist.ctypes.data, stats), "lio_sor_filter")
    return _from_records(out, n_out.value), dist[:n].copy(), tuple(stats), rc


def sor_debug_grid(xyz, mean_k=10, device_id=0):
    """Test hook, read-only -> IcpGridInfo: the grid lio_sor_filter lays over the cloud at `mean_k`, by the filter's own code."""
    pts, stride = _as_points(xyz)
    out = IcpGridInfo()
    _check(load_library().lio_sor_debug_grid(device_id, pts.ctypes.data, len(pts), stride, int(mean_k), C.byref(out)), "lio_sor_debug_grid")
    return out


def local_map_default_config(**overrides):
    return _default_config(LocalMapConfig, "lio_local_map_default_config", overrides)


def global_map_default_config(**overrides):
    return _default_config(GlobalMapConfig, "lio_global_map_default_config", overrides)


def _from_records_stride(buf, n, stride):
    """n records of `stride` bytes (x, y, z @0,4,8, intensity @16) in a uint8 buffer -> [n,4] float32."""
    rec = buf[:n * stride].view(np.float32).reshape(n, stride // 4)
    return np.concatenate([rec[:, :3], rec[:, 4:5]], axis=1).copy()


def height_map_default_config(**overrides):
    return _default_config(HeightMapConfig, "lio_height_map_default_config", overrides, convert={"voxel": lambda v: (C.c_float * 3)(*v)})


def _height_map_call(call, what, want_grid):
    """One call into a grid buffer kept from the last one, as a node keeps it; a second only when the grid has outgrown the
    buffer (ERR_ARG with rows x cols filled in).  -> (grid [rows, cols] float32 (NaN: no elevation) or None, HeightMapInfo)."""
    info = HeightMapInfo()

    def make_call(cells):
        buf = _scratch("height_map", (cells if want_grid else 0,))
        return call(buf.ctypes.data if want_grid else None, buf.size, info), buf
    buf = _call_with_cells("height_map", 1 << 18, make_call, lambda: info.rows * info.cols if want_grid else 0, what)
    n = info.rows * info.cols
    return (buf[:n].reshape((info.rows, info.cols), order="F").copy(order="F") if want_grid else None), info     # grid_map::Matrix is column-major


_SCRATCH_CELLS = {}


def _call_with_cells(key, default_cells, make_call, cells_of, what):
    """make_call(cells) -> (rc, its buffers): one call into scratch buffers sized for `cells` grid cells, the size the last call
    under `key` needed.  When it is refused (-1) with cells_of() -- the rows x cols it reports -- above that, the size is
    remembered and the call is made once more.  -> the buffers of the call that counts, its rc checked."""
    cells = _SCRATCH_CELLS.get(key, default_cells)
    rc, bufs = make_call(cells)
    if rc == -1 and cells_of() > cells:
        cells = _SCRATCH_CELLS[key] = cells_of()
        rc, bufs = make_call(cells)
    _check(rc, what)
    return bufs


# processPointcloud, helpers.cpp:97-105 (grid_map_pcl's loader)
def height_map(xyz, cfg=None, want_grid=True, device_id=0):
    """-> (elevation grid [rows, cols] or None, HeightMapInfo).  xyz: [n, >= 3] float32."""
    cfg = cfg or height_map_default_config()
    a = np.asarray(xyz, np.float32)
    p = np.ascontiguousarray((a if a.ndim == 2 else a.reshape(-1, 3))[:, :3])
    lib = load_library()
    return _height_map_call(lambda g, cap, info: lib.lio_height_map(device_id, p.ctypes.data, len(p), 12, C.byref(cfg), g, cap, C.byref(info)),
                            "lio_height_map", want_grid)


def terrain_default_config(**overrides):
    return _default_config(TerrainConfig, "lio_terrain_default_config", overrides)


def _terrain_layers_out(buf, info, mask):
    """the requested layers of one call -> {name: [rows, cols] float32 (NaN: no value)}, column-major as grid_map::Matrix"""
    n = info.rows * info.cols
    names = [name for k, name in enumerate(TERRAIN_LAYERS) if (mask >> k) & 1]
    return {name: buf[i * n:(i + 1) * n].reshape((info.rows, info.cols), order="F").copy(order="F") for i, name in enumerate(names)}


# grid_map_demos' filter chain behind elevation_inpainted
def terrain_layers(grid, resolution, length, position, cfg=None, device_id=0):
    """-> ({layer name: [rows, cols] float32}, TerrainInfo).  grid: [rows, cols] float32, NaN = no elevation; length and
    position: those of the HeightMapInfo the grid came with."""
    cfg = cfg or terrain_default_config()
    g = np.asfortranarray(np.asarray(grid, np.float32))
    if g.ndim != 2:
        raise ValueError("grid must be [rows, cols]")
    rows, cols = g.shape
    buf = np.empty(max(bin(cfg.layers & 0xff).count("1") * rows * cols, 1), np.float32)
    info = TerrainInfo()
    ln, ps = (C.c_double * 2)(*length), (C.c_double * 2)(*position)
    _check(load_library().lio_terrain_layers(device_id, g.ctypes.data, rows, cols, float(resolution), ln, ps, C.byref(cfg), buf.ctypes.data,
                                             buf.size, C.byref(info)), "lio_terrain_layers")
    return _terrain_layers_out(buf, info, cfg.layers), info


# pcl::RadiusOutlierRemoval of the draft ogmGeneration.cpp
def radius_filter(xyzi, radius=0.5, min_neighbors=10, want_counts=True, device_id=0):
    """-> (kept [m,4], n_neighbors [n] int32 with -1 for a dropped point, or None).  xyzi: [n,4] float32 (x, y, z, intensity).
    want_counts = False runs the form that stops counting once a point is known to stay: the same kept set."""
    rec = _as_xyzi_records(np.asarray(xyzi, np.float32).reshape(-1, 4))
    n = len(rec)
    out = np.zeros((max(n, 1), 8), np.float32)
    cnt = np.zeros(max(n, 1), np.int32) if want_counts else None
    n_out = C.c_size_t()
    _check(load_library().lio_radius_filter(device_id, rec.ctypes.data, n, 32, float(radius), int(min_neighbors), out.ctypes.data, 32,
                                            C.byref(n_out), cnt.ctypes.data if want_counts else None), "lio_radius_filter")
    return _from_records(out, n_out.value), (cnt[:n].copy() if want_counts else None)


def ogm_default_config(**overrides):
    return _default_config(OgmConfig, "lio_ogm_default_config", overrides)


def _ogm_call(call, what, want_grid):
    """One call that asks for the geometry and the counts, a second that fills a grid of that size.  -> (grid [height, width]
    int8, row-major as nav_msgs/OccupancyGrid.data, or None; OgmInfo)."""
    info = OgmInfo()
    _check(call(None, 0, info), what)
    cells = info.width * info.height
    if not want_grid or cells == 0:
        return (np.zeros((info.height, info.width), np.int8) if want_grid else None), info
    buf = np.zeros(cells, np.int8)
    _check(call(buf.ctypes.data, buf.size, info), what)
    return buf.reshape(info.height, info.width), info


# the draft's main(): PassThroughFilter, RadiusOutlierFilter, SetMapTopicMsg
def occupancy_grid(xyz, cfg=None, want_grid=True, device_id=0):
    """-> (grid [height, width] int8 (100 = occupied) or None, OgmInfo).  xyz: [n, >= 3] float32."""
    cfg = cfg or ogm_default_config()
    a = np.asarray(xyz, np.float32)
    p = np.ascontiguousarray((a if a.ndim == 2 else a.reshape(-1, 3))[:, :3])
    lib = load_library()
    return _ogm_call(lambda g, cap, info: lib.lio_occupancy_grid(device_id, p.ctypes.data, len(p), 12, C.byref(cfg), g, cap, C.byref(info)),
                     "lio_occupancy_grid", want_grid)


# grid_map_sdf
def sdf_default_config(**overrides):
    return _default_config(SdfConfig, "lio_sdf_default_config", overrides)


class Sdf(_Owner):
    """grid_map::SignedDistanceField resident on the device: build it from an elevation grid (or from a keyframe store,
    KeyframeStore.sdf_map), then query it."""

    def __init__(self, device_id=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        self.info = SdfInfo()
        _check(self.lib.lio_sdf_create(device_id, C.byref(self.h)), "lio_sdf_create")

    def build(self, grid, resolution, length, position, cfg=None):
        """-> SdfInfo.  grid: [rows, cols] float32; length and position: those of the HeightMapInfo the grid came with."""
        cfg = cfg or sdf_default_config()
        g = np.asfortranarray(np.asarray(grid, np.float32))
        if g.ndim != 2:
            raise ValueError("grid must be [rows, cols]")
        ln, ps = (C.c_double * 2)(*length), (C.c_double * 2)(*position)
        info = self.info = SdfInfo()
        _check(self.lib.lio_sdf_build(self.h, g.ctypes.data, g.shape[0], g.shape[1], float(resolution), ln, ps, C.byref(cfg), C.byref(info)),
               "lio_sdf_build")
        return info

    def nodes(self):
        """-> [layers, cols, rows, 4] float32: {distance, dx, dy, dz} in the reference's data_ order."""
        i = self.info
        out = np.empty((i.layers, i.cols, i.rows, 4), np.float32)
        _check(self.lib.lio_sdf_nodes(self.h, out.ctypes.data, out.size), "lio_sdf_nodes")
        return out

    def query(self, positions, want_derivative=True):
        """valueAndDerivative -> (value [n] float64, derivative [n, 3] float64 or None)"""
        p = np.ascontiguousarray(positions, np.float64).reshape(-1, 3)
        val = np.empty(len(p), np.float64)
        der = np.empty((len(p), 3), np.float64) if want_derivative else None
        _check(self.lib.lio_sdf_query(self.h, p.ctypes.data, len(p), val.ctypes.data, der.ctypes.data if want_derivative else None), "lio_sdf_query")
        return val, der

    def to_point_cloud(self, decimation=1, lower=float("nan"), upper=float("nan"), cap_points=None):
        """GridMapRosConverter::toPointCloud(SignedDistanceField) -> [n, 4] float32 {x, y, z, distance}: every decimation-th
        node whose distance lies in [lower, upper] (NaN: no bound on that side), z, then y, then x.  cap_points None: asks for
        the count first, then for the points; only the kept nodes cross PCIe."""
        n = C.c_size_t()

        def call(out):
            return self.lib.lio_sdf_to_point_cloud(self.h, int(decimation), float(lower), float(upper), out.ctypes.data if out.size else None, len(out),
                                                   C.byref(n))
        out = np.zeros((0 if cap_points is None else int(cap_points), 4), np.float32)
        rc = call(out)
        if rc == -3 and cap_points is None:                                     # LIO_ERR_CAPACITY: n tells the need
            out = np.zeros((n.value, 4), np.float32)
            rc = call(out)
        _check(rc, "lio_sdf_to_point_cloud")
        return out[:n.value]

    def memory(self):
        """-> (bytes of the field, bytes of the build's workspace) the object holds on the device"""
        field, work = C.c_size_t(), C.c_size_t()
        _check(self.lib.lio_sdf_memory(self.h, C.byref(field), C.byref(work)), "lio_sdf_memory")
        return field.value, work.value

    def _release(self):
        self.lib.lio_sdf_destroy(self.h)


# grid_map_filters' MedianFillFilter
def median_fill_default_config(**overrides):
    return _default_config(MedianFillConfig, "lio_median_fill_default_config", overrides)


def median_fill(grid, resolution, cfg=None, mask_in=None, want_fill_mask=True, want_cleaned_mask=False, device_id=0):
    """-> (filled grid [rows, cols] float32, fill mask or None, cleaned mask or None, MedianFillInfo).  grid: [rows, cols]
    float32, non-finite = hole; mask_in: the fill mask of a previous run (non-zero = fill), used as it is."""
    cfg = cfg or median_fill_default_config()
    g = np.asfortranarray(np.asarray(grid, np.float32))
    if g.ndim != 2:
        raise ValueError("grid must be [rows, cols]")
    m = None if mask_in is None else np.asfortranarray(np.asarray(mask_in, np.float32))
    if m is not None and m.shape != g.shape:
        raise ValueError("mask_in must have the grid's shape")
    filled = np.empty(g.shape, np.float32, order="F")
    mask = np.empty(g.shape, np.float32, order="F") if want_fill_mask else None
    cleaned = np.empty(g.shape, np.float32, order="F") if want_cleaned_mask and m is None else None
    info = MedianFillInfo()
    ptr = lambda a: None if a is None else a.ctypes.data
    _check(load_library().lio_median_fill(device_id, g.ctypes.data, g.shape[0], g.shape[1], float(resolution), C.byref(cfg), ptr(m), filled.ctypes.data,
                                          ptr(mask), ptr(cleaned), C.byref(info)), "lio_median_fill")
    return filled, mask, cleaned, info


# GridMap::atPosition on layers resident on the device
def grid_sample_default_config(**overrides):
    return _default_config(GridSampleConfig, "lio_grid_sample_default_config", overrides)


# grid_map's region iterators on layers resident on the device
def grid_region_default_config(**overrides):
    return _default_config(GridRegionConfig, "lio_grid_region_default_config", overrides)


_REGION_KINDS = {"line": (REGION_LINE, 4), "circle": (REGION_CIRCLE, 3), "ellipse": (REGION_ELLIPSE, 5), "polygon": (REGION_POLYGON, 0)}


def pack_regions(regions):
    """regions: ("line", x0, y0, x1, y1), ("circle", cx, cy, r), ("ellipse", cx, cy, lx, ly, rotation) and
    ("polygon", [(x, y), ...]) tuples -> (a GRID_REGION_DTYPE array, the polygons' vertices [m, 2] float64)"""
    rec = np.zeros(len(regions), GRID_REGION_DTYPE)
    verts = []
    for q, r in enumerate(regions):
        kind, n_par = _REGION_KINDS[r[0]]
        rec["kind"][q] = kind
        if kind == REGION_POLYGON:
            v = np.asarray(r[1], np.float64).reshape(-1, 2)
            rec["first_vertex"][q], rec["n_vertices"][q] = len(verts), len(v)
            verts.extend(v.tolist())
        else:
            rec["p"][q, :n_par] = r[1:1 + n_par]
    return rec, np.asarray(verts, np.float64).reshape(-1, 2)


def footprint_polygons(poses, length, width):
    """poses: [n, 3] (x, y, yaw) -> (regions, vertices) of the n rectangles length (along the heading) x width centred on them:
    what Grid.region_reduce takes for a vehicle footprint along a path"""
    p = np.asarray(poses, np.float64).reshape(-1, 3)
    c, s = np.cos(p[:, 2]), np.sin(p[:, 2])
    hl, hw = 0.5 * float(length), 0.5 * float(width)
    corners = np.array([[hl, hw], [-hl, hw], [-hl, -hw], [hl, -hw]])
    verts = np.empty((len(p), 4, 2))
    verts[:, :, 0] = p[:, None, 0] + c[:, None] * corners[None, :, 0] - s[:, None] * corners[None, :, 1]
    verts[:, :, 1] = p[:, None, 1] + s[:, None] * corners[None, :, 0] + c[:, None] * corners[None, :, 1]
    rec = np.zeros(len(p), GRID_REGION_DTYPE)
    rec["kind"], rec["n_vertices"], rec["first_vertex"] = REGION_POLYGON, 4, 4 * np.arange(len(p))
    return rec, verts.reshape(-1, 2)


def _expression_names(names):
    """{variable: layer id} -> the names, the ids and their number as lio_grid_filter_expression takes them"""
    keys = [str(k).encode() for k in names]
    ids = [int(v) for v in names.values()]
    return (C.c_char_p * len(keys))(*keys), (C.c_int32 * len(ids))(*ids), len(keys)


def grid_expression_check(expression, names):
    """Compiles `expression` over `names` ({variable: layer id}) without a grid or a device; LioError names what is refused.
    -> a GRID_EXPRESSION_INFO_DTYPE record (n_ops, n_passes, layers_read, stack_depth)"""
    info = np.zeros(1, GRID_EXPRESSION_INFO_DTYPE)
    _check(load_library().lio_grid_expression_check(expression.encode(), *_expression_names(names), info.ctypes.data), "lio_grid_expression_check")
    return info[0]


def grid_expression_host(expression, names, layers):
    """The program of `expression` run serially on the host over layers [n, rows, cols] float32, names[k] standing for
    layers[k] (the text the kernels run).  -> [rows, cols] float32"""
    a = np.asarray(layers, np.float32)
    flat = np.ascontiguousarray(np.stack([l.ravel(order="F") for l in a]))
    out = np.empty(a.shape[1:], np.float32, order="F")
    keys = [str(k).encode() for k in names]
    _check(load_library().lio_debug_grid_expression_host(expression.encode(), (C.c_char_p * len(keys))(*keys), len(keys), _f32p(flat), a.shape[1], a.shape[2],
                                                         _f32p(out)), "lio_debug_grid_expression_host")
    return out


class Grid(_Owner):
    """A set of up to GRID_MAX_LAYERS [rows, cols] float32 layers resident on the device: upload them (or let
    KeyframeStore.planning_grid leave its grids here), then sample them at positions."""

    def __init__(self, device_id=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        _check(self.lib.lio_grid_create(device_id, C.byref(self.h)), "lio_grid_create")

    def set_layers(self, layers, resolution, length, position):
        """layers: [n_layers, rows, cols] float32 (or a list of [rows, cols]); they become layers 0 .. n_layers - 1"""
        a = np.asarray(layers, np.float32)
        if a.ndim != 3:
            raise ValueError("layers must be [n_layers, rows, cols]")
        flat = np.ascontiguousarray(np.stack([l.ravel(order="F") for l in a]))
        ln, ps = (C.c_double * 2)(*length), (C.c_double * 2)(*position)
        _check(self.lib.lio_grid_set_layers(self.h, flat.ctypes.data, a.shape[0], a.shape[1], a.shape[2], float(resolution), ln, ps), "lio_grid_set_layers")

    def info(self):
        info = GridInfo()
        _check(self.lib.lio_grid_info(self.h, C.byref(info)), "lio_grid_info")
        return info

    def layer(self, k):
        """-> layer k as [rows, cols] float32"""
        i = self.info()
        out = np.empty((i.rows, i.cols), np.float32, order="F")
        _check(self.lib.lio_grid_get_layer(self.h, int(k), out.ctypes.data, out.size), "lio_grid_get_layer")
        return out

    def sample(self, positions, layer_ids=(0,), cfg=None, want_method=True, **overrides):
        """atPosition -> (values [n_layers, n] float32, method used [n_layers, n] uint8 or None, GridSampleInfo).
        positions: [n, 2] float64 (x, y); overrides: method, border_mode."""
        cfg = cfg or grid_sample_default_config(**overrides)
        p = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
        ids = np.ascontiguousarray(layer_ids, np.int32).reshape(-1)
        val = np.empty((len(ids), len(p)), np.float32)
        used = np.empty((len(ids), len(p)), np.uint8) if want_method else None
        info = GridSampleInfo()
        _check(self.lib.lio_grid_sample(self.h, ids.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), C.byref(cfg), p.ctypes.data, len(p),
                                        val.ctypes.data, used.ctypes.data if want_method else None, C.byref(info)), "lio_grid_sample")
        return val, used, info

    @staticmethod
    def _regions(regions, vertices):
        if isinstance(regions, np.ndarray) and regions.dtype == GRID_REGION_DTYPE:
            rec = np.ascontiguousarray(regions)
            verts = np.zeros((0, 2)) if vertices is None else vertices
        else:
            rec, verts = pack_regions(regions)
        return rec, np.ascontiguousarray(verts, np.float64).reshape(-1, 2)

    def region_reduce(self, regions, layer_ids=(0,), vertices=None, cfg=None, **overrides):
        """grid_map's Line / Circle / Ellipse / PolygonIterator with the reduction a caller would loop for ->
        (stats [n_layers, n] GRID_REGION_STAT_DTYPE, n_cells [n] int32, status [n] uint8, GridRegionInfo).
        regions: the tuples pack_regions takes, or a GRID_REGION_DTYPE array with `vertices`; overrides: threshold."""
        cfg = cfg or grid_region_default_config(**overrides)
        rec, verts = self._regions(regions, vertices)
        ids = np.ascontiguousarray(layer_ids, np.int32).reshape(-1)
        n = len(rec)
        stats = np.zeros((len(ids), n), GRID_REGION_STAT_DTYPE)
        n_cells, status = np.zeros(n, np.int32), np.zeros(n, np.uint8)
        info = GridRegionInfo()
        _check(self.lib.lio_grid_region_reduce(self.h, ids.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), C.byref(cfg), rec.ctypes.data, n,
                                               verts.ctypes.data, len(verts), stats.ctypes.data, n_cells.ctypes.data, status.ctypes.data, C.byref(info)),
               "lio_grid_region_reduce")
        return stats, n_cells, status, info

    def region_cells(self, regions, vertices=None, cap_cells=None):
        """-> (offsets [n + 1] int64, cells int32: column-major linear indices col * rows + row in the iterator's order,
        status [n] uint8, GridRegionInfo).  cap_cells None: asks for the need first, then for the cells."""
        rec, verts = self._regions(regions, vertices)
        n = len(rec)
        offsets, status = np.zeros(n + 1, np.int64), np.zeros(n, np.uint8)
        info = GridRegionInfo()

        def call(cells):
            return self.lib.lio_grid_region_cells(self.h, rec.ctypes.data, n, verts.ctypes.data, len(verts), offsets.ctypes.data,
                                                  cells.ctypes.data if cells.size else None, cells.size, status.ctypes.data, C.byref(info))
        cells = np.zeros(0 if cap_cells is None else int(cap_cells), np.int32)
        rc = call(cells)
        if rc == -3 and cap_cells is None and 0 < offsets[n] < 2 ** 31:         # LIO_ERR_CAPACITY: offsets[n] tells the need
            cells = np.zeros(int(offsets[n]), np.int32)
            rc = call(cells)
        _check(rc, "lio_grid_region_cells")
        return offsets, cells[:int(offsets[n])], status, info

    def transform(self, dst, transform, height_layer=0, sample_ratio=0.0):
        """GridMap::getTransformedMap into `dst` (another Grid on the same device): afterwards it holds every layer this one
        holds, in the new geometry.  transform: [3, 4] (or [4, 4]) float64, the rows of [R | t].
        -> a GRID_TRANSFORM_INFO_DTYPE record."""
        t = np.ascontiguousarray(np.asarray(transform, np.float64).reshape(-1, 4)[:3]).reshape(12)
        info = np.zeros(1, GRID_TRANSFORM_INFO_DTYPE)
        _check(self.lib.lio_grid_transform(self.h, t.ctypes.data_as(C.POINTER(C.c_double)), int(height_layer), float(sample_ratio), dst.h, info.ctypes.data),
               "lio_grid_transform")
        return info[0]

    def to_occupancy(self, layer, data_min, data_max):
        """GridMapRosConverter::toOccupancyGrid on layer `layer` -> (data [rows * cols] int8 in the message's order, a
        GRID_OCCUPANCY_DESC_DTYPE record)"""
        i = self.info()
        data = np.zeros(i.rows * i.cols, np.int8)
        desc = np.zeros(1, GRID_OCCUPANCY_DESC_DTYPE)
        _check(self.lib.lio_grid_to_occupancy(self.h, int(layer), float(data_min), float(data_max), data.ctypes.data, data.size, desc.ctypes.data),
               "lio_grid_to_occupancy")
        return data, desc[0]

    def submap(self, dst, position, length):
        """GridMap::getSubmap into `dst` (another Grid on the same device): every layer this one holds, cropped to the cells
        the window position +- length / 2 covers.  -> a GRID_SUBMAP_INFO_DTYPE record; success = 0 (a requested centre outside
        the map) leaves dst without layers."""
        ps, ln = (C.c_double * 2)(*position), (C.c_double * 2)(*length)
        info = np.zeros(1, GRID_SUBMAP_INFO_DTYPE)
        _check(self.lib.lio_grid_submap(self.h, ps, ln, dst.h, info.ctypes.data), "lio_grid_submap")
        return info[0]

    def move(self, position):
        """GridMap::move, in place: the map is re-centred on `position` by whole cells; the cells that enter are NaN.
        -> a GRID_MOVE_INFO_DTYPE record"""
        ps = (C.c_double * 2)(*position)
        info = np.zeros(1, GRID_MOVE_INFO_DTYPE)
        _check(self.lib.lio_grid_move(self.h, ps, info.ctypes.data), "lio_grid_move")
        return info[0]

    def extend_to_include(self, other):
        """GridMap::extendToInclude: this map grows, aligned with its own cells, until it covers `other` (another Grid on the
        same device).  -> a GRID_EXTEND_INFO_DTYPE record"""
        info = np.zeros(1, GRID_EXTEND_INFO_DTYPE)
        _check(self.lib.lio_grid_extend_to_include(self.h, other.h, info.ctypes.data), "lio_grid_extend_to_include")
        return info[0]

    def add_data_from(self, other, extend=True, overwrite=True, layer_ids=None, basic_layers=()):
        """GridMap::addDataFrom(other, extend, overwrite, copyAllLayers, layers).  layer_ids None: every layer `other` holds.
        basic_layers: the ids that stand for basicLayers_ (the validity test that `overwrite` = False respects).
        -> a GRID_ADD_INFO_DTYPE record"""
        ids = np.zeros(0, np.int32) if layer_ids is None else np.ascontiguousarray(layer_ids, np.int32).reshape(-1)
        if layer_ids is not None and len(ids) == 0:
            raise ValueError("layer_ids is empty: pass None to copy every layer")
        mask = 0
        for k in basic_layers:
            mask |= 1 << int(k)
        info = np.zeros(1, GRID_ADD_INFO_DTYPE)
        _check(self.lib.lio_grid_add_data_from(self.h, other.h, int(bool(extend)), int(bool(overwrite)),
                                               ids.ctypes.data_as(C.POINTER(C.c_int32)) if len(ids) else None, len(ids), mask, info.ctypes.data),
               "lio_grid_add_data_from")
        return info[0]

    @staticmethod
    def _image_in(image):
        """-> (contiguous [rows, cols, channels] array, channels, depth code)"""
        a = np.asarray(image)
        if a.ndim == 2:
            a = a[:, :, None]
        depth = {np.dtype(np.uint8): IMAGE_8U, np.dtype(np.uint16): IMAGE_16U, np.dtype(np.float32): IMAGE_32F}.get(a.dtype)
        if a.ndim != 3 or depth is None:
            raise ValueError("image must be [rows, cols] or [rows, cols, channels] of uint8, uint16 or float32")
        return np.ascontiguousarray(a), a.shape[2], depth

    def to_image(self, layer, channels=1, depth=IMAGE_8U, lower=float("nan"), upper=float("nan")):
        """GridMapCvConverter::toImage -> ([rows, cols, channels] uint8 / uint16 / float32, a GRID_IMAGE_INFO_DTYPE record).
        lower and upper both NaN: the layer's finite extremes."""
        i = self.info()
        img = np.zeros((i.rows, i.cols, int(channels) if channels in (1, 3, 4) else 1), IMAGE_DTYPES.get(depth, np.uint8))
        info = np.zeros(1, GRID_IMAGE_INFO_DTYPE)
        _check(self.lib.lio_grid_to_image(self.h, int(layer), int(channels), int(depth), float(lower), float(upper), img.ctypes.data, img.nbytes,
                                          info.ctypes.data), "lio_grid_to_image")
        return img, info[0]

    def add_layer_from_image(self, layer, image, lower=0.0, upper=1.0, alpha_threshold=0.5, resolution=0.0, position=(0.0, 0.0)):
        """GridMapCvConverter::addLayerFromImage into layer `layer`; a grid without layers takes its geometry from the image's
        size, `resolution` and `position` (initializeFromImage).  -> a GRID_FROM_IMAGE_INFO_DTYPE record"""
        a, channels, depth = self._image_in(image)
        ps = (C.c_double * 2)(*position)
        info = np.zeros(1, GRID_FROM_IMAGE_INFO_DTYPE)
        _check(self.lib.lio_grid_add_layer_from_image(self.h, int(layer), a.ctypes.data, a.shape[0], a.shape[1], channels, depth, float(lower), float(upper),
                                                      float(alpha_threshold), float(resolution), ps, info.ctypes.data), "lio_grid_add_layer_from_image")
        return info[0]

    def add_color_layer_from_image(self, layer, image, resolution=0.0, position=(0.0, 0.0)):
        """GridMapCvConverter::addColorLayerFromImage (uint8, 3 or 4 channels): the cells hold (c0 << 16) + (c1 << 8) + c2 as
        a float's bits.  -> a GRID_FROM_IMAGE_INFO_DTYPE record"""
        a, channels, depth = self._image_in(image)
        ps = (C.c_double * 2)(*position)
        info = np.zeros(1, GRID_FROM_IMAGE_INFO_DTYPE)
        _check(self.lib.lio_grid_add_color_layer_from_image(self.h, int(layer), a.ctypes.data, a.shape[0], a.shape[1], channels, depth, float(resolution), ps,
                                                            info.ctypes.data), "lio_grid_add_color_layer_from_image")
        return info[0]

    def from_occupancy(self, layer, data, width, height, resolution, origin):
        """GridMapRosConverter::fromOccupancyGrid into layer `layer`: data [width * height] int8 in the message's order.
        -> a GRID_FROM_OCCUPANCY_INFO_DTYPE record"""
        d = np.ascontiguousarray(data, np.int8).reshape(-1)
        og = (C.c_double * 2)(*origin)
        info = np.zeros(1, GRID_FROM_OCCUPANCY_INFO_DTYPE)
        _check(self.lib.lio_grid_from_occupancy(self.h, int(layer), d.ctypes.data, d.size, int(width), int(height), float(resolution), og, info.ctypes.data),
               "lio_grid_from_occupancy")
        return info[0]

    def _compacted(self, what, call, fields, dtype, cap):
        """asks for the count first when cap is None (LIO_ERR_CAPACITY tells the need), then for the records"""
        n = C.c_size_t()
        out = np.zeros((0 if cap is None else int(cap), fields), dtype)
        rc = call(out, n)
        if rc == -3 and cap is None:
            out = np.zeros((n.value, fields), dtype)
            rc = call(out, n)
        _check(rc, what)
        return out[:n.value]

    def to_point_cloud(self, point_layer, layer_ids=None, basic_layers=(), cap_points=None):
        """GridMapRosConverter::toPointCloud -> [n, F] float32 in the iterator's order: point_layer gives x, y, z, every other
        listed layer one field (its words unchanged).  layer_ids None: every layer the grid holds, ascending."""
        held = self.info().layer_mask
        ids = np.ascontiguousarray([k for k in range(GRID_MAX_LAYERS) if (held >> k) & 1] if layer_ids is None else layer_ids, np.int32).reshape(-1)
        mask = 0
        for k in basic_layers:
            mask |= 1 << int(k)
        fields = sum(3 if int(k) == int(point_layer) else 1 for k in ids)
        nf = C.c_int32()

        def call(out, n):
            return self.lib.lio_grid_to_point_cloud(self.h, int(point_layer), ids.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), mask,
                                                    out.ctypes.data if out.size else None, len(out), C.byref(n), C.byref(nf))
        return self._compacted("lio_grid_to_point_cloud", call, max(fields, 1), np.float32, cap_points)

    def to_grid_cells(self, layer, lower, upper, cap_cells=None):
        """GridMapRosConverter::toGridCells -> [n, 2] float64: the centres of the cells of `layer` within [lower, upper]"""
        def call(out, n):
            return self.lib.lio_grid_to_grid_cells(self.h, int(layer), float(lower), float(upper), out.ctypes.data if out.size else None, len(out), C.byref(n))
        return self._compacted("lio_grid_to_grid_cells", call, 2, np.float64, cap_cells)

    def filter_radius(self, in_layer, out_layer, op, radius):
        """grid_map_filters' MinInRadiusFilter (op GF_MIN) or MeanInRadiusFilter (GF_MEAN) of layer `in_layer` into `out_layer`,
        which it replaces.  -> a GRID_FILTER_INFO_DTYPE record"""
        info = np.zeros(1, GRID_FILTER_INFO_DTYPE)
        _check(self.lib.lio_grid_filter_radius(self.h, int(in_layer), int(out_layer), int(op), float(radius), info.ctypes.data), "lio_grid_filter_radius")
        return info[0]

    def filter_window(self, in_layer, out_layer, op, edge_handling, window_size=0, window_length=0.0, weights=None):
        """SlidingWindowMathExpressionFilter: op GW_SUM .. GW_WEIGHTED_SUM over the window of edge_handling GW_INSIDE ..
        GW_EDGE_MEAN.  window_size 0: derived from window_length.  weights: [size, size] (K[a, b] against W[a, b]), with
        GW_WEIGHTED_SUM only.  out_layer may be in_layer.  -> a GRID_FILTER_INFO_DTYPE record"""
        k = None if weights is None else np.ascontiguousarray(np.asarray(weights, np.float32).ravel(order="F"))
        info = np.zeros(1, GRID_FILTER_INFO_DTYPE)
        _check(self.lib.lio_grid_filter_window(self.h, int(in_layer), int(out_layer), int(op), int(edge_handling), int(window_size), float(window_length),
                                               None if k is None else _f32p(k), info.ctypes.data), "lio_grid_filter_window")
        return info[0]

    def filter_curvature(self, in_layer, out_layer):
        """CurvatureFilter of layer `in_layer` into `out_layer`.  -> a GRID_FILTER_INFO_DTYPE record"""
        info = np.zeros(1, GRID_FILTER_INFO_DTYPE)
        _check(self.lib.lio_grid_filter_curvature(self.h, int(in_layer), int(out_layer), info.ctypes.data), "lio_grid_filter_curvature")
        return info[0]

    def filter_threshold(self, condition_layer, out_layer, upper, threshold, set_to):
        """ThresholdFilter, in place on `out_layer`: upper False sets where !(condition >= threshold), True where
        !(condition <= threshold).  -> a GRID_FILTER_INFO_DTYPE record (n_changed: the cells set)"""
        info = np.zeros(1, GRID_FILTER_INFO_DTYPE)
        _check(self.lib.lio_grid_filter_threshold(self.h, int(condition_layer), int(out_layer), int(bool(upper)), float(threshold), float(set_to),
                                                  info.ctypes.data), "lio_grid_filter_threshold")
        return info[0]

    def duplicate_layer(self, in_layer, out_layer):
        """DuplicationFilter: `out_layer` becomes a copy of `in_layer`, device to device"""
        _check(self.lib.lio_grid_duplicate_layer(self.h, int(in_layer), int(out_layer)), "lio_grid_duplicate_layer")

    def delete_layers(self, layer_ids):
        """DeletionFilter: the listed layers leave the object"""
        ids = np.ascontiguousarray(layer_ids, np.int32).reshape(-1)
        _check(self.lib.lio_grid_delete_layers(self.h, ids.ctypes.data_as(C.POINTER(C.c_int32)) if len(ids) else None, len(ids)), "lio_grid_delete_layers")

    def filter_expression(self, expression, names, out_layer):
        """MathExpressionFilter: the EigenLab `expression` over the layers that `names` ({variable: layer id}) lists, stored as
        `out_layer`, which may be a layer it reads.  -> a GRID_EXPRESSION_INFO_DTYPE record"""
        info = np.zeros(1, GRID_EXPRESSION_INFO_DTYPE)
        _check(self.lib.lio_grid_filter_expression(self.h, expression.encode(), *_expression_names(names), int(out_layer), info.ctypes.data),
               "lio_grid_filter_expression")
        return info[0]

    def memory(self):
        """-> bytes the object holds on the device"""
        n = C.c_size_t()
        _check(self.lib.lio_grid_memory(self.h, C.byref(n)), "lio_grid_memory")
        return n.value

    def _release(self):
        self.lib.lio_grid_destroy(self.h)


def kf_store_planning_grid(store, grid, pose, *args, **kw):
    """KeyframeStore.planning_map's arguments and result; the chain also leaves its grids in `grid` (a Grid, or None)"""
    return store.planning_grid(grid, pose, *args, **kw)


# signedDistanceFromOccupancy (SignedDistance2d.cpp:272-287) on the data of a nav_msgs/OccupancyGrid
def occupancy_sdf(grid, resolution, occupied_min=100, device_id=0):
    """-> [height, width] float32 in the grid's layout.  grid: [height, width] int8, row-major as occupancy_grid returns it."""
    g = np.ascontiguousarray(grid, np.int8)
    if g.ndim != 2:
        raise ValueError("grid must be [height, width]")
    out = np.empty(g.shape, np.float32)
    _check(load_library().lio_occupancy_sdf(device_id, g.ctypes.data, g.shape[1], g.shape[0], float(resolution), int(occupied_min), out.ctypes.data),
           "lio_occupancy_sdf")
    return out


# extractCloud, MO:1556-1588
def assemble_map(clouds_xyzi, poses, leaf, s2m=None, device_id=0, want_output=True):
    recs = [_as_xyzi_records(c) for c in clouds_xyzi]
    n = len(recs)
    ptrs = (C.c_void_p * max(n, 1))(*[r.ctypes.data for r in recs])
    npts = (C.c_size_t * max(n, 1))(*[len(r) for r in recs])
    p = np.ascontiguousarray(poses, np.float32).reshape(n, 6)
    total = sum(len(r) for r in recs)
    out = _scratch("assemble", (max(total, 1), 8)) if want_output else None
    n_out = C.c_size_t()
    rc = _check(load_library().lio_assemble_map(s2m.h if s2m is not None else None, device_id, n, ptrs, npts, 32,
                                                _f32p(p), leaf, out.ctypes.data if want_output else None, 32,
                                                C.byref(n_out)), "lio_assemble_map")
    return (_from_records(out, n_out.value) if want_output else None), n_out.value, rc


class KeyframeStore(_Owner):
    """surfCloudKeyFrames (MO:128) kept in HBM."""

    def __init__(self, device_id=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        _check(self.lib.lio_kf_store_create(device_id, C.byref(self.h)), "lio_kf_store_create")

    def add(self, cloud_xyzi):                      # surfCloudKeyFrames.push_back, MO:2141
        rec = _as_xyzi_records(cloud_xyzi)
        kid = C.c_int32()
        _check(self.lib.lio_kf_store_add(self.h, rec.ctypes.data, len(rec), 32, C.byref(kid)), "lio_kf_store_add")
        return kid.value

    def add_from_handle(self, s2m, scan=0):         # MO:2136-2142 without leaving the device
        kid = C.c_int32()
        _check(self.lib.lio_kf_store_add_from_handle(self.h, s2m.h, scan, C.byref(kid)), "lio_kf_store_add_from_handle")
        return kid.value

    def add_device(self, dev_ptr, n, stride):
        kid = C.c_int32()
        _check(self.lib.lio_kf_store_add_device(self.h, C.c_void_p(dev_ptr), n, stride, C.byref(kid)), "lio_kf_store_add_device")
        return kid.value

    def __len__(self):
        return self.lib.lio_kf_store_count(self.h)

    def assemble(self, ids, poses, leaf, s2m=None, want_output=True, max_out=None):   # extractCloud, MO:1556-1588
        ids_a = np.ascontiguousarray(ids, np.int32)
        p = np.ascontiguousarray(poses, np.float32).reshape(len(ids_a), 6)
        if want_output and max_out is None:          # room for every selected point: the filter may pass its input through
            max_out = sum(int(self.lib.lio_kf_store_points(self.h, int(i))) for i in ids_a)
        out = np.zeros((max(max_out or 1, 1), 8), np.float32) if want_output else None
        n_out = C.c_size_t()
        rc = _check(self.lib.lio_assemble_map_resident(
            s2m.h if s2m is not None else None, self.h, len(ids_a), ids_a.ctypes.data_as(C.POINTER(C.c_int32)), _f32p(p),
            leaf, out.ctypes.data if want_output else None, 32, C.byref(n_out)), "lio_assemble_map_resident")
        return (_from_records(out, n_out.value) if want_output else None), n_out.value, rc

    def set_poses(self, first, poses, times=None):   # cloudKeyPoses6D: MO:2107-2120 (one), correctPoses MO:2184-2196 (all)
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        t = None if times is None else np.ascontiguousarray(times, np.float64).reshape(len(p))
        _check(self.lib.lio_kf_store_set_poses(self.h, first, len(p), _f32p(p),
                                               None if t is None else t.ctypes.data_as(C.POINTER(C.c_double))),
               "lio_kf_store_set_poses")

    def assemble_nearby(self, time_cur, leaf, s2m=None, want_ids=True, want_output=True, **cfg):
        """extractSurroundingKeyFrames MO:1590-1603 + extractCloud MO:1556-1588 on the device -> (map or None, n_map, ids or
        None, rc).  cfg: search_radius, pose_density, recent_window_s (lio_nearby_config)."""
        c = nearby_default_config(**cfg)
        n = len(self)
        ids = np.zeros(max(2 * n, 1), np.int32) if want_ids else None   # the list holds at most 2N entries
        cap = max(sum(int(self.lib.lio_kf_store_points(self.h, i)) for i in range(n)), 1) if want_output else 0
        while True:
            out = np.zeros((cap, 8), np.float32) if want_output else None
            n_ids, n_out = C.c_int32(), C.c_size_t()
            rc = self.lib.lio_assemble_map_nearby(
                s2m.h if s2m is not None else None, self.h, C.byref(c), time_cur, leaf,
                ids.ctypes.data_as(C.POINTER(C.c_int32)) if want_ids else None, len(ids) if want_ids else 0, C.byref(n_ids),
                out.ctypes.data if want_output else None, 32, cap, C.byref(n_out))
            if want_output and rc == -1 and n_out.value > cap:    # (more map than one copy of every cloud: room, and again)
                cap = n_out.value
                continue
            _check(rc, "lio_assemble_map_nearby")
            break
        return ((_from_records(out, n_out.value) if want_output else None), n_out.value,
                (ids[:n_ids.value].copy() if want_ids else None), rc)

    def loop_icp(self, key_cur, key_pre, search_num, leaf, cfg=None, pose_index=-1, want_clouds=False):
        """performRSLoopClosure MO:1098-1143 on the device -> (IcpResult, rc, clouds or None); clouds = (source submap,
        target submap, closed_cloud) as [n,4] arrays."""
        cfg = cfg or icp_default_config()
        res = IcpResult()
        cl = None
        if want_clouds:
            pts = lambda k: int(self.lib.lio_kf_store_points(self.h, k))
            cap_s = max(pts(key_cur), 1)
            cap_t = max(sum(pts(k) for k in range(max(key_pre - search_num, 0), min(key_pre + search_num, len(self) - 1) + 1)), 1)
            bufs = [np.zeros((cap_s, 8), np.float32), np.zeros((cap_t, 8), np.float32), np.zeros((cap_s, 8), np.float32)]
            cl = IcpClouds(bufs[0].ctypes.data, bufs[1].ctypes.data, bufs[2].ctypes.data, cap_s, cap_t, cap_s, 0, 0, 0, 32)
        rc = _check(self.lib.lio_kf_store_loop_icp(self.h, key_cur, key_pre, search_num, pose_index, leaf, C.byref(cfg), C.byref(res),
                                                   C.byref(cl) if cl is not None else None), "lio_kf_store_loop_icp")
        clouds = None
        if want_clouds:
            clouds = (_from_records(bufs[0], cl.n_source), _from_records(bufs[1], cl.n_target), _from_records(bufs[2], cl.n_closed))
        return res, rc, clouds

    def local_map(self, pose, cfg=None, want_output=True, max_out=None):   # publishLocalMap, MO:2447-2540
        """-> (cloud [m,4] in the yaw-aligned vehicle frame or None, LocalMapInfo, rc).  pose: transformTobeMapped."""
        cfg = cfg or local_map_default_config()
        p = np.ascontiguousarray(pose, np.float32).reshape(6)
        n = len(self)
        if want_output and max_out is None:          # room for every summed point: nothing downstream adds any
            max_out = sum(int(self.lib.lio_kf_store_points(self.h, i)) for i in range(max(n - max(cfg.n_keyframes, 0), 0), n))
        out = np.zeros((max(max_out or 1, 1), 8), np.float32) if want_output else None
        n_out, info = C.c_size_t(), LocalMapInfo()
        rc = _check(self.lib.lio_kf_store_local_map(self.h, C.byref(cfg), _f32p(p), out.ctypes.data if want_output else None, 32,
                                                    len(out) if want_output else 0, C.byref(n_out), C.byref(info)),
                    "lio_kf_store_local_map")
        return (_from_records(out, n_out.value) if want_output else None), info, rc

    def height_map(self, pose, lm_cfg=None, cfg=None, want_grid=True):   # publishLocalMap + cloudMapInfoHandler, without the cloud
        """-> (elevation grid [rows, cols] or None, HeightMapInfo, LocalMapInfo)."""
        lm_cfg = lm_cfg or local_map_default_config()
        cfg = cfg or height_map_default_config()
        p = np.ascontiguousarray(pose, np.float32).reshape(6)
        lm_info = LocalMapInfo()
        grid, info = _height_map_call(
            lambda g, cap, info: self.lib.lio_kf_store_height_map(self.h, C.byref(lm_cfg), _f32p(p), C.byref(cfg), g, cap, C.byref(lm_info),
                                                                  C.byref(info)), "lio_kf_store_height_map", want_grid)
        return grid, info, lm_info

    def terrain_map(self, pose, lm_cfg=None, hm_cfg=None, cfg=None, want_grid=True):   # height_map, then the filter chain on the device grid
        """-> (elevation grid [rows, cols] or None, {layer name: [rows, cols]}, TerrainInfo, HeightMapInfo, LocalMapInfo).  One
        call into buffers kept from the last one; a second only when the grid has outgrown them."""
        lm_cfg = lm_cfg or local_map_default_config()
        hm_cfg = hm_cfg or height_map_default_config()
        cfg = cfg or terrain_default_config()
        p = np.ascontiguousarray(pose, np.float32).reshape(6)
        n_layers = bin(cfg.layers & 0xff).count("1")
        lm_info, hm_info, info = LocalMapInfo(), HeightMapInfo(), TerrainInfo()

        def make_call(cells):
            grid = _scratch("terrain_grid", (cells,))
            layers = _scratch("terrain_layers", (max(cells * n_layers, 1),))
            return self.lib.lio_kf_store_terrain_map(self.h, C.byref(lm_cfg), _f32p(p), C.byref(hm_cfg), C.byref(cfg),
                                                     grid.ctypes.data if want_grid else None, grid.size, layers.ctypes.data, layers.size,
                                                     C.byref(lm_info), C.byref(hm_info), C.byref(info)), (grid, layers)
        grid, layers = _call_with_cells("terrain_map", 1 << 16, make_call, lambda: info.rows * info.cols, "lio_kf_store_terrain_map")
        n = info.rows * info.cols
        elev = grid[:n].reshape((info.rows, info.cols), order="F").copy(order="F") if want_grid else None
        return elev, _terrain_layers_out(layers, info, cfg.layers), info, hm_info, lm_info

    def sdf_map(self, sdf, pose, lm_cfg=None, hm_cfg=None, cfg=None, want_grid=True):   # height_map, then grid_map_sdf on the device grid
        """Builds `sdf` (an Sdf) -> (elevation grid [rows, cols] or None, SdfInfo, HeightMapInfo, LocalMapInfo)."""
        lm_cfg = lm_cfg or local_map_default_config()
        hm_cfg = hm_cfg or height_map_default_config()
        cfg = cfg or sdf_default_config()
        p = np.ascontiguousarray(pose, np.float32).reshape(6)
        lm_info, hm_info = LocalMapInfo(), HeightMapInfo()
        info = sdf.info = SdfInfo()

        def make_call(cells):
            grid = _scratch("sdf_grid", (cells,))
            return self.lib.lio_kf_store_sdf(self.h, C.byref(lm_cfg), _f32p(p), C.byref(hm_cfg), C.byref(cfg), grid.ctypes.data if want_grid else None,
                                             grid.size, sdf.h, C.byref(lm_info), C.byref(hm_info), C.byref(info)), grid
        grid = _call_with_cells("sdf_map", 1 << 16, make_call, lambda: hm_info.rows * hm_info.cols if want_grid else 0, "lio_kf_store_sdf")
        n = hm_info.rows * hm_info.cols
        elev = grid[:n].reshape((hm_info.rows, hm_info.cols), order="F").copy(order="F") if want_grid else None
        return elev, info, hm_info, lm_info

    def planning_grid(self, grid_out, pose, *args, **kw):
        """planning_map, which also leaves the raw grid (layer 0), the filled grid (1) and the eight terrain layers (2 .. 9) in
        grid_out (a Grid; None: planning_map through the same entry point)."""
        return self._planning("lio_kf_store_planning_grid", (grid_out.h if grid_out is not None else None,), pose, *args, **kw)

    def planning_map(self, pose, lm_cfg=None, hm_cfg=None, fill_cfg=None, terrain_cfg=None, sdf=None, sdf_cfg=None, want_grid=True,
                     want_filled=True, want_fill_mask=True):
        """The height map's chain once, then the median fill (fill_cfg), the terrain layers (terrain_cfg) and the field (sdf, an
        Sdf) on the grid it leaves on the device; a stage whose argument is None is absent.  -> dict: grid, filled, fill_mask
        ([rows, cols] or None), layers ({name: [rows, cols]} or None), lm_info, hm_info, fill_info, terrain_info, sdf_info."""
        return self._planning("lio_kf_store_planning_map", (), pose, lm_cfg, hm_cfg, fill_cfg, terrain_cfg, sdf, sdf_cfg, want_grid, want_filled,
                              want_fill_mask)

    def _planning(self, entry, more_args, pose, lm_cfg=None, hm_cfg=None, fill_cfg=None, terrain_cfg=None, sdf=None, sdf_cfg=None, want_grid=True,
                  want_filled=True, want_fill_mask=True):
        """the entry point `entry` with the chain's arguments followed by more_args"""
        lm_cfg = lm_cfg or local_map_default_config()
        hm_cfg = hm_cfg or height_map_default_config()
        if sdf is not None and sdf_cfg is None:
            sdf_cfg = sdf_default_config()
        p = np.ascontiguousarray(pose, np.float32).reshape(6)
        n_layers = bin(terrain_cfg.layers & 0xff).count("1") if terrain_cfg is not None else 0
        lm_info, hm_info, fill_info, terrain_info, sdf_info = LocalMapInfo(), HeightMapInfo(), MedianFillInfo(), TerrainInfo(), SdfInfo()
        if sdf is not None:
            sdf.info = sdf_info
        want_filled = want_filled and fill_cfg is not None
        want_fill_mask = want_fill_mask and fill_cfg is not None
        ref = lambda c: None if c is None else C.byref(c)

        def make_call(cells):
            bufs = {k: _scratch("planning_" + k, (max(cells * m, 1),)) for k, m in (("grid", 1), ("filled", 1), ("fill_mask", 1), ("layers", n_layers))}
            io = PlanningMapBuffers()
            for k, want in (("grid", want_grid), ("filled", want_filled), ("fill_mask", want_fill_mask), ("layers", n_layers > 0)):
                setattr(io, k, bufs[k].ctypes.data if want else None)
                setattr(io, k + "_cap", bufs[k].size if want else 0)
            return getattr(self.lib, entry)(self.h, C.byref(lm_cfg), _f32p(p), C.byref(hm_cfg), ref(fill_cfg), ref(terrain_cfg),
                                            sdf.h if sdf is not None else None, ref(sdf_cfg), C.byref(io), C.byref(lm_info),
                                            C.byref(hm_info), C.byref(fill_info), C.byref(terrain_info), C.byref(sdf_info), *more_args), bufs
        bufs = _call_with_cells("planning_map", 1 << 16, make_call, lambda: hm_info.rows * hm_info.cols, entry)
        n, shape = hm_info.rows * hm_info.cols, (hm_info.rows, hm_info.cols)
        take = lambda k, want: bufs[k][:n].reshape(shape, order="F").copy(order="F") if want else None
        return dict(grid=take("grid", want_grid), filled=take("filled", want_filled), fill_mask=take("fill_mask", want_fill_mask),
                    layers=_terrain_layers_out(bufs["layers"], terrain_info, terrain_cfg.layers) if n_layers else None,
                    lm_info=lm_info, hm_info=hm_info, fill_info=fill_info, terrain_info=terrain_info, sdf_info=sdf_info)

    def global_map(self, cfg=None, want_ids=True, want_output=True):   # publishGlobalMap, MO:992-1041
        """-> (cloud [m,4] or None, ids (the kept list, duplicates included) or None, GlobalMapInfo)."""
        cfg = cfg or global_map_default_config()
        n = len(self)
        ids = np.zeros(max(n, 1), np.int32) if want_ids else None        # without the recent suffix: at most one entry per pose
        cap = max(sum(int(self.lib.lio_kf_store_points(self.h, i)) for i in range(n)), 1) if want_output else 0
        while True:
            out = np.zeros((cap, 8), np.float32) if want_output else None
            n_ids, n_out, info = C.c_int32(), C.c_size_t(), GlobalMapInfo()
            rc = self.lib.lio_kf_store_global_map(
                self.h, C.byref(cfg), ids.ctypes.data_as(C.POINTER(C.c_int32)) if want_ids else None, len(ids) if want_ids else 0,
                C.byref(n_ids), out.ctypes.data if want_output else None, 32, cap, C.byref(n_out), C.byref(info))
            if want_output and rc == -1 and n_out.value > cap:    # (a keyframe selected twice: more map than one copy of every cloud)
                cap = n_out.value
                continue
            _check(rc, "lio_kf_store_global_map")
            break
        return ((_from_records(out, n_out.value) if want_output else None), (ids[:n_ids.value].copy() if want_ids else None), info)

    def export_map(self, resolution=0.0, chunk_points=0, stride=32, want_full=True, want_ds=True):   # saveMapService, MO:935-962
        """-> (globalSurfCloud [n,4] or None, its filtered copy [m,4] or None (None when resolution == 0), (n_full, n_ds,
        voxel_passthrough)).  A first call counts, a second fills."""
        cfg = ExportConfig(float(resolution), int(chunk_points))
        n_full, n_ds, vpt = C.c_size_t(), C.c_size_t(), C.c_int32()
        _check(self.lib.lio_kf_store_export_map(self.h, C.byref(cfg), None, stride, 0, C.byref(n_full), None, stride, 0, C.byref(n_ds),
                                                C.byref(vpt)), "lio_kf_store_export_map")
        want_ds = want_ds and resolution != 0
        if not (want_full or want_ds):
            return None, None, (n_full.value, n_ds.value, vpt.value)
        full = np.zeros(max(n_full.value, 1) * stride, np.uint8) if want_full else None
        ds = np.zeros(max(n_ds.value, 1) * stride, np.uint8) if want_ds else None
        _check(self.lib.lio_kf_store_export_map(self.h, C.byref(cfg), full.ctypes.data if want_full else None, stride, n_full.value,
                                                C.byref(n_full), ds.ctypes.data if want_ds else None, stride, n_ds.value, C.byref(n_ds),
                                                C.byref(vpt)), "lio_kf_store_export_map")
        return ((_from_records_stride(full, n_full.value, stride) if want_full else None),
                (_from_records_stride(ds, n_ds.value, stride) if want_ds else None), (n_full.value, n_ds.value, vpt.value))

    def occupancy_grid(self, map_resolution=0.0, cfg=None, want_grid=True):   # the draft ogmGeneration.cpp on the saved map
        """-> (grid [height, width] int8 or None, OgmInfo, n_map = the points of the map the chain ran on)."""
        cfg = cfg or ogm_default_config()
        n_map = C.c_size_t()
        grid, info = _ogm_call(lambda g, cap, info: self.lib.lio_kf_store_occupancy_grid(self.h, float(map_resolution), C.byref(cfg), g, cap,
                                                                                         C.byref(n_map), C.byref(info)),
                               "lio_kf_store_occupancy_grid", want_grid)
        return grid, info, n_map.value

    def get_keyframe(self, kid, pose=None):           # surfCloudKeyFrames[kid], or transformPointCloud of it (MO:849-868)
        """-> [n,4] (x, y, z, intensity): the stored cloud bit for bit, or under pose = [roll,pitch,yaw,x,y,z]."""
        p = None if pose is None else np.ascontiguousarray(pose, np.float32).reshape(6)
        pp = None if p is None else _f32p(p)
        n = C.c_size_t()
        _check(self.lib.lio_kf_store_get_keyframe(self.h, kid, pp, None, 32, 0, C.byref(n)), "lio_kf_store_get_keyframe")
        out = np.zeros((max(n.value, 1), 8), np.float32)
        _check(self.lib.lio_kf_store_get_keyframe(self.h, kid, pp, out.ctypes.data, 32, len(out), C.byref(n)), "lio_kf_store_get_keyframe")
        return _from_records(out, n.value)

    def detect_loop(self, radius, time_diff, time_cur):   # detectLoopClosureDistance, MO:1271-1304
        """-> (key_cur, key_pre) or None."""
        kc, kp = C.c_int32(), C.c_int32()
        rc = _check(self.lib.lio_kf_store_detect_loop(self.h, radius, time_diff, time_cur, C.byref(kc), C.byref(kp)),
                    "lio_kf_store_detect_loop")
        return (kc.value, kp.value) if rc == 1 else None

    # ---- Scan Context (performSCLoopClosure MO:1163-1269): descriptor k belongs to keyframe k
    @staticmethod
    def _sc_cfg(cfg):
        return C.byref(cfg) if cfg is not None else None

    def sc_add(self, cloud, cfg=None):               # scManager.makeAndSaveScancontextAndKeys, MO:2156
        pts, stride = _as_points(cloud)
        kid = C.c_int32()
        _check(self.lib.lio_kf_store_sc_add(self.h, pts.ctypes.data, len(pts), stride, self._sc_cfg(cfg), C.byref(kid)), "lio_kf_store_sc_add")
        return kid.value

    def sc_add_device(self, dev_ptr, n, stride, cfg=None):
        kid = C.c_int32()
        _check(self.lib.lio_kf_store_sc_add_device(self.h, C.c_void_p(dev_ptr), n, stride, self._sc_cfg(cfg), C.byref(kid)),
               "lio_kf_store_sc_add_device")
        return kid.value

    def sc_add_from_handle(self, s2m, cfg=None):     # the cloud s2m's last downsampleAndScan2MapOptimization staged, in place
        kid = C.c_int32()
        _check(self.lib.lio_kf_store_sc_add_from_handle(self.h, s2m.h, self._sc_cfg(cfg), C.byref(kid)), "lio_kf_store_sc_add_from_handle")
        return kid.value

    def sc_count(self):
        return self.lib.lio_kf_store_sc_count(self.h)

    def sc_geometry(self):
        """-> (num_rings, num_sectors) of the store's descriptors; (0, 0) while it holds none."""
        r, s = C.c_int32(), C.c_int32()
        _check(self.lib.lio_kf_store_sc_geometry(self.h, C.byref(r), C.byref(s)), "lio_kf_store_sc_geometry")
        return r.value, s.value

    def sc_get(self, kid):
        """-> (desc [rings, sectors], ring_key, sector_key) of descriptor kid, sized by the store's geometry."""
        rings, sectors = self.sc_geometry()
        desc, rk, sk = np.zeros((rings, sectors), np.float32), np.zeros(rings, np.float32), np.zeros(sectors, np.float64)
        _check(self.lib.lio_kf_store_sc_get(self.h, kid, desc.ctypes.data, rk.ctypes.data, sk.ctypes.data), "lio_kf_store_sc_get")
        return desc, rk, sk

    def sc_detect(self, cfg=None):                   # scManager.detectLoopClosureID, MO:1175
        """-> ScResult; loop_id = -1: no loop.  Then loop_icp(len(self) - 1, loop_id, search_num, leaf, pose_index=0)."""
        cfg = cfg or sc_default_config()
        res = ScResult()
        _check(self.lib.lio_kf_store_sc_detect(self.h, C.byref(cfg), C.byref(res)), "lio_kf_store_sc_detect")
        return res

    def _release(self):
        self.lib.lio_kf_store_destroy(self.h)
