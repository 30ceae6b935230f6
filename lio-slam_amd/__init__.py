"""MI355X-native scan-to-map registration path (C ABI: include/liogpu.h).

This package is the Python test/bench harness around lio-slam_amd/libliogpu.so
(hand-written HIP for gfx950).  The directory name is not a Python identifier;
import it with `importlib.import_module("lio-slam_amd")`.  There is no CPU
fallback: a missing library or GPU raises.
"""
from .api import (LioError, ScanToMap, S2MConfig, S2MResult, S2MProfile, DeskewConfig,
                  lib_path, load_library, build_library, deskew, curvature, imu_deskew_info,
                  transform_update, pack_xyzirt, deskew_default_config, voxel_grid, assemble_map, KeyframeStore, STATUS_NAMES,
                  extract_features, FeatureConfig, range_image, RangeImageConfig, PinnedBuffer, DeviceBuffer, PC2Layout, deskew_pc2,
                  NearbyConfig, nearby_default_config, IcpConfig, IcpResult, IcpClouds, ICP_STATES, icp_default_config, icp_align,
                  icp_debug_trace, IcpGridInfo, icp_debug_grid, sor_debug_grid, ScConfig, ScResult, sc_default_config, sc_make, sc_distance,
                  LocalMapConfig, LocalMapInfo, sor_filter, local_map_default_config,
                  HeightMapConfig, HeightMapInfo, height_map, height_map_default_config,
                  TerrainConfig, TerrainInfo, TERRAIN_LAYERS, terrain_layers, terrain_default_config,
                  GlobalMapConfig, GlobalMapInfo, ExportConfig, global_map_default_config, STAGED_DS, STAGED_RAW,
                  OgmConfig, OgmInfo, ogm_default_config, radius_filter, occupancy_grid,
                  SdfConfig, SdfInfo, Sdf, SDF_NODE_LIMIT, sdf_default_config, occupancy_sdf,
                  MedianFillConfig, MedianFillInfo, PlanningMapBuffers, median_fill, median_fill_default_config,
                  Grid, GridSampleConfig, GridSampleInfo, GridInfo, grid_sample_default_config, kf_store_planning_grid, GRID_MAX_LAYERS,
                  GRID_NEAREST, GRID_LINEAR, GRID_CUBIC_CONVOLUTION, GRID_CUBIC, GRID_OUTSIDE, GRID_LAYER_ELEVATION, GRID_LAYER_FILLED,
                  GRID_LAYER_TERRAIN,
                  GridRegion, GridRegionConfig, GridRegionStat, GridRegionInfo, GRID_REGION_DTYPE, GRID_REGION_STAT_DTYPE,
                  grid_region_default_config, pack_regions, footprint_polygons, REGION_LINE, REGION_CIRCLE, REGION_ELLIPSE, REGION_POLYGON,
                  REGION_OK, REGION_EMPTY, REGION_INVALID, REGION_MAX_VERTICES, REGION_MAX_WALK,
                  GRID_TRANSFORM_INFO_DTYPE, GRID_OCCUPANCY_DESC_DTYPE, GRID_TRANSFORM_MAX_SOURCE_CELLS,
                  GRID_SUBMAP_INFO_DTYPE, GRID_MOVE_INFO_DTYPE, GRID_EXTEND_INFO_DTYPE, GRID_ADD_INFO_DTYPE,
                  GRID_IMAGE_INFO_DTYPE, GRID_FROM_IMAGE_INFO_DTYPE, GRID_FROM_OCCUPANCY_INFO_DTYPE, IMAGE_8U, IMAGE_16U, IMAGE_32F)

__all__ = ["LioError", "ScanToMap", "S2MConfig", "S2MResult", "S2MProfile", "DeskewConfig",
           "lib_path", "load_library", "build_library", "deskew", "curvature", "imu_deskew_info",
           "transform_update", "pack_xyzirt", "deskew_default_config", "voxel_grid", "assemble_map", "KeyframeStore", "STATUS_NAMES",
           "extract_features", "FeatureConfig", "range_image", "RangeImageConfig", "PinnedBuffer", "DeviceBuffer", "PC2Layout", "deskew_pc2",
           "NearbyConfig", "nearby_default_config", "IcpConfig", "IcpResult", "IcpClouds", "ICP_STATES", "icp_default_config", "icp_align",
           "icp_debug_trace", "IcpGridInfo", "icp_debug_grid", "sor_debug_grid", "ScConfig", "ScResult", "sc_default_config", "sc_make", "sc_distance",
           "LocalMapConfig", "LocalMapInfo", "sor_filter", "local_map_default_config",
           "HeightMapConfig", "HeightMapInfo", "height_map", "height_map_default_config",
           "TerrainConfig", "TerrainInfo", "TERRAIN_LAYERS", "terrain_layers", "terrain_default_config",
           "GlobalMapConfig", "GlobalMapInfo", "ExportConfig", "global_map_default_config", "STAGED_DS", "STAGED_RAW",
           "OgmConfig", "OgmInfo", "ogm_default_config", "radius_filter", "occupancy_grid",
           "SdfConfig", "SdfInfo", "Sdf", "SDF_NODE_LIMIT", "sdf_default_config", "occupancy_sdf",
           "MedianFillConfig", "MedianFillInfo", "PlanningMapBuffers", "median_fill", "median_fill_default_config",
           "Grid", "GridSampleConfig", "GridSampleInfo", "GridInfo", "grid_sample_default_config", "kf_store_planning_grid", "GRID_MAX_LAYERS",
           "GRID_NEAREST", "GRID_LINEAR", "GRID_CUBIC_CONVOLUTION", "GRID_CUBIC", "GRID_OUTSIDE", "GRID_LAYER_ELEVATION", "GRID_LAYER_FILLED",
           "GRID_LAYER_TERRAIN",
           "GridRegion", "GridRegionConfig", "GridRegionStat", "GridRegionInfo", "GRID_REGION_DTYPE", "GRID_REGION_STAT_DTYPE",
           "grid_region_default_config", "pack_regions", "footprint_polygons", "REGION_LINE", "REGION_CIRCLE", "REGION_ELLIPSE", "REGION_POLYGON",
           "REGION_OK", "REGION_EMPTY", "REGION_INVALID", "REGION_MAX_VERTICES", "REGION_MAX_WALK",
           "GRID_TRANSFORM_INFO_DTYPE", "GRID_OCCUPANCY_DESC_DTYPE", "GRID_TRANSFORM_MAX_SOURCE_CELLS",
           "GRID_SUBMAP_INFO_DTYPE", "GRID_MOVE_INFO_DTYPE", "GRID_EXTEND_INFO_DTYPE", "GRID_ADD_INFO_DTYPE",
           "GRID_IMAGE_INFO_DTYPE", "GRID_FROM_IMAGE_INFO_DTYPE", "GRID_FROM_OCCUPANCY_INFO_DTYPE", "IMAGE_8U", "IMAGE_16U", "IMAGE_32F"]
