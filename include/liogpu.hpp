// liogpu.hpp -- header-only C++ mirror of the reference's member functions over
// the C ABI in liogpu.h.  Names follow class mapOptimization (MO =
// src/liorf/src/mapOptmization.cpp) so that the patched node reads like the
// original: scan2MapOptimization() MO:1839, transformUpdate() MO:1867.
// No PCL/ROS dependency: clouds are passed as (pointer, count, stride).
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "liogpu.h"

namespace liogpu {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

class ScanToMap {
public:
    // transformTobeMapped [roll,pitch,yaw,x,y,z] (MO:171) and isDegenerate (MO:176) live here
    // exactly like the members they replace.
    float transformTobeMapped[6] = {0, 0, 0, 0, 0, 0};
    bool isDegenerate = false;
    lio_s2m_result last{};

    explicit ScanToMap(const lio_s2m_config* cfg = nullptr)
    {
        lio_s2m_config c;
        if (cfg) c = *cfg; else lio_s2m_default_config(&c);
        check(lio_s2m_create(&c, &h_), "lio_s2m_create");
    }
    ~ScanToMap() { lio_s2m_destroy(h_); }
    ScanToMap(const ScanToMap&) = delete;
    ScanToMap& operator=(const ScanToMap&) = delete;

    // kdtreeSurfFromMap->setInputCloud(laserCloudSurfFromMapDS), MO:1846
    void setInputCloud(const void* pts, size_t n, size_t stride_bytes)
    {
        check(lio_s2m_set_map(h_, pts, n, stride_bytes), "lio_s2m_set_map");
    }

    // The loop MO:1848-1859.  Returns the status: LIO_OK, LIO_TOO_FEW_POINTS (MO:1862-1864: the
    // caller prints the ROS_WARN) or LIO_TOO_FEW_CORR.  The caller keeps the guards MO:1841-1844
    // and calls transformUpdate() afterwards (MO:1861).
    int scan2MapOptimization(const void* laserCloudSurfLastDS, size_t n, size_t stride_bytes)
    {
        const int rc = lio_s2m_register(h_, laserCloudSurfLastDS, n, stride_bytes, transformTobeMapped, &last);
        if (rc < 0) check(rc, "lio_s2m_register");
        isDegenerate = last.is_degenerate != 0;
        return rc;
    }

    // The same on the `data` blob of msgIn->cloud_deskewed (sensor_msgs/PointCloud2, cloud_info.msg:27): what
    // pcl::fromROSMsg(msgIn->cloud_deskewed, *laserCloudSurfLast) MO:440 + downsample + the loop do, minus the copy into
    // a pcl::PointCloud.  point_step / off_x come from msg.point_step / the "x" entry of msg.fields.
    int scan2MapOptimizationPC2(const void* data, size_t width_times_height, uint32_t point_step, uint32_t off_x, bool pin_host = false)
    {
        lio_pc2_layout lay{};
        lay.point_step = point_step; lay.off_x = off_x; lay.off_intensity = -1; lay.off_ring = -1; lay.off_time = -1;
        lay.pin_host = pin_host ? 1 : 0;
        const int rc = lio_s2m_register_pc2(h_, data, width_times_height, &lay, transformTobeMapped, &last);
        if (rc < 0) check(rc, "lio_s2m_register_pc2");
        isDegenerate = last.is_degenerate != 0;
        return rc;
    }

    // downsampleCurrentScan() MO:1605-1611 + the loop MO:1848-1859 in one device chain, from the blob of
    // msgIn->cloud_deskewed (MO:440): `downSizeFilterSurf.filter(*laserCloudSurfLastDS)` runs on the GPU and the registration
    // starts from its output without a host round trip.  laserCloudSurfLastDSNum = n_downsampled afterwards (MO:1610); pass
    // laserCloudSurfLastDS->points.data() as ds_out (room for width*height PointType records) if the host copy is needed.
    int downsampleAndScan2MapOptimization(const void* data, size_t width_times_height, uint32_t point_step, uint32_t off_x,
                                          int32_t off_intensity, float mappingSurfLeafSize, void* ds_out = nullptr,
                                          size_t ds_stride = 32, bool pin_host = false)
    {
        lio_pc2_layout lay{};
        lay.point_step = point_step; lay.off_x = off_x; lay.off_intensity = off_intensity; lay.off_ring = -1; lay.off_time = -1;
        lay.pin_host = pin_host ? 1 : 0;
        const int rc = lio_s2m_register_raw(h_, data, width_times_height, &lay, mappingSurfLeafSize, transformTobeMapped, &last,
                                            ds_out, ds_stride, &n_downsampled);
        if (rc < 0) check(rc, "lio_s2m_register_raw");
        isDegenerate = last.is_degenerate != 0;
        return rc;
    }
    size_t n_downsampled = 0;

    // ---- extension beyond this reference (upstream LIO-SAM) ----
    // kdtreeCornerFromMap->setInputCloud(laserCloudCornerFromMapDS)
    void setInputCloudCorner(const void* pts, size_t n, size_t stride_bytes)
    {
        check(lio_s2m_set_corner_map(h_, pts, n, stride_bytes), "lio_s2m_set_corner_map");
    }
    // upstream loop body: cornerOptimization(); surfOptimization(); combineOptimizationCoeffs(); LMOptimization(iterCount)
    int scan2MapOptimization(const void* laserCloudCornerLastDS, size_t n_corner,
                             const void* laserCloudSurfLastDS, size_t n_surf, size_t stride_bytes)
    {
        const int rc = lio_s2m_register_cs(h_, laserCloudCornerLastDS, n_corner, laserCloudSurfLastDS, n_surf,
                                           stride_bytes, transformTobeMapped, &last);
        if (rc < 0) check(rc, "lio_s2m_register_cs");
        isDegenerate = last.is_degenerate != 0;
        return rc;
    }

    // transformUpdate + constraintTransformation, MO:1867-1907
    void transformUpdate(bool imuAvailable, int imuType, float imuRollInit, float imuPitchInit,
                         float imuRPYWeight, float rotation_tollerance, float z_tollerance)
    {
        lio_transform_update(transformTobeMapped, imuAvailable ? 1 : 0, imuType, imuRollInit, imuPitchInit,
                             imuRPYWeight, rotation_tollerance, z_tollerance);
    }

    // publishFrames MO:2330-2345: cloud_registered (LIO_STAGED_DS) / cloud_registered_raw (LIO_STAGED_RAW) under the final
    // pose, from the clouds still staged on the device; `out` holds out_cap pcl::PointXYZI records.  Returns the points written.
    size_t registeredCloud(int32_t which, const float pose[6], void* out, size_t out_cap)
    {
        size_t n = 0;
        check(lio_s2m_registered_cloud(h_, which, pose, out, 32, out_cap, &n), "lio_s2m_registered_cloud");
        return n;
    }

    lio_s2m_handle* handle() { return h_; }

private:
    static void check(int rc, const char* what)
    {
        if (rc < 0) throw Error(rc, std::string(what) + ": " + lio_last_error());
    }
    lio_s2m_handle* h_ = nullptr;
};

// surfCloudKeyFrames (MO:128) + cloudKeyPoses6D (MO:130) on the device, and extractSurroundingKeyFrames() MO:1590-1603
// + extractCloud() MO:1556-1588 on them in one call
class KeyframeStore {
public:
    explicit KeyframeStore(int32_t device_id = 0) { check(lio_kf_store_create(device_id, &s_), "lio_kf_store_create"); }
    ~KeyframeStore() { lio_kf_store_destroy(s_); }
    KeyframeStore(const KeyframeStore&) = delete;
    KeyframeStore& operator=(const KeyframeStore&) = delete;

    // saveKeyFramesAndFactor MO:2107-2142: the scan `s2m` has just registered becomes keyframe id, with its pose and time
    int32_t addFromHandle(ScanToMap& s2m, const float pose6d[6], double time, int32_t scan = 0)
    {
        int32_t id = -1;
        check(lio_kf_store_add_from_handle(s_, s2m.handle(), scan, &id), "lio_kf_store_add_from_handle");
        check(lio_kf_store_set_poses(s_, id, 1, pose6d, &time), "lio_kf_store_set_poses");
        return id;
    }
    // correctPoses MO:2184-2196: every pose [roll,pitch,yaw,x,y,z] x n, the times kept
    void setPoses(int32_t first, int32_t n, const float* poses6d, const double* times = nullptr)
    {
        check(lio_kf_store_set_poses(s_, first, n, poses6d, times), "lio_kf_store_set_poses");
    }
    // extractSurroundingKeyFrames(): the local map of timeLaserInfoCur becomes s2m's resident map; returns its size
    size_t extractSurroundingKeyFrames(ScanToMap& s2m, double timeLaserInfoCur, float surroundingKeyframeMapLeafSize,
                                       const lio_nearby_config* cfg = nullptr)
    {
        lio_nearby_config c;
        if (cfg) c = *cfg; else lio_nearby_default_config(&c);
        int32_t n_ids = 0;
        size_t n_map = 0;
        check(lio_assemble_map_nearby(s2m.handle(), s_, &c, timeLaserInfoCur, surroundingKeyframeMapLeafSize, nullptr, 0, &n_ids,
                                      nullptr, 0, 0, &n_map), "lio_assemble_map_nearby");
        return n_map;
    }
    // detectLoopClosureDistance MO:1271-1304 over the stored poses; false: no loop candidate
    bool detectLoopClosureDistance(float historyKeyframeSearchRadius, double historyKeyframeSearchTimeDiff, double timeLaserInfoCur,
                                   int32_t* latestID, int32_t* closestID)
    {
        const int rc = lio_kf_store_detect_loop(s_, historyKeyframeSearchRadius, historyKeyframeSearchTimeDiff, timeLaserInfoCur, latestID,
                                                closestID);
        check(rc, "lio_kf_store_detect_loop");
        return rc == 1;
    }
    // performRSLoopClosure MO:1098-1143: both submaps from the resident clouds, ICP, fitness score, corrected pose.
    // Returns res.accepted (false also for the size guards of MO:1104); cfg == nullptr: the literals of MO:1112-1115.
    bool performLoopClosureICP(int32_t loopKeyCur, int32_t loopKeyPre, int32_t historyKeyframeSearchNum, float loopClosureICPSurfLeafSize,
                               lio_icp_result& res, const lio_icp_config* cfg = nullptr, int32_t pose_index = -1)
    {
        lio_icp_config c;
        if (cfg) c = *cfg; else lio_icp_default_config(&c);
        check(lio_kf_store_loop_icp(s_, loopKeyCur, loopKeyPre, historyKeyframeSearchNum, pose_index, loopClosureICPSurfLeafSize, &c, &res,
                                    nullptr), "lio_kf_store_loop_icp");
        return res.accepted != 0;
    }
    // publishLocalMap MO:2447-2540: the newest keyframes summed, cropped in the vehicle frame of transformTobeMapped,
    // outliers removed, downsampled; `out` holds out_cap pcl::PointXYZI records.  Returns the points written; what
    // publishCloud(pubLocalMap, ...) MO:2541 sends.  cfg == nullptr: the defaults of UT:219-229.
    size_t publishLocalMap(const float transformTobeMapped[6], void* out, size_t out_cap, const lio_local_map_config* cfg = nullptr,
                           lio_local_map_info* info = nullptr)
    {
        lio_local_map_config c;
        if (cfg) c = *cfg; else lio_local_map_default_config(&c);
        size_t n = 0;
        check(lio_kf_store_local_map(s_, &c, transformTobeMapped, out, 32, out_cap, &n, info), "lio_kf_store_local_map");
        return n;
    }
    // publishLocalMap followed by the height-map node's cloudMapInfoHandler (grid_map_pcl_loader_node.cpp:47-54) without the
    // cloud in between: `grid` holds grid_cap floats, column-major info.rows x info.cols (grid_map::Matrix); grid == nullptr
    // asks for the geometry only.  Returns the number of cells.  Null configs: the defaults with roll = pitch = 0.
    size_t heightMap(const float transformTobeMapped[6], float* grid, size_t grid_cap, lio_height_map_info& info,
                     const lio_height_map_config* cfg = nullptr, const lio_local_map_config* lm_cfg = nullptr,
                     lio_local_map_info* lm_info = nullptr)
    {
        lio_local_map_config lm;
        if (lm_cfg) lm = *lm_cfg; else lio_local_map_default_config(&lm);
        lio_height_map_config c;
        if (cfg) c = *cfg; else lio_height_map_default_config(&c);
        check(lio_kf_store_height_map(s_, &lm, transformTobeMapped, &c, grid, grid_cap, lm_info, &info), "lio_kf_store_height_map");
        return (size_t)info.rows * (size_t)info.cols;
    }
    // heightMap followed by grid_map_demos' filter chain (smooth, surface normals, slope, roughness, edges, traversability) on
    // the device grid: `layers` holds layers_cap floats and receives the layers whose bit is set in cfg.layers, in
    // LIO_TERRAIN_* order, each info.rows x info.cols, column-major, NaN = no value; `grid` (may be nullptr) the elevation.
    // The defaults of lio_terrain_default_config are tuned for a 0.02 m grid: at the loader's 0.2 m pass a config with
    // normal_radius, smooth_radius and edge_window_length scaled by 10.  Returns the number of cells.
    size_t terrainMap(const float transformTobeMapped[6], float* grid, size_t grid_cap, float* layers, size_t layers_cap,
                      lio_terrain_info& info, const lio_terrain_config* cfg = nullptr, const lio_height_map_config* hm_cfg = nullptr,
                      const lio_local_map_config* lm_cfg = nullptr, lio_height_map_info* hm_info = nullptr,
                      lio_local_map_info* lm_info = nullptr)
    {
        lio_local_map_config lm;
        if (lm_cfg) lm = *lm_cfg; else lio_local_map_default_config(&lm);
        lio_height_map_config hm;
        if (hm_cfg) hm = *hm_cfg; else lio_height_map_default_config(&hm);
        lio_terrain_config c;
        if (cfg) c = *cfg; else lio_terrain_default_config(&c);
        lio_height_map_info hi;
        check(lio_kf_store_terrain_map(s_, &lm, transformTobeMapped, &hm, &c, grid, grid_cap, layers, layers_cap, lm_info,
                                       hm_info ? hm_info : &hi, &info), "lio_kf_store_terrain_map");
        return (size_t)info.rows * (size_t)info.cols;
    }
    // publishGlobalMap MO:992-1041 from the stored poses and clouds; `out` holds out_cap pcl::PointXYZI records.  Returns the
    // points written: what publishCloud(pubLaserCloudSurround, ...) MO:1040 sends.  cfg == nullptr: the yaml defaults.
    size_t publishGlobalMap(void* out, size_t out_cap, const lio_global_map_config* cfg = nullptr, lio_global_map_info* info = nullptr)
    {
        lio_global_map_config c;
        if (cfg) c = *cfg; else lio_global_map_default_config(&c);
        int32_t n_ids = 0;
        size_t n = 0;
        check(lio_kf_store_global_map(s_, &c, nullptr, 0, &n_ids, out, 32, out_cap, &n, info), "lio_kf_store_global_map");
        return n;
    }
    // saveMapService MO:935-962: globalSurfCloud into out_full (nullptr: its size only) and, when resolution != 0, its
    // voxel-filtered copy into out_ds; both pcl::PointXYZI records.  chunk_points = 0: the default transfer chunk.
    void exportMap(float resolution, void* out_full, size_t full_cap, size_t& n_full, void* out_ds, size_t ds_cap, size_t& n_ds,
                   int32_t chunk_points = 0, int32_t* voxel_passthrough = nullptr)
    {
        const lio_export_config c = { resolution, chunk_points };
        check(lio_kf_store_export_map(s_, &c, out_full, 32, full_cap, &n_full, out_ds, 32, ds_cap, &n_ds, voxel_passthrough),
              "lio_kf_store_export_map");
    }
    // keyframe `id` as stored (pose6d == nullptr) or under a pose; returns its size (out == nullptr: the size only)
    size_t getKeyframe(int32_t id, void* out, size_t out_cap, const float* pose6d = nullptr)
    {
        size_t n = 0;
        check(lio_kf_store_get_keyframe(s_, id, pose6d, out, 32, out_cap, &n), "lio_kf_store_get_keyframe");
        return n;
    }
    // The draft ogmGeneration.cpp on the map saveMapService would write at `map_resolution` (0: unfiltered): slice on z, radius
    // outlier removal, raster.  `grid` holds grid_cap cells (nullptr: geometry and counts only) and receives info.width x
    // info.height bytes, row-major, 100 = occupied: the data of a nav_msgs::OccupancyGrid whose info.resolution is
    // cfg->resolution and whose origin is info.origin.  Returns the number of cells.  cfg == nullptr: the draft's defaults.
    size_t occupancyGrid(float map_resolution, int8_t* grid, size_t grid_cap, lio_ogm_info& info, const lio_ogm_config* cfg = nullptr,
                         size_t* n_map = nullptr)
    {
        lio_ogm_config c;
        if (cfg) c = *cfg; else lio_ogm_default_config(&c);
        check(lio_kf_store_occupancy_grid(s_, map_resolution, &c, grid, grid_cap, n_map, &info), "lio_kf_store_occupancy_grid");
        return (size_t)info.width * (size_t)info.height;
    }
    // heightMap followed by grid_map_sdf's SignedDistanceField on the device grid: `sdf` (a SignedDistanceField below) receives
    // the field, `grid` (may be nullptr) the elevation.  hm_cfg->resolution is the field's.  Returns the number of nodes.
    size_t signedDistanceField(const float transformTobeMapped[6], lio_sdf* sdf, lio_sdf_info& info, float* grid = nullptr, size_t grid_cap = 0,
                               const lio_sdf_config* cfg = nullptr, const lio_height_map_config* hm_cfg = nullptr,
                               const lio_local_map_config* lm_cfg = nullptr, lio_height_map_info* hm_info = nullptr,
                               lio_local_map_info* lm_info = nullptr)
    {
        lio_local_map_config lm;
        if (lm_cfg) lm = *lm_cfg; else lio_local_map_default_config(&lm);
        lio_height_map_config hm;
        if (hm_cfg) hm = *hm_cfg; else lio_height_map_default_config(&hm);
        lio_sdf_config c;
        if (cfg) c = *cfg; else lio_sdf_default_config(&c);
        check(lio_kf_store_sdf(s_, &lm, transformTobeMapped, &hm, &c, grid, grid_cap, sdf, lm_info, hm_info, &info), "lio_kf_store_sdf");
        return (size_t)info.rows * (size_t)info.cols * (size_t)info.layers;
    }
    // The one chain of a planning node: heightMap's stages once, then grid_map_filters' MedianFillFilter (fill), the terrain
    // layers (terrain) and the signed distance field (sdf with sdf_cfg) on the grid left on the device; a stage whose pointer
    // is nullptr is absent.  `out` names the host buffers (each may be nullptr).  Returns the number of cells.
    size_t planningMap(const float transformTobeMapped[6], const lio_planning_map_buffers& out, const lio_median_fill_config* fill,
                       const lio_terrain_config* terrain, lio_sdf* sdf, const lio_sdf_config* sdf_cfg, lio_height_map_info& hm_info,
                       lio_median_fill_info* fill_info = nullptr, lio_terrain_info* terrain_info = nullptr, lio_sdf_info* sdf_info = nullptr,
                       const lio_height_map_config* hm_cfg = nullptr, const lio_local_map_config* lm_cfg = nullptr,
                       lio_local_map_info* lm_info = nullptr)
    {
        lio_local_map_config lm;
        if (lm_cfg) lm = *lm_cfg; else lio_local_map_default_config(&lm);
        lio_height_map_config hm;
        if (hm_cfg) hm = *hm_cfg; else lio_height_map_default_config(&hm);
        check(lio_kf_store_planning_map(s_, &lm, transformTobeMapped, &hm, fill, terrain, sdf, sdf_cfg, &out, lm_info, &hm_info, fill_info,
                                        terrain_info, sdf_info), "lio_kf_store_planning_map");
        return (size_t)hm_info.rows * (size_t)hm_info.cols;
    }
    // planningMap, which also leaves its grids on the device in `grid` (a GridLayers below, may be nullptr): layer 0 the raw
    // grid, layer 1 the filled grid, layers 2 .. 9 the terrain layers.  `out` may name no buffer at all: then only positions go
    // up and values come down (GridLayers::atPosition).
    size_t planningGrid(const float transformTobeMapped[6], lio_grid* grid, const lio_planning_map_buffers& out, const lio_median_fill_config* fill,
                        const lio_terrain_config* terrain, lio_sdf* sdf, const lio_sdf_config* sdf_cfg, lio_height_map_info& hm_info,
                        lio_median_fill_info* fill_info = nullptr, lio_terrain_info* terrain_info = nullptr, lio_sdf_info* sdf_info = nullptr,
                        const lio_height_map_config* hm_cfg = nullptr, const lio_local_map_config* lm_cfg = nullptr,
                        lio_local_map_info* lm_info = nullptr)
    {
        lio_local_map_config lm;
        if (lm_cfg) lm = *lm_cfg; else lio_local_map_default_config(&lm);
        lio_height_map_config hm;
        if (hm_cfg) hm = *hm_cfg; else lio_height_map_default_config(&hm);
        check(lio_kf_store_planning_grid(s_, &lm, transformTobeMapped, &hm, fill, terrain, sdf, sdf_cfg, &out, lm_info, &hm_info, fill_info,
                                         terrain_info, sdf_info, grid), "lio_kf_store_planning_grid");
        return (size_t)hm_info.rows * (size_t)hm_info.cols;
    }
    lio_kf_store* get() { return s_; }

private:
    static void check(int rc, const char* what)
    {
        if (rc < 0) throw Error(rc, std::string(what) + ": " + lio_last_error());
    }
    lio_kf_store* s_ = nullptr;
};

// grid_map::SignedDistanceField resident on the device (grid_map_sdf/SignedDistanceField.hpp): built from an elevation grid
// or by KeyframeStore::signedDistanceField, queried by valueAndDerivative.
class SignedDistanceField {
public:
    explicit SignedDistanceField(int32_t device_id = 0)
    {
        const int rc = lio_sdf_create(device_id, &s_);
        if (rc < 0) throw Error(rc, std::string("lio_sdf_create: ") + lio_last_error());
    }
    ~SignedDistanceField() { lio_sdf_destroy(s_); }
    SignedDistanceField(const SignedDistanceField&) = delete;
    SignedDistanceField& operator=(const SignedDistanceField&) = delete;

    // SignedDistanceField(gridMap, "elevation", minHeight, maxHeight) on a host grid, column-major rows x cols
    // (grid_map::Matrix); length and position: the grid map's.  cfg == nullptr: the band of the finite cells, NaN refused.
    void build(const float* elevation, int32_t rows, int32_t cols, double resolution, const double length[2], const double position[2],
               lio_sdf_info& info, const lio_sdf_config* cfg = nullptr)
    {
        lio_sdf_config c;
        if (cfg) c = *cfg; else lio_sdf_default_config(&c);
        check(lio_sdf_build(s_, elevation, rows, cols, resolution, length, position, &c, &info), "lio_sdf_build");
    }
    // valueAndDerivative for n positions (x, y, z); derivative (n x 3) may be nullptr
    void valueAndDerivative(const double* positions, size_t n, double* value, double* derivative = nullptr)
    {
        check(lio_sdf_query(s_, positions, n, value, derivative), "lio_sdf_query");
    }
    // data_: {distance, dx, dy, dz} per node, (z * cols + col) * rows + row
    void nodes(float* out, size_t cap_floats) { check(lio_sdf_nodes(s_, out, cap_floats), "lio_sdf_nodes"); }
    lio_sdf* get() { return s_; }

private:
    static void check(int rc, const char* what)
    {
        if (rc < 0) throw Error(rc, std::string(what) + ": " + lio_last_error());
    }
    lio_sdf* s_ = nullptr;
};

// The layers of a grid_map::GridMap resident on the device: uploaded, or left there by KeyframeStore::planningGrid, and sampled
// by GridMap::atPosition with its four InterpolationMethods.
class GridLayers {
public:
    explicit GridLayers(int32_t device_id = 0)
    {
        const int rc = lio_grid_create(device_id, &g_);
        if (rc < 0) throw Error(rc, std::string("lio_grid_create: ") + lio_last_error());
    }
    ~GridLayers() { lio_grid_destroy(g_); }
    GridLayers(const GridLayers&) = delete;
    GridLayers& operator=(const GridLayers&) = delete;

    // n_layers host layers, one after the other, each column-major rows x cols (grid_map::Matrix); length and position: the grid map's
    void setLayers(const float* layers, int32_t n_layers, int32_t rows, int32_t cols, double resolution, const double length[2], const double position[2])
    {
        check(lio_grid_set_layers(g_, layers, n_layers, rows, cols, resolution, length, position), "lio_grid_set_layers");
    }
    // atPosition(layer, position, method) for n positions (x, y) on each of the n_layers layers of layer_ids: values[k * n + q];
    // method_used (may be nullptr) the same for the method that produced the value, LIO_GRID_OUTSIDE where the reference throws
    void atPosition(const int32_t* layer_ids, int32_t n_layers, const double* positions, size_t n, float* values, int32_t method = LIO_GRID_NEAREST,
                    uint8_t* method_used = nullptr, lio_grid_sample_info* info = nullptr, int32_t border_mode = 0)
    {
        lio_grid_sample_config c;
        lio_grid_sample_default_config(&c);
        c.method = method; c.border_mode = border_mode;
        check(lio_grid_sample(g_, layer_ids, n_layers, &c, positions, n, values, method_used, info), "lio_grid_sample");
    }
    // grid_map's Line / Circle / Ellipse / PolygonIterator over n regions with the reduction a caller would loop for:
    // stats[k * n + q] is layer layer_ids[k] over region q; n_cells and status (each may be nullptr) per region; `vertices` holds
    // the polygons' (x, y) pairs.  threshold: what n_below counts below.
    void regionReduce(const int32_t* layer_ids, int32_t n_layers, const lio_grid_region* regions, size_t n, const double* vertices, size_t n_vertices,
                      lio_grid_region_stat* stats, float threshold = 0.5f, int32_t* n_cells = nullptr, uint8_t* status = nullptr,
                      lio_grid_region_info* info = nullptr)
    {
        lio_grid_region_config c;
        lio_grid_region_default_config(&c);
        c.threshold = threshold;
        check(lio_grid_region_reduce(g_, layer_ids, n_layers, &c, regions, n, vertices, n_vertices, stats, n_cells, status, info), "lio_grid_region_reduce");
    }
    // the cells themselves, in the iterator's order: returns LIO_ERR_CAPACITY (no throw) when cap_cells is too small, with
    // offsets[n] the need
    int regionCells(const lio_grid_region* regions, size_t n, const double* vertices, size_t n_vertices, int64_t* offsets, int32_t* cells, size_t cap_cells,
                    uint8_t* status = nullptr, lio_grid_region_info* info = nullptr)
    {
        const int rc = lio_grid_region_cells(g_, regions, n, vertices, n_vertices, offsets, cells, cap_cells, status, info);
        if (rc != LIO_ERR_CAPACITY) check(rc, "lio_grid_region_cells");
        return rc;
    }
    // GridMap::getTransformedMap into dst (on the same device): dst then holds every layer this object holds, in the new geometry.
    // transform: the rows of [R | t]
    void transformInto(GridLayers& dst, const double transform[12], int32_t height_layer = LIO_GRID_LAYER_ELEVATION, double sample_ratio = 0.0,
                       lio_grid_transform_info* info = nullptr)
    {
        check(lio_grid_transform(g_, transform, height_layer, sample_ratio, dst.g_, info), "lio_grid_transform");
    }
    // GridMapRosConverter::toOccupancyGrid on one layer: data receives rows x cols cells in the message's order
    void toOccupancyGrid(int32_t layer, float data_min, float data_max, int8_t* data, size_t cap_cells, lio_grid_occupancy_desc* desc = nullptr)
    {
        check(lio_grid_to_occupancy(g_, layer, data_min, data_max, data, cap_cells, desc), "lio_grid_to_occupancy");
    }
    // GridMap::getSubmap into dst (on the same device): every layer this object holds, cropped.  Returns isSuccess; false (a
    // requested centre outside the map) leaves dst without layers
    bool getSubmap(GridLayers& dst, const double position[2], const double length[2], lio_grid_submap_info* info = nullptr)
    {
        lio_grid_submap_info i;
        check(lio_grid_submap(g_, position, length, dst.g_, &i), "lio_grid_submap");
        if (info) *info = i;
        return i.success != 0;
    }
    // GridMap::move, in place: returns whether the map moved by at least one cell
    bool move(const double position[2], lio_grid_move_info* info = nullptr)
    {
        lio_grid_move_info i;
        check(lio_grid_move(g_, position, &i), "lio_grid_move");
        if (info) *info = i;
        return i.moved != 0;
    }
    // GridMap::extendToInclude: returns whether the map was resized
    bool extendToInclude(GridLayers& other, lio_grid_extend_info* info = nullptr)
    {
        lio_grid_extend_info i;
        check(lio_grid_extend_to_include(g_, other.g_, &i), "lio_grid_extend_to_include");
        if (info) *info = i;
        return i.resized != 0;
    }
    // GridMap::addDataFrom.  n_layers = 0 (layer_ids nullptr): copyAllLayers.  basic_mask: bit k, layer k is one of basicLayers_
    void addDataFrom(GridLayers& other, bool extend_map, bool overwrite_data, const int32_t* layer_ids = nullptr, int32_t n_layers = 0,
                     uint32_t basic_mask = 0, lio_grid_add_info* info = nullptr)
    {
        check(lio_grid_add_data_from(g_, other.g_, extend_map ? 1 : 0, overwrite_data ? 1 : 0, layer_ids, n_layers, basic_mask, info), "lio_grid_add_data_from");
    }
    // GridMapCvConverter::toImage<Type, NChannels>: depth LIO_IMAGE_*; lower = upper = NAN: the layer's finite extremes
    void toImage(int32_t layer, int32_t channels, int32_t depth, float lower, float upper, void* image, size_t cap_bytes, lio_grid_image_info* info = nullptr)
    {
        check(lio_grid_to_image(g_, layer, channels, depth, lower, upper, image, cap_bytes, info), "lio_grid_to_image");
    }
    // GridMapCvConverter::addLayerFromImage; a grid without layers takes its geometry from the call (initializeFromImage)
    void addLayerFromImage(int32_t layer, const void* image, int32_t rows, int32_t cols, int32_t channels, int32_t depth, float lower = 0.0f,
                           float upper = 1.0f, double alpha_threshold = 0.5, double resolution = 0.0, const double* position = nullptr,
                           lio_grid_from_image_info* info = nullptr)
    {
        check(lio_grid_add_layer_from_image(g_, layer, image, rows, cols, channels, depth, lower, upper, alpha_threshold, resolution, position, info),
              "lio_grid_add_layer_from_image");
    }
    // GridMapCvConverter::addColorLayerFromImage (8U, 3 or 4 channels)
    void addColorLayerFromImage(int32_t layer, const void* image, int32_t rows, int32_t cols, int32_t channels, double resolution = 0.0,
                                const double* position = nullptr, lio_grid_from_image_info* info = nullptr)
    {
        check(lio_grid_add_color_layer_from_image(g_, layer, image, rows, cols, channels, LIO_IMAGE_8U, resolution, position, info),
              "lio_grid_add_color_layer_from_image");
    }
    // GridMapRosConverter::fromOccupancyGrid into `layer`
    void fromOccupancyGrid(int32_t layer, const int8_t* data, size_t n, uint32_t width, uint32_t height, float resolution, const double origin[2],
                           lio_grid_from_occupancy_info* info = nullptr)
    {
        check(lio_grid_from_occupancy(g_, layer, data, n, width, height, resolution, origin, info), "lio_grid_from_occupancy");
    }
    // GridMapRosConverter::toPointCloud / toGridCells: return LIO_ERR_CAPACITY (no throw) when the buffer is too small, with
    // *n_out the need
    int toPointCloud(int32_t point_layer, const int32_t* layer_ids, int32_t n_layers, uint32_t basic_mask, float* points, size_t cap_points, size_t* n_out,
                     int32_t* n_fields = nullptr)
    {
        const int rc = lio_grid_to_point_cloud(g_, point_layer, layer_ids, n_layers, basic_mask, points, cap_points, n_out, n_fields);
        if (rc != LIO_ERR_CAPACITY) check(rc, "lio_grid_to_point_cloud");
        return rc;
    }
    int toGridCells(int32_t layer, float lower, float upper, double* cells, size_t cap_cells, size_t* n_out)
    {
        const int rc = lio_grid_to_grid_cells(g_, layer, lower, upper, cells, cap_cells, n_out);
        if (rc != LIO_ERR_CAPACITY) check(rc, "lio_grid_to_grid_cells");
        return rc;
    }
    // grid_map_filters on a layer the object holds; the result replaces out_layer.  MinInRadiusFilter / MeanInRadiusFilter
    // (op LIO_GF_MIN / LIO_GF_MEAN):
    void filterInRadius(int32_t in_layer, int32_t out_layer, int32_t op, double radius, lio_grid_filter_info* info = nullptr)
    {
        check(lio_grid_filter_radius(g_, in_layer, out_layer, op, radius, info), "lio_grid_filter_radius");
    }
    // SlidingWindowMathExpressionFilter: op LIO_GW_SUM .. LIO_GW_WEIGHTED_SUM, edge_handling LIO_GW_INSIDE .. LIO_GW_EDGE_MEAN;
    // window_size 0: from window_length; weights (size x size, column-major) with LIO_GW_WEIGHTED_SUM only
    void filterSlidingWindow(int32_t in_layer, int32_t out_layer, int32_t op, int32_t edge_handling, int32_t window_size, double window_length = 0.0,
                             const float* weights = nullptr, lio_grid_filter_info* info = nullptr)
    {
        check(lio_grid_filter_window(g_, in_layer, out_layer, op, edge_handling, window_size, window_length, weights, info), "lio_grid_filter_window");
    }
    // CurvatureFilter
    void filterCurvature(int32_t in_layer, int32_t out_layer, lio_grid_filter_info* info = nullptr)
    {
        check(lio_grid_filter_curvature(g_, in_layer, out_layer, info), "lio_grid_filter_curvature");
    }
    // ThresholdFilter, in place on out_layer: upper false is lower_threshold, true upper_threshold
    void filterThreshold(int32_t condition_layer, int32_t out_layer, bool upper, double threshold, double set_to, lio_grid_filter_info* info = nullptr)
    {
        check(lio_grid_filter_threshold(g_, condition_layer, out_layer, upper ? 1 : 0, threshold, set_to, info), "lio_grid_filter_threshold");
    }
    // DuplicationFilter and DeletionFilter
    void duplicateLayer(int32_t in_layer, int32_t out_layer) { check(lio_grid_duplicate_layer(g_, in_layer, out_layer), "lio_grid_duplicate_layer"); }
    void deleteLayers(const int32_t* layer_ids, int32_t n_layers) { check(lio_grid_delete_layers(g_, layer_ids, n_layers), "lio_grid_delete_layers"); }
    // MathExpressionFilter: an EigenLab expression over the layers names[k] -> layer_ids[k], stored as out_layer (which it may read)
    void filterMathExpression(const char* expression, const char* const* names, const int32_t* layer_ids, int32_t n_names, int32_t out_layer,
                              lio_grid_expression_info* info = nullptr)
    {
        check(lio_grid_filter_expression(g_, expression, names, layer_ids, n_names, out_layer, info), "lio_grid_filter_expression");
    }
    void layer(int32_t k, float* out, size_t cap_floats) { check(lio_grid_get_layer(g_, k, out, cap_floats), "lio_grid_get_layer"); }
    lio_grid_desc info()
    {
        lio_grid_desc d;
        check(lio_grid_info(g_, &d), "lio_grid_info");
        return d;
    }
    lio_grid* get() { return g_; }

private:
    static void check(int rc, const char* what)
    {
        if (rc < 0) throw Error(rc, std::string(what) + ": " + lio_last_error());
    }
    lio_grid* g_ = nullptr;
};

// grid_map_filters' MedianFillFilter::update on a host grid, column-major rows x cols (grid_map::Matrix): `filled` receives
// the output layer, fill_mask and cleaned_mask (each may be nullptr) the masks; mask_in (may be nullptr) is the fill mask of a
// previous run.  cfg == nullptr: the constructor's defaults.
inline void medianFill(const float* elevation, int32_t rows, int32_t cols, double resolution, float* filled, lio_median_fill_info& info,
                       const lio_median_fill_config* cfg = nullptr, const float* mask_in = nullptr, float* fill_mask = nullptr,
                       float* cleaned_mask = nullptr, int32_t device_id = 0)
{
    lio_median_fill_config c;
    if (cfg) c = *cfg; else lio_median_fill_default_config(&c);
    const int rc = lio_median_fill(device_id, elevation, rows, cols, resolution, &c, mask_in, filled, fill_mask, cleaned_mask, &info);
    if (rc < 0) throw Error(rc, std::string("lio_median_fill: ") + lio_last_error());
}

}  // namespace liogpu
