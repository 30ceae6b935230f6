// lio_localmap.h -- what the planning local map (lio_localmap.hip) offers the chains that go on from it.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/liogpu.h"
#include "lio_pool.h"

#define LIO_SOR_MAX_K 32           // mean_k is in [1, LIO_SOR_MAX_K]: the per-lane candidate list has mean_k + 1 entries of LDS

// what one filter call reports besides its cloud
struct LioSorReport {
    int n_finite = 0;              // points that took part
    int passthrough = 0;           // 1: at most mean_k finite points, nothing was filtered
    double mean = 0.0, stddev = 0.0, threshold = 0.0;
};

int lio_sor_check(int32_t mean_k, float stddev_mul);          // LIO_OK or LIO_ERR_ARG

// pcl::StatisticalOutlierRemoval::applyFilter on a device-resident float4 cloud (x, y, z, intensity), on stream `s`;
// synchronous.  `out` receives the inliers in input order.  d_mean_dist (device, n floats, may be null): dist_i, NaN for a
// skipped point.  Returns LIO_OK, or 1 for the pass-through of a cloud of at most mean_k finite points.
int lio_sor_device(const float4* d_pts, int n, int mean_k, float stddev_mul, LioTemp& out, int* n_out, float* d_mean_dist,
                   LioSorReport* rep, hipStream_t s);

// M = Translation(-tX, -tY, -tZ) * Rz(-yaw) of MO:2474-2488 as 3 x 4 row-major, from transformTobeMapped.
void lio_local_map_vehicle_frame(const float pose[6], float M[12]);

// pcl::transformPointCloud under M and the two pass-throughs (-left <= x' <= right, -back <= y' <= front, both inclusive) in
// one order-preserving compaction: `out` receives the survivors, transformed.  Synchronous (the count sizes what follows).
int lio_crop_device(const float4* d_in, int n, const float M[12], float front, float left, float back, float right, LioTemp& out,
                    int* n_out, hipStream_t s);

struct LocalMapBufs {
    LioTemp d_kf, d_poses, d_chunks, world, cropped, inl, ds;
    const float4* cur = nullptr;   // the local map, in one of the buffers above
    int n_cur = 0;
};

// MO:2447-2540 up to the cloud on the device: B.cur / B.n_cur = the local map (null / 0 for an empty store or an empty sum),
// complete when this returns.  What lio_kf_store_local_map copies out and lio_kf_store_height_map goes on with.
int lio_local_map_device(lio_kf_store* st, const lio_local_map_config* cfg, const float* pose, LocalMapBufs& B, size_t* n_out,
                         lio_local_map_info* info, hipStream_t s);
