// lio_localmap.h -- what the entry points of the planning local map (lio_mapbuild.hip) need from lio_localmap.hip.
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
