// lio_heightmap.h -- what the planning height map (lio_heightmap.hip) offers the chain that goes on from it (lio_terrain.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/liogpu.h"
#include "lio_gridmath.h"
#include "lio_pool.h"

// R1 = Rx(-roll) * Ry(-pitch), R2 = Rx(roll) * Ry(pitch) (PointcloudProcessor.cpp:131-154), 3 x 3 row-major, formed in fp32
// as helpers.cpp:107-139 forms them.  R2 is not R1's inverse.
void lio_hm_rotations(float roll, float pitch, float R1[9], float R2[9]);

// GridMapPclLoader.cpp:80-85 as one order-preserving compaction: `out` receives, for every point that has finite coordinates
// and that the ego filter keeps in the levelled frame, R2 * (R1 * p) (w = 0).  level == 0: the finite points as they are.
// Synchronous.
int lio_hm_level_ego(const float4* d_in, int n, const float R1[9], const float R2[9], int level, LioTemp& out, int* n_out, hipStream_t s);

// GridMapPclLoader.cpp:97-108 + GridMap::setGeometry, on the host in fp64, from pcl::getMinMax3D of the cloud (K7's box pass)
void lio_hm_geometry(const float mn[3], const float mx[3], double resolution, LioGridGeom* g);

// pairs[i] = (cell of point i = row + col * rows, or rows * cols for a point outside the grid; i).  counters[0] += the
// points inside.
void lio_hm_launch_keys(const float4* d_pts, int n, const LioGridGeom& g, uint2* pairs, int* counters, hipStream_t s);

// From the pairs stably sorted by cell: the elevation layer, the hole filling, the grid copied to `grid` (host, column-major
// rows x cols) and counters[0..2] = points binned, cells with an elevation, cells filled.  `counters`: the device words
// lio_hm_launch_keys added to.  Synchronous.  `keep` (optional): receives the device grid instead of the pool, for a caller
// that goes on from it (the terrain layers); `grid` may then be NULL, and nothing but the counters crosses.
int lio_hm_grid(const float4* d_pts, const uint2* d_sorted, int n, const LioGridGeom& g, const lio_height_map_config* cfg, float* grid,
                int* counters, int h_counters[3], hipStream_t s, LioTemp* keep = nullptr);

int lio_height_map_check(const lio_height_map_config* c);     // LIO_OK or LIO_ERR_ARG

// helpers.cpp:97-105 on a device-resident float4 cloud (w is not read): the reference's order, everything on the device, the
// grid copy last.  Host waits, each for a number that sizes the next launch: outlier filter 3 (box, grid choice, compaction
// count), voxel filter 2, ego filter 1, the box, and the grid copy with the counters.  `keep` (optional) receives the device
// grid, which is then built whether or not `grid` is given.
int lio_height_map_device(const float4* d_in, int n, const lio_height_map_config* cfg, float* grid, size_t grid_cap, lio_height_map_info* info,
                          hipStream_t s, LioTemp* keep = nullptr);
