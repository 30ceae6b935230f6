// lio_cloud.h -- what every chain over a device-resident float4 cloud (x, y, z, intensity) shares, defined in lio_cloud.hip:
// the device check, the record conversions in and out, the upload of a host cloud, the box pass, the cloud laid out as its
// own search target and K7 (pcl::VoxelGrid by sorting, kernels in lio_voxsort.h).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "lio_pool.h"
#include "lio_types.h"

#define LIO_VS_THREADS 256
#define LIO_VS_BINS 256

struct LioVsGrid { float inv; int min_b0, min_b1, min_b2, mul1, mul2; };

// pcl::VoxelGrid's grid over the cloud's bounding box mn / mx (inv = 1 / leaf), on the host (lio_voxel_grid_device) or on the
// device (the pose filter of lio_assemble_map_nearby, whose box never leaves the device).  Returns 0 and fills g / *n_keys;
// 1 when PCL passes the input through (the index overflows; also a box that is not finite, which PCL does not define);
// 2 when the grid holds more than 2^31 - 1 voxels although the extent test passed.
__host__ __device__ inline int lio_vs_grid_from_box(const float mn[3], const float mx[3], float inv, LioVsGrid* g, long long* n_keys)
{
    const long long dx = (long long)((mx[0] - mn[0]) * inv) + 1, dy = (long long)((mx[1] - mn[1]) * inv) + 1,
                    dz = (long long)((mx[2] - mn[2]) * inv) + 1;
    bool finite_box = true;
    for (int a = 0; a < 3; ++a) finite_box = finite_box && (mn[a] <= mx[a]) && fabsf(mn[a]) <= 3.0e38f && fabsf(mx[a]) <= 3.0e38f;
    if (!finite_box || dx <= 0 || dy <= 0 || dz <= 0 || (double)dx * (double)dy * (double)dz > 2147483647.0) return 1;
    g->inv = inv;
    g->min_b0 = (int)floorf(mn[0] * inv); g->min_b1 = (int)floorf(mn[1] * inv); g->min_b2 = (int)floorf(mn[2] * inv);
    const int d0 = (int)floorf(mx[0] * inv) - g->min_b0 + 1, d1 = (int)floorf(mx[1] * inv) - g->min_b1 + 1,
              d2 = (int)floorf(mx[2] * inv) - g->min_b2 + 1;
    g->mul1 = d0; g->mul2 = d0 * d1;
    *n_keys = (long long)d0 * d1 * d2;
    return *n_keys > 2147483647LL ? 2 : 0;
}

// the voxel index of pcl::VoxelGrid, x-fastest over the cloud's own bounding box
__device__ __forceinline__ unsigned lio_vs_key(const LioVsGrid& g, float x, float y, float z)
{
    const int i0 = (int)(floorf(x * g.inv) - (float)g.min_b0);
    const int i1 = (int)(floorf(y * g.inv) - (float)g.min_b1);
    const int i2 = (int)(floorf(z * g.inv) - (float)g.min_b2);
    return (unsigned)(i0 + i1 * g.mul1 + i2 * g.mul2);
}

// The workspace of K7.  B: LioTemp (pool temporaries, recycled when the call returns) or LioDevBytes (a workspace kept from
// one call to the next, so that nothing has to be waited for before the call returns).  The templates below exist for both.
template <class B> struct LioVoxWs { B bbox, large, pairs_a, pairs_b, hist, blk_heads, seg_start, d_no, row_total; };

int lio_check_device(int device_id);                 // LIO_ERR_NO_DEVICE without a device (there is no CPU fallback)

// records (x,y,z at xyz_off, FLOAT32 intensity at int_off, < 0 = the record carries none) -> float4 (x,y,z,intensity), on `s`
void lio_rec_to_xyzi4(const unsigned char* src, size_t stride, size_t xyz_off, int int_off, int n, float4* dst, hipStream_t s);
// n > 0 records of `stride` bytes -> `raw` (allocated here), then lio_rec_to_xyzi4 (x,y,z at byte 0) into dst[0 .. n); nothing waits
int lio_upload_xyzi(const void* pts, size_t n, size_t stride, int int_off, LioTemp& raw, float4* dst, hipStream_t s,
                    hipMemcpyKind kind = hipMemcpyHostToDevice);
// n float4 (x, y, z, intensity) -> PointXYZI-compatible host records; waits for `s`
int lio_copy_out(const float4* d_pts, int n, void* out, size_t out_stride, hipStream_t s);

// getMinMax3D of a device-resident cloud (n > 0) in two halves, so that a caller whose box is already in `bbox`
// (k_transform_clouds_bbox) takes the second alone: clear + k_vox_bbox, then the copy, the wait and the decoding.
template <class B> int lio_cloud_box_launch(const float4* d_in, int n, B& bbox, hipStream_t s);
template <class B> int lio_cloud_box_wait(B& bbox, float mn[3], float mx[3], hipStream_t s);

// A cloud as its own search target (the loop-closure alignment, the outlier filter, the radius filter): the cloud as SoA and
// as (x, y, z, 0), a uniform grid over the box of the coordinates that take part, the cloud cell-sorted into it.
struct LioSearchTarget {
    LioTemp tx, ty, tz, t4;
    LioTemp cell_of, cell_count, cell_start, tiles, sorted;
    LioGrid g;                // the caller's choice between the two steps
    float edge = 1.0f;
    bool any = false;         // the box holds a point on every axis
    int occupied = -1;        // occupied cells of a trial grid (-1: none was laid)
};
// n > 0 points: the SoA copy, then the box of the coordinates within LIO_MAX_COORD (per axis) -> mn / mx and T.any, under one
// host wait.  Without a point on some axis mn / mx are not a box: the caller's rule decides what follows.
int lio_search_target_box(const float4* d_pts, int n, hipStream_t s, LioSearchTarget& T, float mn[3], float mx[3]);
// the cell sort into T.g: T.cell_start (n_cells + 1) and T.sorted (x, y, z, bits(index in the caller's order)); nothing waits
int lio_search_target_sort(int n, hipStream_t s, LioSearchTarget& T);

// Room for sorting n pairs and summing their segments (ws) and for n centroids (out).
template <class B> int lio_vsort_reserve(int n, B& out, LioVoxWs<B>& ws);
// Stable LSD radix sort of the n pairs in ws.pairs_a by their low `bits` key bits; returns the buffer that holds the result.
template <class B> uint2* lio_vsort_pairs(int n, int bits, hipStream_t s, LioVoxWs<B>& ws);
// Segments (voxels) of the sorted pairs `a` and the in-order centroid of each -> out[0 .. ws.d_no[0]); nothing waits.
template <class B> int lio_vsort_centroids(const float4* d_in, const uint2* a, int n, B& out, hipStream_t s, LioVoxWs<B>& ws);

// K7 on a device-resident float4 cloud: `out` receives the centroids, *n_out their number.
// Returns LIO_OK, or 1 when PCL would pass the cloud through (voxel index overflow).
// `ws`: the temporaries; `box` (optional) receives min[3], max[3] of the INPUT cloud, a box around the output.  Complete when
// it returns: the sorting form always ends with the wait for the voxel count.
// have_box: ws.bbox already holds the bounding box of d_in (k_transform_clouds_bbox), no pass for it.
template <class B>
int lio_voxel_grid_device(const float4* d_in, int n, float leaf, B& out, int* n_out, hipStream_t s, LioVoxWs<B>& ws, float* box,
                          bool have_box = false);
// the same in pool temporaries of its own; complete when it returns
int lio_voxel_grid_device(const float4* d_in, int n, float leaf, LioTemp& out, int* n_out, hipStream_t s);
