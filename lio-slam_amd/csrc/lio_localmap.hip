// lio_localmap.hip -- the planning local map of publishLocalMap (MO:2442-2541) behind the K6 sum:
//   crop     pcl::transformPointCloud into the yaw-aligned vehicle frame (MO:2474-2489) and the two pcl::PassThrough filters
//            (MO:296-302, MO:2502-2506) as one predicate, compacted in order
//   filter   pcl::StatisticalOutlierRemoval<PointXYZI>::applyFilter (MO:293-294, MO:2513-2514), restated for the device:
//            k_sor_search   one lane per point, the exact mean_k + 1 nearest squared distances by Chebyshev shells of cells
//                           outwards over a cell-sorted grid of the cloud itself, no distance gate; the candidate list in LDS
//            k_sor_stats    mean, standard deviation and threshold from the workgroups' fp64 sums, in a fixed order
//            then the same order-preserving compaction
// DESIGN.md section 4d lists the conventions (parity unpinned, restated from memory).  -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <cmath>
#include <string.h>

#include "lio_localmap.h"
#include "lio_cloud.h"
#include "lio_compact.h"
#include "lio_icp.h"
#include "lio_kernels.h"
#include "lio_kfstore.h"
#include "lio_pool.h"
#include "lio_s2m_device.h"
#include "lio_wg.h"

#define SOR_LIST (LIO_SOR_MAX_K + 1)

// the points that take part in the filter: the ones the cell sort bins (finite, and within the map grid's coordinate bound)
__device__ __forceinline__ bool lm_finite(const float4& p)
{
    return fabsf(p.x) <= LIO_MAX_COORD && fabsf(p.y) <= LIO_MAX_COORD && fabsf(p.z) <= LIO_MAX_COORD;
}

// ---- crop -------------------------------------------------------------------------------------------------------------
struct LmCropPred {
    const float4* src;
    float M[12];
    float x_lo, x_hi, y_lo, y_hi;
    __device__ bool operator()(int i, float4& q) const
    {
        const float4 p = src[i];
        if (!(fabsf(p.x) <= FLT_MAX && fabsf(p.y) <= FLT_MAX && fabsf(p.z) <= FLT_MAX)) return false;
        q.x = ((M[0] * p.x + M[1] * p.y) + M[2] * p.z) + M[3];            // pcl::transformPointCloud, per point
        q.y = ((M[4] * p.x + M[5] * p.y) + M[6] * p.z) + M[7];
        q.z = ((M[8] * p.x + M[9] * p.y) + M[10] * p.z) + M[11];
        q.w = p.w;
        return q.x >= x_lo && q.x <= x_hi && q.y >= y_lo && q.y <= y_hi;   // PassThrough keeps both limits
    }
};

void lio_local_map_vehicle_frame(const float pose[6], float M[12])
{
    const float yaw = pose[2], x = pose[3], y = pose[4], z = pose[5];
    const float c = cosf(-yaw), s = sinf(-yaw);
    const float tx = x * c - y * s, ty = y * c + x * s, tz = z;            // MO:2474-2476
    const float m[12] = { c, -s, 0.0f, -tx, s, c, 0.0f, -ty, 0.0f, 0.0f, 1.0f, -tz };
    memcpy(M, m, sizeof(m));
}

int lio_crop_device(const float4* d_in, int n, const float M[12], float front, float left, float back, float right, LioTemp& out,
                    int* n_out, hipStream_t s)
{
    LmCropPred pred;
    pred.src = d_in;
    memcpy(pred.M, M, sizeof(pred.M));
    pred.x_lo = -left; pred.x_hi = right; pred.y_lo = -back; pred.y_hi = front;
    return compact_device(pred, n, out, n_out, s);
}

// ---- statistical outlier removal ------------------------------------------------------------------------------------------
struct LioSorStats {
    double mean, stddev, threshold;
    int n_finite, passthrough;
};

struct LioSorParams {
    LioGrid g;
    float cell;                    // cell edge
    const int* cell_start;         // n_cells + 1; the last entry = the points in the grid = the finite points
    const float4* sorted;          // the cloud, cell-sorted
    const float4* pts;             // the cloud as given
    int n, k;                      // k = mean_k + 1 list entries
    float* mean_dist;              // [n]
    double* partials;              // [workgroup][3]: sum of dist, sum of dist^2, points
};

// The list of lane t is s_d2[0 .. k)[t], ascending.  The bank of an entry is t mod 32 whatever the entry: the lanes of a
// wave never conflict, however far apart they are in their insertions.  `worst` mirrors the last entry.
__device__ __forceinline__ void sor_scan_run(const float4* __restrict__ sorted, int beg, int end, float qx, float qy, float qz,
                                             float (*s_d2)[256], int k, float& worst)
{
    const int t = (int)threadIdx.x;
    for (int s = beg; s < end; ++s) {
        const float4 m = sorted[s];
        const float dx = qx - m.x, dy = qy - m.y, dz = qz - m.z;
        const float d2 = ((dx * dx) + dy * dy) + dz * dz;          // FLANN L2_Simple
        if (d2 < worst) {                                          // (an equal distance changes nothing in the multiset)
            int j = k - 1;
            while (j > 0) {
                const float v = s_d2[j - 1][t];
                if (!(v > d2)) break;
                s_d2[j][t] = v;
                --j;
            }
            s_d2[j][t] = d2;
            worst = s_d2[k - 1][t];
        }
    }
}

// Shell r = the cells at Chebyshev distance r from the query's own.  A point of shell r is more than (r - 1) e away along one
// axis at least, so once the list is full and its worst entry is at most ((r - 1) e - slack)^2 no later shell can change
// it: the argument of the alignment's nearest neighbour (lio_icp.hip) with k entries in place of one.  No gate: a lane walks
// until its list is settled or the grid ends; shells are clipped to the grid.
__device__ static void sor_nearest(const LioSorParams& P, float qx, float qy, float qz, float (*s_d2)[256])
{
    const LioGrid& g = P.g;
    const float e = P.cell;
    const int k = P.k, t = (int)threadIdx.x;
    for (int j = 0; j < k; ++j) s_d2[j][t] = INFINITY;
    float worst = INFINITY;
    const int cx = min(max((int)floorf((qx - g.ox) * g.inv_cell), 0), g.nx - 1);
    const int cy = min(max((int)floorf((qy - g.oy) * g.inv_cell), 0), g.ny - 1);
    const int cz = min(max((int)floorf((qz - g.oz) * g.inv_cell), 0), g.nz - 1);
    const int r_far = max(max(max(cx, g.nx - 1 - cx), max(cy, g.ny - 1 - cy)), max(cz, g.nz - 1 - cz));
    const float span = fmaxf(fmaxf(fabsf(qx - g.ox), fabsf(qy - g.oy)), fabsf(qz - g.oz));
    const float slack = 1.0e-3f * e + 1.0e-5f * span;
    for (int r = 0; r <= r_far; ++r) {
        if (r > 1) {
            const float lb = (float)(r - 1) * e - slack;
            if (lb > 0.0f && lb * lb * 0.99999f >= worst) break;  // (worst = inf while the list is not full)
        }
        const int z0 = max(cz - r, 0), z1 = min(cz + r, g.nz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, g.ny - 1);
        for (int z = z0; z <= z1; ++z) {
            for (int y = y0; y <= y1; ++y) {
                const int row = (z * g.ny + y) * g.nx;
                if (abs(z - cz) == r || abs(y - cy) == r) {          // a face of the shell: one contiguous run of the row
                    const int xa = max(cx - r, 0), xb = min(cx + r, g.nx - 1);
                    if (xa <= xb) sor_scan_run(P.sorted, P.cell_start[row + xa], P.cell_start[row + xb + 1], qx, qy, qz, s_d2, k, worst);
                } else {                                               // the two end cells of the row
                    const int xl = cx - r, xh = cx + r;
                    if (xl >= 0) sor_scan_run(P.sorted, P.cell_start[row + xl], P.cell_start[row + xl + 1], qx, qy, qz, s_d2, k, worst);
                    if (xh < g.nx) sor_scan_run(P.sorted, P.cell_start[row + xh], P.cell_start[row + xh + 1], qx, qy, qz, s_d2, k, worst);
                }
            }
        }
    }
}

// One lane per point, in the caller's order.  dist_i -> mean_dist[i] (NaN: the point takes no part); the workgroup's sums
// -> partials, folded in a fixed order: xor butterfly 32 .. 1 in the wave, the waves ascending.
__global__ __launch_bounds__(256) void k_sor_search(LioSorParams P)
{
    __shared__ float s_d2[SOR_LIST][256];
    __shared__ double s_part[4][3];
    const int i = blockIdx.x * 256 + (int)threadIdx.x, t = (int)threadIdx.x;
    const int n_fin = P.cell_start[P.g.n_cells];
    double v[3] = { 0.0, 0.0, 0.0 };
    if (i < P.n) {
        const float4 p = P.pts[i];
        float dist = __int_as_float(0x7fc00000);
        if (lm_finite(p)) {
            dist = 0.0f;
            if (n_fin >= P.k) {                                       // (else: the cloud passes through, k_sor_stats says so)
                sor_nearest(P, p.x, p.y, p.z, s_d2);
                double sum = 0.0;                                     // entry 0 = the point itself, or a duplicate of it
                for (int j = 1; j < P.k; ++j) sum += (double)(float)sqrt((double)s_d2[j][t]);     // sqrtf, correctly rounded
                dist = (float)(sum / (double)(P.k - 1));
            }
            v[0] = (double)dist; v[1] = (double)(dist * dist); v[2] = 1.0;
        }
        P.mean_dist[i] = dist;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[a] += __shfl_xor(v[a], off);
    }
    const int lane = t & 63, wave = t >> 6;
    if (lane == 0) { s_part[wave][0] = v[0]; s_part[wave][1] = v[1]; s_part[wave][2] = v[2]; }
    __syncthreads();
    if (t < 3) P.partials[(size_t)blockIdx.x * 3 + t] = ((s_part[0][t] + s_part[1][t]) + s_part[2][t]) + s_part[3][t];
}

// One workgroup: thread t adds the partials of the workgroups t, t + 256, .. in ascending order, then the same butterfly
// and wave order; thread 0 forms the threshold.  The shape depends on the number of points alone.
__global__ __launch_bounds__(256) void k_sor_stats(const double* __restrict__ partials, int n_wg, int k, double stddev_mul, LioSorStats* __restrict__ st)
{
    __shared__ double s_part[4][3];
    const int t = (int)threadIdx.x;
    double v[3] = { 0.0, 0.0, 0.0 };
    for (int b = t; b < n_wg; b += 256)
#pragma unroll
        for (int a = 0; a < 3; ++a) v[a] += partials[(size_t)b * 3 + a];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[a] += __shfl_xor(v[a], off);
    }
    if ((t & 63) == 0) { s_part[t >> 6][0] = v[0]; s_part[t >> 6][1] = v[1]; s_part[t >> 6][2] = v[2]; }
    __syncthreads();
    if (t != 0) return;
    double w[3];
    for (int a = 0; a < 3; ++a) w[a] = ((s_part[0][a] + s_part[1][a]) + s_part[2][a]) + s_part[3][a];
    const int n = (int)w[2];
    st->n_finite = n;
    if (n < k) {                                                      // at most mean_k points: nothing is filtered
        st->passthrough = 1; st->mean = 0.0; st->stddev = 0.0; st->threshold = INFINITY;
        return;
    }
    const double mean = w[0] / (double)n;
    const double var = (w[1] - w[0] * w[0] / (double)n) / ((double)n - 1.0);
    const double sd = sqrt(var);
    st->passthrough = 0; st->mean = mean; st->stddev = sd; st->threshold = mean + stddev_mul * sd;
}

struct LmSorPred {
    const float4* src;
    const float* mean_dist;
    const LioSorStats* st;
    __device__ bool operator()(int i, float4& q) const
    {
        q = src[i];
        const float d = mean_dist[i];
        return d == d && (double)d <= st->threshold;                 // (NaN: a skipped point)
    }
};

int lio_sor_check(int32_t mean_k, float stddev_mul)
{
    if (mean_k < 1 || mean_k > LIO_SOR_MAX_K) return lio_fail(LIO_ERR_ARG, "mean_k must be in [1, 32]");
    if (!std::isfinite(stddev_mul)) return lio_fail(LIO_ERR_ARG, "stddev_mul must be finite");
    return LIO_OK;
}

// The filter's steps up to its grid: the box step of lio_cloud.h (one empty cell at the origin without a point on some axis),
// then lio_icp_choose_grid at (mean_k + 1) / 3 points per occupied cell.  lio_sor_device and the test hook
// lio_sor_debug_grid both go through here.
static int sor_lay_grid(const float4* d_pts, int n, int mean_k, hipStream_t s, LioSearchTarget& T)
{
    float mn[3], mx[3];
    const int rc = lio_search_target_box(d_pts, n, s, T, mn, mx);
    if (rc != LIO_OK) return rc;
    if (!T.any) { mn[0] = mn[1] = mn[2] = 0.0f; mx[0] = mx[1] = mx[2] = 0.0f; }       // no finite point: one empty cell
    // Edge: the walk stops after shell 1 once the sphere of one edge around the point holds the k entries; on a surface
    // that sphere holds about pi times the points of a cell, so k / 3 per occupied cell (3.7 at mean_k 10).
    return lio_icp_choose_grid(T.tx.as<float>(), T.ty.as<float>(), T.tz.as<float>(), n, mn, mx, (float)(mean_k + 1) / 3.0f, s, &T.g, &T.edge,
                               &T.occupied);
}

int lio_sor_device(const float4* d_pts, int n, int mean_k, float stddev_mul, LioTemp& out, int* n_out, float* d_mean_dist,
                   LioSorReport* rep, hipStream_t s)
{
    *n_out = 0;
    *rep = LioSorReport();
    int rc = lio_sor_check(mean_k, stddev_mul);
    if (rc != LIO_OK) return rc;
    if (n <= 0) { rep->passthrough = 1; rep->threshold = INFINITY; HIPCHK(out.alloc(16)); return 1; }
    // ---- the cloud as its own search target: SoA, box of its finite points, grid (sor_lay_grid), cell sort
    LioSearchTarget tg;
    LioTemp dist, partials, d_st;
    if (!d_mean_dist) { HIPCHK(dist.alloc(sizeof(float) * (size_t)n)); d_mean_dist = dist.as<float>(); }
    if ((rc = sor_lay_grid(d_pts, n, mean_k, s, tg)) != LIO_OK) return rc;
    const int n_wg = (n + 255) / 256;
    HIPCHK(partials.alloc(sizeof(double) * 3 * (size_t)n_wg));
    HIPCHK(d_st.alloc(sizeof(LioSorStats)));
    if ((rc = lio_search_target_sort(n, s, tg)) != LIO_OK) return rc;
    LioSorParams P;
    memset(&P, 0, sizeof(P));
    P.g = tg.g; P.cell = tg.edge;
    P.cell_start = tg.cell_start.as<int>(); P.sorted = tg.sorted.as<float4>(); P.pts = d_pts;
    P.n = n; P.k = mean_k + 1;
    P.mean_dist = d_mean_dist; P.partials = partials.as<double>();
    hipLaunchKernelGGL(k_sor_search, dim3(n_wg), dim3(256), 0, s, P);
    hipLaunchKernelGGL(k_sor_stats, dim3(1), dim3(256), 0, s, partials.as<double>(), n_wg, mean_k + 1, (double)stddev_mul, d_st.as<LioSorStats>());
    LmSorPred pred;
    pred.src = d_pts; pred.mean_dist = d_mean_dist; pred.st = d_st.as<LioSorStats>();
    LioSorStats h_st;
    HIPCHK(hipMemcpyAsync(&h_st, d_st.p, sizeof(h_st), hipMemcpyDeviceToHost, s));        // (lands under the compaction's wait)
    if ((rc = compact_device(pred, n, out, n_out, s)) != LIO_OK) return rc;
    rep->n_finite = h_st.n_finite; rep->passthrough = h_st.passthrough;
    rep->mean = h_st.mean; rep->stddev = h_st.stddev; rep->threshold = h_st.threshold;
    return h_st.passthrough ? 1 : LIO_OK;
}

// ------------------------------------------------ planning local map (publishLocalMap MO:2442-2541)
// The entry points: the outlier filter on a host cloud, and the chain on the resident keyframe store (lio_kfstore.h).
extern "C" int lio_sor_filter(int32_t device_id, const void* pts, size_t n, size_t stride, int32_t mean_k, float stddev_mul, void* out,
                              size_t out_stride, size_t* n_out, float* mean_dist, double stats[3])
try {
    if (!n_out || (n && !pts)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (stride < 12 || (stride & 3) || (out && (out_stride < 20 || (out_stride & 3))))
        return lio_fail(LIO_ERR_ARG, "stride must be >= 12, the output stride >= 20, both multiples of 4");
    if (n > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    int rc = lio_sor_check(mean_k, stddev_mul);
    if (rc != LIO_OK) return rc;
    *n_out = 0;
    if (stats) { stats[0] = 0.0; stats[1] = 0.0; stats[2] = INFINITY; }
    if (n == 0) return 1;                                  // nothing to filter: the pass-through of at most mean_k points
    if ((rc = lio_check_device(device_id)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    LioTemp raw, xyzi, inl, dist;
    HIPCHK(xyzi.alloc(n * sizeof(float4)));
    if (mean_dist) HIPCHK(dist.alloc(n * sizeof(float)));
    if ((rc = lio_upload_xyzi(pts, n, stride, stride >= 20 ? 16 : -1, raw, xyzi.as<float4>(), s)) != LIO_OK) return rc;
    int no = 0;
    LioSorReport rep;
    rc = lio_sor_device(xyzi.as<float4>(), (int)n, mean_k, stddev_mul, inl, &no, mean_dist ? dist.as<float>() : nullptr, &rep, s);
    if (rc < 0) return rc;
    if (mean_dist) HIPCHK(hipMemcpyAsync(mean_dist, dist.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
    const int rc2 = lio_copy_out(inl.as<float4>(), no, out, out_stride, s);
    if (rc2 < 0) return rc2;
    HIPCHK(hipStreamSynchronize(s));
    if (stats) { stats[0] = rep.mean; stats[1] = rep.stddev; stats[2] = rep.threshold; }
    *n_out = (size_t)no;
    return rc;
} LIO_CATCH

extern "C" int lio_sor_debug_grid(int32_t device_id, const void* pts, size_t n, size_t stride, int32_t mean_k, lio_icp_grid_info* out)
try {
    if (!out || (n && !pts)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (stride < 12 || (stride & 3)) return lio_fail(LIO_ERR_ARG, "stride must be >= 12 and a multiple of 4");
    if (n > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    int rc = lio_sor_check(mean_k, 1.0f);
    if (rc != LIO_OK) return rc;
    memset(out, 0, sizeof(*out));
    out->occupied = -1;
    if ((rc = lio_check_device(device_id)) != LIO_OK) return rc;
    if (!n) return LIO_OK;
    hipStream_t s = nullptr;
    LioTemp raw, xyzi;
    HIPCHK(xyzi.alloc(n * sizeof(float4)));
    if ((rc = lio_upload_xyzi(pts, n, stride, stride >= 20 ? 16 : -1, raw, xyzi.as<float4>(), s)) != LIO_OK) return rc;
    LioSearchTarget tg;
    if ((rc = sor_lay_grid(xyzi.as<float4>(), (int)n, mean_k, s, tg)) != LIO_OK) return rc;
    out->any = tg.any ? 1 : 0;
    out->origin[0] = tg.g.ox; out->origin[1] = tg.g.oy; out->origin[2] = tg.g.oz;
    out->edge = tg.edge; out->inv_cell = tg.g.inv_cell;
    out->nx = tg.g.nx; out->ny = tg.g.ny; out->nz = tg.g.nz; out->n_cells = tg.g.n_cells;
    out->occupied = tg.occupied;
    return LIO_OK;
} LIO_CATCH

extern "C" void lio_local_map_default_config(lio_local_map_config* cfg)
{
    if (!cfg) return;
    cfg->n_keyframes = 30;                                 // localMapKeyFramesNumber, UT:219
    cfg->front = 70.0f; cfg->left = 40.0f; cfg->back = 20.0f; cfg->right = 40.0f;        // UT:220-223
    cfg->remove_outliers = 1;                              // useRemovingOutliers, UT:227
    cfg->mean_k = 10;                                      // meanK, UT:228
    cfg->stddev_mul = 1.0f;                                // stddevThreshold, UT:229
    cfg->downsample = 1;                                   // useDownSamplingLocalMap, UT:224
    cfg->leaf = 0.01f;                                     // localMappingSurfLeafSize, UT:226
}

int lio_local_map_device(lio_kf_store* st, const lio_local_map_config* cfg, const float* pose, LocalMapBufs& B, size_t* n_out,
                         lio_local_map_info* info, hipStream_t s)
{
    LioTemp &d_kf = B.d_kf, &d_poses = B.d_poses, &d_chunks = B.d_chunks, &world = B.world, &cropped = B.cropped, &inl = B.inl, &ds = B.ds;
    B.cur = nullptr; B.n_cur = 0;
    if (cfg->n_keyframes < 1) return lio_fail(LIO_ERR_ARG, "n_keyframes must be >= 1");
    if (!std::isfinite(cfg->front) || !std::isfinite(cfg->left) || !std::isfinite(cfg->back) || !std::isfinite(cfg->right) ||
        !(-cfg->left <= cfg->right) || !(-cfg->back <= cfg->front))
        return lio_fail(LIO_ERR_ARG, "front, left, back, right must be finite with -left <= right and -back <= front");
    if ((cfg->remove_outliers != 0 && cfg->remove_outliers != 1) || (cfg->downsample != 0 && cfg->downsample != 1))
        return lio_fail(LIO_ERR_ARG, "remove_outliers and downsample are 0 or 1");
    int rc = lio_sor_check(cfg->mean_k, cfg->stddev_mul);
    if (rc != LIO_OK) return rc;
    if (!(cfg->leaf > 0.0f) || !std::isfinite(cfg->leaf)) return lio_fail(LIO_ERR_ARG, "leaf must be positive and finite");
    for (int j = 0; j < 6; ++j) if (!std::isfinite(pose[j])) return lio_fail(LIO_ERR_ARG, "non-finite pose");
    if (n_out) *n_out = 0;
    if (info) memset(info, 0, sizeof(*info));
    if ((rc = lio_check_device(st->device_id)) != LIO_OK) return rc;
    const int N = (int)st->off.size();
    if (N == 0) return LIO_OK;                             // MO:2444-2445
    const int first = N < cfg->n_keyframes ? 0 : N - cfg->n_keyframes;                     // startPoseNum, MO:2462
    // ---- the keyframe sum (lio_kfstore.h) over first .. N - 1 under the stored poses
    std::vector<int32_t> ids;
    for (int id = first; id < N; ++id) {
        if (!st->has_pose[(size_t)id]) return lio_fail(LIO_ERR_ARG, "a keyframe has no pose (lio_kf_store_set_poses)");
        ids.push_back(id);
    }
    LioKfSum t;
    lio_kf_sum_tables(st, ids.data(), ids.data(), (int)ids.size(), t);
    const size_t total = t.total;
    if (total > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "too many points");
    if (info) { info->first_keyframe = first; info->n_keyframes = N - first; info->n_summed = (int)total; }
    if (total == 0) return LIO_OK;
    if ((rc = lio_kf_sum_upload(t, t.poses.data(), d_kf, d_poses, d_chunks, s)) != LIO_OK) return rc;
    HIPCHK(world.alloc(total * sizeof(float4)));
    lio_kf_sum_launch(st, d_kf.as<LioKfDesc>(), d_poses.as<float>(), d_chunks.as<int2>(), (int)t.kf.size(), (int)t.chunks.size(), world.as<float4>(), s);
    // ---- vehicle frame + the two pass-throughs (the wait for the count also covers the descriptors' copies)
    float M[12];
    lio_local_map_vehicle_frame(pose, M);
    int n_cur = 0;
    if ((rc = lio_crop_device(world.as<float4>(), (int)total, M, cfg->front, cfg->left, cfg->back, cfg->right, cropped, &n_cur, s)) != LIO_OK)
        return rc;
    const float4* cur = cropped.as<float4>();
    if (info) info->n_cropped = n_cur;
    if (cfg->remove_outliers) {                            // MO:2510-2516
        LioSorReport rep;
        int n_inl = 0;
        if ((rc = lio_sor_device(cur, n_cur, cfg->mean_k, cfg->stddev_mul, inl, &n_inl, nullptr, &rep, s)) < 0) return rc;
        cur = inl.as<float4>(); n_cur = n_inl;
        if (info) { info->sor_mean = rep.mean; info->sor_stddev = rep.stddev; info->sor_threshold = rep.threshold; }
    }
    if (info) info->n_inliers = n_cur;
    if (cfg->downsample) {                                 // MO:2517-2540
        int n_ds = 0;
        if ((rc = lio_voxel_grid_device(cur, n_cur, cfg->leaf, ds, &n_ds, s)) < 0) return rc;
        if (info) info->voxel_passthrough = rc == 1 ? 1 : 0;
        if (n_cur > 0) { cur = ds.as<float4>(); n_cur = n_ds; }
    }
    if (info) info->n_out = n_cur;
    if (n_out) *n_out = (size_t)n_cur;
    B.cur = cur; B.n_cur = n_cur;
    return LIO_OK;
}

extern "C" int lio_kf_store_local_map(lio_kf_store* st, const lio_local_map_config* cfg, const float* pose, void* out, size_t out_stride,
                                      size_t out_cap, size_t* n_out, lio_local_map_info* info)
try {
    if (!st || !cfg || !pose) return lio_fail(LIO_ERR_ARG, "null argument");
    if (out && (out_stride < 20 || (out_stride & 3))) return lio_fail(LIO_ERR_ARG, "output stride must be >= 20 and a multiple of 4");
    hipStream_t s = nullptr;
    LocalMapBufs B;
    int rc = lio_local_map_device(st, cfg, pose, B, n_out, info, s);
    if (rc != LIO_OK) return rc;
    if (out && (size_t)B.n_cur > out_cap) return lio_fail(LIO_ERR_ARG, "out holds fewer records than the local map (*n_out)");
    if ((rc = lio_copy_out(B.cur, B.n_cur, out, out_stride, s)) < 0) return rc;
    return LIO_OK;
} LIO_CATCH
