// lio_heightmap.hip -- the planning height map of grid_map_pcl's loader as the fork rewrote it (GridMapPclLoader.cpp,
// PointcloudProcessor.cpp, helpers.cpp:97-105), behind the outlier and voxel filters:
//   level    R1, the ego-vehicle height filter in the levelled frame, R2 (GridMapPclLoader.cpp:80-85), one compaction
//   box      pcl::getMinMax3D -> the grid's geometry on the host (GridMapPclLoader.cpp:97-108, GridMap.cpp:44-59)
//   keys     getIndexFromPosition per point in fp64 (GridMapMath.cpp:147-160); the stable sort by cell is K7's (lio_voxsort.h)
//   ranges   every cell's run of the sorted pairs, and the points gathered into that order
//   mean     (float)(sum of (double) z in input order / count), one cell per lane (helpers.cpp:141-149)
//   cluster  connected components of a cell's points under fp32 squared distance <= tol^2 by label propagation, one
//            workgroup per cell, the cell in LDS when it fits and in global memory when not; ordered fp64 means; min / max
//   fill     the four nearest valid cells of a 10 x 10 window by the reference's insertion cascade; a pure stencil
// DESIGN.md section 4e lists the conventions (parity unpinned).  -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <cmath>
#include <string.h>
#include <utility>

#include "lio_heightmap.h"
#include "lio_cloud.h"
#include "lio_compact.h"
#include "lio_localmap.h"
#include "lio_planning.h"
#include "lio_pool.h"
#include "lio_s2m_device.h"
#include "lio_wg.h"

#define HM_TILE 1024               // points of a cell the cluster kernel keeps in LDS (16 KiB); longer cells stay in global memory
#define HM_NAN __int_as_float(0x7fc00000)

// ---- level, ego filter, un-level ---------------------------------------------------------------------------------------
struct HmEgoPred {
    const float4* src;
    float R1[9], R2[9];
    int level;
    __device__ bool operator()(int i, float4& q) const
    {
        const float4 p = src[i];
        if (!(fabsf(p.x) <= LIO_MAX_COORD && fabsf(p.y) <= LIO_MAX_COORD && fabsf(p.z) <= LIO_MAX_COORD)) return false;
        if (!level) { q = make_float4(p.x, p.y, p.z, 0.0f); return true; }
        const float x = (R1[0] * p.x + R1[1] * p.y) + R1[2] * p.z;        // pcl::transformPointCloud, no translation
        const float y = (R1[3] * p.x + R1[4] * p.y) + R1[5] * p.z;
        const float z = (R1[6] * p.x + R1[7] * p.y) + R1[8] * p.z;
        const float ax = fabsf(x), ay = fabsf(y);
        bool keep = true;                                                  // PointcloudProcessor.cpp:39-55
        if (ax < 20.0f && ay < 30.0f) keep = (ax < 2.5f && ay < 5.0f) ? (z < 1.0f) : (z < 2.0f);
        q.x = (R2[0] * x + R2[1] * y) + R2[2] * z;
        q.y = (R2[3] * x + R2[4] * y) + R2[5] * z;
        q.z = (R2[6] * x + R2[7] * y) + R2[8] * z;
        q.w = 0.0f;
        return keep;
    }
};

// Eigen::AngleAxisf::toRotationMatrix for a unit axis, term by term
static void hm_axis_rotation(float angle, int axis, float R[9])
{
    const float s = sinf(angle), c = cosf(angle);
    float ax[3] = { 0.0f, 0.0f, 0.0f }, sa[3], ca[3];
    ax[axis] = 1.0f;
    for (int k = 0; k < 3; ++k) { sa[k] = s * ax[k]; ca[k] = (1.0f - c) * ax[k]; }
    float tmp = ca[0] * ax[1];
    R[1] = tmp - sa[2]; R[3] = tmp + sa[2];
    tmp = ca[0] * ax[2];
    R[2] = tmp + sa[1]; R[6] = tmp - sa[1];
    tmp = ca[1] * ax[2];
    R[5] = tmp - sa[0]; R[7] = tmp + sa[0];
    for (int k = 0; k < 3; ++k) R[k * 3 + k] = ca[k] * ax[k] + c;
}

static void hm_mul(const float A[9], const float B[9], float C[9])
{
    float t[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) t[i * 3 + j] = (A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j]) + A[i * 3 + 2] * B[6 + j];
    memcpy(C, t, sizeof(t));
}

// getRigidBodyTransform (helpers.cpp:107-118): rotation = I; *= Rx; *= Ry; *= Rz(0); then Affine3f::rotate on the identity
static void hm_rigid(float rx, float ry, float R[9])
{
    const float I[9] = { 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f };
    float M[9], A[9];
    memcpy(M, I, sizeof(I));
    hm_axis_rotation(rx, 0, A); hm_mul(M, A, M);
    hm_axis_rotation(ry, 1, A); hm_mul(M, A, M);
    hm_axis_rotation(0.0f, 2, A); hm_mul(M, A, M);
    hm_mul(I, M, R);
}

void lio_hm_rotations(float roll, float pitch, float R1[9], float R2[9])
{
    hm_rigid(-roll, -pitch, R1);
    hm_rigid(roll, pitch, R2);
}

int lio_hm_level_ego(const float4* d_in, int n, const float R1[9], const float R2[9], int level, LioTemp& out, int* n_out, hipStream_t s)
{
    HmEgoPred pred;
    pred.src = d_in; pred.level = level;
    memcpy(pred.R1, R1, sizeof(pred.R1));
    memcpy(pred.R2, R2, sizeof(pred.R2));
    return compact_device(pred, n, out, n_out, s);
}

// ---- geometry (the box comes from K7's box pass, lio_cloud_box_launch) -----------------------------------------------
void lio_hm_geometry(const float mn[3], const float mx[3], double resolution, LioGridGeom* g)
{
    int sz[2];
    double position[2];
    for (int a = 0; a < 2; ++a) {
        const float len = mx[a] - mn[a], sum = mx[a] + mn[a];             // pcl::PointXYZ members: float arithmetic
        const double size = std::round((double)len / resolution);        // GridMap.cpp:49-50
        sz[a] = size >= 2147483647.0 ? INT_MAX : (int)size;
        position[a] = (double)sum / 2.0;
    }
    *g = lio_gm_geom(sz[0], sz[1], resolution, position[0], position[1]);
}

// ---- binning ------------------------------------------------------------------------------------------------------------
// getIndexFromPosition: v = ((p - 0.5 length_) - position_) / resolution, index = (int)(-v).  An index equal to the size falls
// into the reference's extra row or column, which nobody reads; a negative one cannot occur for finite input.  Both are
// keyed behind the last cell.
__global__ __launch_bounds__(256) void k_hm_keys(LioGridGeom B, const float4* __restrict__ p, int n, uint2* __restrict__ pairs, int* __restrict__ counters)
{
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    bool in = false;
    if (i < n) {
        const float4 v = p[i];
        const double a = -((((double)v.x - B.half[0]) - B.pos[0]) / B.res);
        const double b = -((((double)v.y - B.half[1]) - B.pos[1]) / B.res);
        in = a > -1.0 && a < (double)B.rows && b > -1.0 && b < (double)B.cols;       // (int) truncates toward zero
        const unsigned key = in ? (unsigned)((int)a + (int)b * B.rows) : (unsigned)(B.rows * B.cols);
        pairs[i] = make_uint2(key, (unsigned)i);
    }
    const unsigned long long m = __ballot(in);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&counters[0], __popcll(m));
}

void lio_hm_launch_keys(const float4* d_pts, int n, const LioGridGeom& g, uint2* pairs, int* counters, hipStream_t s)
{
    hipLaunchKernelGGL(k_hm_keys, dim3((n + 255) / 256), dim3(256), 0, s, g, d_pts, n, pairs, counters);
}

// range[c] = [first, last + 1) of cell c in the sorted pairs ((0, 0), from the memset, for an empty cell); sorted_pts = the points
// in that order.  The sort is stable: a cell's points keep their input order.
__global__ __launch_bounds__(256) void k_hm_ranges(const uint2* __restrict__ sorted, const float4* __restrict__ p, int n, unsigned n_cells,
                                                   int2* __restrict__ range, float4* __restrict__ sorted_pts)
{
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    const uint2 e = sorted[i];
    sorted_pts[i] = p[e.y];
    if (e.x >= n_cells) return;
    if (i == 0 || sorted[i - 1].x != e.x) range[e.x].x = i;
    if (i == n - 1 || sorted[i + 1].x != e.x) range[e.x].y = i + 1;
}

// ---- elevation without clustering --------------------------------------------------------------------------------------------
// calculateMeanOfPointPositions(cloud).z(): the fp64 sum of z in input order, divided by the count, rounded to float.  The
// additions are a serial chain by contract, so a cell is one lane's.  A lane walks its own run of sorted_pts and uses z of
// every 16-byte record: strided across the wave, 3/4 of the traffic unused, at about 7 points per cell.
__global__ __launch_bounds__(256) void k_hm_mean(const int2* __restrict__ range, const float4* __restrict__ sorted_pts, int n_cells,
                                                 int min_pts, int max_pts, float* __restrict__ layer)
{
    const int c = blockIdx.x * 256 + (int)threadIdx.x;
    if (c >= n_cells) return;
    const int2 r = range[c];
    const int m = r.y - r.x;
    float h = HM_NAN;
    if (m > 0 && m >= min_pts && m <= max_pts) {
        double sum = 0.0;
        for (int j = r.x; j < r.y; ++j) sum += (double)sorted_pts[j].z;
        h = (float)(sum / (double)m);
    }
    layer[c] = h;
}

// ---- elevation with clustering -----------------------------------------------------------------------------------------------
// Where a cell's points and labels live while it is clustered: LDS (HmLds) for up to HM_TILE points, global memory (HmGlobal)
// beyond.  Labels are positions inside the cell.
struct HmLds {
    float *x, *y, *z;
    int* lab;
    __device__ __forceinline__ float3 pt(int j) const { return make_float3(x[j], y[j], z[j]); }
    __device__ __forceinline__ float zz(int j) const { return z[j]; }
};
struct HmGlobal {
    const float4* p;
    int* lab;
    __device__ __forceinline__ float3 pt(int j) const { const float4 v = p[j]; return make_float3(v.x, v.y, v.z); }
    __device__ __forceinline__ float zz(int j) const { return p[j].z; }
};

struct HmClusterParams {
    const int2* range;
    const float4* sorted_pts;
    int* label;                    // [n], by sorted position: the labels of the cells that do not fit into LDS
    float* layer;
    int n_cells, min_pts, max_pts, cl_min, cl_max, use_max;
    float tol2;
};

// (h, r): a component's height and its first member; r < 0 = none.  std::min_element / std::max_element return the first of
// equal heights, and pcl::EuclideanClusterExtraction emits its clusters by ascending first member.
__device__ __forceinline__ bool hm_better(float h, int r, float bh, int br, int use_max)
{
    if (r < 0) return false;
    if (br < 0) return true;
    if (h == bh) return r < br;
    return use_max ? h > bh : h < bh;
}

// The components of m points by label propagation: every point starts as its own label; a sweep gives each point the smallest
// label within the tolerance, then labels are shortened through their own label (both only lower a label, to a member of the
// same component); sweeps repeat until one changes nothing, when every point carries its component's first member.  A sweep
// reads labels others are lowering: that changes how many sweeps it takes, never the fixed point.  Then the ordered fp64 mean
// of every kept component, and the first smallest (largest) of them.
template <class Acc>
__device__ void hm_cluster_cell(const Acc& A, int m, const HmClusterParams& P, float* s_h, int* s_r, float* out)
{
    const int t = (int)threadIdx.x;
    for (int j = t; j < m; j += 256) A.lab[j] = j;
    __syncthreads();
    for (;;) {
        int changed = 0;
        for (int i = t; i < m; i += 256) {
            const float3 q = A.pt(i);
            const int mine = A.lab[i];
            int best = mine;
            for (int j = 0; j < m; ++j) {
                const float3 v = A.pt(j);
                const float dx = q.x - v.x, dy = q.y - v.y, dz = q.z - v.z;
                const float d2 = ((dx * dx) + dy * dy) + dz * dz;        // FLANN L2_Simple
                if (d2 <= P.tol2) best = min(best, A.lab[j]);
            }
            if (best < mine) { A.lab[i] = best; changed = 1; }
        }
        if (!__syncthreads_or(changed)) break;
        for (int i = t; i < m; i += 256) { const int l = A.lab[i]; const int ll = A.lab[l]; if (ll < l) A.lab[i] = ll; }
        __syncthreads();
    }
    float bh = 0.0f;
    int br = -1;
    for (int r = t; r < m; r += 256) {
        if (A.lab[r] != r) continue;
        int cnt = 0;
        double sum = 0.0;
        for (int j = r; j < m; ++j)
            if (A.lab[j] == r) { sum += (double)A.zz(j); ++cnt; }
        if (cnt < P.cl_min || cnt > P.cl_max) continue;
        const float h = (float)(sum / (double)cnt);
        if (hm_better(h, r, bh, br, P.use_max)) { bh = h; br = r; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float oh = __shfl_xor(bh, off);
        const int orr = __shfl_xor(br, off);
        if (hm_better(oh, orr, bh, br, P.use_max)) { bh = oh; br = orr; }
    }
    if ((t & 63) == 0) { s_h[t >> 6] = bh; s_r[t >> 6] = br; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 4; ++w)
            if (hm_better(s_h[w], s_r[w], bh, br, P.use_max)) { bh = s_h[w]; br = s_r[w]; }
        *out = br >= 0 ? bh : HM_NAN;
    }
    __syncthreads();
}

// One workgroup per cell, the cells dealt out round robin; every branch on a cell is uniform over the workgroup.
__global__ __launch_bounds__(256) void k_hm_cluster(HmClusterParams P)
{
    __shared__ float s_x[HM_TILE], s_y[HM_TILE], s_z[HM_TILE];
    __shared__ int s_lab[HM_TILE];
    __shared__ float s_h[4];
    __shared__ int s_r[4];
    for (int c = blockIdx.x; c < P.n_cells; c += (int)gridDim.x) {
        const int2 r = P.range[c];
        const int m = r.y - r.x;
        if (!(m > 0 && m >= P.min_pts && m <= P.max_pts)) {
            if (threadIdx.x == 0) P.layer[c] = HM_NAN;
            continue;
        }
        if (m <= HM_TILE) {
            for (int j = (int)threadIdx.x; j < m; j += 256) {
                const float4 v = P.sorted_pts[r.x + j];
                s_x[j] = v.x; s_y[j] = v.y; s_z[j] = v.z;
            }
            HmLds A;
            A.x = s_x; A.y = s_y; A.z = s_z; A.lab = s_lab;
            hm_cluster_cell(A, m, P, s_h, s_r, &P.layer[c]);           // (its first barrier covers the stores above)
        } else {
            HmGlobal A;
            A.p = P.sorted_pts + r.x; A.lab = P.label + r.x;
            hm_cluster_cell(A, m, P, s_h, s_r, &P.layer[c]);
        }
    }
}

// ---- hole filling and the counts -----------------------------------------------------------------------------------------
// One lane per cell; reads `pre`, writes `post`: no cell sees another's fill.  fill == 0 copies (the reference as written:
// its pass searches a layer copied before any cell was computed, finds nothing and changes nothing).  fill == 1: the four
// nearest valid cells of rows [r - 5, r + 5) x cols [c - 5, c + 5), clipped, rows outermost, by the strict-< insertion
// cascade of GridMapPclLoader.cpp:225-249.  The distances are sqrt of small integers and only compared: the integers are.
// counters[1] += cells valid before the fill, counters[2] += cells filled.
__global__ __launch_bounds__(256) void k_hm_fill(const float* __restrict__ pre, float* __restrict__ post, int rows, int cols, int fill,
                                                 int* __restrict__ counters)
{
    const int c = blockIdx.x * 256 + (int)threadIdx.x;
    bool valid = false, filled = false;
    if (c < rows * cols) {
        float h = pre[c];
        valid = h == h;
        if (!valid && fill) {
            const int row = c % rows, col = c / rows;
            int d1 = INT_MAX, d2 = INT_MAX, d3 = INT_MAX, d4 = INT_MAX;
            float v1 = 0.0f, v2 = 0.0f, v3 = 0.0f, v4 = 0.0f;
            const int i0 = max(row - 5, 0), i1 = min(row + 5, rows), j0 = max(col - 5, 0), j1 = min(col + 5, cols);
            for (int i = i0; i < i1; ++i) {
                for (int j = j0; j < j1; ++j) {
                    const float v = pre[i + j * rows];
                    if (!(v == v)) continue;
                    const int d = (i - row) * (i - row) + (j - col) * (j - col);
                    if (d < d1) { d4 = d3; v4 = v3; d3 = d2; v3 = v2; d2 = d1; v2 = v1; d1 = d; v1 = v; }
                    else if (d < d2) { d4 = d3; v4 = v3; d3 = d2; v3 = v2; d2 = d; v2 = v; }
                    else if (d < d3) { d4 = d3; v4 = v3; d3 = d; v3 = v; }
                    else if (d < d4) { d4 = d; v4 = v; }
                }
            }
            if (d4 != INT_MAX) {
                h = (float)(((((double)v1 + (double)v2) + (double)v3) + (double)v4) / 4.0);
                filled = true;
            }
        }
        post[c] = h;
    }
    const unsigned long long mv = __ballot(valid), mf = __ballot(filled);
    if ((threadIdx.x & 63) == 0) {
        if (mv) atomicAdd(&counters[1], __popcll(mv));
        if (mf) atomicAdd(&counters[2], __popcll(mf));
    }
}

int lio_hm_grid(const float4* d_pts, const uint2* d_sorted, int n, const LioGridGeom& g, const lio_height_map_config* cfg, float* grid,
                int* counters, int h_counters[3], hipStream_t s, LioTemp* keep)
{
    const int n_cells = g.rows * g.cols;
    LioTemp range, sorted_pts, label, pre, post;
    HIPCHK(range.alloc(sizeof(int2) * (size_t)n_cells));
    HIPCHK(sorted_pts.alloc(sizeof(float4) * (size_t)n));
    HIPCHK(pre.alloc(sizeof(float) * (size_t)n_cells));
    HIPCHK(post.alloc(sizeof(float) * (size_t)n_cells));
    HIPCHK(hipMemsetAsync(range.p, 0, sizeof(int2) * (size_t)n_cells, s));
    hipLaunchKernelGGL(k_hm_ranges, dim3((n + 255) / 256), dim3(256), 0, s, d_sorted, d_pts, n, (unsigned)n_cells, range.as<int2>(),
                       sorted_pts.as<float4>());
    if (cfg->use_cluster) {
        HIPCHK(label.alloc(sizeof(int) * (size_t)n));
        HmClusterParams P;
        P.range = range.as<int2>(); P.sorted_pts = sorted_pts.as<float4>(); P.label = label.as<int>(); P.layer = pre.as<float>();
        P.n_cells = n_cells; P.min_pts = cfg->min_points_per_cell; P.max_pts = cfg->max_points_per_cell;
        P.cl_min = cfg->cluster_min_points; P.cl_max = cfg->cluster_max_points; P.use_max = cfg->use_max_height;
        P.tol2 = (float)((double)cfg->cluster_tolerance * (double)cfg->cluster_tolerance);      // what PCL hands FLANN
        hipLaunchKernelGGL(k_hm_cluster, dim3(n_cells < 4096 ? n_cells : 4096), dim3(256), 0, s, P);
    } else {
        hipLaunchKernelGGL(k_hm_mean, dim3((n_cells + 255) / 256), dim3(256), 0, s, range.as<int2>(), sorted_pts.as<float4>(), n_cells,
                           cfg->min_points_per_cell, cfg->max_points_per_cell, pre.as<float>());
    }
    hipLaunchKernelGGL(k_hm_fill, dim3((n_cells + 255) / 256), dim3(256), 0, s, pre.as<float>(), post.as<float>(), g.rows, g.cols,
                       cfg->fill_holes, counters);
    if (grid) HIPCHK(hipMemcpyAsync(grid, post.p, sizeof(float) * (size_t)n_cells, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_counters, counters, 3 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (keep) std::swap(keep->p, post.p);                  // the caller goes on from the device grid (and owns it)
    return LIO_OK;
}

// ------------------------------------------------ planning height map (grid_map_pcl's loader, helpers.cpp:97-105)
// The chain (it needs the outlier filter, K7 and K7's sort) and the entry points.
extern "C" void lio_height_map_default_config(lio_height_map_config* cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->roll = 0.0f; cfg->pitch = 0.0f;
    cfg->level_and_ego_filter = 1;                         // GridMapPclLoader.cpp:80-85
    cfg->remove_outliers = 1; cfg->mean_k = 10; cfg->stddev_mul = 1.0f;                  // parameters.yaml outlier_removal
    cfg->downsample = 0; cfg->voxel[0] = cfg->voxel[1] = cfg->voxel[2] = 0.1f;           // downsampling
    cfg->resolution = 0.2;                                 // grid_map
    cfg->min_points_per_cell = 1; cfg->max_points_per_cell = 1000000000;
    cfg->use_cluster = 0; cfg->cluster_tolerance = 1.0f;   // cluster_extraction
    cfg->cluster_min_points = 1; cfg->cluster_max_points = 1000000000; cfg->use_max_height = 0;
    cfg->fill_holes = 0;                                   // the reference as written
}

int lio_height_map_check(const lio_height_map_config* c)
{
    const int32_t flags[] = { c->level_and_ego_filter, c->remove_outliers, c->downsample, c->use_cluster, c->use_max_height, c->fill_holes };
    for (int32_t f : flags)
        if (f != 0 && f != 1) return lio_fail(LIO_ERR_ARG, "the flags of lio_height_map_config are 0 or 1");
    if (!std::isfinite(c->roll) || !std::isfinite(c->pitch)) return lio_fail(LIO_ERR_ARG, "roll and pitch must be finite");
    if (!(c->resolution >= 1e-4) || !std::isfinite(c->resolution)) return lio_fail(LIO_ERR_ARG, "resolution must be at least 1e-4");
    int rc = lio_sor_check(c->mean_k, c->stddev_mul);
    if (rc != LIO_OK) return rc;
    if (c->downsample) {                                   // K7 takes one leaf
        if (!(c->voxel[0] > 0.0f) || !std::isfinite(c->voxel[0]) || c->voxel[1] != c->voxel[0] || c->voxel[2] != c->voxel[0])
            return lio_fail(LIO_ERR_ARG, "downsample needs one positive, finite voxel size on all three axes");
    }
    if (c->min_points_per_cell < 0 || c->max_points_per_cell < 0 || c->cluster_min_points < 0 || c->cluster_max_points < 0)
        return lio_fail(LIO_ERR_ARG, "point counts must not be negative");
    if (c->use_cluster && (!(c->cluster_tolerance >= 0.0f) || !std::isfinite(c->cluster_tolerance)))
        return lio_fail(LIO_ERR_ARG, "cluster_tolerance must be finite and not negative");
    return LIO_OK;
}

int lio_height_map_device(const float4* d_in, int n, const lio_height_map_config* cfg, float* grid, size_t grid_cap, lio_height_map_info* info,
                          hipStream_t s, LioTemp* keep)
{
    int rc;
    const float4* cur = d_in;
    int n_cur = n;
    LioTemp inl, ds, lev;
    info->n_in = n;
    if (cfg->remove_outliers) {                            // PointcloudProcessor.cpp:62-70
        LioSorReport rep;
        int n_inl = 0;
        if ((rc = lio_sor_device(cur, n_cur, cfg->mean_k, cfg->stddev_mul, inl, &n_inl, nullptr, &rep, s)) < 0) return rc;
        cur = inl.as<float4>(); n_cur = n_inl;
    }
    info->n_inliers = n_cur;
    if (cfg->downsample && n_cur > 0) {                    // PointcloudProcessor.cpp:114-122
        int n_ds = 0;
        if ((rc = lio_voxel_grid_device(cur, n_cur, cfg->voxel[0], ds, &n_ds, s)) < 0) return rc;
        info->voxel_passthrough = rc == 1 ? 1 : 0;
        cur = ds.as<float4>(); n_cur = n_ds;
    }
    float R1[9], R2[9];
    lio_hm_rotations(cfg->roll, cfg->pitch, R1, R2);
    int n_lev = 0;
    if ((rc = lio_hm_level_ego(cur, n_cur, R1, R2, cfg->level_and_ego_filter, lev, &n_lev, s)) != LIO_OK) return rc;
    cur = lev.as<float4>(); n_cur = n_lev;
    info->n_filtered = n_cur;
    if (n_cur == 0) return LIO_OK;                         // no point: no grid
    float mn[3], mx[3];
    LioTemp bbox;                                          // K7's box pass (k_vox_bbox)
    if ((rc = lio_cloud_box_launch(cur, n_cur, bbox, s)) != LIO_OK) return rc;
    if ((rc = lio_cloud_box_wait(bbox, mn, mx, s)) != LIO_OK) return rc;
    HIPCHK(hipGetLastError());
    LioGridGeom g;
    lio_hm_geometry(mn, mx, cfg->resolution, &g);
    info->rows = g.rows; info->cols = g.cols;
    for (int a = 0; a < 2; ++a) { info->length[a] = g.len[a]; info->position[a] = g.pos[a]; }
    if (g.rows == 0 || g.cols == 0) return LIO_OK;         // (the reference asserts in GridMap::setGeometry)
    if ((long long)g.rows * g.cols > 0x7fffffffLL - 1024) return lio_fail(LIO_ERR_CAPACITY, "the grid has more than 2^31 cells");
    const size_t n_cells = (size_t)g.rows * (size_t)g.cols;
    if (!grid && !keep) return LIO_OK;                     // the geometry only
    if (grid && n_cells > grid_cap) return lio_fail(LIO_ERR_ARG, "grid holds fewer cells than rows x cols (info)");
    // ---- cells: keys, K7's stable sort (the key space: the cells and one key behind them), then lio_hm_grid
    LioVoxWs<LioTemp> ws;
    LioTemp counters;
    const int n_blocks = (n_cur + LIO_VS_THREADS * 4 - 1) / (LIO_VS_THREADS * 4);
    HIPCHK(ws.pairs_a.alloc(sizeof(uint2) * (size_t)n_cur));
    HIPCHK(ws.pairs_b.alloc(sizeof(uint2) * (size_t)n_cur));
    HIPCHK(ws.hist.alloc(sizeof(int) * (size_t)LIO_VS_BINS * n_blocks));
    HIPCHK(ws.row_total.alloc(sizeof(int) * LIO_VS_BINS));
    HIPCHK(counters.alloc(4 * sizeof(int)));
    HIPCHK(hipMemsetAsync(counters.p, 0, 4 * sizeof(int), s));
    lio_hm_launch_keys(cur, n_cur, g, ws.pairs_a.as<uint2>(), counters.as<int>(), s);
    int bits = 1;
    while (bits < 31 && (1LL << bits) < (long long)n_cells + 1) ++bits;
    const uint2* sorted = lio_vsort_pairs<LioTemp>(n_cur, bits, s, ws);
    int hc[3] = { 0, 0, 0 };
    if ((rc = lio_hm_grid(cur, sorted, n_cur, g, cfg, grid, counters.as<int>(), hc, s, keep)) != LIO_OK) return rc;
    info->n_binned = hc[0]; info->n_valid_cells = hc[1]; info->n_filled_cells = hc[2];
    return LIO_OK;
}

extern "C" int lio_height_map(int32_t device_id, const void* pts, size_t n, size_t stride, const lio_height_map_config* cfg, float* grid,
                              size_t grid_cap, lio_height_map_info* info)
try {
    if (!cfg || !info || (n && !pts)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (stride < 12 || (stride & 3)) return lio_fail(LIO_ERR_ARG, "stride must be >= 12 and a multiple of 4");
    if (n > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    int rc = lio_height_map_check(cfg);
    if (rc != LIO_OK) return rc;
    memset(info, 0, sizeof(*info));
    if (n == 0) return LIO_OK;                             // an empty cloud: rows = cols = 0
    if ((rc = lio_check_device(device_id)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    LioTemp raw, xyzi;
    HIPCHK(xyzi.alloc(n * sizeof(float4)));
    if ((rc = lio_upload_xyzi(pts, n, stride, -1, raw, xyzi.as<float4>(), s)) != LIO_OK) return rc;
    rc = lio_height_map_device(xyzi.as<float4>(), (int)n, cfg, grid, grid_cap, info, s);
    const hipError_t e = hipStreamSynchronize(s);          // (an early return: `raw` goes back to the pool when this returns)
    if (rc < 0) return rc;                                 // the chain's own error comes first
    HIPCHK(e);
    return rc;
} LIO_CATCH

// The local map's stages, then the chain above on the device cloud they leave: the planning chain (lio_planning.hip) without a
// stage behind the height map.
extern "C" int lio_kf_store_height_map(lio_kf_store* st, const lio_local_map_config* lm, const float* pose, const lio_height_map_config* cfg,
                                       float* grid, size_t grid_cap, lio_local_map_info* lm_info, lio_height_map_info* info)
try {
    if (!st || !lm || !pose || !cfg || !info) return lio_fail(LIO_ERR_ARG, "null argument");
    return lio_planning_chain(st, lm, pose, cfg, { .out = { .grid = grid, .grid_cap = grid_cap }, .lm_info = lm_info, .hm_info = info });
} LIO_CATCH
