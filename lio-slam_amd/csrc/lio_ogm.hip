// lio_ogm.hip -- the planner's occupancy grid: the chain of the fork's draft ogmGeneration.cpp (OG) on the device.
//   slice    pcl::PassThrough<PointXYZ> on z (OG:74-93): one predicate, compacted in order
//   filter   pcl::RadiusOutlierRemoval (OG:96-112), restated for the device:
//            k_ogm_search   one lane per point in cell-sorted order, the exact count of points with d2 < r2 over the nine
//                           runs of three cells around the point's cell of a cell-sorted grid of the cloud itself; a register
//                           counter, written through the sort's permutation
//            then the same order-preserving compaction
//   raster   SetMapTopicMsg (OG:115-188): k_ogm_box (the box, by default over all points but the last, as written),
//            k_ogm_mark (byte stores of 100), k_ogm_occupied (the count over the grid)
// DESIGN.md section 4h lists the conventions (parity unpinned).  -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <cmath>
#include <string.h>

#include "lio_ogm.h"
#include "lio_cloud.h"
#include "lio_compact.h"
#include "lio_kernels.h"
#include "lio_pool.h"
#include "lio_stageclock.h"
#include "lio_wg.h"

namespace {

struct OgmInts { const int* p; LIO_HD int at(int i) const { return p[i]; } };
struct OgmPts { const float4* p; LIO_HD float4 at(int i) const { return p[i]; } };

// ---- slice ------------------------------------------------------------------------------------------------------------
struct OgmSlicePred {
    const float4* src;
    float lo, hi;
    int negative;
    __device__ bool operator()(int i, float4& q) const
    {
        q = src[i];
        if (!(fabsf(q.x) <= FLT_MAX && fabsf(q.y) <= FLT_MAX && fabsf(q.z) <= FLT_MAX)) return false;   // PassThrough drops these first
        const bool inside = q.z >= lo && q.z <= hi;                                                     // both limits inclusive
        return negative ? !inside : inside;
    }
};

// ---- radius outlier removal -------------------------------------------------------------------------------------------
struct OgmSearch {
    LioGrid g;
    const int* cell_start;         // n_cells + 1; the last entry = the points that take part
    const float4* sorted;          // the cloud, cell-sorted; w = bits(input index)
    float r2;
    int stop_above;                // INT_MAX: the exact count; min_neighbors: a lane stops once it is exceeded
    int* count;                    // [n], by input index
};

// Lane s owns sorted point s: the lanes of a wave sit in the same or in neighbouring cells and walk the same runs.
__global__ __launch_bounds__(256) void k_ogm_search(OgmSearch P)
{
    const int s = blockIdx.x * 256 + (int)threadIdx.x;
    const OgmInts cs = { P.cell_start };
    if (s >= cs.at(P.g.n_cells)) return;
    const OgmPts pts = { P.sorted };
    const float4 q = pts.at(s);
    P.count[__float_as_int(q.w)] = lio_ogm_count(P.g, cs, pts, q.x, q.y, q.z, P.r2, P.stop_above);
}

struct OgmKeepPred {
    const float4* src;
    const int* count;
    int min_neighbors;
    __device__ bool operator()(int i, float4& q) const
    {
        q = src[i];
        return count[i] > min_neighbors;                               // (-1: the point takes no part)
    }
};

// ---- raster ------------------------------------------------------------------------------------------------------------
// bbox[0..1] = min x, y (ordered uint), bbox[3..4] = max; the third axis is carried along unused
__global__ __launch_bounds__(256) void k_ogm_box(const float4* __restrict__ pts, int m, unsigned* __restrict__ bbox)
{
    float mn[3] = { INFINITY, INFINITY, 0.0f }, mx[3] = { -INFINITY, -INFINITY, 0.0f };
    for (int i = blockIdx.x * 256 + (int)threadIdx.x; i < m; i += (int)gridDim.x * 256) {
        const float4 p = pts[i];
        mn[0] = fminf(mn[0], p.x); mx[0] = fmaxf(mx[0], p.x);
        mn[1] = fminf(mn[1], p.y); mx[1] = fmaxf(mx[1], p.y);
    }
    __shared__ LioWgBoxLds<4> s_box;
    float lo, hi;
    lio_wg_box(mn, mx, s_box, lo, hi);
    if (threadIdx.x < 2) {
        const int a = (int)threadIdx.x;
        atomicMin(&bbox[a], lio_f2ord(lo));
        atomicMax(&bbox[3 + a], lio_f2ord(hi));
    }
}

// every writer writes 100: plain byte stores; counts[0] += the points that were not skipped
__global__ __launch_bounds__(256) void k_ogm_mark(const float4* __restrict__ pts, int n, LioOgmRaster R, signed char* __restrict__ grid,
                                                  int* __restrict__ counts)
{
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    long long cell = -1;
    if (i < n) {
        const float4 p = pts[i];
        cell = lio_ogm_raster_cell(R, p.x, p.y);
        if (cell >= 0) grid[cell] = 100;
    }
    const unsigned long long m = __ballot(cell >= 0);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&counts[0], __popcll(m));
}

// counts[1] += the bytes of value 100 among the n16 16-byte words of the (zero-padded) grid
__global__ __launch_bounds__(256) void k_ogm_occupied(const uint4* __restrict__ grid16, int n16, int* __restrict__ counts)
{
    int c = 0;
    for (int i = blockIdx.x * 256 + (int)threadIdx.x; i < n16; i += (int)gridDim.x * 256) {
        const uint4 v = grid16[i];
        const unsigned w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 32; b += 8) c += ((w[a] >> b) & 0xffu) == 100u ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&counts[1], c);
}

// The chain's clock takes its marks in order: 0 before the slice (lio_ogm_device), here 1 (before the grid build), 2 (before
// the search), 3 (before the compaction), 4 (after it), then 5 after the raster and 6 after the grid copy.
int radius_device(const float4* d_pts, int n, float radius, int min_neighbors, LioTemp& out, int* n_out, int* d_count, hipStream_t s,
                  LioStageClock* clk)
{
    *n_out = 0;
    int rc = lio_radius_check(radius, min_neighbors);
    if (rc != LIO_OK) return rc;
    if (clk) clk->mark(s);
    if (n <= 0) {
        HIPCHK(out.alloc(16));
        if (clk) { clk->mark(s); clk->mark(s); clk->mark(s); }
        return LIO_OK;
    }
    // ---- the cloud as its own search target (lio_cloud.h): the box of the points that take part, one empty cell at the origin
    // without one, the grid from the radius alone, the cell sort
    LioSearchTarget tg;
    LioTemp own;
    const bool exact = d_count != nullptr;
    if (!exact) { HIPCHK(own.alloc(sizeof(int) * (size_t)n)); d_count = own.as<int>(); }
    float mn[3], mx[3];
    if ((rc = lio_search_target_box(d_pts, n, s, tg, mn, mx)) != LIO_OK) return rc;
    if (!tg.any) { mn[0] = mn[1] = mn[2] = 0.0f; mx[0] = mx[1] = mx[2] = 0.0f; }
    lio_ogm_choose_grid(mn, mx, radius, &tg.g);
    if ((rc = lio_search_target_sort(n, s, tg)) != LIO_OK) return rc;
    HIPCHK(hipMemsetAsync(d_count, 0xff, sizeof(int) * (size_t)n, s));               // -1: takes no part
    if (clk) clk->mark(s);
    OgmSearch P;
    memset(&P, 0, sizeof(P));
    P.g = tg.g; P.cell_start = tg.cell_start.as<int>(); P.sorted = tg.sorted.as<float4>();
    P.r2 = (float)((double)radius * (double)radius);
    P.stop_above = exact ? INT_MAX : min_neighbors;
    P.count = d_count;
    hipLaunchKernelGGL(k_ogm_search, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P);
    if (clk) clk->mark(s);
    OgmKeepPred pred;
    pred.src = d_pts; pred.count = d_count; pred.min_neighbors = min_neighbors;
    if ((rc = compact_device(pred, n, out, n_out, s)) != LIO_OK) return rc;
    if (clk) clk->mark(s);
    return LIO_OK;
}

thread_local LioStageTimes<LIO_OGM_N_STAGES> t_times;

}  // namespace

float* lio_ogm_times_wanted(void) { return t_times.on ? t_times.ms : nullptr; }

int lio_radius_check(float radius, int32_t min_neighbors)
{
    if (!std::isfinite(radius) || !(radius > 0.0f)) return lio_fail(LIO_ERR_ARG, "radius must be finite and positive");
    if (min_neighbors < 0) return lio_fail(LIO_ERR_ARG, "min_neighbors must not be negative");
    return LIO_OK;
}

int lio_ogm_check(const lio_ogm_config* cfg)
{
    if (!cfg) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!std::isfinite(cfg->z_min) || !std::isfinite(cfg->z_max) || cfg->z_min > cfg->z_max)
        return lio_fail(LIO_ERR_ARG, "z_min and z_max must be finite and z_min <= z_max");
    if ((cfg->z_negative | 1) != 1 || (cfg->remove_outliers | 1) != 1 || (cfg->whole_box | 1) != 1)
        return lio_fail(LIO_ERR_ARG, "z_negative, remove_outliers and whole_box must be 0 or 1");
    if (!std::isfinite(cfg->resolution) || cfg->resolution < 1e-4) return lio_fail(LIO_ERR_ARG, "resolution must be finite and at least 1e-4");
    if (cfg->remove_outliers) return lio_radius_check(cfg->radius, cfg->min_neighbors);
    return LIO_OK;
}

int lio_radius_device(const float4* d_pts, int n, float radius, int min_neighbors, LioTemp& out, int* n_out, int* d_count, hipStream_t s)
{
    return radius_device(d_pts, n, radius, min_neighbors, out, n_out, d_count, s, nullptr);
}

int lio_ogm_device(const float4* d_pts, int n, const lio_ogm_config& cfg, int8_t* grid, size_t grid_cap, lio_ogm_info* info, hipStream_t s,
                   float* times)
{
    memset(info, 0, sizeof(*info));
    info->n_in = n;
    if (times) memset(times, 0, sizeof(float) * LIO_OGM_N_STAGES);
    int rc = lio_ogm_check(&cfg);
    if (rc != LIO_OK) return rc;
    if (n <= 0) return LIO_OK;
    LioStageClock clk(times != nullptr);
    // ---- slice
    clk.mark(s);
    LioTemp sl, inl;
    OgmSlicePred slice;
    slice.src = d_pts; slice.lo = cfg.z_min; slice.hi = cfg.z_max; slice.negative = cfg.z_negative;
    int n_cur = 0;
    if ((rc = compact_device(slice, n, sl, &n_cur, s)) != LIO_OK) return rc;
    const float4* cur = sl.as<float4>();
    info->n_slice = n_cur;
    // ---- filter
    if (cfg.remove_outliers) {
        int n_inl = 0;
        if ((rc = radius_device(cur, n_cur, cfg.radius, cfg.min_neighbors, inl, &n_inl, nullptr, s, &clk)) != LIO_OK) return rc;
        cur = inl.as<float4>(); n_cur = n_inl;
    } else {
        for (int k = 1; k <= 4; ++k) clk.mark(s);
    }
    info->n_inliers = n_cur;
    if (n_cur == 0) { HIPCHK(hipStreamSynchronize(s)); return LIO_OK; }
    // ---- raster: the box (OG:139 stops one point short; a single point is its own box), the geometry on the host
    const int m = (cfg.whole_box || n_cur == 1) ? n_cur : n_cur - 1;
    LioTemp bbox, counts, d_grid;
    HIPCHK(bbox.alloc(6 * sizeof(unsigned)));
    HIPCHK(counts.alloc(2 * sizeof(int)));
    unsigned hb[6];
    lio_ord_box_clear(hb);
    HIPCHK(hipMemcpyAsync(bbox.p, hb, sizeof(hb), hipMemcpyHostToDevice, s));
    {
        const int nb = (m + 255) / 256;
        hipLaunchKernelGGL(k_ogm_box, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, s, cur, m, bbox.as<unsigned>());
    }
    HIPCHK(hipMemcpyAsync(hb, bbox.p, sizeof(hb), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    float mn[3], mx[3];
    lio_ord_box_decode(hb, mn, mx);
    LioOgmRaster R;
    R.x_min = (double)mn[0] + 0.0; R.y_min = (double)mn[1] + 0.0;       // (+ 0.0: a box that starts at -0 reports 0)
    R.res = cfg.resolution;
    info->origin[0] = R.x_min; info->origin[1] = R.y_min;
    if (!lio_ogm_dims(R.x_min, (double)mx[0], R.y_min, (double)mx[1], R.res, &R.width, &R.height))
        return lio_fail(LIO_ERR_CAPACITY, "the occupancy grid has more than 2^31 - 1 cells");
    R.j_end = cfg.whole_box ? R.height : R.height - 1;
    info->width = R.width; info->height = R.height;
    const size_t cells = (size_t)R.width * (size_t)R.height;
    if (cells == 0) return LIO_OK;
    if (grid && cells > grid_cap) return lio_fail(LIO_ERR_ARG, "grid holds fewer cells than width x height (info)");
    const size_t padded = (cells + 15) & ~(size_t)15;
    HIPCHK(d_grid.alloc(padded));
    HIPCHK(hipMemsetAsync(d_grid.p, 0, padded, s));
    HIPCHK(hipMemsetAsync(counts.p, 0, 2 * sizeof(int), s));
    hipLaunchKernelGGL(k_ogm_mark, dim3((unsigned)((n_cur + 255) / 256)), dim3(256), 0, s, cur, n_cur, R, d_grid.as<signed char>(), counts.as<int>());
    {
        const int n16 = (int)(padded / 16), nb = (n16 + 255) / 256;
        hipLaunchKernelGGL(k_ogm_occupied, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, s, d_grid.as<uint4>(), n16, counts.as<int>());
    }
    int hc[2] = { 0, 0 };
    HIPCHK(hipMemcpyAsync(hc, counts.p, sizeof(hc), hipMemcpyDeviceToHost, s));
    clk.mark(s);
    if (grid) HIPCHK(hipMemcpyAsync(grid, d_grid.p, cells, hipMemcpyDeviceToHost, s));
    clk.mark(s);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    info->n_binned = hc[0]; info->n_occupied = hc[1];
    if (times)
        for (int k = 0; k < LIO_OGM_N_STAGES; ++k) times[k] = clk.ms((size_t)k);
    return LIO_OK;
}

extern "C" void lio_ogm_default_config(lio_ogm_config* cfg)
{
    if (!cfg) return;
    cfg->z_min = 0.2f; cfg->z_max = 2.0f;    // thre_z_min, thre_z_max OG:205-206
    cfg->z_negative = 0;                     // flag_pass_through OG:207
    cfg->remove_outliers = 1;                // OG:227 runs the filter unconditionally
    cfg->radius = 0.5f;                      // thre_radius OG:208
    cfg->min_neighbors = 10;                 // thres_point_count OG:210
    cfg->resolution = 0.05;                  // map_resolution OG:209
    cfg->whole_box = 0;                      // as written
}

// Test and measurement hook: enable != 0 makes the calling thread's next chains record their stage boundaries; ms (may be
// NULL) receives the last chain's slice, grid build, search, compaction, raster and grid copy, in ms.
extern "C" int lio_ogm_debug_stage_ms(int32_t enable, float ms[6])
try {
    return t_times.hook(enable, ms);
} LIO_CATCH

extern "C" int lio_radius_filter(int32_t device_id, const void* pts, size_t n, size_t stride, float radius, int32_t min_neighbors, void* out,
                                 size_t out_stride, size_t* n_out, int32_t* n_neighbors)
try {
    if (!n_out || (n && !pts)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (stride < 12 || (stride & 3) || (out && (out_stride < 20 || (out_stride & 3))))
        return lio_fail(LIO_ERR_ARG, "stride must be >= 12, the output stride >= 20, both multiples of 4");
    if (n > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    int rc = lio_radius_check(radius, min_neighbors);
    if (rc != LIO_OK) return rc;
    *n_out = 0;
    if (n == 0) return LIO_OK;
    if ((rc = lio_check_device(device_id)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    LioTemp raw, xyzi, inl, cnt;
    HIPCHK(xyzi.alloc(n * sizeof(float4)));
    if (n_neighbors) HIPCHK(cnt.alloc(n * sizeof(int)));
    if ((rc = lio_upload_xyzi(pts, n, stride, stride >= 20 ? 16 : -1, raw, xyzi.as<float4>(), s)) != LIO_OK) return rc;
    int no = 0;
    if ((rc = lio_radius_device(xyzi.as<float4>(), (int)n, radius, min_neighbors, inl, &no, n_neighbors ? cnt.as<int>() : nullptr, s)) != LIO_OK)
        return rc;
    if (n_neighbors) HIPCHK(hipMemcpyAsync(n_neighbors, cnt.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
    if ((rc = lio_copy_out(inl.as<float4>(), no, out, out_stride, s)) < 0) return rc;
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    *n_out = (size_t)no;
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_occupancy_grid(int32_t device_id, const void* pts, size_t n, size_t stride, const lio_ogm_config* cfg, int8_t* grid,
                                  size_t grid_cap, lio_ogm_info* info)
try {
    lio_ogm_info local;
    if (!info) info = &local;
    memset(info, 0, sizeof(*info));
    if (!cfg || (n && !pts)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (stride < 12 || (stride & 3)) return lio_fail(LIO_ERR_ARG, "stride must be >= 12 and a multiple of 4");
    if (n > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    int rc = lio_ogm_check(cfg);
    if (rc != LIO_OK) return rc;
    if (n == 0) return LIO_OK;                             // OG:134: an empty cloud, no grid
    if ((rc = lio_check_device(device_id)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    LioTemp raw, xyzi;
    HIPCHK(xyzi.alloc(n * sizeof(float4)));
    if ((rc = lio_upload_xyzi(pts, n, stride, stride >= 20 ? 16 : -1, raw, xyzi.as<float4>(), s)) != LIO_OK) return rc;
    rc = lio_ogm_device(xyzi.as<float4>(), (int)n, *cfg, grid, grid_cap, info, s, lio_ogm_times_wanted());
    (void)hipStreamSynchronize(s);                         // (an early return above leaves nothing in flight on the temporaries)
    return rc;
} LIO_CATCH
