// lio_s2m_map.hip -- the resident map of a scan-to-map handle (include/liogpu.h): the three forms of set_map with their
// common head and tail (bounding box, grid plan, neighbourhood rows), sharing one handle's map with another, and the shard
// settings that say which part of the map's grid a handle owns.
#include <hip/hip_runtime.h>
#include <math.h>
#include <chrono>

#include "lio_gridplan.h"
#include "lio_handle.h"
#include "lio_multi.h"
#include "lio_wg.h"

// ------------------------------------------------------------------ set_map
static int lio_map_reserve(lio_s2m_handle* h, size_t n)
{
    const size_t nn = n ? n : 1;
    HIPCHK(h->d_mx.grow(nn));
    HIPCHK(h->d_my.grow(nn));
    HIPCHK(h->d_mz.grow(nn));
    HIPCHK(h->d_map4.grow(nn));
    HIPCHK(h->d_sorted.grow(nn));
    HIPCHK(h->d_cell_of.grow(nn));
    return LIO_OK;
}

// common head of the set-map entry points: n is refused if too large, the handle's device made current, the buffers of the
// points reserved; *t0 = the start of the upload time the profile reports
static int lio_map_begin(lio_s2m_handle* h, size_t n, std::chrono::steady_clock::time_point* t0)
{
    if (n >= (1ull << 25)) return lio_fail(LIO_ERR_CAPACITY, "map too large ((2k+1)^2 x n records must fit a 31-bit offset)");
    if (const int rc = lio_enter(h); rc != LIO_OK) return rc;
    *t0 = std::chrono::steady_clock::now();
    h->has_map = false;
    return lio_map_reserve(h, n);
}

// common tail: d_mx/d_my/d_mz/d_map4 hold the n map points -> bounding box, grid, neighbourhood rows
// `box` (optional): min[3], max[3] of a box known to contain every map point -- the grid is laid over it without a bounding-box
// pass and its read-back (any enclosing box gives an exact search; the grid is only a few cells larger) -- and the call
// returns with the build still in flight on the handle's stream: the registrations that follow are ordered behind it,
// sharers wait for ev_mapl[1], the build time is resolved when the profile is read.
static int lio_map_finish(lio_s2m_handle* h, size_t n, std::chrono::steady_clock::time_point t0, const float* box = nullptr)
{
    float mn[3], mx[3];
    // (a box that is not finite -- a keyframe cloud of nothing but non-finite points -- is ignored: the box is then computed here)
    for (int a = 0; a < 3 && box; ++a)
        if (!(box[a] <= box[3 + a]) || !(fabsf(box[a]) <= 1.0e15f) || !(fabsf(box[3 + a]) <= 1.0e15f)) box = nullptr;   // (LIO_MAX_COORD)
    if (box) {
        for (int a = 0; a < 3; ++a) { mn[a] = n ? box[a] : 0.0f; mx[a] = n ? box[3 + a] : 0.0f; }
    } else {
        unsigned init[6];
        lio_ord_box_clear(init);
        HIPCHK(hipMemcpyAsync(h->d_bbox, init, sizeof(init), hipMemcpyHostToDevice, h->stream));
        if (n) lio_launch_map_bbox(h->d_mx, h->d_my, h->d_mz, (int)n, h->d_bbox, h->stream);
        unsigned hb[6];
        HIPCHK(hipMemcpyAsync(hb, h->d_bbox, sizeof(hb), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        lio_ord_box_decode(hb, mn, mx);
        bool empty = (n == 0) || hb[0] == LIO_ORD_NO_MIN;
        // (a map without a single finite point leaves the reduction at its identities, max < min: an empty grid, every point outside it)
        for (int a = 0; a < 3 && !empty; ++a) empty = !(mn[a] <= mx[a]);
        for (int a = 0; a < 3 && empty; ++a) mn[a] = mx[a] = 0.0f;
    }

    auto t1 = std::chrono::steady_clock::now();

    // the plan (lio_gridplan.h): the main grid, the occupied cells where the table count hangs on them, then the tables
    const LioGridOverrides ov = lio_grid_overrides_from_env();
    LioGridPlan plan = lio_plan_grid(h->cfg, h->c.gate_reach, mn, mx, n, box != nullptr, ov);
    int occ = -1;
    if (plan.want_occupancy) {
        const LioGrid& g = plan.grid;
        HIPCHK(h->d_cell_count.grow((size_t)g.n_cells + 1));
        lio_launch_map_occupancy(g, h->d_mx, h->d_my, h->d_mz, (int)n, h->d_cell_count, h->stream);
        HIPCHK(hipMemcpyAsync(&occ, h->d_cell_count + g.n_cells, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    lio_plan_tables(plan, h->cfg, mn, mx, n, occ, ov);
    h->grid = plan.grid;
    const LioGrid& g = h->grid;
    HIPCHK(h->d_cell_count.grow(plan.n_cell_count));
    HIPCHK(h->d_cell_start.grow((size_t)g.n_cells + 1));
    HIPCHK(h->d_nbr_start.grow(plan.n_nbr_start));
    HIPCHK(h->d_nbr_pts.grow(plan.n_nbr_pts, 1.05));
    HIPCHK(h->d_tile_sums.grow(2 * ((size_t)lio_scan_tiles((int)(plan.len_a + plan.len_b)) + 1)));   // (64-bit pair sums)
    HIPCHK(h->d_nbr_slot.grow(plan.n_nbr_slot, 1.05));

    HIPCHK(hipEventRecord(box ? h->ev_mapl[0] : h->ev_map[0], h->stream));
    if (n) {
        lio_launch_map_build(g, h->d_mx, h->d_my, h->d_mz, (int)n, h->d_cell_of, h->d_cell_count,
                             h->d_cell_start, h->d_tile_sums, h->d_sorted, h->d_nbr_start, h->d_nbr_pts, h->d_nbr_slot, h->cfg.use_lds != 0, h->stream);
    } else {
        HIPCHK(hipMemsetAsync(h->d_cell_start, 0, sizeof(int) * ((size_t)g.n_cells + 1), h->stream));
        HIPCHK(hipMemsetAsync(h->d_nbr_start, 0, sizeof(int) * plan.n_nbr_start, h->stream));
    }
    HIPCHK(hipEventRecord(box ? h->ev_mapl[1] : h->ev_map[1], h->stream));
    HIPCHK(hipGetLastError());
    if (box) {
        h->map_timing_pending = true;
    } else {
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipGetLastError());
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, h->ev_map[0], h->ev_map[1]));
        h->prof.map_build_ms = ms;
        h->map_timing_pending = false;
        HIPCHK(hipEventRecord(h->ev_mapl[1], h->stream));            // "map ready" for sharers (already true)
    }
    h->prof.map_upload_ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
    h->prof.n_map = (int64_t)n;
    h->prof.n_cells = g.n_cells;
    h->prof.map_x_sub = g.xs;
    h->prof.map_tight_tables = plan.n_tb;
    h->prof.map_first_try = g.tb_try;
    h->prof.map_pts_per_cell = plan.pts_per_cell;
    h->n_map = n;
    h->has_map = true;
    h->graph_dirty = true;
    h->map_epoch++;
    return LIO_OK;
}

extern "C" int lio_s2m_set_map(lio_s2m_handle* h, const void* pts, size_t n, size_t stride)
try {
    if (!h) return lio_fail(LIO_ERR_ARG, "null handle");
    if (n > 0 && !pts) return lio_fail(LIO_ERR_ARG, "null map pointer");
    if (stride < 12 || (stride & 3)) return lio_fail(LIO_ERR_ARG, "stride_bytes must be >= 12 and a multiple of 4");
    if (h->multi) return lio_multi_set_map(h, pts, n, stride);
    if (h->map_src) return lio_fail(LIO_ERR_ARG, "this handle searches another handle's map (lio_s2m_share_map)");
    std::chrono::steady_clock::time_point t0;
    const int rc = lio_map_begin(h, n, &t0);
    if (rc != LIO_OK) return rc;
    HIPCHK(h->d_map_stage.grow((n ? n : 1) * stride));
    if (n) {
        HIPCHK(hipMemcpyAsync(h->d_map_stage, pts, n * stride, hipMemcpyHostToDevice, h->stream));
        lio_launch_aos_to_soa(h->d_map_stage, stride, (int)n, h->d_mx, h->d_my, h->d_mz, h->d_map4, h->stream);
    }
    return lio_map_finish(h, n, t0);
} LIO_CATCH

// Device-resident form used by lio_assemble_map: d_xyzi = float4 (x,y,z,intensity)[n] on h's device.
int lio_s2m_set_map_device_xyzi(lio_s2m_handle* h, const float4* d_xyzi, size_t n)
{
    if (!h) return lio_fail(LIO_ERR_ARG, "null handle");
    std::chrono::steady_clock::time_point t0;
    const int rc = lio_map_begin(h, n, &t0);
    if (rc != LIO_OK) return rc;
    HIPCHK(hipDeviceSynchronize());        // the producer ran on another stream
    lio_launch_xyzi4_to_soa(d_xyzi, (int)n, h->d_mx, h->d_my, h->d_mz, h->d_map4, h->stream);
    return lio_map_finish(h, n, t0);
}

// The same for a producer that ran on THIS handle's stream (lio_assemble_map_resident) and knows a box around the
// points: no device-wide wait, no bounding-box pass, no wait at the end (see lio_map_finish).
int lio_s2m_set_map_device_bbox(lio_s2m_handle* h, const float4* d_xyzi, size_t n, const float box[6])
{
    if (!h || !box) return lio_fail(LIO_ERR_ARG, "null argument");
    if (h->multi || h->map_src) return lio_fail(LIO_ERR_ARG, "this handle cannot take a device-resident map");
    h->run_pending = false;
    std::chrono::steady_clock::time_point t0;
    const int rc = lio_map_begin(h, n, &t0);
    if (rc != LIO_OK) return rc;
    lio_launch_xyzi4_to_soa(d_xyzi, (int)n, h->d_mx, h->d_my, h->d_mz, h->d_map4, h->stream);
    return lio_map_finish(h, n, t0, box);
}

hipStream_t lio_s2m_stream_of(lio_s2m_handle* h) { return h ? h->stream : nullptr; }
bool lio_s2m_takes_device_map(const lio_s2m_handle* h) { return h && !h->multi && !h->map_src; }

extern "C" int lio_s2m_set_global_grid(lio_s2m_handle* h, const float origin[3], const int32_t dims[3])
try {
    if (!h || !origin || !dims) return lio_fail(LIO_ERR_ARG, "null argument");
    for (int a = 0; a < 3; ++a) { h->gorigin[a] = origin[a]; h->gdims[a] = dims[a]; }
    h->has_global = true;
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_s2m_set_scan_shard(lio_s2m_handle* h, int32_t rank, int32_t world)
try {
    if (h && h->multi) return lio_refuse_multi();
    if (!h || world < 1 || rank < 0 || rank >= world) return lio_fail(LIO_ERR_ARG, "need 0 <= rank < world");
    h->block_rank = rank;
    h->block_world = world;
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_s2m_set_shard(lio_s2m_handle* h, int32_t axis, int32_t lo, int32_t hi)
try {
    if (h && h->multi) return lio_refuse_multi();
    if (!h) return lio_fail(LIO_ERR_ARG, "null handle");
    if (axis < 0) { h->shard.axis = -1; return LIO_OK; }
    if (axis > 2 || !h->has_global) return lio_fail(LIO_ERR_ARG, "set_global_grid first; axis in 0..2");
    const float cell = lio_gate_cell(h->cfg);
    h->shard.axis = axis;
    h->shard.gorigin = h->gorigin[axis];
    h->shard.inv_cell = 1.0f / cell;
    h->shard.gdim = h->gdims[axis];
    h->shard.lo = lo;
    h->shard.hi = hi;
    h->plan_ranks = 0;                 // (per-point ownership only; lio_s2m_set_shard_plan adds whole-workgroup ownership)
    h->graph_dirty = true;
    return LIO_OK;
} LIO_CATCH

// The full slab plan: rank `rank` of `n_ranks` owns cells [bounds[rank], bounds[rank+1]) along `axis` and HOLDS the map
// points of the cells [bounds[rank] - halo_cells, bounds[rank+1] + halo_cells) (what the caller passed to lio_s2m_set_map).
// With the whole plan known, a workgroup of scan points that fits one rank's held region is processed wholly by that rank
// (k_shard_cull); halo_cells = 1 reduces to lio_s2m_set_shard.  Every rank must be given the same bounds and halo.
extern "C" int lio_s2m_set_shard_plan(lio_s2m_handle* h, int32_t axis, int32_t n_ranks, int32_t rank, const int32_t* bounds,
                                      int32_t halo_cells)
try {
    if (!h || !bounds) return lio_fail(LIO_ERR_ARG, "null argument");
    if (h->multi) return lio_refuse_multi();
    if (n_ranks < 1 || n_ranks > 8 || rank < 0 || rank >= n_ranks || halo_cells < 1)
        return lio_fail(LIO_ERR_ARG, "need 1 <= n_ranks <= 8, 0 <= rank < n_ranks, halo_cells >= 1");
    for (int r = 0; r < n_ranks; ++r)
        if (bounds[r] > bounds[r + 1]) return lio_fail(LIO_ERR_ARG, "bounds must be non-decreasing");
    const int rc = lio_s2m_set_shard(h, axis, bounds[rank], bounds[rank + 1]);
    if (rc != LIO_OK) return rc;
    h->plan_ranks = halo_cells > 1 ? n_ranks : 0;
    h->plan_rank = rank;
    h->plan_halo = halo_cells;
    for (int r = 0; r <= n_ranks; ++r) h->plan_bounds[r] = bounds[r];
    return LIO_OK;
} LIO_CATCH

// Streaming (the metric includes the per-scan H2D): a second handle searches THIS handle's resident
// map, with its own stream and its own scan buffers, so that batch k+1 can be uploaded and tile-sorted while
// batch k iterates.  The map owner must outlive the sharer; replacing the map needs both streams idle.
extern "C" int lio_s2m_share_map(lio_s2m_handle* h, lio_s2m_handle* map_owner)
try {
    if (!h || h == map_owner) return lio_fail(LIO_ERR_ARG, "need two different handles");
    if (h->multi || (map_owner && map_owner->multi)) return lio_fail(LIO_ERR_ARG, "not available on a multi-device handle");
    if (map_owner && (map_owner->map_src || map_owner->cfg.device_id != h->cfg.device_id))
        return lio_fail(LIO_ERR_ARG, "the map owner must hold its own map on the same device");
    if (map_owner && h->cfg.use_lds && !map_owner->cfg.use_lds)
        return lio_fail(LIO_ERR_ARG, "cfg.use_lds needs the cell-sorted copy of the map, which only an owner created with use_lds builds");
    h->map_src = map_owner;
    h->map_epoch = map_owner ? map_owner->map_epoch : 0;
    h->graph_dirty = true;
    return LIO_OK;
} LIO_CATCH
