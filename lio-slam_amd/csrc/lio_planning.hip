// lio_planning.hip -- the one planning chain behind every entry point that starts from the resident keyframes: the local map
// (lio_localmap.hip) and the height map (lio_heightmap.hip) once, then the median fill (lio_medianfill.hip), the terrain
// layers (lio_terrain.hip) and the signed distance field (lio_sdf.hip), each on the device grid the stage before it leaves,
// with a resident layer set (lio_gridsample.hip) as an optional sink for the grids.  No kernel lives here: every stage is
// its own file's *_device function.  lio_kf_store_height_map, lio_kf_store_terrain_map and lio_kf_store_sdf (each in its
// stage's file) are this chain with one stage; here are lio_kf_store_planning_map and lio_kf_store_planning_grid.
// DESIGN.md sections 4j (the chain) and 4k (the sink).
#include <hip/hip_runtime.h>
#include <string.h>

#include "lio_planning.h"
#include "lio_gridsample.h"
#include "lio_heightmap.h"
#include "lio_kfstore.h"
#include "lio_localmap.h"
#include "lio_medianfill.h"
#include "lio_pool.h"
#include "lio_sdf.h"
#include "lio_terrain.h"

namespace {
// The chain's failure rule, stated once.  Armed from the moment the sink's geometry is set until its copies have been waited
// for, the guard makes every way out in between -- a stage's refusal, a HIPCHK -- wait for the stream, so that nothing is in
// flight on a temporary that goes back to the pool, and leave the sink without layers (include/liogpu.h).  It is declared
// behind the chain's temporaries: it runs before they are released.
struct ChainGuard {
    lio_grid* sink;
    hipStream_t s;
    bool armed;
    ~ChainGuard()
    {
        if (!armed) return;
        (void)hipStreamSynchronize(s);                     // (the error that armed exit returns comes first)
        if (sink) lio_grid_clear(sink);
    }
};
}

int lio_planning_chain(lio_kf_store* st, const lio_local_map_config* lm, const float* pose, const lio_height_map_config* hm,
                       LioPlanningRequest rq)
{
    lio_height_map_info hm_local;
    lio_median_fill_info fill_local;
    lio_terrain_info terrain_local;
    lio_sdf_info sdf_local;
    if (!rq.hm_info) rq.hm_info = &hm_local;
    if (!rq.fill_info) rq.fill_info = &fill_local;
    if (!rq.terrain_info) rq.terrain_info = &terrain_local;
    if (!rq.sdf_info) rq.sdf_info = &sdf_local;
    lio_height_map_info* const hm_info = rq.hm_info;
    memset(hm_info, 0, sizeof(*hm_info));
    memset(rq.fill_info, 0, sizeof(*rq.fill_info));
    memset(rq.terrain_info, 0, sizeof(*rq.terrain_info));
    memset(rq.sdf_info, 0, sizeof(*rq.sdf_info));
    if (!st || !lm || !pose || !hm || (rq.sdf && !rq.sdf_cfg)) return lio_fail(LIO_ERR_ARG, "null argument");
    int rc = lio_height_map_check(hm);
    if (rc != LIO_OK) return rc;
    LioMfParams P;
    LioTerrPlan plan;
    if (rq.fill) {
        if ((rc = lio_median_fill_check(rq.fill, hm->resolution, &P)) != LIO_OK) return rc;
        lio_median_fill_info_begin(rq.fill_info, P, 0, 0);
    }
    if (rq.terrain) {
        if ((rc = lio_terrain_check(rq.terrain, hm->resolution, &plan)) != LIO_OK) return rc;
        rq.terrain_info->normal_method_used = plan.method_used; rq.terrain_info->edge_window_size = plan.window;
    }
    if (rq.sdf) {
        if ((rc = lio_sdf_config_check(rq.sdf_cfg)) != LIO_OK) return rc;
        if ((rc = lio_sdf_begin(rq.sdf, st->device_id)) != LIO_OK) return rc;
    }
    if (rq.sink && (rc = lio_grid_begin(rq.sink, st->device_id)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    LocalMapBufs B;
    if ((rc = lio_local_map_device(st, lm, pose, B, nullptr, rq.lm_info, s)) != LIO_OK) return rc;
    if (B.n_cur == 0) return LIO_OK;                       // an empty store or an empty crop: rows = cols = 0
    if (!rq.fill && !rq.terrain && !rq.sdf && !rq.sink) return lio_height_map_device(B.cur, B.n_cur, hm, rq.out.grid, rq.out.grid_cap, hm_info, s);      // nothing goes on from the grid
    LioTemp d_grid, d_filled;
    rc = lio_height_map_device(B.cur, B.n_cur, hm, rq.out.grid, rq.out.grid_cap, hm_info, s, &d_grid);
    const int rows = hm_info->rows, cols = hm_info->cols;  // (before rc is looked at: what a caller with too small a buffer reads)
    if (rq.fill) { rq.fill_info->rows = rows; rq.fill_info->cols = cols; }
    if (rq.terrain) { rq.terrain_info->rows = rows; rq.terrain_info->cols = cols; }
    if (rq.sdf) { rq.sdf_info->rows = rows; rq.sdf_info->cols = cols; }
    if (rc != LIO_OK) return rc;
    if (!d_grid.p) return LIO_OK;                          // no point left or no extent along an axis: no grid, nothing behind it
    const size_t n_cells = (size_t)rows * (size_t)cols;
    if (rq.fill && ((rq.out.filled && n_cells > rq.out.filled_cap) || (rq.out.fill_mask && n_cells > rq.out.fill_mask_cap)))
        return lio_fail(LIO_ERR_ARG, "filled or fill_mask holds fewer floats than the grid has cells (info)");
    if (rq.terrain && rq.out.layers && (size_t)plan.n_out * n_cells > rq.out.layers_cap)
        return lio_fail(LIO_ERR_ARG, "layers holds fewer floats than the requested layers (info)");
    if (rq.sink && (rc = lio_grid_set_geometry(rq.sink, rows, cols, hm->resolution, hm_info->length, hm_info->position)) != LIO_OK) return rc;
    ChainGuard guard = { rq.sink, s, true };
    const float* d_elev = d_grid.as<float>();
    float* d_sink[LIO_GRID_LAYER_TERRAIN + LIO_TERRAIN_N_LAYERS];      // the sink's slots in use
    memset(d_sink, 0, sizeof(d_sink));
    if (rq.sink) {
        if ((rc = lio_grid_layer_slot(rq.sink, LIO_GRID_LAYER_ELEVATION, &d_sink[LIO_GRID_LAYER_ELEVATION])) != LIO_OK) return rc;
        if (rq.fill && (rc = lio_grid_layer_slot(rq.sink, LIO_GRID_LAYER_FILLED, &d_sink[LIO_GRID_LAYER_FILLED])) != LIO_OK) return rc;
        for (int k = 0; rq.terrain && k < LIO_TERRAIN_N_LAYERS; ++k)
            if ((rc = lio_grid_layer_slot(rq.sink, LIO_GRID_LAYER_TERRAIN + k, &d_sink[LIO_GRID_LAYER_TERRAIN + k])) != LIO_OK) return rc;
        HIPCHK(hipMemcpyAsync(d_sink[LIO_GRID_LAYER_ELEVATION], d_elev, sizeof(float) * n_cells, hipMemcpyDeviceToDevice, s));
    }
    if (rq.fill) {
        P.rows = rows; P.cols = cols;
        HIPCHK(d_filled.alloc(sizeof(float) * n_cells));
        if ((rc = lio_median_fill_device(d_elev, P, nullptr, d_filled.as<float>(), rq.out.filled, rq.out.fill_mask, nullptr, rq.fill_info, s)) != LIO_OK) return rc;
        d_elev = d_filled.as<float>();
        if (rq.sink) HIPCHK(hipMemcpyAsync(d_sink[LIO_GRID_LAYER_FILLED], d_elev, sizeof(float) * n_cells, hipMemcpyDeviceToDevice, s));
    }
    if (rq.terrain) {
        if ((rc = lio_terrain_set_geometry(&plan, rows, cols, hm->resolution, hm_info->length, hm_info->position)) != LIO_OK) return rc;
        if ((rc = lio_terrain_device(d_elev, plan, rq.out.layers, rq.terrain_info, s, rq.sink ? d_sink + LIO_GRID_LAYER_TERRAIN : nullptr)) != LIO_OK) return rc;
    }
    if (rq.sink) HIPCHK(hipStreamSynchronize(s));          // the copies out of the temporaries are complete before these go back to the pool
    guard.armed = false;                                   // from here on the grids and the layers stay, whatever becomes of the field
    if (rq.sdf) {
        if ((rc = lio_sdf_check(rq.sdf_cfg, rows, cols, hm->resolution, hm_info->length, hm_info->position)) != LIO_OK) return rc;
        rc = lio_sdf_build_device(rq.sdf, d_elev, rows, cols, hm->resolution, hm_info->length, hm_info->position, *rq.sdf_cfg, rq.sdf_info, s);
        (void)hipStreamSynchronize(s);                     // (an early return leaves nothing in flight on the grid)
    }
    return rc;
}

extern "C" int lio_kf_store_planning_map(lio_kf_store* st, const lio_local_map_config* lm, const float* pose, const lio_height_map_config* hm,
                                         const lio_median_fill_config* fill, const lio_terrain_config* terrain, lio_sdf* sdf,
                                         const lio_sdf_config* sdf_cfg, const lio_planning_map_buffers* out, lio_local_map_info* lm_info,
                                         lio_height_map_info* hm_info, lio_median_fill_info* fill_info, lio_terrain_info* terrain_info,
                                         lio_sdf_info* sdf_info)
try {
    return lio_planning_chain(st, lm, pose, hm, { .fill = fill, .terrain = terrain, .sdf_cfg = sdf_cfg, .sdf = sdf,
                                                  .out = out ? *out : lio_planning_map_buffers{}, .lm_info = lm_info, .hm_info = hm_info,
                                                  .fill_info = fill_info, .terrain_info = terrain_info, .sdf_info = sdf_info });
} LIO_CATCH

// The same chain, which also leaves its grids in the resident layer set `grid_out` (NULL: none).
extern "C" int lio_kf_store_planning_grid(lio_kf_store* st, const lio_local_map_config* lm, const float* pose, const lio_height_map_config* hm,
                                          const lio_median_fill_config* fill, const lio_terrain_config* terrain, lio_sdf* sdf,
                                          const lio_sdf_config* sdf_cfg, const lio_planning_map_buffers* out, lio_local_map_info* lm_info,
                                          lio_height_map_info* hm_info, lio_median_fill_info* fill_info, lio_terrain_info* terrain_info,
                                          lio_sdf_info* sdf_info, lio_grid* grid_out)
try {
    return lio_planning_chain(st, lm, pose, hm, { .fill = fill, .terrain = terrain, .sdf_cfg = sdf_cfg, .sdf = sdf,
                                                  .out = out ? *out : lio_planning_map_buffers{}, .lm_info = lm_info, .hm_info = hm_info,
                                                  .fill_info = fill_info, .terrain_info = terrain_info, .sdf_info = sdf_info, .sink = grid_out });
} LIO_CATCH
