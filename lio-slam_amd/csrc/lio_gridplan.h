// lio_gridplan.h -- the host arithmetic that lays out a map's search grid, its tight row tables and a scan's tile grid.
// Plain host C++, no HIP and no handle: lio_map_finish (lio_s2m_map.hip) runs the two steps around the device's occupancy
// count, lio_debug_grid_plan runs the same two for tests/test_nn_cases_cpu.py, which pins every field without a GPU.
// The search's exactness rests on these bits (-ffp-contract=off): which operand is float, which double, and the order stay.
#pragma once
#include <math.h>
#include <stdlib.h>
#include <algorithm>

#include "../../include/liogpu.h"
#include "lio_types.h"

// the cell size the gate radius needs: sqrt(max_sq_dist) + 0.1 % (the least cfg.cell_size lio_s2m_create accepts) ...
static inline float lio_gate_cell_min(const lio_s2m_config& cfg) { return sqrtf(cfg.max_sq_dist) * 1.001f; }
// ... and the one in effect (before division by cell_div)
static inline float lio_gate_cell(const lio_s2m_config& cfg) { return cfg.cell_size > 0.0f ? cfg.cell_size : lio_gate_cell_min(cfg); }

// LioConsts::gate_reach
static inline float lio_gate_reach(float max_sq_dist)
{   // each step rounded to fp32 on its own, as the device did
    volatile float r = sqrtf(max_sq_dist);
    r = r * 1.0001f;
    r = r + 1e-6f;
    return r;
}

// What the environment overrides for A/B runs, read at every map set (lio_grid_overrides_from_env).
struct LioGridOverrides {
    int x_sub = 0;                       // LIO_X_SUB = 1 | 2 | 4 | 8 (0: not given, or another value: ignored)
    bool has_tight = false;              // LIO_TIGHT = a comma separated, descending list of fractions (0 = none)
    int n_tight = 0;
    float tight[LIO_TB_MAX] = {};
    bool has_try = false;                // LIO_TRY = the table an unbounded query tries first
    int try_lvl = -1;
};

static inline LioGridOverrides lio_grid_overrides_from_env()
{
    LioGridOverrides ov;
    { const char* e = getenv("LIO_X_SUB"); const int v = e ? atoi(e) : 0; if (v == 1 || v == 2 || v == 4 || v == 8) ov.x_sub = v; }
    if (const char* e = getenv("LIO_TIGHT")) {
        ov.has_tight = true;
        for (const char* p = e; *p && ov.n_tight < LIO_TB_MAX;) {
            char* q = nullptr;
            const float v = strtof(p, &q);
            if (q == p) break;
            if (v >= 0.05f && v <= 1.0f && (ov.n_tight == 0 || v < ov.tight[ov.n_tight - 1])) ov.tight[ov.n_tight++] = v;
            p = (*q == ',') ? q + 1 : q;
            if (*q != ',') break;
        }
    }
    if (const char* e = getenv("LIO_TRY")) { ov.has_try = true; ov.try_lvl = atoi(e); }            // (A/B runs)
    return ov;
}

// The plan of one map set.  lio_plan_grid fills the first block, lio_plan_tables the rest.
struct LioGridPlan {
    LioGrid grid;
    float cell;                          // edge of the main grid's cells, after the growth steps
    int grow_steps;                      // times the cell grew by 1.5 to satisfy the size cap and the long-map rule
    bool want_occupancy;                 // the table count is to be decided from the occupied cells (lio_launch_map_occupancy)
    // ---- lio_plan_tables
    int n_tb;                            // tight row tables
    float pts_per_cell;                  // map points per occupied cell (0: not counted)
    size_t len_a, len_b, rows_b;         // buckets of the main rows, buckets and rows of the tight tables
    size_t reps;                         // row records per map point
    size_t n_cell_count, n_nbr_start, n_nbr_pts, n_nbr_slot;   // elements of the handle's buffers of those names
};

static inline bool lio_spacing_fits(float far_end, float slack) { return nextafterf(far_end, INFINITY) - far_end <= 0.5f * slack; }

// Step 1: the main grid over the box [mn, mx] of the n map points.  caller_box: the box came from the caller and the map
// set stays asynchronous (no read-back, hence no occupancy count).
static inline LioGridPlan lio_plan_grid(const lio_s2m_config& cfg, float gate_reach, const float mn[3], const float mx[3], size_t n,
                                        bool caller_box, const LioGridOverrides& ov)
{
    LioGridPlan p = {};
    // cell edge = gate radius (+0.1 %) / k; the candidate scan visits (2k+1)^3 cells
    int kdiv = cfg.cell_div;
    if (kdiv != 1 && kdiv != 2 && kdiv != 3) kdiv = 2;
    float cell = lio_gate_cell(cfg) / (float)kdiv;
    // x subdivision of the row buckets (LioGrid::xs, cfg.x_sub): auto = 4 for a batch handle, 1 for a node's handle (measured,
    // DESIGN.md section 6); LIO_X_SUB = 1 | 2 | 4 | 8 in the environment overrides it for A/B runs
    int xsub = cfg.x_sub > 0 ? cfg.x_sub : (cfg.max_batch >= 8 ? 4 : 1);
    if (ov.x_sub) xsub = ov.x_sub;
    // Long maps.  lio_cell_coord rounds (v - origin) at the fp32 spacing of the grid's EXTENT, so along y and z -- where the rows
    // around the query's are all the search sees -- a map point within the bound can be counted one cell too far once that
    // spacing comes near the grid's slack: the width of the rows searched (k cells, one for a tight table) less the largest
    // bound searched in them.  A grid is used only while the spacing at its far end is at most half of that slack; beyond,
    // the main grid takes larger cells and a tight table is left out (about 4 km of extent for a 1 m gate; the tables at
    // 4, 2 and 1 km).  Along x the row search takes the run [cell(qx - Rx), cell(qx + Rx)]: rounding is monotone, no margin to
    // lose.  The LDS-staged search (cfg.use_lds, lio_knn_lds) walks cx - k .. cx + k instead: for it the main grid obeys the
    // rule along x as well.  Half of the slack is a margin that held in every emulated case, not a proven bound: the four
    // roundings of a cell difference can add up to about 2.8 spacings in the worst case.
    LioGrid& g = p.grid;
    for (;;) {
        g.k = kdiv;
        g.inv_cell = 1.0f / cell;
        g.ox = mn[0] - 0.5f * cell; g.oy = mn[1] - 0.5f * cell; g.oz = mn[2] - 0.5f * cell;
        const double ex = ((double)mx[0] - g.ox) * g.inv_cell, ey = ((double)mx[1] - g.oy) * g.inv_cell,
                     ez = ((double)mx[2] - g.oz) * g.inv_cell;
        const double cells = (floor(ex) + 2.0) * (floor(ey) + 2.0) * (floor(ez) + 2.0);
        const float slack = (float)kdiv * cell - gate_reach;        // (grows by half a gate radius per step)
        if (cells * xsub <= 256.0 * 1024.0 * 1024.0 && lio_spacing_fits((mx[1] - g.oy) + cell, slack) && lio_spacing_fits((mx[2] - g.oz) + cell, slack) &&
            (!cfg.use_lds || lio_spacing_fits((mx[0] - g.ox) + cell, slack))) {
            g.nx = (int)floor(ex) + 2; g.ny = (int)floor(ey) + 2; g.nz = (int)floor(ez) + 2;
            g.n_cells = g.nx * g.ny * g.nz;
            break;
        }
        cell *= 1.5f;   // larger cells keep the search exact, only less selective
        ++p.grow_steps;
    }
    g.xs = xsub; g.nxf = g.nx * xsub; g.inv_cell_x = g.inv_cell * (float)xsub;
    p.cell = cell;
    // (auto tight rows on a handle set up for batches, see lio_plan_tables: costs one small kernel and a 4-byte read-back; a
    // map whose bounding box is still on the device stays asynchronous and gets one table)
    p.want_occupancy = cfg.tight_rows == 0 && cfg.max_batch >= 8 && !caller_box && n > 0;
    return p;
}

// Step 2: the tight row tables, the first try and the buffer lengths.  occupied: the cells of p.grid that hold a map point,
// as counted on the device where p.want_occupancy asked for it (ignored otherwise).
static inline void lio_plan_tables(LioGridPlan& p, const lio_s2m_config& cfg, const float mn[3], const float mx[3], size_t n,
                                   int occupied, const LioGridOverrides& ov)
{
    const size_t nn = n ? n : 1;
    LioGrid& g = p.grid;
    const int xsub = g.xs;
    // tight rows (LioGrid::tb_*, cfg.tight_rows): further row tables with k = 1 and cells of 0.6 / 0.3 / 0.15 x the gate radius
    // for the queries whose search bound is that small -- most of them from the second iteration on.  LIO_TIGHT = a comma
    // separated, descending list of fractions (0 = none) in the environment for A/B runs.
    float frac[LIO_TB_MAX] = { 0.6f, 0.3f, 0.15f };
    int n_tb = cfg.tight_rows > 0 ? std::min(cfg.tight_rows, LIO_TB_MAX) : 0;
    float pts_per_cell = 0.0f;
    int try_lvl = -1;
    if (cfg.tight_rows == 0 && cfg.max_batch >= 8) {
        // auto, a handle set up for batches: one table always; the finer ones where the map is dense enough to have queries for
        // them.  Points per occupied cell -> point spacing on the surfaces, s = cell / sqrt(points per cell); the fifth neighbour
        // of a query on such a surface is about 1.26 s away; a table is built when its reach is at least that.  (Measured on
        // the parameter sets of tools/param_sets.sh: the sparse 0.5 m maps are fastest with one table -- a second one only adds
        // build time --, the 0.1 m map with three: +39 % registrations/s over one.)
        n_tb = 1;
        if (p.want_occupancy && occupied > 0) {
            pts_per_cell = (float)n / (float)occupied;
            const float spacing = p.cell / sqrtf(pts_per_cell);
            while (n_tb < LIO_TB_MAX && sqrtf(cfg.max_sq_dist) * frac[n_tb] >= 1.26f * spacing) ++n_tb;
            // the table an unbounded query tries first (LioGrid::tb_try): the tightest one 1.75x as wide as the expected
            // distance of the fifth neighbour.  (Measured: +27 % registrations/s on the 0.1 m map, +5 % on the 0.3 m map,
            // -4 % on the 0.5 m maps if forced there: nearly every wave then pays both searches -- the rule leaves those out.)
            for (int l = 0; l < n_tb; ++l)
                if (sqrtf(cfg.max_sq_dist) * frac[l] >= 2.2f * spacing) try_lvl = l;
        }
    }
    if (ov.has_tight) {
        n_tb = ov.n_tight;
        for (int l = 0; l < n_tb; ++l) frac[l] = ov.tight[l];
    }
    if ((double)g.n_cells * xsub > 64.0 * 1024.0 * 1024.0) n_tb = 0;        // (a grid that large is mostly empty buckets already)
    size_t len_b = 0, rows_b = 0;
    for (int l = 0; l < LIO_TB_MAX; ++l) {
        g.tb_row0[l] = 0; g.tb_ny[l] = g.tb_nz[l] = 0; g.tb_oy[l] = g.tb_oz[l] = 0.0f; g.tb_inv_cell[l] = 0.0f; g.tb_reach[l] = -1.0f;
        if (l >= n_tb) continue;
        const float reach = sqrtf(cfg.max_sq_dist) * frac[l], cb = reach * 1.001f;
        const float inv = 1.0f / cb, oy = mn[1] - 0.5f * cb, oz = mn[2] - 0.5f * cb;
        const double ny = floor(((double)mx[1] - oy) * inv) + 2.0, nz = floor(((double)mx[2] - oz) * inv) + 2.0;
        // (bucket indices stay far inside 31 bits, and so do record offsets: every table adds 9 records per point + row padding)
        const double recs = (double)nn * ((2 * g.k + 1) * (2 * g.k + 1) + 9.0 * (l + 1)) + LIO_ROW_ALIGN * ((double)g.ny * g.nz + (double)rows_b + ny * nz);
        if ((double)g.n_cells * xsub + (double)len_b + ny * nz * g.nxf > 192.0 * 1024.0 * 1024.0 || recs > 2040.0 * 1024.0 * 1024.0) { n_tb = l; continue; }
        // (long maps, see lio_plan_grid: the bounded search walks this table for Rx <= reach, i.e. for true distances up to reach / 1.0001)
        const float slack = cb - reach / 1.0001f;
        if (!lio_spacing_fits((mx[1] - oy) + cb, slack) || !lio_spacing_fits((mx[2] - oz) + cb, slack)) { n_tb = l; continue; }
        g.tb_inv_cell[l] = inv; g.tb_oy[l] = oy; g.tb_oz[l] = oz; g.tb_ny[l] = (int)ny; g.tb_nz[l] = (int)nz;
        g.tb_row0[l] = (int)((size_t)g.n_cells * xsub + len_b);
        g.tb_reach[l] = reach;
        rows_b += (size_t)g.tb_ny[l] * g.tb_nz[l];
        len_b += (size_t)g.tb_ny[l] * g.tb_nz[l] * g.nxf;
    }
    if (ov.has_try) try_lvl = ov.try_lvl;
    g.tb_try = (try_lvl >= 0 && try_lvl < n_tb) ? try_lvl : (try_lvl >= n_tb ? n_tb - 1 : -1);
    for (int l = 0; l < LIO_TB_MAX; ++l) {
        // (reach / 1.0002)^2, rounded towards zero by one more part in 10^6
        const float r = g.tb_reach[l] > 0.0f ? g.tb_reach[l] / 1.0002f : 0.0f;
        g.tb_try_b2[l] = r * r * 0.999999f;
    }
    p.n_tb = n_tb;
    p.pts_per_cell = pts_per_cell;
    p.len_a = (size_t)g.n_cells * xsub; p.len_b = len_b; p.rows_b = rows_b;
    p.reps = (size_t)((2 * g.k + 1) * (2 * g.k + 1)) + 9 * (size_t)n_tb;
    p.n_cell_count = (size_t)g.n_cells + p.len_a + len_b;                 // (point counts + row bucket lengths of both tables)
    p.n_nbr_start = p.len_a + len_b + 1;
    p.n_nbr_pts = nn * p.reps + LIO_ROW_ALIGN * ((size_t)g.ny * g.nz + rows_b) + 4 * LIO_ROW_ALIGN;
    p.n_nbr_slot = nn * p.reps;
}

// Scan-local tile grid over the box [mn, mx] of one scan (lio_s2m_batch_upload): tiles of edge `tile`, doubled until the grid
// has at most 262144 of them.  key_offset is the caller's.
static inline LioScanTiles lio_plan_scan_tiles(const float mn[3], const float mx[3], float tile, int shard_axis)
{
    LioScanTiles t;
    for (;;) {
        t.inv_tile = 1.0f / tile;
        const double ex = floor(((double)mx[0] - mn[0]) * t.inv_tile) + 1.0, ey = floor(((double)mx[1] - mn[1]) * t.inv_tile) + 1.0,
                     ez = floor(((double)mx[2] - mn[2]) * t.inv_tile) + 1.0;
        if (ex * ey * ez <= 262144.0) { t.ntx = (int)ex; t.nty = (int)ey; t.ntz = (int)ez; break; }
        tile *= 2.0f;
    }
    t.ox = mn[0]; t.oy = mn[1]; t.oz = mn[2];
    t.key_offset = 0;
    // Order of the tiles = order of the association workgroups' points.  Unsharded: x fastest.  With a sharded map
    // the shard axis varies slowest, so a workgroup's 256 points form a slice about one tile thick ACROSS that
    // axis and k_shard_cull can drop it on every rank but one or two.  (Lidar frame; effective while the
    // vehicle's heading stays within ~45 degrees of a map axis, merely less effective -- never wrong -- otherwise.)
    t.mx = 1; t.my = t.ntx; t.mz = t.ntx * t.nty;
    if (shard_axis == 0) { t.mz = 1; t.my = t.ntz; t.mx = t.ntz * t.nty; }
    else if (shard_axis == 1) { t.mx = 1; t.mz = t.ntx; t.my = t.ntx * t.ntz; }
    return t;
}
