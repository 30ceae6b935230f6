// lio_ogm.h -- the planner's occupancy grid (lio_ogm.hip): what the entry points need, and the index arithmetic of the
// radius filter and of the raster as __host__ __device__ functions over an accessor, so that the kernels (device arrays) and
// a host program (checked arrays) run the same text.  DESIGN.md section 4h lists the conventions (parity unpinned).
// Everything here relies on -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include "../../include/liogpu.h"
#include "lio_pool.h"
#include "lio_gridmath.h"
#include "lio_types.h"

#define LIO_OGM_MAX_COORD 1.0e15f      // LIO_MAX_COORD: the bound of the cell sort
#define LIO_OGM_MAX_CELLS (1LL << 22)  // the cap of the search grid

// ---- the radius filter -------------------------------------------------------------------------------------------------
// the points that take part: the ones the cell sort bins
LIO_HD bool lio_ogm_takes_part(float x, float y, float z)
{
    return fabsf(x) <= LIO_OGM_MAX_COORD && fabsf(y) <= LIO_OGM_MAX_COORD && fabsf(z) <= LIO_OGM_MAX_COORD;
}

// lio_cell_coord (lio_s2m_device.h), the formula that bins the cloud: the same text, so the same cell
LIO_HD int lio_ogm_cell_coord(float v, float origin, float inv_cell, int n)
{
    float c = floorf((v - origin) * inv_cell);
    c = fminf(fmaxf(c, -4.0f), (float)(n + 3));
    return (int)c;
}

// the cell of a point of the grid's box, clamped (a binned point is inside: the clamp never acts on one)
LIO_HD void lio_ogm_cell(const LioGrid& g, float x, float y, float z, int& cx, int& cy, int& cz)
{
    cx = lio_ogm_cell_coord(x, g.ox, g.inv_cell, g.nx); cx = cx < 0 ? 0 : (cx > g.nx - 1 ? g.nx - 1 : cx);
    cy = lio_ogm_cell_coord(y, g.oy, g.inv_cell, g.ny); cy = cy < 0 ? 0 : (cy > g.ny - 1 ? g.ny - 1 : cy);
    cz = lio_ogm_cell_coord(z, g.oz, g.inv_cell, g.nz); cz = cz < 0 ? 0 : (cz > g.nz - 1 ? g.nz - 1 : cz);
}

// The edge of the search grid: the radius plus the slack of section 4b (1e-3 of the edge, 1e-5 of the box's longest side, which
// bounds |q - origin|), enlarged until the grid has at most 2^22 cells.  Fills *g as lio_icp_choose_grid does.
inline float lio_ogm_choose_grid(const float mn[3], const float mx[3], float radius, LioGrid* g)
{
    const float ext = fmaxf(fmaxf(mx[0] - mn[0], mx[1] - mn[1]), mx[2] - mn[2]);
    float e = radius * 1.001f + 1.0e-5f * ext;
    for (;;) {
        *g = LioGrid();
        g->ox = mn[0]; g->oy = mn[1]; g->oz = mn[2];
        g->inv_cell = 1.0f / e;
        g->nx = (int)fminf(floorf((mx[0] - mn[0]) * g->inv_cell), 1.0e9f) + 1;
        g->ny = (int)fminf(floorf((mx[1] - mn[1]) * g->inv_cell), 1.0e9f) + 1;
        g->nz = (int)fminf(floorf((mx[2] - mn[2]) * g->inv_cell), 1.0e9f) + 1;
        g->k = 1; g->xs = 1; g->nxf = g->nx; g->inv_cell_x = g->inv_cell; g->tb_try = -1;
        for (int l = 0; l < LIO_TB_MAX; ++l) g->tb_reach[l] = -1.0f;
        const long long nc = (long long)g->nx * g->ny * g->nz;
        if (nc <= LIO_OGM_MAX_CELLS) { g->n_cells = (int)nc; return e; }
        e *= 1.26f;
    }
}

// Run k (0 .. 8) of the 27 cells around (cx, cy, cz): the row (cy + k % 3 - 1, cz + k / 3 - 1), x cells cx - 1 .. cx + 1
// clipped to the grid, as [beg, end) of the cell-sorted cloud.  false: the row is outside the grid.  A::at(i) =
// cell_start[i], i in [0, n_cells].
template <class A>
LIO_HD bool lio_ogm_run(const LioGrid& g, const A& cell_start, int cx, int cy, int cz, int k, int& beg, int& end)
{
    const int y = cy + k % 3 - 1, z = cz + k / 3 - 1;
    if (y < 0 || y >= g.ny || z < 0 || z >= g.nz) return false;
    const int row = (z * g.ny + y) * g.nx;
    const int xa = cx - 1 < 0 ? 0 : cx - 1, xb = cx + 1 > g.nx - 1 ? g.nx - 1 : cx + 1;
    beg = cell_start.at(row + xa);
    end = cell_start.at(row + xb + 1);
    return true;
}

// FLANN L2_Simple in fp32, and the strict test against r2 = (float)((double)radius * radius)
LIO_HD bool lio_ogm_within(float qx, float qy, float qz, float mx, float my, float mz, float r2)
{
    const float dx = qx - mx, dy = qy - my, dz = qz - mz;
    const float d2 = ((dx * dx) + dy * dy) + dz * dz;
    return d2 < r2;
}

// k_i of the point (qx, qy, qz) over the cell-sorted cloud; stops once the count exceeds `stop_above` (INT_MAX: never).
// S::at(i) = sorted point i as float4 (x, y, z, -), i in [0, cell_start[n_cells]).
template <class A, class S>
LIO_HD int lio_ogm_count(const LioGrid& g, const A& cell_start, const S& sorted, float qx, float qy, float qz, float r2, int stop_above)
{
    int cx, cy, cz;
    lio_ogm_cell(g, qx, qy, qz, cx, cy, cz);
    int cnt = 0;
    for (int k = 0; k < 9; ++k) {
        int beg, end;
        if (!lio_ogm_run(g, cell_start, cx, cy, cz, k, beg, end)) continue;
        for (int c = beg; c < end; ++c) {
            const float4 m = sorted.at(c);
            cnt += lio_ogm_within(qx, qy, qz, m.x, m.y, m.z, r2) ? 1 : 0;
        }
        if (cnt > stop_above) break;
    }
    return cnt;
}

// ---- the raster ----------------------------------------------------------------------------------------------------------
struct LioOgmRaster {
    double x_min, y_min, res;
    int width, height;
    int j_end;                     // rows that can be filled: height - 1 as written, height for whole_box
};

// (int)((v - v_min) / resolution) of the draft, toward zero; false where the conversion would leave int (such a point is
// outside every grid that passed the 2^31 - 1 cell check)
LIO_HD bool lio_ogm_axis_index(double v, double v_min, double res, int& idx)
{
    const double d = (v - v_min) / res;
    if (!(d > -2147483648.0 && d < 2147483648.0)) return false;
    idx = (int)d;
    return true;
}

// the cell of a point, or -1 where the draft skips it: i < 0 || i >= width || j < 0 || j >= j_end
LIO_HD long long lio_ogm_raster_cell(const LioOgmRaster& R, float x, float y)
{
    int i, j;
    if (!lio_ogm_axis_index((double)x, R.x_min, R.res, i) || i < 0 || i >= R.width) return -1;
    if (!lio_ogm_axis_index((double)y, R.y_min, R.res, j) || j < 0 || j >= R.j_end) return -1;
    return (long long)i + (long long)j * (long long)R.width;
}

// width and height from the box, in fp64, toward zero.  false: more than 2^31 - 1 cells.
inline bool lio_ogm_dims(double x_min, double x_max, double y_min, double y_max, double res, int* width, int* height)
{
    const double w = floor((x_max - x_min) / res), h = floor((y_max - y_min) / res);     // (both quotients are >= 0)
    *width = *height = 0;
    if (!(w <= 2147483647.0) || !(h <= 2147483647.0) || w * h > 2147483647.0) return false;
    *width = (int)w; *height = (int)h;
    return true;
}

// ---- the host side (lio_ogm.hip)
// LIO_OK or LIO_ERR_ARG, before any device is touched
int lio_radius_check(float radius, int32_t min_neighbors);
int lio_ogm_check(const lio_ogm_config* cfg);

// pcl::RadiusOutlierRemoval on a device-resident float4 cloud (x, y, z, intensity) on stream `s`; synchronous.  `out`
// receives the kept points in input order.  d_count (device, n ints, may be null): k_i, -1 for a point that takes no part;
// null selects the form that stops a lane once k_i > min_neighbors.
int lio_radius_device(const float4* d_pts, int n, float radius, int min_neighbors, LioTemp& out, int* n_out, int* d_count, hipStream_t s);

// stage times of one chain, in ms (HIP events on the chain's stream): slice, grid build, search, compaction, raster, grid copy
enum { LIO_OGM_N_STAGES = 6 };

// The draft's chain on a device-resident float4 cloud on stream `s`: slice, filter, raster; the grid (may be null) and *info
// to the host.  Synchronous.  info->n_in is set to n.  times (may be null): LIO_OGM_N_STAGES floats, filled with the stage times.
int lio_ogm_device(const float4* d_pts, int n, const lio_ogm_config& cfg, int8_t* grid, size_t grid_cap, lio_ogm_info* info, hipStream_t s,
                   float* times);
float* lio_ogm_times_wanted(void);           // the calling thread's request (lio_ogm_debug_stage_ms): where its times go, or null
