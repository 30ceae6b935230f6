// lio_terrain.hip -- the terrain layers a planner steers by, from the elevation grid the height map leaves on the device:
// grid_map_demos/config/filters_demo_filter_chain.yaml behind `elevation_inpainted`,
//   main   smooth (MeanInRadiusFilter.cpp:59-79), the surface normal (NormalVectorsFilter.cpp: area :195-251, raster
//          :304-394), slope = acos(normal_z), roughness = |input - smooth|, traversability and its two ThresholdFilters
//   edges  the windowed standard deviation of slope (SlidingWindowMathExpressionFilter.cpp:74-92)
// One lane per cell.  A workgroup owns a tile of LIO_TILE_ROWS x LIO_TILE_COLS cells (lio_gridtile.h) and stages it with the
// halo of the largest stencil into LDS: at a radius of 3 cells a value is read about 37 times by its neighbours' circles,
// once from memory.  `edges` needs the neighbours' slope, so it is a second kernel over the slope layer; everything else
// needs the input tile only.  The per-cell arithmetic is in lio_terrain.h; smooth and edges are the grid filters' own cells
// (lio_gridfilter.h: MEAN in a radius, STDDEV over a cropped window), called from here without their counters.  DESIGN.md
// section 4g lists the conventions (parity unpinned).  -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <cmath>
#include <string.h>

#include "lio_terrain.h"
#include "lio_cloud.h"
#include "lio_planning.h"
#include "lio_pool.h"

// out: LIO_TERRAIN_N_LAYERS layers of rows x cols (this kernel writes all but LIO_TERRAIN_EDGES).  counters[0..3] += finite
// input cells, normals written, circles of fewer than 3 points, degenerate covariances.
__global__ __launch_bounds__(LIO_TILE_LANES) void k_terr_main(LioTerrParams P, const float* __restrict__ in, float* __restrict__ out,
                                                                      int* __restrict__ counters)
{
    extern __shared__ __attribute__((aligned(16))) float s_tile[];
    int r, c;
    const LioTile T = lio_tile_stage(in, P.G.rows, P.G.cols, P.halo, s_tile, r, c);
    LioTerrCell o;
    o.valid = o.normal = o.few = o.degenerate = false;
    if (r < P.G.rows && c < P.G.cols) {
        lio_terr_cell(P, T, r, c, &o);
        const size_t n_cells = (size_t)P.G.rows * (size_t)P.G.cols, at = (size_t)r + (size_t)c * (size_t)P.G.rows;
        out[LIO_TERRAIN_SMOOTH * n_cells + at] = o.smooth;
        out[LIO_TERRAIN_NORMAL_X * n_cells + at] = o.nx;
        out[LIO_TERRAIN_NORMAL_Y * n_cells + at] = o.ny;
        out[LIO_TERRAIN_NORMAL_Z * n_cells + at] = o.nz;
        out[LIO_TERRAIN_SLOPE * n_cells + at] = o.slope;
        out[LIO_TERRAIN_ROUGHNESS * n_cells + at] = o.rough;
        out[LIO_TERRAIN_TRAVERSABILITY * n_cells + at] = o.trav;
    }
    const unsigned long long mv = __ballot(o.valid), mn = __ballot(o.normal), mf = __ballot(o.few), md = __ballot(o.degenerate);
    if ((threadIdx.x & 63) == 0) {
        if (mv) atomicAdd(&counters[0], __popcll(mv));
        if (mn) atomicAdd(&counters[1], __popcll(mn));
        if (mf) atomicAdd(&counters[2], __popcll(mf));
        if (md) atomicAdd(&counters[3], __popcll(md));
    }
}

__global__ __launch_bounds__(LIO_TILE_LANES) void k_terr_edges(LioTerrParams P, const float* __restrict__ slope, float* __restrict__ edges)
{
    extern __shared__ __attribute__((aligned(16))) float s_tile[];
    int r, c;
    const LioTile T = lio_tile_stage(slope, P.G.rows, P.G.cols, P.margin, s_tile, r, c);
    if (r < P.G.rows && c < P.G.cols)
        edges[(size_t)r + (size_t)c * (size_t)P.G.rows] = lio_gf_window_cell<LIO_GW_STDDEV, LIO_GW_CROP>(lio_terr_edge_window(P), T, nullptr, r, c).value;
}

// ---- the host side ------------------------------------------------------------------------------------------------------
extern "C" void lio_terrain_default_config(lio_terrain_config* cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->normal_method = 0;                                // surface_normals: no `algorithm`, so area
    cfg->normal_axis = 2;                                  // normal_vector_positive_axis: z
    cfg->normal_radius = 0.05;                             // surface_normals.radius
    cfg->smooth_radius = 0.06;                             // mean_in_radius.radius
    cfg->edge_window_size = 0;
    cfg->edge_window_length = 0.05;                        // edge_detection.window_length
    cfg->slope_critical = 0.6f; cfg->roughness_critical = 0.1f;
    cfg->slope_weight = 0.5f; cfg->roughness_weight = 0.5f;
    cfg->layers = (1u << LIO_TERRAIN_N_LAYERS) - 1u;
}

int lio_terrain_check(const lio_terrain_config* c, double resolution, LioTerrPlan* plan)
{
    memset(plan, 0, sizeof(*plan));
    if (!(resolution >= 1e-4) || !std::isfinite(resolution)) return lio_fail(LIO_ERR_ARG, "resolution must be at least 1e-4");
    if (c->normal_method != 0 && c->normal_method != 1) return lio_fail(LIO_ERR_ARG, "normal_method is 0 (area) or 1 (raster)");
    if (c->normal_axis < 0 || c->normal_axis > 2) return lio_fail(LIO_ERR_ARG, "normal_axis is 0, 1 or 2");
    const double lengths[] = { c->normal_radius, c->smooth_radius, c->edge_window_length };
    for (double v : lengths)
        if (!std::isfinite(v) || v < 0.0) return lio_fail(LIO_ERR_ARG, "radii and the window length must be finite and not negative");
    const float factors[] = { c->slope_critical, c->roughness_critical, c->slope_weight, c->roughness_weight };
    for (float v : factors)
        if (!std::isfinite(v) || v < 0.0f) return lio_fail(LIO_ERR_ARG, "criticals and weights must be finite and not negative");
    if (c->layers >> LIO_TERRAIN_N_LAYERS) return lio_fail(LIO_ERR_ARG, "layers has bits beyond LIO_TERRAIN_N_LAYERS");
    // the window: SlidingWindowIterator::setWindowLength (SlidingWindowIterator.cpp:35-42); an even explicit size throws there
    if (c->edge_window_size < 0 || (c->edge_window_size != 0 && c->edge_window_size % 2 == 0))
        return lio_fail(LIO_ERR_ARG, "edge_window_size must be odd (0: from edge_window_length)");
    LioGfWindow W;                                         // (its rows and columns come with the geometry: lio_terr_edge_window)
    if (lio_gf_window_plan(0, 0, resolution, LIO_GW_CROP, c->edge_window_size, c->edge_window_length, &W))
        return lio_fail(LIO_ERR_ARG, "the edge window reaches further than 32 cells");
    const bool fallback = c->normal_method == 0 && c->normal_radius <= 0.0;                // NormalVectorsFilter.cpp:39-51
    const int method = (c->normal_method == 1 || fallback) ? 1 : 0;
    double reach = c->smooth_radius / resolution;
    if (method == 0 && c->normal_radius / resolution > reach) reach = c->normal_radius / resolution;
    if (reach > (double)LIO_TILE_MAX_REACH) return lio_fail(LIO_ERR_ARG, "a radius reaches further than 32 cells");
    LioTerrParams& P = plan->P;
    P.r_smooth = c->smooth_radius; P.r_normal = c->normal_radius;
    P.method = method; P.axis = c->normal_axis;
    P.halo = lio_gf_halo(reach);
    P.margin = W.margin;
    P.s_crit = c->slope_critical; P.r_crit = c->roughness_critical; P.w_s = c->slope_weight; P.w_r = c->roughness_weight;
    plan->mask = c->layers;
    plan->n_out = __builtin_popcount(c->layers);
    plan->window = W.size;
    plan->method_used = fallback ? 1 : 0;
    return LIO_OK;
}

int lio_terrain_set_geometry(LioTerrPlan* plan, int rows, int cols, double resolution, const double length[2], const double position[2])
{
    if (const char* why = lio_gm_axes_refusal(rows, cols, resolution, length, position)) return lio_fail(LIO_ERR_ARG, why);
    plan->P.G = lio_gm_geom(rows, cols, resolution, position[0], position[1]);
    return LIO_OK;
}

int lio_terrain_device(const float* d_grid, const LioTerrPlan& plan, float* layers, lio_terrain_info* info, hipStream_t s, float* const* d_dst)
{
    const LioTerrParams& P = plan.P;
    const size_t n_cells = (size_t)P.G.rows * (size_t)P.G.cols;
    LioTemp out, counters;
    HIPCHK(out.alloc(sizeof(float) * LIO_TERRAIN_N_LAYERS * n_cells));
    HIPCHK(counters.alloc(4 * sizeof(int)));
    HIPCHK(hipMemsetAsync(counters.p, 0, 4 * sizeof(int), s));
    const unsigned tiles = lio_tile_count(P.G.rows, P.G.cols);
    const size_t lds_main = lio_tile_lds_bytes(P.halo, sizeof(float)), lds_edges = lio_tile_lds_bytes(P.margin, sizeof(float));
    float* d_out = out.as<float>();
    hipLaunchKernelGGL(k_terr_main, dim3(tiles), dim3(LIO_TILE_LANES), lds_main, s, P, d_grid, d_out, counters.as<int>());
    hipLaunchKernelGGL(k_terr_edges, dim3(tiles), dim3(LIO_TILE_LANES), lds_edges, s, P, (const float*)(d_out + LIO_TERRAIN_SLOPE * n_cells),
                       d_out + LIO_TERRAIN_EDGES * n_cells);
    if (layers) {                                          // the requested layers in enum order, neighbours in one copy
        size_t at = 0;
        for (int k = 0; k < LIO_TERRAIN_N_LAYERS;) {
            if (!((plan.mask >> k) & 1u)) { ++k; continue; }
            int e = k;
            while (e < LIO_TERRAIN_N_LAYERS && ((plan.mask >> e) & 1u)) ++e;
            HIPCHK(hipMemcpyAsync(layers + at, d_out + (size_t)k * n_cells, sizeof(float) * (size_t)(e - k) * n_cells, hipMemcpyDeviceToHost, s));
            at += (size_t)(e - k) * n_cells;
            k = e;
        }
    }
    if (d_dst)                                             // a resident layer set takes all of them
        for (int k = 0; k < LIO_TERRAIN_N_LAYERS; ++k)
            if (d_dst[k]) HIPCHK(hipMemcpyAsync(d_dst[k], d_out + (size_t)k * n_cells, sizeof(float) * n_cells, hipMemcpyDeviceToDevice, s));
    int hc[4] = { 0, 0, 0, 0 };
    HIPCHK(hipMemcpyAsync(hc, counters.p, sizeof(hc), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    info->n_valid_cells = hc[0]; info->n_normal_cells = hc[1]; info->n_few_points = hc[2]; info->n_degenerate = hc[3];
    return LIO_OK;
}

extern "C" int lio_terrain_layers(int32_t device_id, const float* elevation, int32_t rows, int32_t cols, double resolution, const double* length,
                                  const double* position, const lio_terrain_config* cfg, float* layers, size_t layers_cap, lio_terrain_info* info)
try {
    if (!cfg || !info || !length || !position) return lio_fail(LIO_ERR_ARG, "null argument");
    if (rows < 0 || cols < 0) return lio_fail(LIO_ERR_ARG, "rows and cols must not be negative");
    LioTerrPlan plan;
    int rc = lio_terrain_check(cfg, resolution, &plan);
    if (rc != LIO_OK) return rc;
    memset(info, 0, sizeof(*info));
    info->normal_method_used = plan.method_used; info->edge_window_size = plan.window;
    info->rows = rows; info->cols = cols;
    if (rows == 0 || cols == 0) return LIO_OK;             // no cell: nothing written
    if (!elevation) return lio_fail(LIO_ERR_ARG, "null argument");
    if ((long long)rows * cols > 0x7fffffffLL - 1024) return lio_fail(LIO_ERR_CAPACITY, "the grid has more than 2^31 cells");
    if ((rc = lio_terrain_set_geometry(&plan, rows, cols, resolution, length, position)) != LIO_OK) return rc;
    const size_t n_cells = (size_t)rows * (size_t)cols;
    if (layers && (size_t)plan.n_out * n_cells > layers_cap) return lio_fail(LIO_ERR_ARG, "layers holds fewer floats than the requested layers (info)");
    if ((rc = lio_check_device(device_id)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    LioTemp grid;
    HIPCHK(grid.alloc(sizeof(float) * n_cells));
    HIPCHK(hipMemcpyAsync(grid.p, elevation, sizeof(float) * n_cells, hipMemcpyHostToDevice, s));
    rc = lio_terrain_device(grid.as<float>(), plan, layers, info, s);
    const hipError_t e = hipStreamSynchronize(s);          // (an early return: `grid` goes back to the pool when this returns)
    if (rc < 0) return rc;
    HIPCHK(e);
    return rc;
} LIO_CATCH

// The height map's chain, then the terrain layers on the device grid it leaves: the planning chain (lio_planning.hip) with the
// terrain layers as its one stage.
extern "C" int lio_kf_store_terrain_map(lio_kf_store* st, const lio_local_map_config* lm, const float* pose, const lio_height_map_config* hm,
                                        const lio_terrain_config* cfg, float* grid, size_t grid_cap, float* layers, size_t layers_cap,
                                        lio_local_map_info* lm_info, lio_height_map_info* hm_info, lio_terrain_info* info)
try {
    if (!st || !lm || !pose || !hm || !cfg || !hm_info || !info) return lio_fail(LIO_ERR_ARG, "null argument");
    return lio_planning_chain(st, lm, pose, hm, { .terrain = cfg, .out = { .grid = grid, .grid_cap = grid_cap, .layers = layers, .layers_cap = layers_cap },
                                                  .lm_info = lm_info, .hm_info = hm_info, .terrain_info = info });
} LIO_CATCH
