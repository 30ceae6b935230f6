// lio_gridfilter.hip -- a new layer derived from one the resident object holds: grid_map_filters' MinInRadiusFilter,
// MeanInRadiusFilter, SlidingWindowMathExpressionFilter (four edge modes, seven expressions), CurvatureFilter, ThresholdFilter,
// DuplicationFilter and DeletionFilter.  The arithmetic is lio_gridfilter.h's; this file is the kernels and the entry points.
//   k_gf_radius<op>         one lane per cell, the 32 x 8 tile of lio_gridtile.h with a halo of
//                           floor(radius / resolution + 0.5) + 1 cells staged into LDS by lio_tile_stage: a value is read by
//                           every circle that holds it, once from memory.
//   k_gf_window<op, edge>   the same tile with the half-window as halo.  EDGE_MEAN walks the clipped block first for its
//                           fill, STDDEV walks the window twice; both passes read LDS.  The weights are a device buffer
//                           uploaded by the call; their index is the same in every lane, so they are scalar loads.
//   k_gf_curvature          five direct loads a cell, no LDS: consecutive lanes read consecutive rows of a column, the four
//                           neighbours are the same cache lines one word or one column apart, and there is no barrier.
//   k_gf_threshold          elementwise, in place.
// A cell the filter does not write receives the quiet NaN in the same pass (the reference's mapOut.add(output_layer)), so
// no launch clears the layer first.  Counters: per-wave ballots and one integer atomic per wave and counter (lio_wave_count).
// conventions, deviations, resources, times.  -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <cmath>
#include <string.h>

#include "lio_gridfilter.h"
#include "lio_gridsample.h"
#include "lio_gridobj.h"
#include "lio_cloud.h"
#include "lio_pool.h"
#include "lio_wg.h"

namespace {

enum { GF_CNT_VISITED = 0, GF_CNT_WRITTEN, GF_CNT_CHANGED, GF_N_CNT };

struct GfLayer {                   // a layer as it lies in memory: column-major, rows the contiguous axis
    const float* p;
    int rows;
    __device__ __forceinline__ float at(int i, int j) const { return p[(size_t)i + (size_t)j * (size_t)rows]; }
};

// the cell's word and the two counts every tiled filter keeps; every lane of the wave arrives
__device__ __forceinline__ void gf_finish(const LioGfCell& o, bool in_grid, float* __restrict__ out, int rows, int r, int c,
                                          unsigned long long* __restrict__ counters)
{
    if (in_grid) out[(size_t)r + (size_t)c * (size_t)rows] = o.written ? o.value : LIO_QNAN;
    lio_wave_count(counters, GF_CNT_VISITED, o.visited);
    lio_wave_count(counters, GF_CNT_WRITTEN, o.written);
}

template <int OP>
__global__ __launch_bounds__(LIO_TILE_LANES) void k_gf_radius(LioGfRadius P, const float* __restrict__ in, float* __restrict__ out,
                                                        unsigned long long* __restrict__ counters)
{
    extern __shared__ __attribute__((aligned(16))) float s_tile[];
    int r, c;
    const LioTile T = lio_tile_stage(in, P.G.rows, P.G.cols, P.halo, s_tile, r, c);
    const bool in_grid = r < P.G.rows && c < P.G.cols;
    LioGfCell o;
    o.value = LIO_QNAN;
    o.visited = o.written = false;
    if (in_grid) o = lio_gf_radius_cell<OP>(P, T, r, c);
    gf_finish(o, in_grid, out, P.G.rows, r, c, counters);
}

template <int OP, int EDGE>
__global__ __launch_bounds__(LIO_TILE_LANES) void k_gf_window(LioGfWindow P, const float* __restrict__ in, const float* __restrict__ weights,
                                                        float* __restrict__ out, unsigned long long* __restrict__ counters)
{
    extern __shared__ __attribute__((aligned(16))) float s_tile[];
    int r, c;
    const LioTile T = lio_tile_stage(in, P.rows, P.cols, P.margin, s_tile, r, c);
    const bool in_grid = r < P.rows && c < P.cols;
    LioGfCell o;
    o.value = LIO_QNAN;
    o.visited = o.written = false;
    if (in_grid) o = lio_gf_window_cell<OP, EDGE>(P, T, weights, r, c);
    gf_finish(o, in_grid, out, P.rows, r, c, counters);
}

__global__ __launch_bounds__(256) void k_gf_curvature(const float* __restrict__ in, float* __restrict__ out, int rows, int cols, int n_cells, float L2,
                                                      unsigned long long* __restrict__ counters)
{
    const int lin = (int)blockIdx.x * 256 + (int)threadIdx.x;
    LioGfCell o;
    o.value = LIO_QNAN;
    o.visited = o.written = false;
    if (lin < n_cells) {
        const GfLayer L = { in, rows };
        o = lio_gf_curvature_cell(rows, cols, L2, L, lin % rows, lin / rows);
        out[lin] = o.written ? o.value : LIO_QNAN;
    }
    lio_wave_count(counters, GF_CNT_VISITED, o.visited);
    lio_wave_count(counters, GF_CNT_WRITTEN, o.written);
}

// condition and out may be the same layer: a cell reads its own word before it writes it, and no other
__global__ __launch_bounds__(256) void k_gf_threshold(const float* condition, unsigned* out, int n_cells, int upper, double threshold, unsigned set_to,
                                                      unsigned long long* __restrict__ counters)
{
    const int lin = (int)blockIdx.x * 256 + (int)threadIdx.x;
    bool sets = false;
    if (lin < n_cells) {
        sets = lio_gf_threshold_sets(condition[lin], upper, threshold);
        if (sets) out[lin] = set_to;
    }
    lio_wave_count(counters, GF_CNT_VISITED, lin < n_cells);
    lio_wave_count(counters, GF_CNT_CHANGED, sets);
}

thread_local LioStageTimes<1> t_gf;                        // two marks around the kernel; 0 where none was launched

// One launch between the clock's two marks: the counters cleared before it, then down under the call's one host wait.
template <class Launch>
int gf_run(hipStream_t s, unsigned long long hc[GF_N_CNT], const Launch& launch)
{
    LioGridCounters counters;
    HIPCHK(counters.alloc(GF_N_CNT));
    HIPCHK(counters.clear(s));
    LioStageClock clk(t_gf.on);
    clk.mark(s);
    launch(counters.d());
    clk.mark(s);
    const int rc = counters.finish(hc, s, nullptr);
    if (rc == LIO_OK) t_gf.read(clk);
    return rc;
}

bool gf_id_ok(int32_t id) { return id >= 0 && id < LIO_GRID_MAX_LAYERS; }

// what every filter asks of its object once its own arguments have passed
int gf_object_check(const lio_grid* g, int32_t in_layer)
{
    if (!g) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!g->mask) return lio_fail(LIO_ERR_ARG, "the object holds no layers (lio_grid_set_layers, lio_kf_store_planning_grid)");
    if (!lio_grid_has_layer(g, in_layer)) return lio_fail(LIO_ERR_ARG, "the object holds no such layer");
    return LIO_OK;
}

// Where a filter writes: the slot of out_layer, or (out_layer is the layer read) a block from the pool that takes the layer's
// place once the kernel that filled it has completed; the old block then goes to the pool.
struct GfTarget {
    LioTemp fresh;
    float* d = nullptr;
    int prepare(lio_grid* g, int out_layer, bool aside, size_t cells)
    {
        if (!aside) return lio_grid_layer_slot(g, out_layer, &d);
        HIPCHK(fresh.alloc(sizeof(float) * cells));
        d = fresh.as<float>();
        return LIO_OK;
    }
    void swap_in(lio_grid* g, int k)
    {
        if (!fresh.p) return;
        LioDevBuf<float>& b = g->d_layer[k];
        const size_t cap = lio_pool_disown(fresh.p);
        if (b.p) lio_pool_adopt(b.p, b.cap * sizeof(float), g->device_id);
        b.p = (float*)fresh.p;
        b.cap = cap / sizeof(float);
        fresh.p = nullptr;
    }
};

void gf_fill_info(lio_grid_filter_info* info, const lio_grid* g, int window_size, const unsigned long long hc[GF_N_CNT])
{
    if (!info) return;
    info->rows = g->G.rows; info->cols = g->G.cols;
    info->window_size = window_size;
    info->n_visited = (int64_t)hc[GF_CNT_VISITED];
    info->n_written = (int64_t)hc[GF_CNT_WRITTEN];
    info->n_changed = (int64_t)hc[GF_CNT_CHANGED];
}

typedef void (*GfWindowKernel)(LioGfWindow, const float*, const float*, float*, unsigned long long*);

template <int OP>
GfWindowKernel gf_window_kernel_of(int edge)
{
    switch (edge) {
    case LIO_GW_INSIDE: return k_gf_window<OP, LIO_GW_INSIDE>;
    case LIO_GW_CROP: return k_gf_window<OP, LIO_GW_CROP>;
    case LIO_GW_EMPTY: return k_gf_window<OP, LIO_GW_EMPTY>;
    default: return k_gf_window<OP, LIO_GW_EDGE_MEAN>;
    }
}

GfWindowKernel gf_window_kernel(int op, int edge)
{
    switch (op) {
    case LIO_GW_SUM: return gf_window_kernel_of<LIO_GW_SUM>(edge);
    case LIO_GW_MEAN_OF_FINITES: return gf_window_kernel_of<LIO_GW_MEAN_OF_FINITES>(edge);
    case LIO_GW_MIN_OF_FINITES: return gf_window_kernel_of<LIO_GW_MIN_OF_FINITES>(edge);
    case LIO_GW_MAX_OF_FINITES: return gf_window_kernel_of<LIO_GW_MAX_OF_FINITES>(edge);
    case LIO_GW_NUMBER_OF_FINITES: return gf_window_kernel_of<LIO_GW_NUMBER_OF_FINITES>(edge);
    case LIO_GW_STDDEV: return gf_window_kernel_of<LIO_GW_STDDEV>(edge);
    default: return gf_window_kernel_of<LIO_GW_WEIGHTED_SUM>(edge);
    }
}

const char* const GF_CROP_WEIGHTS = "with LIO_GW_CROP the window and the weights disagree in size at the border";

}  // namespace

extern "C" int lio_grid_filter_radius(lio_grid* g, int32_t in_layer, int32_t out_layer, int32_t op, double radius, lio_grid_filter_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    t_gf.clear();
    if (op != LIO_GF_MIN && op != LIO_GF_MEAN) return lio_fail(LIO_ERR_ARG, "op is LIO_GF_MIN or LIO_GF_MEAN");
    if (!gf_id_ok(in_layer) || !gf_id_ok(out_layer)) return lio_fail(LIO_ERR_ARG, "a layer id is outside 0 .. 15");
    if (in_layer == out_layer) return lio_fail(LIO_ERR_ARG, "out_layer is in_layer: the filter would clear the layer it reads");
    if (!std::isfinite(radius) || radius < 0.0) return lio_fail(LIO_ERR_ARG, "radius must be finite and not negative");
    int rc = gf_object_check(g, in_layer);
    if (rc != LIO_OK) return rc;
    LioGfRadius P;
    if (const char* why = lio_gf_radius_plan(g->G, radius, &P)) return lio_fail(LIO_ERR_ARG, why);
    if ((rc = lio_check_device(g->device_id)) != LIO_OK) return rc;
    LioGridRollback undo(g, false);                          // after a failure g holds the layers it held
    GfTarget out;
    if ((rc = out.prepare(g, out_layer, false, 0)) != LIO_OK) return rc;
    const float* d_in = g->d_layer[in_layer].p;
    hipStream_t s = nullptr;
    unsigned long long hc[GF_N_CNT];
    rc = gf_run(s, hc, [&](unsigned long long* d_cnt) {
        const dim3 grid(lio_tile_count(P.G.rows, P.G.cols)), block(LIO_TILE_LANES);
        if (op == LIO_GF_MIN) hipLaunchKernelGGL(k_gf_radius<LIO_GF_MIN>, grid, block, lio_tile_lds_bytes(P.halo, sizeof(float)), s, P, d_in, out.d, d_cnt);
        else hipLaunchKernelGGL(k_gf_radius<LIO_GF_MEAN>, grid, block, lio_tile_lds_bytes(P.halo, sizeof(float)), s, P, d_in, out.d, d_cnt);
    });
    if (rc != LIO_OK) return rc;
    undo.commit();
    gf_fill_info(info, g, 0, hc);
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_filter_window(lio_grid* g, int32_t in_layer, int32_t out_layer, int32_t op, int32_t edge_handling, int32_t window_size,
                                      double window_length, const float* weights, lio_grid_filter_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    t_gf.clear();
    if (op < 0 || op >= LIO_GW_N_OPS) return lio_fail(LIO_ERR_ARG, "op is LIO_GW_SUM .. LIO_GW_WEIGHTED_SUM");
    if (edge_handling < 0 || edge_handling >= LIO_GW_N_EDGES) return lio_fail(LIO_ERR_ARG, "edge_handling is LIO_GW_INSIDE .. LIO_GW_EDGE_MEAN");
    if (!gf_id_ok(in_layer) || !gf_id_ok(out_layer)) return lio_fail(LIO_ERR_ARG, "a layer id is outside 0 .. 15");
    if (window_size < 0 || (window_size != 0 && window_size % 2 == 0)) return lio_fail(LIO_ERR_ARG, "window_size must be odd (0: from window_length)");
    if (window_size > LIO_GW_MAX_SIZE) return lio_fail(LIO_ERR_ARG, "the window reaches further than 32 cells");
    if (!std::isfinite(window_length) || window_length < 0.0) return lio_fail(LIO_ERR_ARG, "window_length must be finite and not negative");
    if (op == LIO_GW_WEIGHTED_SUM && !weights) return lio_fail(LIO_ERR_ARG, "LIO_GW_WEIGHTED_SUM needs weights: null argument");
    if (op != LIO_GW_WEIGHTED_SUM && weights) return lio_fail(LIO_ERR_ARG, "weights given to an op that reads none");
    if (op == LIO_GW_WEIGHTED_SUM && edge_handling == LIO_GW_CROP && window_size > 1) return lio_fail(LIO_ERR_ARG, GF_CROP_WEIGHTS);
    int rc = gf_object_check(g, in_layer);
    if (rc != LIO_OK) return rc;
    LioGfWindow P;
    if (const char* why = lio_gf_window_plan(g->G.rows, g->G.cols, g->G.res, edge_handling, window_size, window_length, &P)) return lio_fail(LIO_ERR_ARG, why);
    if (op == LIO_GW_WEIGHTED_SUM && edge_handling == LIO_GW_CROP && P.size > 1) return lio_fail(LIO_ERR_ARG, GF_CROP_WEIGHTS);
    if ((rc = lio_check_device(g->device_id)) != LIO_OK) return rc;
    const size_t cells = (size_t)P.rows * (size_t)P.cols;
    LioGridRollback undo(g, false);
    GfTarget out;                                            // the reference iterates over mapIn: out_layer == in_layer reads the old values
    if ((rc = out.prepare(g, out_layer, out_layer == in_layer, cells)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    LioTemp d_weights;
    if (weights) {
        const size_t bytes = sizeof(float) * (size_t)P.size * (size_t)P.size;
        HIPCHK(d_weights.alloc(bytes));
        HIPCHK(hipMemcpyAsync(d_weights.p, weights, bytes, hipMemcpyHostToDevice, s));
    }
    const float* d_in = g->d_layer[in_layer].p;
    unsigned long long hc[GF_N_CNT];
    rc = gf_run(s, hc, [&](unsigned long long* d_cnt) {
        hipLaunchKernelGGL(gf_window_kernel(op, edge_handling), dim3(lio_tile_count(P.rows, P.cols)), dim3(LIO_TILE_LANES), lio_tile_lds_bytes(P.margin, sizeof(float)), s, P, d_in,
                           (const float*)d_weights.as<float>(), out.d, d_cnt);
    });
    if (rc != LIO_OK) return rc;
    out.swap_in(g, out_layer);
    undo.commit();
    gf_fill_info(info, g, P.size, hc);
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_filter_curvature(lio_grid* g, int32_t in_layer, int32_t out_layer, lio_grid_filter_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    t_gf.clear();
    if (!gf_id_ok(in_layer) || !gf_id_ok(out_layer)) return lio_fail(LIO_ERR_ARG, "a layer id is outside 0 .. 15");
    if (in_layer == out_layer) return lio_fail(LIO_ERR_ARG, "out_layer is in_layer: the filter would clear the layer it reads");
    int rc = gf_object_check(g, in_layer);
    if (rc != LIO_OK) return rc;
    if ((rc = lio_check_device(g->device_id)) != LIO_OK) return rc;
    const int rows = g->G.rows, cols = g->G.cols;
    const size_t cells = (size_t)rows * (size_t)cols;
    const float L2 = (float)(g->G.res * g->G.res);           // const float L2 = getResolution() * getResolution()
    LioGridRollback undo(g, false);
    GfTarget out;
    if ((rc = out.prepare(g, out_layer, false, 0)) != LIO_OK) return rc;
    const float* d_in = g->d_layer[in_layer].p;
    hipStream_t s = nullptr;
    unsigned long long hc[GF_N_CNT];
    rc = gf_run(s, hc, [&](unsigned long long* d_cnt) {
        hipLaunchKernelGGL(k_gf_curvature, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, d_in, out.d, rows, cols, (int)cells, L2, d_cnt);
    });
    if (rc != LIO_OK) return rc;
    undo.commit();
    gf_fill_info(info, g, 0, hc);
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_filter_threshold(lio_grid* g, int32_t condition_layer, int32_t out_layer, int32_t upper, double threshold, double set_to,
                                         lio_grid_filter_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    t_gf.clear();
    if (upper != 0 && upper != 1) return lio_fail(LIO_ERR_ARG, "upper is 0 or 1");
    if (!gf_id_ok(condition_layer) || !gf_id_ok(out_layer)) return lio_fail(LIO_ERR_ARG, "a layer id is outside 0 .. 15");
    int rc = gf_object_check(g, condition_layer);
    if (rc != LIO_OK) return rc;
    if (!lio_grid_has_layer(g, out_layer)) return lio_fail(LIO_ERR_ARG, "the object holds no such layer to set (out_layer)");
    if ((rc = lio_check_device(g->device_id)) != LIO_OK) return rc;
    const size_t cells = (size_t)g->G.rows * (size_t)g->G.cols;
    const unsigned word = __builtin_bit_cast(unsigned, (float)set_to);
    const float* d_cond = g->d_layer[condition_layer].p;
    unsigned* d_out = (unsigned*)g->d_layer[out_layer].p;
    hipStream_t s = nullptr;
    unsigned long long hc[GF_N_CNT];
    rc = gf_run(s, hc, [&](unsigned long long* d_cnt) {
        hipLaunchKernelGGL(k_gf_threshold, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, d_cond, d_out, (int)cells, (int)upper, threshold, word, d_cnt);
    });
    if (rc != LIO_OK) return rc;
    hc[GF_CNT_WRITTEN] = hc[GF_CNT_CHANGED];
    gf_fill_info(info, g, 0, hc);
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_duplicate_layer(lio_grid* g, int32_t in_layer, int32_t out_layer)
try {
    t_gf.clear();
    if (!gf_id_ok(in_layer) || !gf_id_ok(out_layer)) return lio_fail(LIO_ERR_ARG, "a layer id is outside 0 .. 15");
    int rc = gf_object_check(g, in_layer);
    if (rc != LIO_OK) return rc;
    if (in_layer == out_layer) return LIO_OK;                // mapOut.add(layer, mapIn[layer]): the layer as it is
    if ((rc = lio_check_device(g->device_id)) != LIO_OK) return rc;
    const size_t cells = (size_t)g->G.rows * (size_t)g->G.cols;
    LioGridRollback undo(g, false);
    float* d = nullptr;
    if ((rc = lio_grid_layer_slot(g, out_layer, &d)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    HIPCHK(hipMemcpyAsync(d, g->d_layer[in_layer].p, sizeof(float) * cells, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    undo.commit();
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_delete_layers(lio_grid* g, const int32_t* layer_ids, int32_t n_layers)
try {
    t_gf.clear();
    if (n_layers < 1 || n_layers > LIO_GRID_MAX_LAYERS) return lio_fail(LIO_ERR_ARG, "n_layers must be in [1, LIO_GRID_MAX_LAYERS]");
    if (!layer_ids) return lio_fail(LIO_ERR_ARG, "null argument");
    unsigned listed = 0;
    int rc = lio_grid_layer_list(layer_ids, n_layers, &listed);
    if (rc != LIO_OK) return rc;
    if (!g) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!g->mask) return lio_fail(LIO_ERR_ARG, "the object holds no layers (lio_grid_set_layers, lio_kf_store_planning_grid)");
    if (listed & ~g->mask) return lio_fail(LIO_ERR_ARG, "a layer id names a layer the object does not hold");
    if (g->mask == listed) lio_grid_clear(g);                // no layer left: the object is as lio_grid_create left it (its memory stays)
    else g->mask &= ~listed;
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_filter_debug_kernel_ms(int32_t enable, float* ms)
try {
    return t_gf.hook(enable, ms);
} LIO_CATCH
