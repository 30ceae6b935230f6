// lio_gridsample.hip -- the planning layers resident on the device and grid_map's GridMap::atPosition on them: the query a
// planner makes of the elevation grid and the terrain layers, once per trajectory point and footprint corner.  The arithmetic
// is lio_gridsample.h's; this file is the object, the guards its entry points share (lio_gridobj.h) and the data movement.
//   k_grid_sample   one lane per position, 256 lanes a block, one instance per interpolation method.  The lane reads its
//                   position as one 16-byte load and forms the geometry once in fp64 (cell, quadrant, tap indices, normalised
//                   coordinates), then loops over the requested layers: gathers the taps, evaluates, runs the fall-back chain.
//                   Finiteness differs from layer to layer; geometry does not.  Values and method bytes of a layer are
//                   written coalesced (lane q to [layer][q]).  Taps are plain global loads: a 550 x 400 layer is 0.88 MB and
//                   stays in L2, so there is no LDS staging and the queries are not sorted by cell.  The counts are per-wave
//                   ballots summed over the layers in lane 0 and one atomic per wave and count, as in k_terr_main.
// conventions, deviations, resources, host waits.  -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <cmath>
#include <string.h>
#include <vector>

#include "lio_gridsample.h"
#include "lio_gridobj.h"
#include "lio_cloud.h"
#include "lio_pool.h"


namespace {

struct GsLayer {                   // a layer on the device
    const float* p;
    int rows;
    __device__ __forceinline__ float at(int r, int c) const { return p[(size_t)r + (size_t)c * (size_t)rows]; }
    __device__ __forceinline__ float at_lin(int k) const { return p[k]; }
};

struct GsLayers { const float* p[LIO_GRID_MAX_LAYERS]; };          // the requested layers, in the caller's order

// counters[0..3] += pairs per method used, counters[4] += pairs outside
template <int METHOD>
__global__ __launch_bounds__(256) void k_grid_sample(LioGridGeom G, GsLayers L, int n_layers, int border, const double2* __restrict__ pos, int n,
                                                     float* __restrict__ values, unsigned char* __restrict__ method_used,
                                                     unsigned long long* __restrict__ counters)
{
    const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const bool live = q < n;
    LioGsQuery Q;
    Q.outside = true;
    if (live) {
        const double2 p = pos[q];
        lio_gs_query(G, METHOD, border, p.x, p.y, &Q);
    }
    unsigned cnt[5] = { 0u, 0u, 0u, 0u, 0u };              // (lane 0's are the wave's)
    for (int k = 0; k < n_layers; ++k) {
        int used = -1;
        if (live) {
            const GsLayer in = { L.p[k], G.rows };
            float v;
            used = lio_gs_eval(G, Q, METHOD, in, &v);
            const size_t at = (size_t)k * (size_t)n + (size_t)q;
            values[at] = v;
            if (method_used) method_used[at] = (unsigned char)used;
        }
        cnt[0] += (unsigned)__popcll(__ballot(used == LIO_GRID_NEAREST));
        if (METHOD >= LIO_GRID_LINEAR) cnt[1] += (unsigned)__popcll(__ballot(used == LIO_GRID_LINEAR));
        if (METHOD == LIO_GRID_CUBIC_CONVOLUTION) cnt[2] += (unsigned)__popcll(__ballot(used == LIO_GRID_CUBIC_CONVOLUTION));
        if (METHOD == LIO_GRID_CUBIC) cnt[3] += (unsigned)__popcll(__ballot(used == LIO_GRID_CUBIC));
        cnt[4] += (unsigned)__popcll(__ballot(used == LIO_GRID_OUTSIDE));
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int m = 0; m < 5; ++m)
            if (cnt[m]) atomicAdd(&counters[m], (unsigned long long)cnt[m]);
    }
}

thread_local LioStageTimes<3> t_stage;                     // four marks around the three stages of lio_grid_sample

}  // namespace

int lio_grid_geometry_check(int rows, int cols, double resolution, const double* length, const double* position)
{
    if (rows < 1 || cols < 1) return lio_fail(LIO_ERR_ARG, "rows and cols must be at least 1");
    if (rows >= LIO_GS_MAX_LINE || cols >= LIO_GS_MAX_LINE) return lio_fail(LIO_ERR_ARG, "rows and cols must be below 2^24");
    if (const char* why = lio_gm_resolution_refusal(resolution)) return lio_fail(LIO_ERR_ARG, why);
    if (const char* why = lio_gm_axes_refusal(rows, cols, resolution, length, position)) return lio_fail(LIO_ERR_ARG, why);
    if ((long long)rows * cols > 0x7fffffffLL - 1024) return lio_fail(LIO_ERR_CAPACITY, "a layer has more than 2^31 - 1024 cells");
    return LIO_OK;
}

void lio_grid_clear(lio_grid* g)
{
    g->mask = 0;
    g->G.rows = g->G.cols = 0;
}

bool lio_grid_has_layer(const lio_grid* g, int layer) { return layer >= 0 && layer < LIO_GRID_MAX_LAYERS && ((g->mask >> layer) & 1u); }

int lio_grid_layer_list(const int32_t* ids, int n, unsigned* listed)
{
    *listed = 0;
    for (int k = 0; k < n; ++k) {
        const int id = ids[k];
        if (id < 0 || id >= LIO_GRID_MAX_LAYERS) return lio_fail(LIO_ERR_ARG, "a layer id is outside 0 .. 15");
        if ((*listed >> id) & 1u) return lio_fail(LIO_ERR_ARG, "a layer id is repeated");
        *listed |= 1u << id;
    }
    return LIO_OK;
}

int LioGridCounters::finish(unsigned long long* host, hipStream_t s, LioStageClock* clk)
{
    HIPCHK(hipMemcpyAsync(host, t.p, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if (clk) clk->mark(s);
    HIPCHK(hipStreamSynchronize(s));                       // (the temporaries go back to the pool after it)
    HIPCHK(hipGetLastError());
    return LIO_OK;
}

int lio_grid_begin(lio_grid* g, int device_id)
{
    if (device_id != g->device_id) return lio_fail(LIO_ERR_ARG, "the keyframe store and the grid live on different devices");
    lio_grid_clear(g);
    return LIO_OK;
}

int lio_grid_set_geometry(lio_grid* g, int rows, int cols, double resolution, const double length[2], const double position[2])
{
    lio_grid_clear(g);
    const int rc = lio_grid_geometry_check(rows, cols, resolution, length, position);
    if (rc != LIO_OK) return rc;
    g->G = lio_gm_geom(rows, cols, resolution, position[0], position[1]);
    return LIO_OK;
}

int lio_grid_layer_slot(lio_grid* g, int layer, float** d_out)
{
    *d_out = nullptr;
    if (layer < 0 || layer >= LIO_GRID_MAX_LAYERS || g->G.rows < 1 || g->G.cols < 1) return lio_fail(LIO_ERR_ARG, "no such layer slot");
    HIPCHK(g->d_layer[layer].grow((size_t)g->G.rows * (size_t)g->G.cols, 1.0, 64, true));
    g->mask |= 1u << layer;
    *d_out = g->d_layer[layer].p;
    return LIO_OK;
}

extern "C" void lio_grid_sample_default_config(lio_grid_sample_config* cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->method = LIO_GRID_NEAREST;                        // atPosition's default argument
    cfg->border_mode = 0;
}

extern "C" int lio_grid_create(int32_t device_id, lio_grid** out)
try {
    if (!out) return lio_fail(LIO_ERR_ARG, "null argument");
    int rc = lio_check_device(device_id);
    if (rc != LIO_OK) return rc;
    lio_grid* g = new lio_grid();
    g->device_id = device_id;
    *out = g;
    return LIO_OK;
} LIO_CATCH

extern "C" void lio_grid_destroy(lio_grid* g)
{
    if (!g) return;
    (void)hipSetDevice(g->device_id);
    (void)hipDeviceSynchronize();
    delete g;
}

extern "C" int lio_grid_set_layers(lio_grid* g, const float* layers, int32_t n_layers, int32_t rows, int32_t cols, double resolution,
                                   const double* length, const double* position)
try {
    if (!length || !position) return lio_fail(LIO_ERR_ARG, "null argument");
    if (n_layers < 1 || n_layers > LIO_GRID_MAX_LAYERS) return lio_fail(LIO_ERR_ARG, "n_layers must be in [1, LIO_GRID_MAX_LAYERS]");
    int rc = lio_grid_geometry_check(rows, cols, resolution, length, position);
    if (rc != LIO_OK) return rc;
    if (!g || !layers) return lio_fail(LIO_ERR_ARG, "null argument");
    if ((rc = lio_check_device(g->device_id)) != LIO_OK) return rc;
    if ((rc = lio_grid_set_geometry(g, rows, cols, resolution, length, position)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    const size_t cells = (size_t)rows * (size_t)cols;
    LioGridRollback undo(g, false);                        // after a failure the geometry holds no layer
    for (int k = 0; k < n_layers; ++k) {
        float* d = nullptr;
        if ((rc = lio_grid_layer_slot(g, k, &d)) != LIO_OK) return rc;
        const hipError_t e = hipMemcpyAsync(d, layers + (size_t)k * cells, sizeof(float) * cells, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) { (void)hipStreamSynchronize(s); HIPCHK(e); }
    }
    HIPCHK(hipStreamSynchronize(s));
    undo.commit();
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_get_layer(lio_grid* g, int32_t layer, float* out, size_t cap_floats)
try {
    if (!g || !out) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!lio_grid_has_layer(g, layer)) return lio_fail(LIO_ERR_ARG, "the object holds no such layer");
    const size_t cells = (size_t)g->G.rows * (size_t)g->G.cols;
    if (cap_floats < cells) return lio_fail(LIO_ERR_ARG, "out holds fewer than rows x cols floats");
    int rc = lio_check_device(g->device_id);
    if (rc != LIO_OK) return rc;
    HIPCHK(hipMemcpy(out, g->d_layer[layer].p, sizeof(float) * cells, hipMemcpyDeviceToHost));
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_info(lio_grid* g, lio_grid_desc* info)
try {
    if (!g || !info) return lio_fail(LIO_ERR_ARG, "null argument");
    memset(info, 0, sizeof(*info));
    info->layer_mask = g->mask;
    if (!g->mask) return LIO_OK;
    info->rows = g->G.rows; info->cols = g->G.cols; info->resolution = g->G.res;
    for (int a = 0; a < 2; ++a) { info->length[a] = g->G.len[a]; info->position[a] = g->G.pos[a]; }
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_memory(lio_grid* g, size_t* bytes)
try {
    if (!g || !bytes) return lio_fail(LIO_ERR_ARG, "null argument");
    size_t n = 0;
    for (const LioDevBuf<float>& b : g->d_layer) n += b.cap * sizeof(float);
    for (const LioDevBytes& b : g->d_region) n += b.cap;
    *bytes = n;
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_sample(lio_grid* g, const int32_t* layer_ids, int32_t n_layers, const lio_grid_sample_config* cfg, const double* positions,
                               size_t n, float* values, uint8_t* method_used, lio_grid_sample_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    if (!layer_ids || !cfg || (n && (!positions || !values))) return lio_fail(LIO_ERR_ARG, "null argument");
    if (cfg->method < LIO_GRID_NEAREST || cfg->method > LIO_GRID_CUBIC) return lio_fail(LIO_ERR_ARG, "method is 0 (nearest), 1 (linear), 2 (cubic convolution) or 3 (cubic)");
    if (cfg->border_mode != 0 && cfg->border_mode != 1) return lio_fail(LIO_ERR_ARG, "border_mode is 0 (as written) or 1 (clamped)");
    if (n_layers < 1 || n_layers > LIO_GRID_MAX_LAYERS) return lio_fail(LIO_ERR_ARG, "n_layers must be in [1, LIO_GRID_MAX_LAYERS]");
    if (!g) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!g->mask) return lio_fail(LIO_ERR_ARG, "the object holds no layers (lio_grid_set_layers, lio_kf_store_planning_grid)");
    unsigned listed = 0;
    int rc = lio_grid_layer_list(layer_ids, n_layers, &listed);
    if (rc != LIO_OK) return rc;
    if (listed & ~g->mask) return lio_fail(LIO_ERR_ARG, "a layer id names a layer the object does not hold");
    GsLayers L;
    memset(&L, 0, sizeof(L));
    for (int k = 0; k < n_layers; ++k) L.p[k] = g->d_layer[layer_ids[k]].p;
    if (n > (size_t)1 << 27) return lio_fail(LIO_ERR_CAPACITY, "more than 2^27 positions in one call");
    if (n == 0) return LIO_OK;
    if ((rc = lio_check_device(g->device_id)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    const size_t pairs = (size_t)n_layers * n;
    LioTemp pos, val, used;
    LioGridCounters counters;
    HIPCHK(pos.alloc(sizeof(double) * 2 * n));
    HIPCHK(val.alloc(sizeof(float) * pairs));
    if (method_used) HIPCHK(used.alloc(pairs));
    HIPCHK(counters.alloc(5));
    LioStageClock clk(t_stage.on);
    clk.mark(s);
    HIPCHK(hipMemcpyAsync(pos.p, positions, sizeof(double) * 2 * n, hipMemcpyHostToDevice, s));
    HIPCHK(counters.clear(s));
    clk.mark(s);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    const double2* d_pos = (const double2*)pos.p;
    unsigned char* d_used = method_used ? used.as<unsigned char>() : nullptr;
    unsigned long long* d_cnt = counters.d();
    switch (cfg->method) {
    case LIO_GRID_NEAREST:
        hipLaunchKernelGGL(k_grid_sample<LIO_GRID_NEAREST>, grid, block, 0, s, g->G, L, n_layers, cfg->border_mode, d_pos, (int)n, val.as<float>(), d_used, d_cnt);
        break;
    case LIO_GRID_LINEAR:
        hipLaunchKernelGGL(k_grid_sample<LIO_GRID_LINEAR>, grid, block, 0, s, g->G, L, n_layers, cfg->border_mode, d_pos, (int)n, val.as<float>(), d_used, d_cnt);
        break;
    case LIO_GRID_CUBIC_CONVOLUTION:
        hipLaunchKernelGGL(k_grid_sample<LIO_GRID_CUBIC_CONVOLUTION>, grid, block, 0, s, g->G, L, n_layers, cfg->border_mode, d_pos, (int)n, val.as<float>(), d_used,
                           d_cnt);
        break;
    default:
        hipLaunchKernelGGL(k_grid_sample<LIO_GRID_CUBIC>, grid, block, 0, s, g->G, L, n_layers, cfg->border_mode, d_pos, (int)n, val.as<float>(), d_used, d_cnt);
        break;
    }
    clk.mark(s);
    unsigned long long hc[5] = { 0, 0, 0, 0, 0 };
    HIPCHK(hipMemcpyAsync(values, val.p, sizeof(float) * pairs, hipMemcpyDeviceToHost, s));
    if (method_used) HIPCHK(hipMemcpyAsync(method_used, used.p, pairs, hipMemcpyDeviceToHost, s));
    if ((rc = counters.finish(hc, s, &clk)) != LIO_OK) return rc;       // the call's one host wait
    if (info) {
        for (int m = 0; m < 4; ++m) info->n_method[m] = (int64_t)hc[m];
        info->n_outside = (int64_t)hc[4];
    }
    t_stage.read(clk);
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_debug_stage_ms(int32_t enable, float ms[3])
try {
    return t_stage.hook(enable, ms);
} LIO_CATCH
