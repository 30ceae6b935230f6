// lio_gridtransform.hip -- the resident planning layers moved into another frame (grid_map's GridMap::getTransformedMap) and
// one of them handed out as a nav_msgs/OccupancyGrid's cells (GridMapRosConverter::toOccupancyGrid).  The arithmetic is
// lio_gridtransform.h's; this file is the kernels and the two entry points.
//   k_gt_scatter    one lane per source cell, 256 lanes a block.  The lane reads its height (coalesced: the linear index is
//                   the memory order), skips a non-finite one, and sends its one or five samples through the transform and
//                   the new map's getIndex; each sample inside is one 64-bit integer atomicMax on the new cell's key.
//                   Integer max does not depend on arrival order, so the keys, and with them every layer, repeat bit for
//                   bit; no float atomic is used.  The two counts are summed over the wave and added once per wave.
//   k_gt_gather     one lane per four consecutive new cells.  It reads their four keys as two 16-byte loads, decodes the
//                   winners, forms the winners' heights again, and per layer gathers four source words and writes them as
//                   one 16-byte store (the layers start 256-byte aligned); the cells past the last whole quad are written
//                   one by one.  A cell whose key is 0 gets the quiet NaN in every layer.
// The source layers are read through L2 (a 550 x 400 layer is 0.88 MB); the scatter's atomics are spread over the new
// grid and meet only where many source cells fall into one new cell (a steep pitch), which is where the maximum is needed.
// conventions, the rule's argument, deviations, resources, host waits.  -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <cmath>
#include <string.h>

#include "lio_gridtransform.h"
#include "lio_gridsample.h"
#include "lio_gridobj.h"
#include "lio_cloud.h"
#include "lio_pool.h"

namespace {

struct GtLayers {                  // the layers both objects hold, packed: source and destination of slot k, n of them
    const unsigned* src[LIO_GRID_MAX_LAYERS];
    unsigned* dst[LIO_GRID_MAX_LAYERS];
    int n, height;                 // height: the slot of the height layer
};

enum { GT_CNT_SOURCE = 0, GT_CNT_OUTSIDE, GT_CNT_WRITTEN, GT_N_CNT };

struct GtKeySink {
    unsigned long long* keys;
    __device__ __forceinline__ void put(size_t at, unsigned long long key) { atomicMax(&keys[at], key); }
};

__device__ __forceinline__ unsigned gt_wave_sum(unsigned v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

__global__ __launch_bounds__(256) void k_gt_scatter(LioGridGeom S, LioGridGeom D, LioGtXf T, double sample_length, int n_samples,
                                                    const float* __restrict__ height, int n_cells, unsigned long long* __restrict__ keys,
                                                    unsigned long long* __restrict__ counters)
{
    const int lin = (int)blockIdx.x * 256 + (int)threadIdx.x;
    unsigned finite = 0u, outside = 0u;
    if (lin < n_cells) {
        const float h = height[lin];
        if (lio_gm_finite(h)) {                              // std::isfinite (getPosition3, GM:260-270)
            GtKeySink sink = { keys };
            finite = 1u;
            outside = (unsigned)lio_gt_cell(S, D, T, sample_length, n_samples, lin, h, sink);
        }
    }
    finite = gt_wave_sum(finite);
    outside = gt_wave_sum(outside);
    if ((threadIdx.x & 63) == 0) {
        if (finite) atomicAdd(&counters[GT_CNT_SOURCE], (unsigned long long)finite);
        if (outside) atomicAdd(&counters[GT_CNT_OUTSIDE], (unsigned long long)outside);
    }
}

// the words new cell `key` takes: w[k] for slot k; returns whether the cell received a value
__device__ __forceinline__ bool gt_winner(const LioGridGeom& S, const LioGtXf& T, double sample_length, const GtLayers& L, unsigned long long key,
                                          int* lin, unsigned* height_word)
{
    if (key == 0ull) { *lin = -1; *height_word = 0x7fc00000u; return false; }
    const unsigned visit = lio_gt_key_visit(key);
    *lin = (int)(visit / 5u);
    const float h = __builtin_bit_cast(float, L.src[L.height][*lin]);
    *height_word = __builtin_bit_cast(unsigned, lio_gt_visit_height(S, T, sample_length, visit, h));
    return true;
}

__global__ __launch_bounds__(256) void k_gt_gather(LioGridGeom S, LioGtXf T, double sample_length, GtLayers L, const unsigned long long* __restrict__ keys,
                                                   long long n_new, unsigned long long* __restrict__ counters)
{
    const long long q = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
    const long long first = 4 * q;
    unsigned written = 0u;
    if (first + 4 <= n_new) {
        const ulonglong2 k01 = ((const ulonglong2*)keys)[2 * q], k23 = ((const ulonglong2*)keys)[2 * q + 1];
        const unsigned long long key[4] = { k01.x, k01.y, k23.x, k23.y };
        int lin[4];
        unsigned hw[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) written += gt_winner(S, T, sample_length, L, key[c], &lin[c], &hw[c]) ? 1u : 0u;
        for (int k = 0; k < L.n; ++k) {
            unsigned w[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) w[c] = lin[c] < 0 ? 0x7fc00000u : (k == L.height ? hw[c] : L.src[k][lin[c]]);
            ((uint4*)L.dst[k])[q] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
        for (long long at = first; at < n_new; ++at) {
            int lin;
            unsigned hw;
            written += gt_winner(S, T, sample_length, L, keys[at], &lin, &hw) ? 1u : 0u;
            for (int k = 0; k < L.n; ++k) L.dst[k][at] = lin < 0 ? 0x7fc00000u : (k == L.height ? hw : L.src[k][lin]);
        }
    }
    written = gt_wave_sum(written);
    if ((threadIdx.x & 63) == 0 && written) atomicAdd(&counters[GT_CNT_WRITTEN], (unsigned long long)written);
}

// data[n - 1 - lin] = the cell of linear index lin: lane q writes data[q], so the bytes go out coalesced and the layer is
// read backwards, coalesced as well
__global__ __launch_bounds__(256) void k_gt_occupancy(const float* __restrict__ layer, long long n, float data_min, float data_max, int8_t* __restrict__ data)
{
    const long long q = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
    if (q < n) data[q] = lio_gt_occupancy(layer[n - 1 - q], data_min, data_max);
}

thread_local LioStageTimes<3> t_gt;                        // four marks around the three stages of lio_grid_transform

// No transformed height may be NaN (the rule's premise): with every term of the z row bounded so that the sum of their
// magnitudes stays far below DBL_MAX, no partial sum overflows, and a sum of finite terms that does not overflow is finite.
bool gt_height_row_is_safe(const LioGridGeom& S, const LioGtXf& T, double sample_length)
{
    const double x = (fabs(S.pos[0]) + S.half[0]) + fabs(sample_length), y = (fabs(S.pos[1]) + S.half[1]) + fabs(sample_length);
    const double bound = ((fabs(T.m[8]) * x + fabs(T.m[9]) * y) + fabs(T.m[10]) * (double)FLT_MAX) + fabs(T.m[11]);
    return bound <= 0.25 * DBL_MAX;                           // (false for a NaN or an infinite bound)
}

}  // namespace

extern "C" int lio_grid_transform(lio_grid* src, const double transform[12], int32_t height_layer, double sample_ratio, lio_grid* dst,
                                  lio_grid_transform_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    if (!transform) return lio_fail(LIO_ERR_ARG, "null argument");
    LioGtXf T;
    for (int k = 0; k < 12; ++k) {
        if (!std::isfinite(transform[k])) return lio_fail(LIO_ERR_ARG, "every entry of the transform must be finite");
        T.m[k] = transform[k];
    }
    if (!std::isfinite(sample_ratio)) return lio_fail(LIO_ERR_ARG, "sample_ratio must be finite");
    if (!src || !dst) return lio_fail(LIO_ERR_ARG, "null argument");
    if (src == dst) return lio_fail(LIO_ERR_ARG, "src and dst are the same object");
    if (src->device_id != dst->device_id) return lio_fail(LIO_ERR_ARG, "src and dst live on different devices");
    if (!src->mask) return lio_fail(LIO_ERR_ARG, "src holds no layers (lio_grid_set_layers, lio_kf_store_planning_grid)");
    if (!lio_grid_has_layer(src, height_layer)) return lio_fail(LIO_ERR_ARG, "height_layer names a layer src does not hold");
    const LioGridGeom S = src->G;
    const double sample_length = S.res * sample_ratio;       // GM:344
    if (!gt_height_row_is_safe(S, T, sample_length)) return lio_fail(LIO_ERR_ARG, "the transform's z row could overflow a transformed height");
    // the new geometry, GM:347-382
    double centre[2], new_length[2], length[2];
    int size[2];
    lio_gt_new_extent(S.len, S.pos, T, centre, new_length);
    for (int a = 0; a < 2; ++a) {
        const double n = lio_gm_size(new_length[a], S.res);
        if (!std::isfinite(centre[a]) || !(n >= 1.0) || !std::isfinite(n)) return lio_fail(LIO_ERR_ARG, "the new map has no cell along an axis (or no finite geometry)");
        if (n >= (double)LIO_GS_MAX_LINE) return lio_fail(LIO_ERR_CAPACITY, "the new map has 2^24 or more cells along an axis");
        size[a] = (int)n;
        length[a] = (double)size[a] * S.res;
    }
    const long long n_new = (long long)size[0] * (long long)size[1], n_src = (long long)S.rows * (long long)S.cols;
    if (n_new > 0x7fffffffLL - 1024) return lio_fail(LIO_ERR_CAPACITY, "the new map has more than 2^31 - 1024 cells");
    if (n_src > LIO_GT_MAX_SOURCE_CELLS) return lio_fail(LIO_ERR_CAPACITY, "src has more than LIO_GRID_TRANSFORM_MAX_SOURCE_CELLS cells");
    int rc = lio_check_device(src->device_id);
    if (rc != LIO_OK) return rc;
    if ((rc = lio_grid_set_geometry(dst, size[0], size[1], S.res, length, centre)) != LIO_OK) return rc;
    LioGridRollback undo(dst, true);                         // after a failure dst holds no layer
    GtLayers L;
    memset(&L, 0, sizeof(L));
    for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k) {
        if (!((src->mask >> k) & 1u)) continue;
        float* d = nullptr;
        if ((rc = lio_grid_layer_slot(dst, k, &d)) != LIO_OK) return rc;
        if (k == height_layer) L.height = L.n;
        L.src[L.n] = (const unsigned*)src->d_layer[k].p;
        L.dst[L.n] = (unsigned*)d;
        ++L.n;
    }
    const LioGridGeom D = dst->G;
    hipStream_t s = nullptr;
    LioTemp keys;
    LioGridCounters counters;
    HIPCHK(keys.alloc(sizeof(unsigned long long) * (size_t)n_new));
    HIPCHK(counters.alloc(GT_N_CNT));
    LioStageClock clk(t_gt.on);
    clk.mark(s);
    HIPCHK(hipMemsetAsync(keys.p, 0, sizeof(unsigned long long) * (size_t)n_new, s));
    HIPCHK(counters.clear(s));
    clk.mark(s);
    unsigned long long* d_cnt = counters.d();
    hipLaunchKernelGGL(k_gt_scatter, dim3((unsigned)((n_src + 255) / 256)), dim3(256), 0, s, S, D, T, sample_length, sample_ratio > 0.0 ? 5 : 1,
                       (const float*)src->d_layer[height_layer].p, (int)n_src, keys.as<unsigned long long>(), d_cnt);
    clk.mark(s);
    const long long quads = (n_new + 3) / 4;
    hipLaunchKernelGGL(k_gt_gather, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, S, T, sample_length, L, keys.as<const unsigned long long>(), n_new,
                       d_cnt);
    unsigned long long hc[GT_N_CNT] = { 0, 0, 0 };
    if ((rc = counters.finish(hc, s, &clk)) != LIO_OK) return rc;       // the call's one host wait
    undo.commit();
    if (info) {
        info->rows = size[0]; info->cols = size[1];
        for (int a = 0; a < 2; ++a) { info->length[a] = length[a]; info->position[a] = centre[a]; }
        info->n_source_cells = (int64_t)hc[GT_CNT_SOURCE];
        info->n_samples_outside = (int64_t)hc[GT_CNT_OUTSIDE];
        info->n_cells_written = (int64_t)hc[GT_CNT_WRITTEN];
    }
    t_gt.read(clk);
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_to_occupancy(lio_grid* g, int32_t layer, float data_min, float data_max, int8_t* data, size_t cap_cells,
                                     lio_grid_occupancy_desc* desc)
try {
    if (desc) memset(desc, 0, sizeof(*desc));
    if (!std::isfinite(data_min) || !std::isfinite(data_max)) return lio_fail(LIO_ERR_ARG, "data_min and data_max must be finite");
    if (!g || !data) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!lio_grid_has_layer(g, layer)) return lio_fail(LIO_ERR_ARG, "the object holds no such layer");
    const size_t cells = (size_t)g->G.rows * (size_t)g->G.cols;
    if (cap_cells < cells) return lio_fail(LIO_ERR_ARG, "data holds fewer than rows x cols cells");
    int rc = lio_check_device(g->device_id);
    if (rc != LIO_OK) return rc;
    hipStream_t s = nullptr;
    LioTemp out;
    HIPCHK(out.alloc(cells));
    hipLaunchKernelGGL(k_gt_occupancy, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, (const float*)g->d_layer[layer].p, (long long)cells, data_min,
                       data_max, out.as<int8_t>());
    HIPCHK(hipMemcpyAsync(data, out.p, cells, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));                       // the call's one host wait
    HIPCHK(hipGetLastError());
    if (desc) {
        desc->width = (uint32_t)g->G.rows; desc->height = (uint32_t)g->G.cols;
        desc->resolution = (float)g->G.res;
        for (int a = 0; a < 2; ++a) desc->origin[a] = g->G.pos[a] - 0.5 * g->G.len[a];
    }
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_transform_debug_stage_ms(int32_t enable, float ms[3])
try {
    return t_gt.hook(enable, ms);
} LIO_CATCH
