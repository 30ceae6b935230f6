// lio_gridgeom.hip -- the resident planning layers cropped (grid_map's GridMap::getSubmap), re-centred (move), grown
// (extendToInclude) and merged (addDataFrom).  The arithmetic is lio_gridgeom.h's; this file is the two kernels and the
// entry points.
//   k_gg_offset     the integer-offset form (submap, move): one lane per destination cell, 256 lanes a block, the linear
//                   index walking rows first (the contiguous axis of the column-major layers), so a wave's loads and stores
//                   are 64 consecutive words of a column, shifted by the row offset.
//   k_gg_position   the fp64 position form (extend, add): one lane per cell of the new geometry.  The cell's centre, then
//                   isInside / getIndex on the old geometry (a resize) and on `other` (an addition), each once per cell; then
//                   the loop over the table of layer pointers.  With extend and a resize the old-self gather, the validity
//                   test on the gathered values and the gather from `other` are this one launch; without a resize the map is
//                   worked on in place and only the words that change are written.
// The table (up to 16 self, 16 destination and 16 other pointers) is a kernel argument by value; the loop index is uniform, so
// the pointers are scalar loads.  Counters: per-wave ballots and one integer atomic per wave and counter (lio_wave_count,
// lio_wg.h).  A resized or moved layer is written into a block from the pool that then takes the layer's place; the old block
// goes to the pool.
// conventions, deviations, resources, times.  -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <cmath>
#include <string.h>

#include "lio_gridgeom.h"
#include "lio_gridsample.h"
#include "lio_gridobj.h"
#include "lio_cloud.h"
#include "lio_pool.h"
#include "lio_wg.h"

namespace {

enum { GG_CNT_CLEARED = 0, GG_CNT_KEPT, GG_CNT_SKIPPED, GG_CNT_OUTSIDE, GG_CNT_INDEX, GG_CNT_COPIED, GG_N_CNT };

__global__ __launch_bounds__(256) void k_gg_offset(LioGgTable T, int d_rows, int n_cells, int s_rows, int s_cols, int off0, int off1,
                                                   unsigned long long* __restrict__ counters)
{
    const int lin = (int)blockIdx.x * 256 + (int)threadIdx.x;
    bool cleared = false;
    if (lin < n_cells) cleared = lio_gg_offset_cell(T, d_rows, s_rows, s_cols, off0, off1, lin % d_rows, lin / d_rows);
    lio_wave_count(counters, GG_CNT_CLEARED, cleared);
}

__global__ __launch_bounds__(256) void k_gg_position(LioGgTable T, LioGridGeom N, LioGridGeom O, LioGridGeom X, int flags, int n_cells,
                                                     unsigned long long* __restrict__ counters)
{
    const int lin = (int)blockIdx.x * 256 + (int)threadIdx.x;
    LioGgCellCount n;
    n.kept = n.skipped_valid = n.outside_other = n.index_outside_self = n.index_outside_other = false;
    n.copied = 0;
    if (lin < n_cells) lio_gg_position_cell(T, N, O, X, flags, lin % N.rows, lin / N.rows, &n);
    lio_wave_count(counters, GG_CNT_KEPT, n.kept);
    lio_wave_count(counters, GG_CNT_SKIPPED, n.skipped_valid);
    lio_wave_count(counters, GG_CNT_OUTSIDE, n.outside_other);
    lio_wave_count(counters, GG_CNT_INDEX, n.index_outside_self);
    lio_wave_count(counters, GG_CNT_INDEX, n.index_outside_other);
    unsigned long long copied = 0;                           // a lane copies 0 .. 16 values: five ballots, one per bit
#pragma unroll
    for (int b = 0; b < 5; ++b) copied += (unsigned long long)__popcll(__ballot((n.copied >> b) & 1)) << b;
    if ((threadIdx.x & 63) == 0 && copied) atomicAdd(&counters[GG_CNT_COPIED], copied);
}

thread_local LioStageTimes<1> t_gg;                        // two marks around the kernel; 0 where none was launched

// Blocks from the pool that take the place of layers once the kernel that filled them has completed.
struct GgFresh {
    LioTemp t[LIO_GRID_MAX_LAYERS];
    hipError_t alloc(int k, size_t cells) { return t[k].alloc(sizeof(float) * cells); }
    unsigned* words(int k) { return t[k].as<unsigned>(); }
    // layer k of g takes its block; the layer's old block, which nothing reads any more, goes to the pool
    void swap_in(lio_grid* g, int k)
    {
        LioDevBuf<float>& b = g->d_layer[k];
        const size_t cap = lio_pool_disown(t[k].p);
        if (b.p) lio_pool_adopt(b.p, b.cap * sizeof(float), g->device_id);
        b.p = (float*)t[k].p;
        b.cap = cap / sizeof(float);
        t[k].p = nullptr;
    }
};

// what two objects of one call must satisfy before anything else is read; b_is_source: b is read as well (a always is)
int gg_pair_check(const lio_grid* a, const lio_grid* b, const char* same, bool b_is_source)
{
    if (!a || !b) return lio_fail(LIO_ERR_ARG, "null argument");
    if (a == b) return lio_fail(LIO_ERR_ARG, same);
    if (a->device_id != b->device_id) return lio_fail(LIO_ERR_ARG, "the two grids live on different devices");
    if (!a->mask || (b_is_source && !b->mask)) return lio_fail(LIO_ERR_ARG, "a source holds no layers (lio_grid_set_layers, lio_kf_store_planning_grid)");
    return LIO_OK;
}

// One launch between the clock's two marks: the counters cleared before it, then down under the call's one host wait.
template <class Launch>
int gg_run(hipStream_t s, unsigned long long hc[GG_N_CNT], const Launch& launch)
{
    LioGridCounters counters;
    HIPCHK(counters.alloc(GG_N_CNT));
    HIPCHK(counters.clear(s));
    LioStageClock clk(t_gg.on);
    clk.mark(s);
    launch(counters.d());
    clk.mark(s);
    const int rc = counters.finish(hc, s, nullptr);
    if (rc == LIO_OK) t_gg.read(clk);
    return rc;
}

struct GgAddResult {
    int resized;
    unsigned long long cnt[GG_N_CNT];
};

// extendToInclude (add = false) and addDataFrom (add = true) behind one launch.  listed: the ids to copy from `other`.
int gg_extend_add(lio_grid* g, lio_grid* other, bool extend, bool add, bool overwrite, unsigned listed, unsigned basic_mask, GgAddResult* out)
{
    memset(out, 0, sizeof(*out));
    t_gg.clear();
    const LioGridGeom O = g->G, X = other->G;
    LioGridGeom N = O;
    bool resized = false;
    if (extend) {
        double position[2], length[2];
        int size[2];
        for (int a = 0; a < 2; ++a) {
            position[a] = O.pos[a]; length[a] = O.len[a];
            if (lio_gg_extend_axis(X.pos[a], X.len[a], &position[a], &length[a])) resized = true;
        }
        if (resized) {
            for (int a = 0; a < 2; ++a) {
                const double n = lio_gm_size(length[a], O.res);                // setGeometry, GM:50
                if (!std::isfinite(position[a]) || !std::isfinite(n) || !(n >= 1.0)) return lio_fail(LIO_ERR_ARG, "the extended map has no finite geometry");
                if (n >= (double)LIO_GS_MAX_LINE) return lio_fail(LIO_ERR_CAPACITY, "the extended map has 2^24 or more cells along an axis");
                size[a] = (int)n;
            }
            if ((long long)size[0] * (long long)size[1] > 0x7fffffffLL - 1024) return lio_fail(LIO_ERR_CAPACITY, "the extended map has more than 2^31 - 1024 cells");
            for (int a = 0; a < 2; ++a) {
                position[a] = lio_gg_align_axis(position[a], O.pos[a], O.res, size[a], a == 0 ? O.rows : O.cols);
                if (!std::isfinite(position[a])) return lio_fail(LIO_ERR_ARG, "the extended map has no finite geometry");
            }
            N = lio_gm_geom(size[0], size[1], O.res, position[0], position[1]);
        }
    }
    out->resized = resized ? 1 : 0;
    if (!resized && !add) return LIO_OK;                     // nothing to extend: nothing touched
    int rc = lio_check_device(g->device_id);
    if (rc != LIO_OK) return rc;
    const unsigned old_mask = g->mask, final_mask = old_mask | (add ? listed : 0u);
    // in place, only the layers that are read (basic) or may be written (listed, new among them) enter the table
    const unsigned in_table = resized ? final_mask : ((listed | basic_mask) & final_mask);
    const size_t cells = (size_t)N.rows * (size_t)N.cols;
    LioGridRollback undo(g, false);                          // after a failure g holds the layers it held
    GgFresh fresh;
    LioGgTable T;
    memset(&T, 0, sizeof(T));
    for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k) {
        if (!((in_table >> k) & 1u)) continue;
        const bool held = (old_mask >> k) & 1u;
        if (resized) {
            HIPCHK(fresh.alloc(k, cells));
            T.dst[T.n] = fresh.words(k);
        } else {
            float* d = g->d_layer[k].p;
            if (!held && (rc = lio_grid_layer_slot(g, k, &d)) != LIO_OK) return rc;
            T.dst[T.n] = (unsigned*)d;
        }
        T.self[T.n] = held ? (const unsigned*)g->d_layer[k].p : nullptr;
        T.other[T.n] = (add && ((listed >> k) & 1u)) ? (const unsigned*)other->d_layer[k].p : nullptr;
        if ((basic_mask >> k) & 1u) T.basic |= 1u << T.n;
        ++T.n;
    }
    hipStream_t s = nullptr;
    const int flags = (resized ? LIO_GG_RESIZE : 0) | (add ? LIO_GG_ADD : 0) | (overwrite ? LIO_GG_OVERWRITE : 0);
    rc = gg_run(s, out->cnt, [&](unsigned long long* d_cnt) {
        hipLaunchKernelGGL(k_gg_position, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, T, N, O, X, flags, (int)cells, d_cnt);
    });
    if (rc != LIO_OK) return rc;
    if (resized) {
        for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k)
            if ((final_mask >> k) & 1u) fresh.swap_in(g, k);
        g->G = N;
    }
    undo.commit();
    g->mask = final_mask;
    return LIO_OK;
}

void gg_fill_geometry(const lio_grid* g, int32_t* rows, int32_t* cols, double length[2], double position[2])
{
    *rows = g->G.rows; *cols = g->G.cols;
    for (int a = 0; a < 2; ++a) { length[a] = g->G.len[a]; position[a] = g->G.pos[a]; }
}

}  // namespace

extern "C" int lio_grid_submap(lio_grid* src, const double position[2], const double length[2], lio_grid* dst, lio_grid_submap_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    t_gg.clear();
    if (!position || !length) return lio_fail(LIO_ERR_ARG, "null argument");
    for (int a = 0; a < 2; ++a) {
        if (!std::isfinite(position[a]) || !std::isfinite(length[a])) return lio_fail(LIO_ERR_ARG, "position and length must be finite");
        if (length[a] < 0.0) return lio_fail(LIO_ERR_ARG, "length must not be negative");
    }
    int rc = gg_pair_check(src, dst, "src and dst are the same object", false);
    if (rc != LIO_OK) return rc;
    const LioGridGeom S = src->G;
    LioGgSubmap M;
    lio_gg_submap_information(S, position, length, &M);
    if (!M.ok) {                                             // isSuccess = false: the reference returns a map without data
        lio_grid_clear(dst);
        return LIO_OK;
    }
    if ((rc = lio_check_device(src->device_id)) != LIO_OK) return rc;
    if ((rc = lio_grid_set_geometry(dst, M.size[0], M.size[1], S.res, M.length, M.position)) != LIO_OK) return rc;
    LioGridRollback undo(dst, true);                         // after a failure dst holds no layer
    LioGgTable T;
    memset(&T, 0, sizeof(T));
    for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k) {
        if (!((src->mask >> k) & 1u)) continue;
        float* d = nullptr;
        if ((rc = lio_grid_layer_slot(dst, k, &d)) != LIO_OK) return rc;
        T.self[T.n] = (const unsigned*)src->d_layer[k].p;
        T.dst[T.n] = (unsigned*)d;
        ++T.n;
    }
    hipStream_t s = nullptr;
    const long long cells = (long long)M.size[0] * (long long)M.size[1];
    unsigned long long hc[GG_N_CNT];
    rc = gg_run(s, hc, [&](unsigned long long* d_cnt) {
        hipLaunchKernelGGL(k_gg_offset, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, T, M.size[0], (int)cells, S.rows, S.cols, M.top_left[0],
                           M.top_left[1], d_cnt);
    });
    if (rc != LIO_OK) return rc;
    undo.commit();
    if (info) {
        info->success = 1;
        info->rows = M.size[0]; info->cols = M.size[1];
        for (int a = 0; a < 2; ++a) {
            info->length[a] = M.length[a]; info->position[a] = M.position[a];
            info->top_left[a] = M.top_left[a]; info->requested_index[a] = M.requested[a];
        }
    }
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_move(lio_grid* g, const double position[2], lio_grid_move_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    t_gg.clear();
    if (!position) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!std::isfinite(position[0]) || !std::isfinite(position[1])) return lio_fail(LIO_ERR_ARG, "position must be finite");
    if (!g) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!g->mask) return lio_fail(LIO_ERR_ARG, "the object holds no layers (lio_grid_set_layers, lio_kf_store_planning_grid)");
    const LioGridGeom O = g->G;
    int shift[2];
    double moved_to[2];
    for (int a = 0; a < 2; ++a) {
        if (!lio_gg_index_shift(position[a] - O.pos[a], O.res, &shift[a]))
            return lio_fail(LIO_ERR_ARG, "the position shift is 2^30 cells or more, or not finite");
        moved_to[a] = O.pos[a] + lio_gg_position_shift(shift[a], O.res);
        if (!std::isfinite(moved_to[a])) return lio_fail(LIO_ERR_ARG, "the moved map has no finite position");
    }
    const LioGridGeom N = lio_gm_geom(O.rows, O.cols, O.res, moved_to[0], moved_to[1]);
    unsigned long long hc[GG_N_CNT] = { 0 };
    if (shift[0] != 0 || shift[1] != 0) {
        int rc = lio_check_device(g->device_id);
        if (rc != LIO_OK) return rc;
        const size_t cells = (size_t)O.rows * (size_t)O.cols;
        GgFresh fresh;
        LioGgTable T;
        memset(&T, 0, sizeof(T));
        for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k) {
            if (!((g->mask >> k) & 1u)) continue;
            HIPCHK(fresh.alloc(k, cells));
            T.self[T.n] = (const unsigned*)g->d_layer[k].p;
            T.dst[T.n] = fresh.words(k);
            ++T.n;
        }
        hipStream_t s = nullptr;
        rc = gg_run(s, hc, [&](unsigned long long* d_cnt) {
            hipLaunchKernelGGL(k_gg_offset, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, T, O.rows, (int)cells, O.rows, O.cols, shift[0], shift[1], d_cnt);
        });
        if (rc != LIO_OK) return rc;
        for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k)
            if ((g->mask >> k) & 1u) fresh.swap_in(g, k);
    }
    g->G = N;
    if (info) {
        info->moved = (shift[0] != 0 || shift[1] != 0) ? 1 : 0;
        for (int a = 0; a < 2; ++a) { info->index_shift[a] = shift[a]; info->position[a] = moved_to[a]; }
        info->n_cells_cleared = (int64_t)hc[GG_CNT_CLEARED];
    }
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_extend_to_include(lio_grid* g, lio_grid* other, lio_grid_extend_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    int rc = gg_pair_check(g, other, "g and other are the same object", true);
    if (rc != LIO_OK) return rc;
    GgAddResult res;
    if ((rc = gg_extend_add(g, other, true, false, false, 0u, 0u, &res)) != LIO_OK) return rc;
    if (info) {
        info->resized = res.resized;
        gg_fill_geometry(g, &info->rows, &info->cols, info->length, info->position);
        info->n_cells_kept = (int64_t)res.cnt[GG_CNT_KEPT];
        info->n_index_outside = (int64_t)res.cnt[GG_CNT_INDEX];
    }
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_add_data_from(lio_grid* g, lio_grid* other, int32_t extend, int32_t overwrite, const int32_t* layer_ids, int32_t n_layers,
                                      uint32_t basic_mask, lio_grid_add_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    if ((extend != 0 && extend != 1) || (overwrite != 0 && overwrite != 1)) return lio_fail(LIO_ERR_ARG, "extend and overwrite are 0 or 1");
    if (n_layers < 0 || n_layers > LIO_GRID_MAX_LAYERS) return lio_fail(LIO_ERR_ARG, "n_layers must be in [0, LIO_GRID_MAX_LAYERS]");
    if (n_layers > 0 && !layer_ids) return lio_fail(LIO_ERR_ARG, "null argument");
    unsigned listed = 0;
    int rc = lio_grid_layer_list(layer_ids, n_layers, &listed);
    if (rc != LIO_OK) return rc;
    if (basic_mask >> LIO_GRID_MAX_LAYERS) return lio_fail(LIO_ERR_ARG, "basic_mask names a layer g does not hold");
    if ((rc = gg_pair_check(g, other, "g and other are the same object", true)) != LIO_OK) return rc;
    if (n_layers == 0) listed = other->mask;                // copyAllLayers
    if (listed & ~other->mask) return lio_fail(LIO_ERR_ARG, "a layer id names a layer other does not hold");
    if (basic_mask & ~g->mask) return lio_fail(LIO_ERR_ARG, "basic_mask names a layer g does not hold");
    GgAddResult res;
    if ((rc = gg_extend_add(g, other, extend != 0, true, overwrite != 0, listed, basic_mask, &res)) != LIO_OK) return rc;
    if (info) {
        info->resized = res.resized;
        gg_fill_geometry(g, &info->rows, &info->cols, info->length, info->position);
        info->n_cells_skipped_valid = (int64_t)res.cnt[GG_CNT_SKIPPED];
        info->n_cells_outside_other = (int64_t)res.cnt[GG_CNT_OUTSIDE];
        info->n_index_outside = (int64_t)res.cnt[GG_CNT_INDEX];
        info->n_values_copied = (int64_t)res.cnt[GG_CNT_COPIED];
    }
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_geom_debug_kernel_ms(int32_t enable, float* ms)
try {
    return t_gg.hook(enable, ms);
} LIO_CATCH
