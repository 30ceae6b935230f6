// lio_gridexpr.hip -- a new layer derived from several the resident object holds, by a user's expression: grid_map_filters'
// MathExpressionFilter.  The compiler and the arithmetic are lio_gridexpr.h's; this file is the kernels and the entry points.
//   k_gx_eval      the storing pass: one lane per cell, a flat index over the column-major layer.  The program is a kernel
//                  argument by value, so every instruction fetch is a scalar load and the dispatch is the same in every lane;
//                  the layers' base pointers travel in the same argument, the scalars of earlier passes are read from a small
//                  device array.  The operand stack below the top is LDS, slot * 256 + lane (no bank conflict, no register
//                  array indexed at run time, no scratch); the top is a register.  The same launch counts the finite results.
//   k_gx_reduce    one map-wide ...OfFinites: float addition in the reference's serial order cannot be re-associated, so one
//                  workgroup walks the layer in memory order.  Four waves evaluate the pass's cell code for the next
//                  LIO_GX_CHUNK cells into LDS while lane 0 of a fifth wave folds the previous chunk with the functor, one
//                  barrier a chunk (the distance field's "one lane per line of the serial sweep").  The scalar leaves through
//                  that lane's vector store.
// All passes of a call are enqueued without a host wait between them; one wait at the end brings the counter down.  The store is
// cell-local and follows every reduction, so out_layer may be a layer the expression reads.  DESIGN.md section 4q.
// -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <string.h>
#include <string>
#include <vector>

#include "lio_gridexpr.h"
#include "lio_gridsample.h"
#include "lio_gridobj.h"
#include "lio_cloud.h"
#include "lio_pool.h"
#include "lio_wg.h"

namespace {

struct GxLayers {
    const float* p[LIO_GRID_MAX_LAYERS];
};

struct GxLdsStack {                // the words below the top of one lane's stack
    float* s;
    __device__ __forceinline__ void put(int slot, float v) { s[slot * LIO_GX_LANES] = v; }
    __device__ __forceinline__ float get(int slot) const { return s[slot * LIO_GX_LANES]; }
};

struct GxCell {                    // lin < 0: a lane past the layer's end, which computes on zeros and stores nothing
    const GxLayers& L;
    const float* slots;
    int lin;
    __device__ __forceinline__ float layer(int id) const { return lin >= 0 ? L.p[id][lin] : 0.0f; }
    __device__ __forceinline__ float slot(int p) const { return slots[p]; }
};

__global__ __launch_bounds__(LIO_GX_LANES) void k_gx_eval(LioGxProgram P, GxLayers L, const float* slots, float* out, int n_cells,
                                                          unsigned long long* __restrict__ counters)
{
    __shared__ float s_stack[(LIO_GX_MAX_STACK - 1) * LIO_GX_LANES];
    const int lin = (int)blockIdx.x * LIO_GX_LANES + (int)threadIdx.x;
    GxLdsStack S = { s_stack + threadIdx.x };
    const GxCell cell = { L, slots, lin < n_cells ? lin : -1 };
    const float v = lio_gx_run_pass(P, P.n_passes - 1, S, cell);
    if (lin < n_cells) out[lin] = v;
    lio_wave_count(counters, 0, lin < n_cells && lio_gm_finite(v));
}

__global__ __launch_bounds__(LIO_GX_LANES + 64) void k_gx_reduce(LioGxProgram P, GxLayers L, float* slots, int pass, int n_cells)
{
    __shared__ float s_stack[(LIO_GX_MAX_STACK - 1) * LIO_GX_LANES];
    __shared__ float s_chunk[2][LIO_GX_CHUNK];
    const int tid = (int)threadIdx.x;
    const bool evaluates = tid < LIO_GX_LANES;
    const int kind = P.kind[pass];
    const int n_chunks = (n_cells + LIO_GX_CHUNK - 1) / LIO_GX_CHUNK;
    LioGxFold F;
    lio_gx_fold_begin(F);
    for (int k = 0; k <= n_chunks; ++k) {                    // step k: chunk k is evaluated, chunk k - 1 folded
        if (evaluates) {
            if (k < n_chunks) {
                GxLdsStack S = { s_stack + tid };
                for (int i = tid; i < LIO_GX_CHUNK; i += LIO_GX_LANES) {
                    const int lin = k * LIO_GX_CHUNK + i;
                    const GxCell cell = { L, slots, lin < n_cells ? lin : -1 };
                    s_chunk[k & 1][i] = lio_gx_run_pass(P, pass, S, cell);
                }
            }
        } else if (tid == LIO_GX_LANES && k > 0) {
            const int first = (k - 1) * LIO_GX_CHUNK;
            const int n = n_cells - first < LIO_GX_CHUNK ? n_cells - first : LIO_GX_CHUNK;
            const float* c = s_chunk[(k - 1) & 1];
            for (int i = 0; i < n; ++i) lio_gx_fold(F, kind, c[i]);
        }
        __syncthreads();
    }
    if (tid == LIO_GX_LANES) slots[pass] = lio_gx_fold_end(F, kind);
}

thread_local LioStageTimes<2> t_gx;                        // the reduction passes, the storing pass

void gx_fill_info(lio_grid_expression_info* info, const LioGxProgram& P, int rows, int cols, long long n_finite)
{
    if (!info) return;
    info->rows = rows; info->cols = cols;
    info->n_ops = P.n_ops; info->n_passes = P.n_passes;
    info->layers_read = P.layers_read;
    info->stack_depth = P.stack_depth;
    info->n_finite = (int64_t)n_finite;
}

}  // namespace

extern "C" int lio_grid_expression_check(const char* expression, const char* const* names, const int32_t* layer_ids, int32_t n_names,
                                         lio_grid_expression_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    LioGxProgram P;
    std::string why;
    const int rc = lio_gx_compile(expression, names, layer_ids, n_names, &P, &why);
    if (rc != LIO_OK) return lio_fail(rc, why.c_str());
    gx_fill_info(info, P, 0, 0, 0);
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_filter_expression(lio_grid* g, const char* expression, const char* const* names, const int32_t* layer_ids, int32_t n_names,
                                          int32_t out_layer, lio_grid_expression_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    t_gx.clear();
    LioGxProgram P;
    std::string why;
    int rc = lio_gx_compile(expression, names, layer_ids, n_names, &P, &why);
    if (rc != LIO_OK) return lio_fail(rc, why.c_str());
    if (out_layer < 0 || out_layer >= LIO_GRID_MAX_LAYERS) return lio_fail(LIO_ERR_ARG, "a layer id is outside 0 .. 15");
    if (!g) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!g->mask) return lio_fail(LIO_ERR_ARG, "the object holds no layers (lio_grid_set_layers, lio_kf_store_planning_grid)");
    if (P.layers_read & ~g->mask) return lio_fail(LIO_ERR_ARG, "the expression reads a layer the object does not hold");
    if ((rc = lio_check_device(g->device_id)) != LIO_OK) return rc;
    const int rows = g->G.rows, cols = g->G.cols;
    const int n_cells = rows * cols;                         // (a layer has fewer than 2^31 cells)
    LioGridRollback undo(g, false);                          // after a failure g holds the layers it held
    float* d_out = nullptr;
    if ((rc = lio_grid_layer_slot(g, out_layer, &d_out)) != LIO_OK) return rc;
    GxLayers L;
    for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k) L.p[k] = (P.layers_read >> k & 1u) ? g->d_layer[k].p : nullptr;
    hipStream_t s = nullptr;
    LioGridCounters counters;                                // one counter, the scalar slots behind it
    HIPCHK(counters.alloc(1, LIO_GX_MAX_REDUCE));
    HIPCHK(counters.clear(s));
    float* d_slots = (float*)(counters.d() + 1);
    LioStageClock clk(t_gx.on);
    clk.mark(s);
    for (int p = 0; p + 1 < P.n_passes; ++p)
        hipLaunchKernelGGL(k_gx_reduce, dim3(1), dim3(LIO_GX_LANES + 64), 0, s, P, L, d_slots, p, n_cells);
    clk.mark(s);
    hipLaunchKernelGGL(k_gx_eval, dim3((unsigned)((n_cells + LIO_GX_LANES - 1) / LIO_GX_LANES)), dim3(LIO_GX_LANES), 0, s, P, L, (const float*)d_slots, d_out,
                       n_cells, counters.d());
    clk.mark(s);
    unsigned long long n_finite = 0;
    if ((rc = counters.finish(&n_finite, s, nullptr)) != LIO_OK) return rc;
    t_gx.read(clk);
    undo.commit();
    gx_fill_info(info, P, rows, cols, (long long)n_finite);
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_debug_grid_expression_host(const char* expression, const char* const* names, int32_t n_names, const float* layers, int32_t rows,
                                              int32_t cols, float* out)
try {
    if (n_names < 0 || n_names > LIO_GX_MAX_NAMES) return lio_fail(LIO_ERR_ARG, "expression: n_names must be in [0, 16]");
    int32_t ids[LIO_GX_MAX_NAMES];
    for (int k = 0; k < LIO_GX_MAX_NAMES; ++k) ids[k] = k;
    LioGxProgram P;
    std::string why;
    const int rc = lio_gx_compile(expression, names, ids, n_names, &P, &why);
    if (rc != LIO_OK) return lio_fail(rc, why.c_str());
    if (!layers || !out) return lio_fail(LIO_ERR_ARG, "null argument");
    if (rows < 1 || cols < 1 || (long long)rows * cols > 0x7fffffffLL) return lio_fail(LIO_ERR_ARG, "rows and cols must be positive, a layer below 2^31 cells");
    const size_t cells = (size_t)rows * (size_t)cols;
    const float* layer[LIO_GX_MAX_NAMES] = {};
    for (int k = 0; k < n_names; ++k) layer[k] = layers + (size_t)k * cells;
    lio_gx_host_run(P, layer, cells, out, nullptr);
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_expression_debug_kernel_ms(int32_t enable, float ms[2])
try {
    return t_gx.hook(enable, ms);
} LIO_CATCH
