// lio_gridconvert.hip -- resident planning layers out as images, point clouds and grid cells, a distance field out as the
// cloud near the surface, and images and occupancy grids in as layers: grid_map_cv's GridMapCvConverter and
// GridMapRosConverter's toPointCloud, toGridCells and fromOccupancyGrid.  The arithmetic and the index maps are
// lio_gridconvert.h's; this file is the kernels and the entry points.
//   k_gc_extremes     minCoeffOfFinites / maxCoeffOfFinites: lio_wg.h's box over a workgroup, then integer atomicMin / atomicMax
//                     on the ordered words across workgroups, so the bounds are the same on every run.
//   k_gc_to_image_direct, k_gc_from_image_direct
//                     what the entries run: one lane per pixel in the image's order (per cell in the layer's order on the way
//                     in), the other side read with a stride.  A planning layer is under a megabyte and stays in L2; measured
//                     on the loader's grid the direct form takes about half the time of the tiled one (DESIGN.md section 6,
//                     "Resident layers out and in"), so by the rule set for this file it is the one kept on the path.
//   k_gc_to_image, k_gc_from_image
//                     the LDS-tiled form, launched only when lio_grid_convert_debug_stage_ms asks for it (the comparison
//                     tools/grid_convert_cost.py repeats, and one test): a 64 x 64 tile of cells through LDS (pitch 65 words).
//                     Out: a wave reads 64 consecutive rows of one column (256 contiguous bytes), stores the cells' pixel
//                     words down a tile column, then writes the tile's run of one image row, lane d the d-th whole dword of
//                     the buffer inside the run, composed from up to four pixels of the tile line; the bytes before the first
//                     and after the last whole dword go one by one.  In: the same tile the other way round.
//   k_gc_occupancy    the message reversed in storage order; no tile.
//   the compactions   lio_compact.h: count per workgroup, scan, the host's one wait for the count and the capacity test, then
//                     emit with the predicate evaluated again.  The predicate yields the cell index; the sink gathers the
//                     record's F floats.  No atomic decides an order.
// The counters are per-wave ballots and one integer atomic per wave and counter.  DESIGN.md section 4o.  -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <cmath>
#include <string.h>

#include "lio_gridconvert.h"
#include "lio_gridsample.h"
#include "lio_gridobj.h"
#include "lio_sdfobj.h"
#include "lio_compact.h"
#include "lio_cloud.h"
#include "lio_pool.h"
#include "lio_wg.h"

namespace {

enum { GC_CNT_A = 0, GC_CNT_B, GC_CNT_C, GC_N_CNT };      // to_image: clamped low, clamped high, non-finite; ingest: transparent / unknown

struct GcTileLine {                // a line of the tile: pixel -> word
    const unsigned* p;
    __device__ __forceinline__ unsigned at(int pixel) const { return p[pixel]; }
};

__global__ __launch_bounds__(256) void k_gc_extremes(const float* __restrict__ layer, int n, unsigned* __restrict__ stats)
{
    __shared__ LioWgBoxLds<4> s_box;
    float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = layer[i];
        if (lio_gm_finite(v)) { mn[0] = fminf(mn[0], v); mx[0] = fmaxf(mx[0], v); }
    }
    float lo = 0.0f, hi = 0.0f;
    lio_wg_box<4>(mn, mx, s_box, lo, hi);
    if (threadIdx.x == 0 && lo <= hi) { atomicMin(&stats[0], lio_f2ord(lo)); atomicMax(&stats[1], lio_f2ord(hi)); }
}

__global__ __launch_bounds__(256) void k_gc_to_image(const float* __restrict__ layer, int rows, int cols, int tiles_r, float lo, float hi, int channels, int depth,
                                                     unsigned char* __restrict__ image, unsigned long long* __restrict__ counters)
{
    __shared__ unsigned s_tile[LIO_GC_TILE * LIO_GC_PITCH];
    const int r0 = ((int)blockIdx.x % tiles_r) * LIO_GC_TILE, c0 = ((int)blockIdx.x / tiles_r) * LIO_GC_TILE;
    const int nr = rows - r0 < LIO_GC_TILE ? rows - r0 : LIO_GC_TILE, nc = cols - c0 < LIO_GC_TILE ? cols - c0 : LIO_GC_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < LIO_GC_TILE; c += 4) {            // (the whole wave stays for the ballots)
        int cls = LIO_GC_IN_RANGE;
        if (lane < nr && c < nc) s_tile[lane * LIO_GC_PITCH + c] = lio_gc_pixel(layer[(size_t)(c0 + c) * (size_t)rows + (size_t)(r0 + lane)], lo, hi, depth, &cls);
        lio_wave_count(counters, GC_CNT_A, cls == LIO_GC_CLAMPED_LOW);
        lio_wave_count(counters, GC_CNT_B, cls == LIO_GC_CLAMPED_HIGH);
        lio_wave_count(counters, GC_CNT_C, cls == LIO_GC_NONFINITE);
    }
    __syncthreads();
    const int px = channels * lio_gc_elem_bytes(depth);
    unsigned* image_words = (unsigned*)image;
    for (int r = wave; r < nr; r += 4) {
        const GcTileLine line = { s_tile + r * LIO_GC_PITCH };
        const size_t at = ((size_t)(r0 + r) * (size_t)cols + (size_t)c0) * (size_t)px;
        const LioGcRun R = lio_gc_run(at, (size_t)nc * (size_t)px);
        for (size_t b = at + lane; b < R.head_end; b += 64) image[b] = (unsigned char)lio_gc_run_byte(line, b - at, px, channels, depth);
        for (size_t d = R.d0 + lane; d < R.d1; d += 64) image_words[d] = lio_gc_run_dword(line, d, at, px, channels, depth);
        for (size_t b = R.tail_begin + lane; b < R.end; b += 64) image[b] = (unsigned char)lio_gc_run_byte(line, b - at, px, channels, depth);
    }
}

__global__ __launch_bounds__(256) void k_gc_to_image_direct(const float* __restrict__ layer, int rows, int cols, float lo, float hi, int channels, int depth,
                                                            unsigned char* __restrict__ image, unsigned long long* __restrict__ counters)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;       // the pixel, in the image's order
    int cls = LIO_GC_IN_RANGE;
    if (q < (long long)rows * cols) {
        const int r = (int)(q / cols), c = (int)(q % cols);
        const unsigned w = lio_gc_pixel(layer[(size_t)c * (size_t)rows + (size_t)r], lo, hi, depth, &cls);
        const int px = channels * lio_gc_elem_bytes(depth);
        for (int b = 0; b < px; ++b) image[(size_t)q * (size_t)px + b] = (unsigned char)lio_gc_pixel_byte(w, b, channels, depth);
    }
    lio_wave_count(counters, GC_CNT_A, cls == LIO_GC_CLAMPED_LOW);
    lio_wave_count(counters, GC_CNT_B, cls == LIO_GC_CLAMPED_HIGH);
    lio_wave_count(counters, GC_CNT_C, cls == LIO_GC_NONFINITE);
}

__global__ __launch_bounds__(256) void k_gc_from_image(LioGcIngest I, int tiles_r, const unsigned char* __restrict__ image, unsigned* __restrict__ layer,
                                                       unsigned long long* __restrict__ counters)
{
    __shared__ unsigned s_tile[LIO_GC_TILE * LIO_GC_PITCH];
    const int r0 = ((int)blockIdx.x % tiles_r) * LIO_GC_TILE, c0 = ((int)blockIdx.x / tiles_r) * LIO_GC_TILE;
    const int nr = I.rows - r0 < LIO_GC_TILE ? I.rows - r0 : LIO_GC_TILE, nc = I.cols - c0 < LIO_GC_TILE ? I.cols - c0 : LIO_GC_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int px = I.channels * lio_gc_elem_bytes(I.depth);
    for (int r = wave; r < LIO_GC_TILE; r += 4) {
        bool transparent = false;
        if (r < nr && lane < nc)
            s_tile[lane * LIO_GC_PITCH + r] = lio_gc_word_from_pixel(I, image + ((size_t)(r0 + r) * (size_t)I.cols + (size_t)(c0 + lane)) * (size_t)px, &transparent);
        lio_wave_count(counters, GC_CNT_A, transparent);
    }
    __syncthreads();
    for (int c = wave; c < nc; c += 4)
        if (lane < nr) layer[(size_t)(c0 + c) * (size_t)I.rows + (size_t)(r0 + lane)] = s_tile[c * LIO_GC_PITCH + lane];
}

__global__ __launch_bounds__(256) void k_gc_from_image_direct(LioGcIngest I, const unsigned char* __restrict__ image, unsigned* __restrict__ layer,
                                                              unsigned long long* __restrict__ counters)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;       // the cell, in the layer's order
    bool transparent = false;
    if (i < (long long)I.rows * I.cols) {
        const int r = (int)(i % I.rows), c = (int)(i / I.rows);
        const int px = I.channels * lio_gc_elem_bytes(I.depth);
        layer[i] = lio_gc_word_from_pixel(I, image + ((size_t)r * (size_t)I.cols + (size_t)c) * (size_t)px, &transparent);
    }
    lio_wave_count(counters, GC_CNT_A, transparent);
}

struct GcFill { unsigned* p[LIO_GRID_MAX_LAYERS]; int n; };          // the layers setGeometry clears

__global__ __launch_bounds__(256) void k_gc_occupancy(const int8_t* __restrict__ data, int n, unsigned* __restrict__ layer, GcFill F,
                                                      unsigned long long* __restrict__ counters)
{
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    bool unknown = false;
    if (i < n) {
        const unsigned w = lio_gc_occupancy_word(data[n - 1 - i]);
        unknown = w == LIO_QNAN_BITS;
        layer[i] = w;
        for (int k = 0; k < F.n; ++k) F.p[k][i] = LIO_QNAN_BITS;
    }
    lio_wave_count(counters, GC_CNT_A, unknown);
}

// ---- the compactions' predicates and sinks --------------------------------------------------------------------------------
struct GcCloudPred {
    LioGcCloud C;
    __device__ __forceinline__ bool operator()(int i, int& cell) const { cell = i; return lio_gc_cloud_kept(C, i); }
};
struct GcCloudSink {
    LioGcCloud C;
    LioGridGeom G;
    unsigned* out;
    __device__ __forceinline__ void operator()(int at, const int& cell) const { lio_gc_cloud_record(C, G, cell, out + (size_t)at * (size_t)C.n_fields); }
};
struct GcCellsPred {
    const float* layer;
    float lower, upper;
    __device__ __forceinline__ bool operator()(int i, int& cell) const { cell = i; return lio_gc_cell_kept(layer[i], lower, upper); }
};
struct GcCellsSink {
    LioGridGeom G;
    double2* out;
    __device__ __forceinline__ void operator()(int at, const int& cell) const
    {
        out[at] = make_double2(lio_gm_centre(G, 0, cell % G.rows), lio_gm_centre(G, 1, cell / G.rows));
    }
};
struct GcSdfPred {
    LioSdfLookup L;
    LioGcSdfVisit V;
    const float4* nodes;
    float lower, upper;
    __device__ __forceinline__ bool operator()(int i, float4& q) const
    {
        int idx[3];
        lio_gc_sdf_node(V, i, idx);
        const float d = nodes[lio_sdf_linear_index(L, idx)].x;
        q = lio_gc_sdf_point(L, idx, d);
        return lio_gc_sdf_kept(d, lower, upper);
    }
};

// four marks around the three stages; cleared where a call makes its clock, so a stage that did not run reads 0
thread_local LioStageTimes<3> t_gc;
thread_local bool t_gc_tiled = false;

// Count and scan, the one wait for the count, the capacity test, emit into a block of the count's size, the records down.
template <class Rec, class Pred, class MakeSink>
int gc_compact_out(const Pred& pred, int n, size_t record_bytes, void* out, size_t cap, size_t* n_out, const MakeSink& make_sink)
{
    hipStream_t s = nullptr;
    t_gc.clear();
    LioStageClock clk(t_gc.on);
    clk.mark(s);
    LioTemp counts, recs;
    int rc = compact_count<Rec>(pred, n, counts, s);
    if (rc != LIO_OK) return rc;
    int total = 0;
    HIPCHK(hipMemcpyAsync(&total, counts.as<int>() + (n + 255) / 256, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    clk.mark(s);
    *n_out = (size_t)total;
    if ((size_t)total > cap) return lio_fail(LIO_ERR_CAPACITY, "more survivors than the buffer holds records (*n_out tells the need)");
    if (total == 0) return LIO_OK;
    HIPCHK(recs.alloc(record_bytes * (size_t)total));
    compact_emit<Rec>(pred, n, counts, make_sink(recs.p), s);
    clk.mark(s);
    HIPCHK(hipMemcpyAsync(out, recs.p, record_bytes * (size_t)total, hipMemcpyDeviceToHost, s));
    clk.mark(s);
    HIPCHK(hipStreamSynchronize(s));                       // (the temporaries go back to the pool after it)
    HIPCHK(hipGetLastError());
    t_gc.read(clk);
    return LIO_OK;
}

int gc_image_format_check(int channels, int depth)
{
    if (channels != 1 && channels != 3 && channels != 4) return lio_fail(LIO_ERR_ARG, "channels must be 1, 3 or 4");
    if (depth != LIO_IMAGE_8U && depth != LIO_IMAGE_16U && depth != LIO_IMAGE_32F) return lio_fail(LIO_ERR_ARG, "depth must be LIO_IMAGE_8U, LIO_IMAGE_16U or LIO_IMAGE_32F");
    return LIO_OK;
}

// The two image ingests behind one launch.  The layer is written whole; after a failure g holds what it held.
int gc_from_image(lio_grid* g, int layer, const void* image, int rows, int cols, const LioGcIngest& I, double resolution, const double* position,
                  lio_grid_from_image_info* info)
{
    if (!image) return lio_fail(LIO_ERR_ARG, "null argument");
    if (layer < 0 || layer >= LIO_GRID_MAX_LAYERS) return lio_fail(LIO_ERR_ARG, "layer is outside 0 .. 15");
    if (rows < 1 || cols < 1) return lio_fail(LIO_ERR_ARG, "rows and cols must be at least 1");
    if (!g) return lio_fail(LIO_ERR_ARG, "null argument");
    const bool empty = g->mask == 0;
    int rc;
    double length[2] = { 0.0, 0.0 };
    if (empty) {
        if (!position) return lio_fail(LIO_ERR_ARG, "null argument");
        length[0] = resolution * rows; length[1] = resolution * cols;      // initializeFromImage, CV:39-40
        if ((rc = lio_grid_geometry_check(rows, cols, resolution, length, position)) != LIO_OK) return rc;
    } else if (g->G.rows != rows || g->G.cols != cols) return lio_fail(LIO_ERR_ARG, "the image's size is not the grid's");
    if ((rc = lio_check_device(g->device_id)) != LIO_OK) return rc;
    LioGridRollback undo(g, empty);                          // after a failure: what it held, nothing where the geometry was set here
    if (empty && (rc = lio_grid_set_geometry(g, rows, cols, resolution, length, position)) != LIO_OK) return rc;
    float* d = nullptr;
    if ((rc = lio_grid_layer_slot(g, layer, &d)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    const size_t cells = (size_t)rows * (size_t)cols, bytes = cells * (size_t)I.channels * (size_t)lio_gc_elem_bytes(I.depth);
    LioTemp img;
    LioGridCounters counters;
    HIPCHK(img.alloc(bytes));
    HIPCHK(counters.alloc(GC_N_CNT));
    t_gc.clear();
    LioStageClock clk(t_gc.on);
    clk.mark(s);
    HIPCHK(hipMemcpyAsync(img.p, image, bytes, hipMemcpyHostToDevice, s));
    HIPCHK(counters.clear(s));
    clk.mark(s);
    if (!t_gc_tiled) {
        hipLaunchKernelGGL(k_gc_from_image_direct, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, I, img.as<unsigned char>(), (unsigned*)d, counters.d());
    } else {
        const int tiles_r = (rows + LIO_GC_TILE - 1) / LIO_GC_TILE, tiles_c = (cols + LIO_GC_TILE - 1) / LIO_GC_TILE;
        hipLaunchKernelGGL(k_gc_from_image, dim3((unsigned)tiles_r * (unsigned)tiles_c), dim3(256), 0, s, I, tiles_r, img.as<unsigned char>(), (unsigned*)d,
                           counters.d());
    }
    clk.mark(s);
    unsigned long long hc[GC_N_CNT] = { 0, 0, 0 };
    if ((rc = counters.finish(hc, s, &clk)) != LIO_OK) return rc;       // the call's one host wait
    t_gc.read(clk);
    undo.commit();
    if (info) {
        info->rows = rows; info->cols = cols;
        info->geometry_set = empty ? 1 : 0;
        info->n_cells_transparent = (int64_t)hc[GC_CNT_A];
        info->n_cells_set = (int64_t)cells - info->n_cells_transparent;
    }
    return LIO_OK;
}

}  // namespace

extern "C" int lio_grid_to_image(lio_grid* g, int32_t layer, int32_t channels, int32_t depth, float lower, float upper, void* image, size_t cap_bytes,
                                 lio_grid_image_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    int rc = gc_image_format_check(channels, depth);
    if (rc != LIO_OK) return rc;
    const bool automatic = lower != lower && upper != upper;
    if (!automatic) {
        if (lower != lower || upper != upper) return lio_fail(LIO_ERR_ARG, "lower and upper are both NaN (the layer's extremes) or both numbers");
        if (!(upper > lower)) return lio_fail(LIO_ERR_ARG, "upper must be greater than lower");
        if (!lio_gm_finite(upper - lower)) return lio_fail(LIO_ERR_ARG, "upper - lower must be finite");
    }
    if (!g || !image) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!lio_grid_has_layer(g, layer)) return lio_fail(LIO_ERR_ARG, "the object holds no such layer");
    const int rows = g->G.rows, cols = g->G.cols;
    const size_t cells = (size_t)rows * (size_t)cols, bytes = cells * (size_t)channels * (size_t)lio_gc_elem_bytes(depth);
    if (cap_bytes < bytes) return lio_fail(LIO_ERR_ARG, "image holds fewer than rows x cols x channels x element size bytes");
    if ((rc = lio_check_device(g->device_id)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    const float* d_layer = g->d_layer[layer].p;
    LioTemp img;
    LioGridCounters counters;
    HIPCHK(img.alloc(bytes + 4));
    HIPCHK(counters.alloc(GC_N_CNT, 1));                   // (the word behind them: the extremes)
    unsigned* d_stats = (unsigned*)(counters.d() + GC_N_CNT);
    t_gc.clear();
    LioStageClock clk(t_gc.on);
    clk.mark(s);
    HIPCHK(counters.clear(s));
    if (automatic) {
        unsigned hs[2] = { LIO_ORD_NO_MIN, LIO_ORD_NO_MAX };
        HIPCHK(hipMemcpyAsync(d_stats, hs, sizeof(hs), hipMemcpyHostToDevice, s));
        const size_t nb = (cells + 255) / 256;
        hipLaunchKernelGGL(k_gc_extremes, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, s, d_layer, (int)cells, d_stats);
        HIPCHK(hipMemcpyAsync(hs, d_stats, sizeof(hs), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                   // the bounds decide the refusal
        HIPCHK(hipGetLastError());
        if (hs[0] == LIO_ORD_NO_MIN && hs[1] == LIO_ORD_NO_MAX) return lio_fail(LIO_ERR_ARG, "the layer has no finite cell: no automatic bounds");
        lower = lio_ord2f(hs[0]); upper = lio_ord2f(hs[1]);
        if (!(upper > lower)) return lio_fail(LIO_ERR_ARG, "the layer's finite extremes are equal: no automatic bounds");
        if (!lio_gm_finite(upper - lower)) return lio_fail(LIO_ERR_ARG, "upper - lower must be finite");
    }
    clk.mark(s);
    if (!t_gc_tiled) {
        hipLaunchKernelGGL(k_gc_to_image_direct, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, d_layer, rows, cols, lower, upper, channels, depth,
                           img.as<unsigned char>(), counters.d());
    } else {
        const int tiles_r = (rows + LIO_GC_TILE - 1) / LIO_GC_TILE, tiles_c = (cols + LIO_GC_TILE - 1) / LIO_GC_TILE;
        hipLaunchKernelGGL(k_gc_to_image, dim3((unsigned)tiles_r * (unsigned)tiles_c), dim3(256), 0, s, d_layer, rows, cols, tiles_r, lower, upper, channels, depth,
                           img.as<unsigned char>(), counters.d());
    }
    clk.mark(s);
    unsigned long long hc[GC_N_CNT] = { 0, 0, 0 };
    HIPCHK(hipMemcpyAsync(image, img.p, bytes, hipMemcpyDeviceToHost, s));
    if ((rc = counters.finish(hc, s, &clk)) != LIO_OK) return rc;
    t_gc.read(clk);
    if (info) {
        info->rows = rows; info->cols = cols;
        info->lower = lower; info->upper = upper;
        info->n_clamped_low = (int64_t)hc[GC_CNT_A]; info->n_clamped_high = (int64_t)hc[GC_CNT_B]; info->n_nonfinite = (int64_t)hc[GC_CNT_C];
        info->n_pixels = (int64_t)cells - info->n_nonfinite;
    }
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_add_layer_from_image(lio_grid* g, int32_t layer, const void* image, int32_t rows, int32_t cols, int32_t channels, int32_t depth,
                                             float lower, float upper, double alpha_threshold, double resolution, const double position[2],
                                             lio_grid_from_image_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    int rc = gc_image_format_check(channels, depth);
    if (rc != LIO_OK) return rc;
    if (depth == LIO_IMAGE_32F && channels != 1) return lio_fail(LIO_ERR_ARG, "a 32F image must have one channel");
    if (!(alpha_threshold >= 0.0 && alpha_threshold <= 1.0)) return lio_fail(LIO_ERR_ARG, "alpha_threshold must be in [0, 1]");
    LioGcIngest I;
    memset(&I, 0, sizeof(I));
    I.rows = rows; I.cols = cols; I.channels = channels; I.depth = depth;
    I.lower = lower; I.upper = upper;
    I.alpha_min = depth == LIO_IMAGE_32F ? 0u : lio_gc_alpha_min(alpha_threshold, depth);
    return gc_from_image(g, layer, image, rows, cols, I, resolution, position, info);
} LIO_CATCH

extern "C" int lio_grid_add_color_layer_from_image(lio_grid* g, int32_t layer, const void* image, int32_t rows, int32_t cols, int32_t channels, int32_t depth,
                                                   double resolution, const double position[2], lio_grid_from_image_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    if (channels != 3 && channels != 4) return lio_fail(LIO_ERR_ARG, "a colour layer takes 3 or 4 channels");
    if (depth != LIO_IMAGE_8U) return lio_fail(LIO_ERR_ARG, "a colour layer takes LIO_IMAGE_8U");
    LioGcIngest I;
    memset(&I, 0, sizeof(I));
    I.rows = rows; I.cols = cols; I.channels = channels; I.depth = depth;
    I.color = 1;
    return gc_from_image(g, layer, image, rows, cols, I, resolution, position, info);
} LIO_CATCH

extern "C" int lio_grid_from_occupancy(lio_grid* g, int32_t layer, const int8_t* data, size_t n, uint32_t width, uint32_t height, float resolution,
                                       const double origin[2], lio_grid_from_occupancy_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    if (!data || !origin) return lio_fail(LIO_ERR_ARG, "null argument");
    if (layer < 0 || layer >= LIO_GRID_MAX_LAYERS) return lio_fail(LIO_ERR_ARG, "layer is outside 0 .. 15");
    if (width < 1 || height < 1 || width >= (uint32_t)LIO_GS_MAX_LINE || height >= (uint32_t)LIO_GS_MAX_LINE)
        return lio_fail(LIO_ERR_ARG, "width and height must be in [1, 2^24)");
    if ((size_t)width * (size_t)height != n) return lio_fail(LIO_ERR_ARG, "n is not width * height");
    const double res = (double)resolution;                 // the message's float32 field
    if (!std::isfinite(res) || res < 1e-4) return lio_fail(LIO_ERR_ARG, "resolution must be finite and at least 1e-4");
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1])) return lio_fail(LIO_ERR_ARG, "origin must be finite");
    const int rows = (int)width, cols = (int)height;
    const double length[2] = { res * (double)rows, res * (double)cols };
    const double position[2] = { origin[0] + 0.5 * length[0], origin[1] + 0.5 * length[1] };
    int rc = lio_grid_geometry_check(rows, cols, res, length, position);
    if (rc != LIO_OK) return rc;
    for (int a = 0; a < 2; ++a)                             // setGeometry's own size, GridMap.cpp:50
        if (round(length[a] / res) != (double)(a == 0 ? rows : cols)) return lio_fail(LIO_ERR_ARG, "round(length / resolution) is not the message's size");
    if (!g) return lio_fail(LIO_ERR_ARG, "null argument");
    const LioGridGeom& G = g->G;
    const bool replace = !g->mask || G.rows != rows || G.cols != cols || G.res != res || G.len[0] != length[0] || G.len[1] != length[1] ||
                         G.pos[0] != position[0] || G.pos[1] != position[1];
    if ((rc = lio_check_device(g->device_id)) != LIO_OK) return rc;
    const unsigned old_mask = g->mask;
    LioGridRollback undo(g, replace);                      // after a failure: what it held where the geometry stayed, nothing where it was replaced
    GcFill F;
    memset(&F, 0, sizeof(F));
    if (replace) {
        if ((rc = lio_grid_set_geometry(g, rows, cols, res, length, position)) != LIO_OK) return rc;
        for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k) {
            if (k == layer || !((old_mask >> k) & 1u)) continue;
            float* p = nullptr;
            if ((rc = lio_grid_layer_slot(g, k, &p)) != LIO_OK) return rc;
            F.p[F.n++] = (unsigned*)p;
        }
    }
    float* d = nullptr;
    if ((rc = lio_grid_layer_slot(g, layer, &d)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    LioTemp msg;
    LioGridCounters counters;
    HIPCHK(msg.alloc(n));
    HIPCHK(counters.alloc(GC_N_CNT));
    t_gc.clear();
    LioStageClock clk(t_gc.on);
    clk.mark(s);
    HIPCHK(hipMemcpyAsync(msg.p, data, n, hipMemcpyHostToDevice, s));
    HIPCHK(counters.clear(s));
    clk.mark(s);
    hipLaunchKernelGGL(k_gc_occupancy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, msg.as<int8_t>(), (int)n, (unsigned*)d, F, counters.d());
    clk.mark(s);
    unsigned long long hc[GC_N_CNT] = { 0, 0, 0 };
    if ((rc = counters.finish(hc, s, &clk)) != LIO_OK) return rc;       // the call's one host wait
    t_gc.read(clk);
    undo.commit();
    if (info) {
        info->rows = rows; info->cols = cols;
        info->geometry_replaced = replace ? 1 : 0;
        for (int a = 0; a < 2; ++a) { info->length[a] = length[a]; info->position[a] = position[a]; }
        info->n_unknown = (int64_t)hc[GC_CNT_A];
    }
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_to_point_cloud(lio_grid* g, int32_t point_layer, const int32_t* layer_ids, int32_t n_layers, uint32_t basic_mask, float* points,
                                       size_t cap_points, size_t* n_out, int32_t* n_fields)
try {
    if (n_out) *n_out = 0;
    if (n_fields) *n_fields = 0;
    if (!layer_ids || !n_out || (cap_points && !points)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (n_layers < 1 || n_layers > LIO_GRID_MAX_LAYERS) return lio_fail(LIO_ERR_ARG, "n_layers must be in [1, LIO_GRID_MAX_LAYERS]");
    unsigned listed = 0;
    int rc = lio_grid_layer_list(layer_ids, n_layers, &listed);
    if (rc != LIO_OK) return rc;
    if (basic_mask >> LIO_GRID_MAX_LAYERS) return lio_fail(LIO_ERR_ARG, "basic_mask names a layer the object does not hold");
    if (!g) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!g->mask) return lio_fail(LIO_ERR_ARG, "the object holds no layers (lio_grid_set_layers, lio_kf_store_planning_grid)");
    if (listed & ~g->mask) return lio_fail(LIO_ERR_ARG, "a layer id names a layer the object does not hold");
    if (!lio_grid_has_layer(g, point_layer)) return lio_fail(LIO_ERR_ARG, "the object does not hold point_layer");
    if (basic_mask & ~g->mask) return lio_fail(LIO_ERR_ARG, "basic_mask names a layer the object does not hold");
    GcCloudPred pred;
    memset(&pred, 0, sizeof(pred));
    LioGcCloud& C = pred.C;
    C.point = (const unsigned*)g->d_layer[point_layer].p;
    C.point_at = -1;
    C.n_layers = n_layers;
    for (int k = 0; k < n_layers; ++k) {
        C.layer[k] = (const unsigned*)g->d_layer[layer_ids[k]].p;
        if (layer_ids[k] == point_layer) C.point_at = k;
        C.n_fields += layer_ids[k] == point_layer ? 3 : 1;
    }
    for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k)
        if ((basic_mask >> k) & 1u) C.basic[C.n_basic++] = (const unsigned*)g->d_layer[k].p;
    if (n_fields) *n_fields = C.n_fields;
    if ((rc = lio_check_device(g->device_id)) != LIO_OK) return rc;
    const LioGridGeom G = g->G;
    return gc_compact_out<int>(pred, G.rows * G.cols, sizeof(float) * (size_t)C.n_fields, points, cap_points, n_out,
                               [&](void* p) { return GcCloudSink{ C, G, (unsigned*)p }; });
} LIO_CATCH

extern "C" int lio_grid_to_grid_cells(lio_grid* g, int32_t layer, float lower, float upper, double* cells, size_t cap_cells, size_t* n_out)
try {
    if (n_out) *n_out = 0;
    if (!n_out || (cap_cells && !cells)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (lower != lower || upper != upper) return lio_fail(LIO_ERR_ARG, "lower and upper must not be NaN");
    if (!g) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!lio_grid_has_layer(g, layer)) return lio_fail(LIO_ERR_ARG, "the object holds no such layer");
    int rc = lio_check_device(g->device_id);
    if (rc != LIO_OK) return rc;
    const LioGridGeom G = g->G;
    const GcCellsPred pred = { g->d_layer[layer].p, lower, upper };
    return gc_compact_out<int>(pred, G.rows * G.cols, sizeof(double2), cells, cap_cells, n_out, [&](void* p) { return GcCellsSink{ G, (double2*)p }; });
} LIO_CATCH

extern "C" int lio_sdf_to_point_cloud(lio_sdf* sdf, int32_t decimation, float lower, float upper, float* points, size_t cap_points, size_t* n_out)
try {
    if (n_out) *n_out = 0;
    if (!n_out || (cap_points && !points)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (decimation < 1) return lio_fail(LIO_ERR_ARG, "decimation must be at least 1");
    if (!sdf) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!sdf->built) return lio_fail(LIO_ERR_ARG, "the object holds no field (lio_sdf_build)");
    int rc = lio_check_device(sdf->device_id);
    if (rc != LIO_OK) return rc;
    GcSdfPred pred;
    pred.L = sdf->L;
    pred.V = lio_gc_sdf_visit(sdf->L, decimation);
    pred.nodes = sdf->d_nodes.p;
    pred.lower = lower; pred.upper = upper;
    const long long n = (long long)pred.V.nx * pred.V.ny * pred.V.nz;       // at most LIO_SDF_NODE_LIMIT
    return gc_compact_out<float4>(pred, (int)n, sizeof(float4), points, cap_points, n_out, [](void* p) { return LioCompactStore<float4>{ (float4*)p }; });
} LIO_CATCH

extern "C" int lio_grid_convert_debug_stage_ms(int32_t enable, int32_t use_tiled, float ms[3])
try {
    t_gc_tiled = use_tiled != 0;
    return t_gc.hook(enable, ms);
} LIO_CATCH
