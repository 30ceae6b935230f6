// lio_sdf.hip -- grid_map_sdf on the device: the signed distance field over the elevation grid the height map leaves, and
// the planar signed distance of an occupancy grid.  The arithmetic is lio_sdf.h's; this file is the data movement.
//   k_sdf_stats   the layer's finite minimum and maximum and its non-finite cells (one host wait: they size the field)
//   k_sdf_cols    the first pass of SignedDistance2d.cpp:169-187 for all (column, layer, class) lines of a slab, the layer
//                 initialisation fused in: ONE LANE RUNS ONE LINE's serial sweep, which is what keeps the reference's bits.
//                 Lane t owns line t = column * 2 slab + (layer, class): the lanes of a wave sit on one or a few columns
//                 and read the same elevation words (broadcast).  A lane's results run along its own line, rows * 4 bytes
//                 from its neighbour's: they are staged through an LDS tile of 64 lines x 32 entries and stored transposed,
//                 128 contiguous bytes per line.
//   k_sdf_rows    the second pass on that intermediate ([column][layer, class][row], i.e. already "transposed"): a wave owns
//                 32 adjacent rows of one layer, lanes 0..31 the transform towards obstacles, 32..63 the one towards free
//                 space; loads are two runs of 128 bytes.  The square root is fused into the sweep and the combination of
//                 SignedDistance2d.cpp:250-259 into its end: one shuffle brings the two classes together and lanes 0..31
//                 store 128 contiguous bytes of the distance layer.
//   k_sdf_nodes   the three differences and the packed {distance, dx, dy, dz} nodes in the reference's order
//   k_sdf_query   valueAndDerivative, one lane per position
// The lower-bound stack of a line (pixel index, z_rhs: 8 bytes a bound) lives in a global workspace interleaved by lane.
// conventions, resources, the workspace bound, host waits.  -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <cmath>
#include <string.h>
#include <vector>

#include "lio_sdf.h"
#include "lio_sdfobj.h"
#include "lio_cloud.h"
#include "lio_planning.h"
#include "lio_pool.h"
#include "lio_stageclock.h"
#include "lio_wg.h"

#define SDF_CHUNK 32               // entries of a line staged per flush of k_sdf_cols; the rows a wave of k_sdf_rows owns

namespace {

// ---- accessors ------------------------------------------------------------------------------------------------------------
struct SdfStack {                  // bound k of this lane: (pixel index, bits of z_rhs)
    uint2* p;
    size_t stride;
    __device__ __forceinline__ int v(int k) const { return (int)p[(size_t)k * stride].x; }
    __device__ __forceinline__ float z(int k) const { return __uint_as_float(p[(size_t)k * stride].y); }
    __device__ __forceinline__ void set(int k, int v, float z) { p[(size_t)k * stride] = make_uint2((unsigned)v, __float_as_uint(z)); }
    __device__ __forceinline__ void set_z(int k, float z) { p[(size_t)k * stride].y = __float_as_uint(z); }
};

struct SdfElevLine {               // a column of the elevation layer as the offsets of one (layer, class)
    const float* col;
    float h, inv_res, fill;
    int cls;
    __device__ __forceinline__ float at(int q) const
    {
        float e = col[q];
        if (!lio_gm_finite(e)) e = fill;                           // nan_policy 1 (policy 0 never gets here with such a cell)
        return lio_sdf_init(e, h, inv_res, cls);
    }
};

struct SdfOccLine {                // a column of an occupancy grid
    const signed char* col;
    int occupied_min, cls;
    __device__ __forceinline__ float at(int q) const { return lio_sdf_init_occupancy((int)col[q] >= occupied_min, cls); }
};

struct SdfMidLine {                // a row of the intermediate: entry c at c * pitch
    const float* p;
    size_t pitch;
    __device__ __forceinline__ float at(int q) const { return p[(size_t)q * pitch]; }
};

struct SdfDist {
    const float* p;
    int rows, cols;
    __device__ __forceinline__ float at(int r, int c, int z) const { return p[((size_t)z * (size_t)cols + (size_t)c) * (size_t)rows + (size_t)r]; }
};

struct SdfNodes { const float4* p; __device__ __forceinline__ float4 at(size_t i) const { return p[i]; } };

struct SdfPass {                   // what both sweeps of a slab need
    int rows, cols;
    int z0, slab;                  // the slab's first layer and its layers
    int occupied_min;              // (occupancy)
    float origin_z, res, inv_res;  // float(min_height), float(resolution), 1.0F / that
    float e_min, e_max;            // the layer's extremes
};
// The stack workspace of a slab holds 2 slab cells bounds, used by one pass after the other: the first pass has 2 slab cols
// lines of at most `rows` bounds, the second 2 slab rows lines of at most `cols`.  Bound k of line l lies at k * lines + l.

// ---- the layer's extremes ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sdf_stats(const float* __restrict__ e, size_t n, unsigned* __restrict__ stats)
{
    float mn = INFINITY, mx = -INFINITY;
    int bad = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = e[i];
        if (lio_gm_finite(v)) { mn = fminf(mn, v); mx = fmaxf(mx, v); }
        else ++bad;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off));
        mx = fmaxf(mx, __shfl_xor(mx, off));
        bad += __shfl_xor(bad, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (mn <= mx) { atomicMin(&stats[0], lio_f2ord(mn)); atomicMax(&stats[1], lio_f2ord(mx)); }
        if (bad) atomicAdd(&stats[2], (unsigned)bad);
    }
}

// ---- first pass: columns ------------------------------------------------------------------------------------------------------
// One wave a workgroup.  mid[(col * 2 slab + lk) * rows + row], lk = 2 * (layer - z0) + class.
template <bool OCC>
__global__ __launch_bounds__(64) void k_sdf_cols(SdfPass P, const void* __restrict__ src, float* __restrict__ mid, uint2* __restrict__ stack)
{
    __shared__ float s_tile[64][SDF_CHUNK + 1];
    const int lane = (int)threadIdx.x, nlk = 2 * P.slab;
    const long long n_lines = (long long)P.cols * nlk;
    const long long t = (long long)blockIdx.x * 64 + lane;
    const int c = (int)(t / nlk), lk = (int)(t % nlk), cls = lk & 1;
    const float h = lio_sdf_layer_height(P.origin_z, P.res, P.z0 + (lk >> 1));
    const int mode = OCC ? LIO_SDF_MIXED : lio_sdf_layer_mode(h, P.e_min, P.e_max);
    const bool used = t < n_lines && lio_sdf_mode_uses(mode, cls);
    SdfStack st = { stack + t, (size_t)n_lines };                  // (only a lane with t < n_lines touches it)
    SdfElevLine el = { (const float*)src + (size_t)(used ? c : 0) * (size_t)P.rows, h, P.inv_res, P.e_min, cls };
    SdfOccLine ol = { (const signed char*)src + (size_t)(used ? c : 0) * (size_t)P.rows, P.occupied_min, cls };
    LioSdfCursor<false> cur;
    if (used) {
        if (OCC) cur.begin(ol, P.rows, st); else cur.begin(el, P.rows, st);
    }
    for (int q0 = 0; q0 < P.rows; q0 += SDF_CHUNK) {
        const int m = P.rows - q0 < SDF_CHUNK ? P.rows - q0 : SDF_CHUNK;
        for (int i = 0; i < m; ++i) {
            float v = 0.0f;
            if (used) v = OCC ? cur.at(ol, st, q0 + i) : cur.at(el, st, q0 + i);
            s_tile[lane][i] = v;
        }
        __syncthreads();
        const int i = lane & (SDF_CHUNK - 1);
        for (int j = lane / SDF_CHUNK; j < 64; j += 64 / SDF_CHUNK) {          // line j of the wave, entry i of the chunk
            const long long line = (long long)blockIdx.x * 64 + j;
            if (line < n_lines && i < m) mid[(size_t)line * (size_t)P.rows + (size_t)(q0 + i)] = s_tile[j][i];
        }
        __syncthreads();
    }
}

// ---- second pass: rows ----------------------------------------------------------------------------------------------------------
// dist[(layer * cols + col) * rows + row]; for an occupancy grid one layer, which is the output itself
template <bool OCC>
__global__ __launch_bounds__(256) void k_sdf_rows(SdfPass P, const float* __restrict__ mid, float* __restrict__ dist, uint2* __restrict__ stack)
{
    const int lane = (int)threadIdx.x & 63;
    const int tiles = (P.rows + SDF_CHUNK - 1) / SDF_CHUNK;
    const long long w = (long long)blockIdx.x * 4 + ((int)threadIdx.x >> 6);      // the wave: (layer of the slab, row tile)
    const int zl = (int)(w / tiles), r = (int)(w % tiles) * SDF_CHUNK + (lane & (SDF_CHUNK - 1)), cls = lane / SDF_CHUNK;
    const bool in_grid = zl < P.slab && r < P.rows;
    const float h = lio_sdf_layer_height(P.origin_z, P.res, P.z0 + zl);
    const int mode = OCC ? LIO_SDF_MIXED : lio_sdf_layer_mode(h, P.e_min, P.e_max);         // the same in every lane of the wave
    const bool used = in_grid && lio_sdf_mode_uses(mode, cls);
    SdfStack st = { stack + ((size_t)(2 * zl + cls) * (size_t)P.rows + (size_t)r), (size_t)(2 * P.slab) * (size_t)P.rows };      // (in_grid lanes only)
    const size_t pitch = (size_t)(2 * P.slab) * (size_t)P.rows;
    SdfMidLine ml = { mid + (used ? (size_t)(2 * zl + cls) * (size_t)P.rows + (size_t)r : 0), pitch };
    LioSdfCursor<true> cur;
    if (used) cur.begin(ml, P.cols, st);
    float* out = dist + ((size_t)(P.z0 + zl) * (size_t)P.cols) * (size_t)P.rows + (size_t)r;
    for (int c = 0; c < P.cols; ++c) {
        float v = 0.0f;
        if (used) v = cur.at(ml, st, c);
        const float other = __shfl_xor(v, SDF_CHUNK);                               // every lane of the wave is here
        if (in_grid && cls == LIO_SDF_TO_OBSTACLE) out[(size_t)c * (size_t)P.rows] = lio_sdf_combine(mode, v, other, P.res);
    }
}

// ---- the nodes ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sdf_nodes(SdfDist D, int layers, float res, float4* __restrict__ nodes)
{
    const size_t n = (size_t)D.rows * (size_t)D.cols * (size_t)layers;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = (int)(i % (size_t)D.rows), c = (int)((i / (size_t)D.rows) % (size_t)D.cols), z = (int)(i / ((size_t)D.rows * (size_t)D.cols));
    nodes[i] = lio_sdf_node(D, r, c, z, D.rows, D.cols, layers, res);
}

__global__ __launch_bounds__(256) void k_sdf_query(LioSdfLookup L, const float4* __restrict__ nodes, const double* __restrict__ pos, int n,
                                                   double* __restrict__ value, double* __restrict__ der)
{
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    const double p[3] = { pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2] };
    double d[3];
    const SdfNodes N = { nodes };
    value[i] = lio_sdf_value(L, N, p, d);
    if (der) { der[3 * (size_t)i] = d[0]; der[3 * (size_t)i + 1] = d[1]; der[3 * (size_t)i + 2] = d[2]; }
}

// ---- the host side --------------------------------------------------------------------------------------------------------------
thread_local LioStageTimes<4> t_stage;                     // lio_sdf_build's four stages: the last complete measurement

// the layers of a slab: as many as fit the workspace budget, at most a wave's worth of (layer, class) pairs
int sdf_slab(size_t cells, int layers)
{
    long long s = LIO_SDF_WS_BUDGET / (24LL * (long long)cells);
    if (s > LIO_SDF_MAX_SLAB) s = LIO_SDF_MAX_SLAB;
    if (s > layers) s = layers;
    return s < 1 ? 1 : (int)s;
}

// bounds of the stack workspace for a slab: lines x line length is 2 slab cells in both passes
size_t sdf_stack_bounds(size_t cells, int slab) { return 2 * (size_t)slab * cells; }

// Both sweeps of the layers [z0, z0 + slab) into dist (all layers) on stream s; nothing waits.
template <bool OCC>
void sdf_launch_slab(const SdfPass& P, const void* src, float* mid, float* dist, uint2* stack, hipStream_t s, LioStageClock* clk)
{
    const unsigned b1 = (unsigned)(((size_t)P.cols * 2 * (size_t)P.slab + 63) / 64);
    hipLaunchKernelGGL(k_sdf_cols<OCC>, dim3(b1), dim3(64), 0, s, P, src, mid, stack);
    if (clk) clk->mark(s);
    const unsigned b2 = (unsigned)(((size_t)P.slab * (size_t)((P.rows + SDF_CHUNK - 1) / SDF_CHUNK) + 3) / 4);
    hipLaunchKernelGGL(k_sdf_rows<OCC>, dim3(b2), dim3(256), 0, s, P, (const float*)mid, dist, stack);
    if (clk) clk->mark(s);
}

}  // namespace

// SignedDistanceField's constructor on a device grid; synchronous.  The geometry was checked (lio_sdf_check).
int lio_sdf_build_device(lio_sdf* sdf, const float* d_elev, int rows, int cols, double resolution, const double* length, const double* position,
                         const lio_sdf_config& cfg, lio_sdf_info* info, hipStream_t s)
{
    sdf->built = false;
    memset(info, 0, sizeof(*info));
    info->rows = rows; info->cols = cols; info->resolution = resolution;
    const size_t cells = (size_t)rows * (size_t)cols;
    if (2 * (long long)cells > LIO_SDF_MAX_NODES) return lio_fail(LIO_ERR_CAPACITY, "the field has more than LIO_SDF_NODE_LIMIT nodes (at least 2 layers)");
    LioStageClock clk(t_stage.on);
    clk.mark(s);
    // ---- the layer's extremes: they size the field
    HIPCHK(sdf->d_stats.grow(4));
    unsigned hs[4] = { LIO_ORD_NO_MIN, LIO_ORD_NO_MAX, 0u, 0u };
    HIPCHK(hipMemcpyAsync(sdf->d_stats.p, hs, sizeof(hs), hipMemcpyHostToDevice, s));
    {
        const size_t nb = (cells + 255) / 256;
        hipLaunchKernelGGL(k_sdf_stats, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, s, d_elev, cells, sdf->d_stats.p);
    }
    HIPCHK(hipMemcpyAsync(hs, sdf->d_stats.p, sizeof(hs), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    clk.mark(s);
    info->n_nan = (int32_t)hs[2];
    if (hs[0] == LIO_ORD_NO_MIN) return lio_fail(LIO_ERR_ARG, "the elevation layer has no finite cell");
    const float e_min = lio_ord2f(hs[0]), e_max = lio_ord2f(hs[1]);
    info->layer_min = e_min; info->layer_max = e_max;
    if (hs[2] && cfg.nan_policy == 0) return lio_fail(LIO_ERR_ARG, "the elevation layer has non-finite cells (info.n_nan): inpaint it, or nan_policy = 1");
    const double min_h = std::isnan(cfg.min_height) ? (double)e_min : cfg.min_height;
    const double max_h = std::isnan(cfg.max_height) ? (double)e_max : cfg.max_height;
    if (!std::isfinite(min_h) || !std::isfinite(max_h) || max_h < min_h) return lio_fail(LIO_ERR_ARG, "max_height must not be below min_height, both finite");
    const long long layers = lio_sdf_num_layers(min_h, max_h, resolution);
    LioSdfLookup L;
    L.rows = rows; L.cols = cols; L.layers = (int)(layers < 0x7fffffffLL ? layers : 0x7fffffffLL);
    L.res = resolution;
    for (int a = 0; a < 2; ++a) L.origin[a] = position[a] + (0.5 * length[a] - 0.5 * resolution);      // lio_gm_centre(G, a, 0)
    L.origin[2] = min_h;
    info->layers = L.layers;
    for (int a = 0; a < 3; ++a) info->origin[a] = L.origin[a];
    if ((double)layers * (double)cells > (double)LIO_SDF_MAX_NODES) return lio_fail(LIO_ERR_CAPACITY, "the field has more than LIO_SDF_NODE_LIMIT nodes");
    SdfPass P;
    memset(&P, 0, sizeof(P));
    P.rows = rows; P.cols = cols;
    P.origin_z = (float)min_h; P.res = (float)resolution; P.inv_res = 1.0f / P.res;
    P.e_min = e_min; P.e_max = e_max;
    for (int z = 0; z < L.layers; ++z) {
        const int mode = lio_sdf_layer_mode(lio_sdf_layer_height(P.origin_z, P.res, z), e_min, e_max);
        ++*(mode == LIO_SDF_ALL_OBSTACLE ? &info->n_all_obstacle : mode == LIO_SDF_ALL_FREE ? &info->n_all_free : &info->n_mixed);
    }
    // ---- the field and the workspace: a buffer that is grown out of is freed after a device-wide wait
    const size_t nodes = cells * (size_t)L.layers;
    const int slab = sdf_slab(cells, L.layers);
    HIPCHK(sdf->d_dist.grow(nodes, 1.0, 64, true));
    HIPCHK(sdf->d_nodes.grow(nodes, 1.0, 64, true));
    HIPCHK(sdf->d_mid.grow(cells * 2 * (size_t)slab, 1.0, 64, true));
    HIPCHK(sdf->d_stack.grow(sdf_stack_bounds(cells, slab), 1.0, 64, true));
    clk.mark(s);                                           // (the sweeps' stage starts after the allocations)
    for (int z0 = 0; z0 < L.layers; z0 += slab) {
        P.z0 = z0; P.slab = L.layers - z0 < slab ? L.layers - z0 : slab;
        sdf_launch_slab<false>(P, d_elev, sdf->d_mid.p, sdf->d_dist.p, sdf->d_stack.p, s, &clk);
    }
    {
        const SdfDist D = { sdf->d_dist.p, rows, cols };
        hipLaunchKernelGGL(k_sdf_nodes, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, s, D, L.layers, P.res, sdf->d_nodes.p);
    }
    clk.mark(s);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (clk.count() >= 4) {
        t_stage.ms[0] = clk.ms(0);
        t_stage.ms[1] = t_stage.ms[2] = 0.0f;
        const size_t n_slabs = (clk.count() - 4) / 2;           // marks: start, statistics read, buffers grown, two a slab, end
        for (size_t k = 0; k < n_slabs; ++k) { t_stage.ms[1] += clk.ms(2 + 2 * k); t_stage.ms[2] += clk.ms(3 + 2 * k); }
        t_stage.ms[3] = clk.ms(2 + 2 * n_slabs);
    }
    sdf->L = L;
    sdf->built = true;
    return LIO_OK;
}

int lio_sdf_config_check(const lio_sdf_config* cfg)
{
    if (!cfg) return lio_fail(LIO_ERR_ARG, "null argument");
    if (cfg->nan_policy != 0 && cfg->nan_policy != 1) return lio_fail(LIO_ERR_ARG, "nan_policy is 0 (refuse) or 1 (the smallest finite elevation)");
    if (std::isinf(cfg->min_height) || std::isinf(cfg->max_height)) return lio_fail(LIO_ERR_ARG, "min_height and max_height must be finite or NaN");
    if (cfg->max_height < cfg->min_height) return lio_fail(LIO_ERR_ARG, "max_height must not be below min_height");
    return LIO_OK;
}

int lio_sdf_begin(lio_sdf* sdf, int device_id)
{
    if (device_id != sdf->device_id) return lio_fail(LIO_ERR_ARG, "the keyframe store and the sdf live on different devices");
    sdf->built = false;
    return LIO_OK;
}

int lio_sdf_check(const lio_sdf_config* cfg, int rows, int cols, double resolution, const double length[2], const double position[2])
{
    int rc = lio_sdf_config_check(cfg);
    if (rc != LIO_OK) return rc;
    if (!length || !position) return lio_fail(LIO_ERR_ARG, "null argument");
    if (rows < 2 || cols < 2) return lio_fail(LIO_ERR_ARG, "rows and cols must be at least 2 (the finite differences)");
    if (rows >= LIO_SDF_MAX_LINE || cols >= LIO_SDF_MAX_LINE) return lio_fail(LIO_ERR_ARG, "rows and cols must be below 2^24");
    if (const char* why = lio_gm_resolution_refusal(resolution)) return lio_fail(LIO_ERR_ARG, why);
    if (const char* why = lio_gm_axes_refusal(rows, cols, resolution, length, position)) return lio_fail(LIO_ERR_ARG, why);
    return LIO_OK;
}

extern "C" void lio_sdf_default_config(lio_sdf_config* cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->min_height = cfg->max_height = (double)NAN;       // the layer's own extremes, as the reference's tests call it
    cfg->nan_policy = 0;
}

extern "C" int lio_sdf_create(int32_t device_id, lio_sdf** out)
try {
    if (!out) return lio_fail(LIO_ERR_ARG, "null argument");
    int rc = lio_check_device(device_id);
    if (rc != LIO_OK) return rc;
    lio_sdf* s = new lio_sdf();
    s->device_id = device_id;
    *out = s;
    return LIO_OK;
} LIO_CATCH

extern "C" void lio_sdf_destroy(lio_sdf* sdf)
{
    if (!sdf) return;
    (void)hipSetDevice(sdf->device_id);
    (void)hipDeviceSynchronize();
    delete sdf;
}

extern "C" int lio_sdf_build(lio_sdf* sdf, const float* elevation, int32_t rows, int32_t cols, double resolution, const double* length,
                             const double* position, const lio_sdf_config* cfg, lio_sdf_info* info)
try {
    lio_sdf_info local;
    if (!info) info = &local;
    memset(info, 0, sizeof(*info));
    int rc = lio_sdf_check(cfg, rows, cols, resolution, length, position);
    if (rc != LIO_OK) return rc;
    info->rows = rows; info->cols = cols; info->resolution = resolution;
    if (sdf) sdf->built = false;
    if (2LL * rows * cols > LIO_SDF_MAX_NODES) return lio_fail(LIO_ERR_CAPACITY, "the field has more than LIO_SDF_NODE_LIMIT nodes (at least 2 layers)");
    if (!sdf || !elevation) return lio_fail(LIO_ERR_ARG, "null argument");
    if ((rc = lio_check_device(sdf->device_id)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    const size_t cells = (size_t)rows * (size_t)cols;
    HIPCHK(sdf->d_elev.grow(cells, 1.0, 64, true));
    HIPCHK(hipMemcpyAsync(sdf->d_elev.p, elevation, sizeof(float) * cells, hipMemcpyHostToDevice, s));
    rc = lio_sdf_build_device(sdf, sdf->d_elev.p, rows, cols, resolution, length, position, *cfg, info, s);
    const hipError_t e = hipStreamSynchronize(s);
    if (rc < 0) return rc;
    HIPCHK(e);
    return rc;
} LIO_CATCH

// The height map's chain, then the build on the device grid it leaves: the planning chain (lio_planning.hip) with the field as
// its one stage.  info and hm_info may be NULL.
extern "C" int lio_kf_store_sdf(lio_kf_store* st, const lio_local_map_config* lm, const float* pose, const lio_height_map_config* hm,
                                const lio_sdf_config* cfg, float* grid, size_t grid_cap, lio_sdf* sdf, lio_local_map_info* lm_info,
                                lio_height_map_info* hm_info, lio_sdf_info* info)
try {
    if (!st || !lm || !pose || !hm || !cfg || !sdf) return lio_fail(LIO_ERR_ARG, "null argument");
    return lio_planning_chain(st, lm, pose, hm, { .sdf_cfg = cfg, .sdf = sdf, .out = { .grid = grid, .grid_cap = grid_cap }, .lm_info = lm_info,
                                                  .hm_info = hm_info, .sdf_info = info });
} LIO_CATCH

extern "C" int lio_sdf_nodes(lio_sdf* sdf, float* nodes, size_t cap_floats)
try {
    if (!sdf || !nodes) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!sdf->built) return lio_fail(LIO_ERR_ARG, "the object holds no field (lio_sdf_build)");
    const size_t n = (size_t)sdf->L.rows * (size_t)sdf->L.cols * (size_t)sdf->L.layers;
    if (cap_floats < 4 * n) return lio_fail(LIO_ERR_ARG, "nodes holds fewer than 4 x rows x cols x layers floats");
    int rc = lio_check_device(sdf->device_id);
    if (rc != LIO_OK) return rc;
    HIPCHK(hipMemcpy(nodes, sdf->d_nodes.p, sizeof(float4) * n, hipMemcpyDeviceToHost));
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_sdf_query(lio_sdf* sdf, const double* positions, size_t n, double* value, double* derivative)
try {
    if (!sdf || (n && (!positions || !value))) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!sdf->built) return lio_fail(LIO_ERR_ARG, "the object holds no field (lio_sdf_build)");
    if (n > 0x7fffffffull / 4) return lio_fail(LIO_ERR_CAPACITY, "too many positions");
    if (n == 0) return LIO_OK;
    int rc = lio_check_device(sdf->device_id);
    if (rc != LIO_OK) return rc;
    hipStream_t s = nullptr;
    LioTemp pos, val, der;
    HIPCHK(pos.alloc(sizeof(double) * 3 * n));
    HIPCHK(val.alloc(sizeof(double) * n));
    if (derivative) HIPCHK(der.alloc(sizeof(double) * 3 * n));
    HIPCHK(hipMemcpyAsync(pos.p, positions, sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_sdf_query, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, sdf->L, (const float4*)sdf->d_nodes.p, (const double*)pos.p, (int)n,
                       val.as<double>(), derivative ? der.as<double>() : nullptr);
    HIPCHK(hipMemcpyAsync(value, val.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    if (derivative) HIPCHK(hipMemcpyAsync(derivative, der.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
    const hipError_t e = hipStreamSynchronize(s);          // (the temporaries go back to the pool after it)
    HIPCHK(e);
    HIPCHK(hipGetLastError());
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_occupancy_sdf(int32_t device_id, const int8_t* grid, int32_t width, int32_t height, float resolution, int32_t occupied_min,
                                 float* out)
try {
    if (!grid || !out) return lio_fail(LIO_ERR_ARG, "null argument");
    if (width < 1 || height < 1 || width >= LIO_SDF_MAX_LINE || height >= LIO_SDF_MAX_LINE) return lio_fail(LIO_ERR_ARG, "width and height must be in [1, 2^24)");
    if ((long long)width * height > 0x7fffffffLL - 1024) return lio_fail(LIO_ERR_ARG, "the grid has more than 2^31 - 1 cells");
    if (!std::isfinite(resolution) || resolution < 1e-4f) return lio_fail(LIO_ERR_ARG, "resolution must be finite and at least 1e-4");
    // signedDistanceFromOccupancy :272-287: the two grids that have no transform
    const size_t cells = (size_t)width * (size_t)height;
    size_t n_obstacle = 0;
    for (size_t i = 0; i < cells; ++i) n_obstacle += (int)grid[i] >= occupied_min ? 1 : 0;
    if (n_obstacle == 0 || n_obstacle == cells) {
        const float v = n_obstacle == 0 ? INFINITY : -INFINITY;
        for (size_t i = 0; i < cells; ++i) out[i] = v;
        return LIO_OK;
    }
    int rc = lio_check_device(device_id);
    if (rc != LIO_OK) return rc;
    hipStream_t s = nullptr;
    SdfPass P;
    memset(&P, 0, sizeof(P));
    P.rows = width; P.cols = height;                       // the message read as the column-major width x height matrix
    P.z0 = 0; P.slab = 1;
    P.occupied_min = occupied_min;
    P.res = resolution;
    LioTemp d_grid, d_mid, d_out, d_stack;
    HIPCHK(d_grid.alloc(cells));
    HIPCHK(d_mid.alloc(sizeof(float) * 2 * cells));
    HIPCHK(d_out.alloc(sizeof(float) * cells));
    HIPCHK(d_stack.alloc(sizeof(uint2) * sdf_stack_bounds(cells, 1)));
    HIPCHK(hipMemcpyAsync(d_grid.p, grid, cells, hipMemcpyHostToDevice, s));
    sdf_launch_slab<true>(P, d_grid.p, d_mid.as<float>(), d_out.as<float>(), d_stack.as<uint2>(), s, nullptr);
    HIPCHK(hipMemcpyAsync(out, d_out.p, sizeof(float) * cells, hipMemcpyDeviceToHost, s));
    const hipError_t e = hipStreamSynchronize(s);
    HIPCHK(e);
    HIPCHK(hipGetLastError());
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_sdf_memory(lio_sdf* sdf, size_t* field_bytes, size_t* workspace_bytes)
try {
    if (!sdf) return lio_fail(LIO_ERR_ARG, "null argument");
    if (field_bytes) *field_bytes = sdf->d_nodes.cap * sizeof(float4) + sdf->d_dist.cap * sizeof(float);
    if (workspace_bytes) *workspace_bytes = sdf->d_mid.cap * sizeof(float) + sdf->d_stack.cap * sizeof(uint2);
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_sdf_debug_stage_ms(int32_t enable, float ms[4])
try {
    return t_stage.hook(enable, ms);
} LIO_CATCH
