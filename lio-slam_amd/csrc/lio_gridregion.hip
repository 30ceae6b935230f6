// lio_gridregion.hip -- grid_map's region iterators (line, circle, ellipse, polygon) on the resident layer set: the cells of
// many regions, and per layer the reduction over them that a planner would loop for.  The arithmetic is lio_gridregion.h's;
// this file is the work mapping and the data movement.
//   k_rg_plan     two lanes per region: lane e forms axis e of an area kind's window, or walks endpoint e of a line into
//                 the map (a serial fp64 accumulation, up to LIO_REGION_MAX_WALK steps); the pair meets through one shuffle
//                 and the even lane writes the 48-byte plan.
//   k_rg_reduce   one wave per region, four a workgroup.  A polygon's vertices are staged in the wave's 1 KiB of LDS.  The
//                 wave sweeps the window column-major, lane = number mod 64: rows are the contiguous axis of the layers, so
//                 a window at least 16 rows high reads whole cache lines.  Membership is tested once per cell and group of
//                 four layers (the accumulators of four layers stay in registers); the gather of a layer is a plain global
//                 load (a 550 x 400 layer is 0.88 MB and stays in L2).  Lane p holds partial sum p of lio_gridregion.h's
//                 order; the tree is five shuffles.  A window is never split over waves: one that covers a large map is
//                 swept by a single wave (DESIGN.md section 4l gives the measured cost).
//   k_rg_cells    one wave per region, in the iterator's order, 64 slots a step: COUNT the members by ballot; after the
//                 exclusive scan over the regions (lio_scan2.h) WRITE them, each at the offset of its region plus the ballot's
//                 prefix below its lane.  No atomic decides a position.
//   k_rg_info     the call's counts from the status bytes and the cell counts, four atomics a wave of at most 256.
// No MFMA: there is no dense contraction here.  DESIGN.md section 4l: conventions, deviations, host waits.  -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <cmath>
#include <string.h>
#include <vector>

#include "lio_gridregion.h"
#include "lio_gridobj.h"
#include "lio_cloud.h"
#include "lio_pool.h"
#include "lio_scan2.h"

namespace {

#define RG_WAVES 4                 // regions a workgroup
#define RG_LCH 4                   // layers a sweep
#define RG_MAX_REGIONS ((size_t)1 << 24)

struct RgLayers { const float* p[LIO_GRID_MAX_LAYERS]; };          // the requested layers, in the caller's order

enum { RG_CNT_OK = 0, RG_CNT_EMPTY, RG_CNT_INVALID, RG_CNT_CELLS, RG_N_CNT };

__global__ __launch_bounds__(256) void k_rg_plan(LioGridGeom G, const LioRgRegion* __restrict__ regions, const double* __restrict__ verts, int n,
                                                 LioRgPlan* __restrict__ plans)
{
    const int gid = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int q = gid >> 1, e = gid & 1;
    const bool live = q < n;
    int s = LIO_REGION_INVALID, lo = 0, hi = 0;
    LioRgRegion R;
    R.kind = LIO_REGION_CIRCLE;
    if (live) {
        R = regions[q];
        s = lio_rg_plan_half(G, R, verts, e, &lo, &hi);
    }
    const int s1 = __shfl_xor(s, 1), lo1 = __shfl_xor(lo, 1), hi1 = __shfl_xor(hi, 1);
    if (live && e == 0) {
        LioRgPlan P;
        lio_rg_plan_join(R, s, lo, hi, s1, lo1, hi1, &P);
        plans[q] = P;
    }
}

// the region of this wave: its plan, its record, a polygon's vertices -> the wave's LDS.  Ends with the barrier.
__device__ __forceinline__ bool rg_stage(const LioRgRegion* __restrict__ regions, const double* __restrict__ verts, const LioRgPlan* __restrict__ plans,
                                         int n, double (*s_v)[2 * LIO_REGION_MAX_VERTICES], int* q_out, LioRgRegion* R, LioRgPlan* P)
{
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int q = (int)blockIdx.x * RG_WAVES + wave;
    const bool live = q < n;
    P->status = LIO_REGION_INVALID;
    R->kind = LIO_REGION_CIRCLE; R->n_vertices = 0;
    if (live) { *P = plans[q]; *R = regions[q]; }
    if (live && R->kind == LIO_REGION_POLYGON && P->status == LIO_REGION_OK) {
        const int nd = 2 * (R->n_vertices < LIO_REGION_MAX_VERTICES ? R->n_vertices : LIO_REGION_MAX_VERTICES);
        for (int k = lane; k < nd; k += 64) s_v[wave][k] = verts[2 * R->first_vertex + k];
    }
    __syncthreads();
    *q_out = q;
    return live;
}

// The call's counters from the regions' status bytes and cell counts: a grid-stride sum, one wave's shuffles, four atomics a
// wave (the kernels that write the status do not count: 10^5 atomics on one address cost more than their sweeps).
#define RG_INFO_BLOCKS 64
__global__ __launch_bounds__(256) void k_rg_info(const unsigned char* __restrict__ status, const int* __restrict__ n_cells, int n,
                                                 unsigned long long* __restrict__ counters)
{
    unsigned long long c[RG_N_CNT] = { 0ull, 0ull, 0ull, 0ull };
    for (int q = (int)blockIdx.x * 256 + (int)threadIdx.x; q < n; q += (int)gridDim.x * 256) {
        const int st = status[q];
        c[st == LIO_REGION_OK ? RG_CNT_OK : (st == LIO_REGION_EMPTY ? RG_CNT_EMPTY : RG_CNT_INVALID)] += 1ull;
        c[RG_CNT_CELLS] += (unsigned long long)n_cells[q];
    }
#pragma unroll
    for (int m = 0; m < RG_N_CNT; ++m) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) c[m] += __shfl_down(c[m], s);
        if ((threadIdx.x & 63) == 0 && c[m]) atomicAdd(&counters[m], c[m]);
    }
}

__global__ __launch_bounds__(256) void k_rg_reduce(LioGridGeom G, RgLayers L, int n_layers, float threshold, const LioRgRegion* __restrict__ regions,
                                                   const double* __restrict__ verts, const LioRgPlan* __restrict__ plans, int n,
                                                   lio_grid_region_stat* __restrict__ stats, int* __restrict__ n_cells, unsigned char* __restrict__ status)
{
    __shared__ double s_v[RG_WAVES][2 * LIO_REGION_MAX_VERTICES];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    int q;
    LioRgRegion R;
    LioRgPlan P;
    if (!rg_stage(regions, verts, plans, n, s_v, &q, &R, &P)) return;
    const int slots = lio_rg_n_slots(P);
    int members = 0;
    for (int k0 = 0; k0 < n_layers; k0 += RG_LCH) {
        LioRgAcc acc[RG_LCH];
#pragma unroll
        for (int j = 0; j < RG_LCH; ++j) lio_rg_acc_clear(&acc[j]);
        int cnt = 0;
        for (int rank = lane; rank < slots; rank += 64) {
            int r, c;
            lio_rg_cell_by_rank(P, rank, &r, &c);
            // (a plan's cells lie in the grid by construction; the test keeps a wrong plan from reading outside it)
            if ((unsigned)r >= (unsigned)G.rows || (unsigned)c >= (unsigned)G.cols) continue;
            if (!lio_rg_member(G, R, s_v[wave], r, c)) continue;
            ++cnt;
            const size_t at = (size_t)r + (size_t)c * (size_t)G.rows;
#pragma unroll
            for (int j = 0; j < RG_LCH; ++j)
                if (k0 + j < n_layers) lio_rg_acc_add(&acc[j], L.p[k0 + j][at], threshold);
        }
#pragma unroll
        for (int j = 0; j < RG_LCH; ++j) {
            if (k0 + j >= n_layers) continue;
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {             // part[k] += part[k + s], k < s (the lanes above hold no result)
                LioRgAcc b;
                b.sum = __shfl_down(acc[j].sum, s);
                b.mn = __shfl_down(acc[j].mn, s);
                b.mx = __shfl_down(acc[j].mx, s);
                b.n_finite = __shfl_down(acc[j].n_finite, s);
                b.n_below = __shfl_down(acc[j].n_below, s);
                lio_rg_acc_fold(&acc[j], b);
            }
            if (lane == 0) {
                lio_grid_region_stat o;
                lio_rg_acc_store(acc[j], &o);
                stats[(size_t)(k0 + j) * (size_t)n + (size_t)q] = o;
            }
        }
        if (k0 == 0) {
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) cnt += __shfl_down(cnt, s);
            members = cnt;
        }
    }
    if (lane == 0) {
        const int st = P.status == LIO_REGION_OK && members == 0 ? LIO_REGION_EMPTY : P.status;
        n_cells[q] = members;
        status[q] = (unsigned char)st;
    }
}

// WRITE false: counts[q] = the members, and the status.  WRITE true (after k_rg_info): the cells at offs[q], unless the call's
// total does not fit `cap` (nothing is written then).
template <bool WRITE>
__global__ __launch_bounds__(256) void k_rg_cells(LioGridGeom G, const LioRgRegion* __restrict__ regions, const double* __restrict__ verts,
                                                  const LioRgPlan* __restrict__ plans, int n, int* __restrict__ counts, unsigned char* __restrict__ status,
                                                  const unsigned long long* __restrict__ counters, const int* __restrict__ offs, int* __restrict__ cells,
                                                  unsigned long long cap)
{
    __shared__ double s_v[RG_WAVES][2 * LIO_REGION_MAX_VERTICES];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    int q;
    LioRgRegion R;
    LioRgPlan P;
    if (!rg_stage(regions, verts, plans, n, s_v, &q, &R, &P)) return;
    if (WRITE && counters[RG_CNT_CELLS] > cap) return;
    const int slots = lio_rg_n_slots(P);
    const long long base = WRITE ? (long long)offs[q] : 0;
    int run = 0;
    for (int t0 = 0; t0 < slots; t0 += 64) {
        const int t = t0 + lane;
        int r = 0, c = 0;
        bool m = false;
        if (t < slots) {
            lio_rg_cell_by_order(P, t, &r, &c);
            m = (unsigned)r < (unsigned)G.rows && (unsigned)c < (unsigned)G.cols && lio_rg_member(G, R, s_v[wave], r, c);
        }
        const unsigned long long b = __ballot(m);
        if (WRITE && m) {
            const long long at = base + run + (long long)__popcll(b & ((1ull << lane) - 1ull));
            if (at >= 0 && (unsigned long long)at < cap) cells[at] = c * G.rows + r;
        }
        run += (int)__popcll(b);
    }
    if (!WRITE && lane == 0) {
        const int st = P.status == LIO_REGION_OK && run == 0 ? LIO_REGION_EMPTY : P.status;
        counts[q] = run;
        status[q] = (unsigned char)st;
    }
}

thread_local LioStageTimes<4> t_rg;                        // five marks around the four stages of lio_grid_region_reduce

// What both entry points refuse before the object or a device is looked at, and the regions as the device reads them.
int rg_pack(const lio_grid_region* regions, size_t n, const double* vertices, size_t n_vertices, std::vector<LioRgRegion>& out)
{
    if (n > RG_MAX_REGIONS) return lio_fail(LIO_ERR_CAPACITY, "more than 2^24 regions in one call");
    if (n && !regions) return lio_fail(LIO_ERR_ARG, "null argument");
    out.resize(n);
    for (size_t q = 0; q < n; ++q) {
        const lio_grid_region& r = regions[q];
        LioRgRegion& o = out[q];
        if (r.kind < LIO_REGION_LINE || r.kind > LIO_REGION_POLYGON) return lio_fail(LIO_ERR_ARG, "a region's kind is 0 (line), 1 (circle), 2 (ellipse) or 3 (polygon)");
        lio_rg_pack(r, &o);
        if (r.kind == LIO_REGION_POLYGON) {
            if (r.n_vertices < 3 || r.n_vertices > LIO_REGION_MAX_VERTICES) return lio_fail(LIO_ERR_ARG, "a polygon has 3 .. LIO_REGION_MAX_VERTICES vertices");
            if (!vertices) return lio_fail(LIO_ERR_ARG, "null argument (vertices)");
            if (r.first_vertex < 0 || (unsigned long long)r.first_vertex > n_vertices || (size_t)r.n_vertices > n_vertices - (size_t)r.first_vertex)
                return lio_fail(LIO_ERR_ARG, "a polygon's vertices leave the vertex array");
        }
    }
    return LIO_OK;
}

size_t rg_up8(size_t v) { return (v + 7) & ~(size_t)7; }

unsigned rg_info_blocks(size_t n) { const size_t b = (n + 255) / 256; return (unsigned)(b < RG_INFO_BLOCKS ? b : RG_INFO_BLOCKS); }

// regions and vertices up, the counters cleared, the plans made: on stream s, nothing waited for
int rg_upload_and_plan(lio_grid* g, const std::vector<LioRgRegion>& packed, const double* vertices, size_t n_vertices, size_t small_bytes, hipStream_t s,
                       LioStageClock& clk)
{
    const size_t n = packed.size();
    LioDevBytes* B = g->d_region;
    HIPCHK(B[LIO_RG_BUF_REGIONS].alloc(sizeof(LioRgRegion) * n));
    HIPCHK(B[LIO_RG_BUF_VERTICES].alloc(sizeof(double) * 2 * n_vertices));
    HIPCHK(B[LIO_RG_BUF_PLANS].alloc(sizeof(LioRgPlan) * n));
    HIPCHK(B[LIO_RG_BUF_SMALL].alloc(small_bytes));
    clk.mark(s);
    HIPCHK(hipMemcpyAsync(B[LIO_RG_BUF_REGIONS].p, packed.data(), sizeof(LioRgRegion) * n, hipMemcpyHostToDevice, s));
    if (n_vertices && vertices) HIPCHK(hipMemcpyAsync(B[LIO_RG_BUF_VERTICES].p, vertices, sizeof(double) * 2 * n_vertices, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(B[LIO_RG_BUF_SMALL].p, 0, 64, s));
    clk.mark(s);
    hipLaunchKernelGGL(k_rg_plan, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, s, g->G, B[LIO_RG_BUF_REGIONS].as<LioRgRegion>(),
                       B[LIO_RG_BUF_VERTICES].as<double>(), (int)n, B[LIO_RG_BUF_PLANS].as<LioRgPlan>());
    clk.mark(s);
    return LIO_OK;
}

void rg_fill_info(lio_grid_region_info* info, const unsigned long long hc[RG_N_CNT])
{
    if (!info) return;
    info->n_ok = (int64_t)hc[RG_CNT_OK]; info->n_empty = (int64_t)hc[RG_CNT_EMPTY];
    info->n_invalid = (int64_t)hc[RG_CNT_INVALID]; info->n_cells = (int64_t)hc[RG_CNT_CELLS];
}

}  // namespace

extern "C" void lio_grid_region_default_config(lio_grid_region_config* cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->threshold = 0.5f;         // the middle of traversability's [0, 1]
}

extern "C" int lio_grid_region_reduce(lio_grid* g, const int32_t* layer_ids, int32_t n_layers, const lio_grid_region_config* cfg, const lio_grid_region* regions,
                                      size_t n, const double* vertices, size_t n_vertices, lio_grid_region_stat* stats, int32_t* n_cells, uint8_t* status,
                                      lio_grid_region_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    if (!layer_ids || !cfg || (n && (!regions || !stats))) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!std::isfinite(cfg->threshold)) return lio_fail(LIO_ERR_ARG, "threshold must be finite");
    if (n_layers < 1 || n_layers > LIO_GRID_MAX_LAYERS) return lio_fail(LIO_ERR_ARG, "n_layers must be in [1, LIO_GRID_MAX_LAYERS]");
    unsigned listed = 0;
    int rc = lio_grid_layer_list(layer_ids, n_layers, &listed);
    if (rc != LIO_OK) return rc;
    std::vector<LioRgRegion> packed;
    if ((rc = rg_pack(regions, n, vertices, n_vertices, packed)) != LIO_OK) return rc;
    if (!g) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!g->mask) return lio_fail(LIO_ERR_ARG, "the object holds no layers (lio_grid_set_layers, lio_kf_store_planning_grid)");
    if (listed & ~g->mask) return lio_fail(LIO_ERR_ARG, "a layer id names a layer the object does not hold");
    if (n == 0) return LIO_OK;
    RgLayers L;
    memset(&L, 0, sizeof(L));
    for (int k = 0; k < n_layers; ++k) L.p[k] = g->d_layer[layer_ids[k]].p;
    if ((rc = lio_check_device(g->device_id)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    LioDevBytes* B = g->d_region;
    const size_t pairs = (size_t)n_layers * n;
    const size_t off_cells = 64, off_status = off_cells + rg_up8(sizeof(int) * n);
    HIPCHK(B[LIO_RG_BUF_STATS].alloc(sizeof(lio_grid_region_stat) * pairs));
    LioStageClock clk(t_rg.on);
    if ((rc = rg_upload_and_plan(g, packed, vertices, n_vertices, off_status + n, s, clk)) != LIO_OK) return rc;
    unsigned char* small = B[LIO_RG_BUF_SMALL].p;
    hipLaunchKernelGGL(k_rg_reduce, dim3((unsigned)((n + RG_WAVES - 1) / RG_WAVES)), dim3(64 * RG_WAVES), 0, s, g->G, L, n_layers, cfg->threshold,
                       B[LIO_RG_BUF_REGIONS].as<LioRgRegion>(), B[LIO_RG_BUF_VERTICES].as<double>(), B[LIO_RG_BUF_PLANS].as<LioRgPlan>(), (int)n,
                       B[LIO_RG_BUF_STATS].as<lio_grid_region_stat>(), (int*)(small + off_cells), small + off_status);
    hipLaunchKernelGGL(k_rg_info, dim3(rg_info_blocks(n)), dim3(256), 0, s, small + off_status, (const int*)(small + off_cells), (int)n,
                       (unsigned long long*)small);
    clk.mark(s);
    unsigned long long hc[RG_N_CNT] = { 0, 0, 0, 0 };
    HIPCHK(hipMemcpyAsync(stats, B[LIO_RG_BUF_STATS].p, sizeof(lio_grid_region_stat) * pairs, hipMemcpyDeviceToHost, s));
    if (n_cells) HIPCHK(hipMemcpyAsync(n_cells, small + off_cells, sizeof(int) * n, hipMemcpyDeviceToHost, s));
    if (status) HIPCHK(hipMemcpyAsync(status, small + off_status, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hc, small, sizeof(hc), hipMemcpyDeviceToHost, s));
    clk.mark(s);
    HIPCHK(hipStreamSynchronize(s));                       // the call's one host wait
    HIPCHK(hipGetLastError());
    rg_fill_info(info, hc);
    t_rg.read(clk);
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_region_cells(lio_grid* g, const lio_grid_region* regions, size_t n, const double* vertices, size_t n_vertices, int64_t* offsets,
                                     int32_t* cells, size_t cap_cells, uint8_t* status, lio_grid_region_info* info)
try {
    if (info) memset(info, 0, sizeof(*info));
    if (!offsets || (cap_cells && !cells)) return lio_fail(LIO_ERR_ARG, "null argument");
    std::vector<LioRgRegion> packed;
    int rc = rg_pack(regions, n, vertices, n_vertices, packed);
    if (rc != LIO_OK) return rc;
    if (!g) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!g->mask) return lio_fail(LIO_ERR_ARG, "the object holds no layers (lio_grid_set_layers, lio_kf_store_planning_grid)");
    offsets[0] = 0;
    if (n == 0) return LIO_OK;
    if ((rc = lio_check_device(g->device_id)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    LioDevBytes* B = g->d_region;
    // no call holds more cells than every region covering the whole grid, nor than the int offsets of the scan can count
    const unsigned long long most = (unsigned long long)n * (unsigned long long)g->G.rows * (unsigned long long)g->G.cols;
    unsigned long long cap = cap_cells < most ? cap_cells : most;
    if (cap > 0x7fffffffull) cap = 0x7fffffffull;
    const size_t n_tiles = (n + LIO_S2_TILE - 1) / LIO_S2_TILE + 1;
    const size_t off_offs = rg_up8(sizeof(int) * n), off_occ = off_offs + rg_up8(sizeof(int) * (n + 1));
    const size_t off_tiles = off_occ + rg_up8(sizeof(int) * (n + 1));
    HIPCHK(B[LIO_RG_BUF_SCAN].alloc(off_tiles + sizeof(unsigned long long) * n_tiles));
    HIPCHK(B[LIO_RG_BUF_CELLS].alloc(sizeof(int) * (size_t)cap));
    LioStageClock clk(false);                              // (off: the stage times are lio_grid_region_reduce's)
    if ((rc = rg_upload_and_plan(g, packed, vertices, n_vertices, 64 + n, s, clk)) != LIO_OK) return rc;
    unsigned char* small = B[LIO_RG_BUF_SMALL].p;
    unsigned char* scan = B[LIO_RG_BUF_SCAN].p;
    int* d_counts = (int*)scan;
    int* d_offs = (int*)(scan + off_offs);
    const dim3 grid((unsigned)((n + RG_WAVES - 1) / RG_WAVES)), block(64 * RG_WAVES);
    hipLaunchKernelGGL(k_rg_cells<false>, grid, block, 0, s, g->G, B[LIO_RG_BUF_REGIONS].as<LioRgRegion>(), B[LIO_RG_BUF_VERTICES].as<double>(),
                       B[LIO_RG_BUF_PLANS].as<LioRgPlan>(), (int)n, d_counts, small + 64, (const unsigned long long*)small, (const int*)nullptr, (int*)nullptr,
                       0ull);
    hipLaunchKernelGGL(k_rg_info, dim3(rg_info_blocks(n)), dim3(256), 0, s, small + 64, (const int*)d_counts, (int)n, (unsigned long long*)small);
    lio_launch_scan2<true>(d_counts, nullptr, (int)n, (unsigned long long*)(scan + off_tiles), d_offs, (int*)(scan + off_occ), s);
    hipLaunchKernelGGL(k_rg_cells<true>, grid, block, 0, s, g->G, B[LIO_RG_BUF_REGIONS].as<LioRgRegion>(), B[LIO_RG_BUF_VERTICES].as<double>(),
                       B[LIO_RG_BUF_PLANS].as<LioRgPlan>(), (int)n, d_counts, small + 64, (const unsigned long long*)small, (const int*)d_offs,
                       B[LIO_RG_BUF_CELLS].as<int>(), cap);
    std::vector<int> counts(n);
    unsigned long long hc[RG_N_CNT] = { 0, 0, 0, 0 };
    HIPCHK(hipMemcpyAsync(counts.data(), d_counts, sizeof(int) * n, hipMemcpyDeviceToHost, s));
    if (status) HIPCHK(hipMemcpyAsync(status, small + 64, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hc, small, sizeof(hc), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));                       // the sizes: the first of this call's two host waits
    HIPCHK(hipGetLastError());
    rg_fill_info(info, hc);
    for (size_t q = 0; q < n; ++q) offsets[q + 1] = offsets[q] + (int64_t)counts[q];
    const unsigned long long total = (unsigned long long)offsets[n];
    if (total != hc[RG_CNT_CELLS]) return lio_fail(LIO_ERR_HIP, "the regions' counts and their sum disagree");
    if (total > 0x7fffffffull) return lio_fail(LIO_ERR_CAPACITY, "more than 2^31 - 1 cells in one call");
    if (total > cap_cells) return lio_fail(LIO_ERR_CAPACITY, "cap_cells is smaller than the regions' cells: offsets[n] tells the need");
    if (total) HIPCHK(hipMemcpy(cells, B[LIO_RG_BUF_CELLS].p, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost));   // the cells: the second
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_grid_region_debug_stage_ms(int32_t enable, float ms[4])
try {
    return t_rg.hook(enable, ms);
} LIO_CATCH
