// lio_sc.hip -- Scan Context loop detection: SCManager (Scancontext.cpp = SC) restated for the device.  DESIGN.md section
// 4c lists what is defined here because Eigen and nanoflann are not functions of their inputs there (parity unpinned).
//   k_sc_fold      makeScancontext SC:151-184, streaming: every workgroup folds its points into the cells in LDS (order-mapped
//                  words, atomic max), then merges the cells it touched into the descriptor's table, one global atomic max
//                  each.  A maximum does not depend on the order: the table is the same for every grid size.
//   k_sc_finish    SC:186-190 + the ring key SC:198-211 (as float, SC:241) + the sector key SC:214-227; one workgroup
//   k_sc_ring_topk the num_candidates nearest ring keys of the prefix, exact, ordered by (fp32 squared distance, index)
//   k_sc_distance  distanceBtnScanContext SC:116-148, one workgroup per candidate: both descriptors, their sector keys and
//                  column norms in LDS; fp64, every sum in ascending index order
// -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <cmath>
#include <string.h>
#include <utility>

#include "lio_sc.h"
#include "lio_handle.h"
#include "lio_kfstore.h"
#include "lio_wg.h"

#define SC_NO_POINT (-1000.0f)   // SC:158
#define SC_FOLD_PTS 2048         // points per workgroup of k_sc_fold (8 per thread), up to SC_FOLD_MAX_WG workgroups
#define SC_FOLD_MAX_WG 256

struct LioScGeom { int rings, sectors; double max_radius, lidar_height; };

// what one detection leaves on the device: the candidate arrays of lio_sc_result
struct LioScCand {
    int32_t idx[LIO_SC_MAX_CANDIDATES];
    float d2[LIO_SC_MAX_CANDIDATES];
    double dist[LIO_SC_MAX_CANDIDATES];
    int32_t align[LIO_SC_MAX_CANDIDATES];
};

// xy2theta SC:23-36: the quotient and atan in fp32, the rest in fp64, rounded to float once
__device__ __forceinline__ float sc_theta(float x, float y)
{
    const double k = 180.0 / M_PI;
    if (x >= 0.0f && y >= 0.0f) return (float)(k * (double)atanf(__fdiv_rn(y, x)));
    if (x < 0.0f && y >= 0.0f) return (float)(180.0 - k * (double)atanf(__fdiv_rn(y, -x)));
    if (x < 0.0f && y < 0.0f) return (float)(180.0 + k * (double)atanf(__fdiv_rn(y, x)));
    return (float)(360.0 - k * (double)atanf(__fdiv_rn(-y, x)));
}

__global__ __launch_bounds__(256) void k_sc_fold(const unsigned char* __restrict__ rec, size_t stride, size_t xyz_off, int n, LioScGeom g,
                                                 unsigned* __restrict__ table)
{
    __shared__ unsigned s_cell[LIO_SC_MAX_CELLS];
    const int cells = g.rings * g.sectors;                             // (<= LIO_SC_MAX_CELLS: lio_sc_check_config)
    const unsigned empty = lio_f2ord(SC_NO_POINT);
    for (int c = threadIdx.x; c < cells; c += 256) s_cell[c] = empty;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float* p = reinterpret_cast<const float*>(rec + (size_t)i * stride + xyz_off);
        const float x = p[0], y = p[1], z = p[2];
        if (!(fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX)) continue;
        if (x == 0.0f && y == 0.0f) continue;                          // (the reference's xy2theta has no value here)
        const float range = __fsqrt_rn(x * x + y * y);
        if ((double)range > g.max_radius) continue;                    // SC:175
        const float angle = sc_theta(x, y);
        const int ring = max(min(g.rings, (int)ceil((double)range / g.max_radius * (double)g.rings)), 1);
        const int sector = max(min(g.sectors, (int)ceil((double)angle / 360.0 * (double)g.sectors)), 1);
        const float zf = (float)((double)z + g.lidar_height);
        atomicMax(&s_cell[(ring - 1) * g.sectors + (sector - 1)], lio_f2ord(zf));
    }
    __syncthreads();
    for (int c = threadIdx.x; c < cells; c += 256) {
        const unsigned v = s_cell[c];
        if (v != empty) atomicMax(&table[c], v);
    }
}

__global__ __launch_bounds__(256) void k_sc_finish(const unsigned* __restrict__ table, int rings, int sectors, float* __restrict__ desc,
                                                   float* __restrict__ rkey, double* __restrict__ skey)
{
    __shared__ float s_d[LIO_SC_MAX_CELLS];
    const int cells = rings * sectors, t = threadIdx.x;
    for (int c = t; c < cells; c += 256) {
        float f = lio_ord2f(table[c]);
        if (f == SC_NO_POINT) f = 0.0f;                                // SC:187-190
        s_d[c] = f;
        desc[c] = f;
    }
    __syncthreads();
    if (t < rings) {                                                   // (rings, sectors <= 256 = the workgroup)
        double sum = 0.0;
        for (int j = 0; j < sectors; ++j) sum += (double)s_d[t * sectors + j];
        rkey[t] = (float)(sum / (double)sectors);
    }
    if (t < sectors) {
        double sum = 0.0;
        for (int r = 0; r < rings; ++r) sum += (double)s_d[r * sectors + t];
        skey[t] = sum / (double)rings;
    }
}

// One workgroup.  keys[i] = (bits of the fp32 squared distance << 32) | i: a non-negative float orders as its bits, so the
// k-th smallest key is the k-th candidate in (distance, index) order.  Every thread reads back only the keys it wrote.
__global__ __launch_bounds__(256) void k_sc_ring_topk(const float* __restrict__ rkey, int rings, int prefix, int query, int k_want,
                                                      unsigned long long* __restrict__ keys, LioScCand* __restrict__ out)
{
    __shared__ float s_q[LIO_SC_MAX_DIM];
    __shared__ unsigned long long s_w[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t < rings) s_q[t] = rkey[(size_t)query * rings + t];
    __syncthreads();
    for (int i = t; i < prefix; i += 256) {
        const float* c = rkey + (size_t)i * rings;
        float d2 = 0.0f;
        for (int d = 0; d < rings; ++d) { const float e = s_q[d] - c[d]; d2 += e * e; }
        keys[i] = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)i;
    }
    unsigned long long lo = 0ull;                                      // the next candidate is the smallest key >= lo
    for (int k = 0; k < k_want; ++k) {
        unsigned long long best = ~0ull;
        for (int i = t; i < prefix; i += 256) { const unsigned long long v = keys[i]; if (v >= lo && v < best) best = v; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(best, off); best = o < best ? o : best; }
        if (lane == 0) s_w[wave] = best;
        __syncthreads();
        best = s_w[0];
        for (int w = 1; w < 4; ++w) best = s_w[w] < best ? s_w[w] : best;
        __syncthreads();
        if (t == 0) { out->idx[k] = (int)(unsigned)best; out->d2[k] = __uint_as_float((unsigned)(best >> 32)); }
        lo = best + 1ull;
    }
}

// Workgroup b: the query `a` against descriptor cand[b] of `base` (cand == NULL: descriptor `fixed`).
__global__ __launch_bounds__(256) void k_sc_distance(const float* __restrict__ a, const float* __restrict__ base, const int32_t* __restrict__ cand,
                                                     int fixed, int rings, int sectors, int radius, double* __restrict__ dist,
                                                     int32_t* __restrict__ align)
{
    __shared__ float s_a[LIO_SC_MAX_CELLS], s_b[LIO_SC_MAX_CELLS];
    __shared__ double s_key[2][LIO_SC_MAX_DIM], s_nrm[2][LIO_SC_MAX_DIM], s_val[LIO_SC_MAX_DIM];
    __shared__ int s_ok[LIO_SC_MAX_DIM];
    __shared__ int s_shift;
    const int cells = rings * sectors, t = threadIdx.x, R = rings, S = sectors;
    const float* b = base + (size_t)(cand ? cand[blockIdx.x] : fixed) * cells;
    for (int c = t; c < cells; c += 256) { s_a[c] = a[c]; s_b[c] = b[c]; }
    __syncthreads();
    if (t < S) {                                                       // sector keys SC:214-227 and column norms
        double sa = 0.0, sb = 0.0, qa = 0.0, qb = 0.0;
        for (int r = 0; r < R; ++r) {
            const double va = (double)s_a[r * S + t], vb = (double)s_b[r * S + t];
            sa += va; sb += vb; qa += va * va; qb += vb * vb;
        }
        s_key[0][t] = sa / (double)R; s_key[1][t] = sb / (double)R;
        s_nrm[0][t] = sqrt(qa); s_nrm[1][t] = sqrt(qb);
    }
    __syncthreads();
    if (t < S) {                                                       // fastAlignUsingVkey SC:93-113: thread t = shift t
        double acc = 0.0;
        for (int j = 0; j < S; ++j) {
            int jj = j - t; if (jj < 0) jj += S;                       // circshift: column j of the shifted = column j - shift
            const double d = s_key[0][j] - s_key[1][jj];
            acc += d * d;
        }
        s_val[t] = sqrt(acc);
    }
    __syncthreads();
    if (t == 0) {
        int arg = 0;
        double mn = 10000000.0;
        for (int s = 0; s < S; ++s) if (s_val[s] < mn) { mn = s_val[s]; arg = s; }
        s_shift = arg;
    }
    __syncthreads();
    const int a0 = s_shift;
    int best_shift = 0;
    double best = 10000000.0;                                          // (thread 0's)
    for (int s = 0; s < S; ++s) {                                      // the search space SC:123-130, ascending
        const int fwd = (s - a0 + S) % S, bwd = (a0 - s + S) % S;
        if ((fwd < bwd ? fwd : bwd) > radius) continue;                // (uniform over the workgroup)
        if (t < S) {                                                   // distDirectSC SC:69-90, thread t = column t
            int jj = t - s; if (jj < 0) jj += S;
            const double n1 = s_nrm[0][t], n2 = s_nrm[1][jj];
            const bool ok = !(n1 == 0.0 || n2 == 0.0);
            double sim = 0.0;
            if (ok) {
                double dot = 0.0;
                for (int r = 0; r < R; ++r) dot += (double)s_a[r * S + t] * (double)s_b[r * S + jj];
                sim = dot / (n1 * n2);
            }
            s_val[t] = sim; s_ok[t] = ok ? 1 : 0;
        }
        __syncthreads();
        if (t == 0) {
            double sum = 0.0;
            int n_eff = 0;
            for (int j = 0; j < S; ++j) if (s_ok[j]) { sum = sum + s_val[j]; ++n_eff; }
            const double d = 1.0 - sum / (double)n_eff;                // (no effective column: NaN, which never wins)
            if (d < best) { best = d; best_shift = s; }
        }
        __syncthreads();
    }
    if (t == 0) { dist[blockIdx.x] = best; align[blockIdx.x] = best_shift; }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
extern "C" void lio_sc_default_config(lio_sc_config* cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->max_radius = 80.0;            // Scancontext.h:84
    cfg->lidar_height = 2.0;           // Scancontext.h:80
    cfg->search_ratio = 0.1;           // Scancontext.h:93
    cfg->dist_thres = 0.3;             // Scancontext.h:95 (the value in force)
    cfg->num_rings = 20;               // Scancontext.h:82
    cfg->num_sectors = 60;             // Scancontext.h:83
    cfg->num_exclude_recent = 30;      // Scancontext.h:89
    cfg->num_candidates = 3;           // Scancontext.h:90
    cfg->tree_period = 10;             // Scancontext.h:99
}

int lio_sc_check_config(const lio_sc_config* c)
{
    if (!c) return lio_fail(LIO_ERR_ARG, "null scan context config");
    if (c->num_rings < 1 || c->num_rings > LIO_SC_MAX_DIM || c->num_sectors < 1 || c->num_sectors > LIO_SC_MAX_DIM)
        return lio_fail(LIO_ERR_ARG, "num_rings and num_sectors must be in [1, LIO_SC_MAX_DIM]");
    if (c->num_rings * c->num_sectors > LIO_SC_MAX_CELLS) return lio_fail(LIO_ERR_ARG, "num_rings * num_sectors must be <= LIO_SC_MAX_CELLS");
    if (!(c->max_radius > 0.0) || !std::isfinite(c->max_radius)) return lio_fail(LIO_ERR_ARG, "max_radius must be positive and finite");
    if (!std::isfinite(c->lidar_height)) return lio_fail(LIO_ERR_ARG, "lidar_height must be finite");
    if (!(c->search_ratio >= 0.0 && c->search_ratio <= 1.0)) return lio_fail(LIO_ERR_ARG, "search_ratio must be in [0, 1]");
    if (std::isnan(c->dist_thres)) return lio_fail(LIO_ERR_ARG, "dist_thres must be a number");
    if (c->num_exclude_recent < 0) return lio_fail(LIO_ERR_ARG, "num_exclude_recent must be >= 0");
    if (c->num_candidates < 1 || c->num_candidates > LIO_SC_MAX_CANDIDATES) return lio_fail(LIO_ERR_ARG, "num_candidates must be in [1, LIO_SC_MAX_CANDIDATES]");
    if (c->tree_period < 1) return lio_fail(LIO_ERR_ARG, "tree_period must be >= 1");
    return LIO_OK;
}

namespace {
int sc_device(int device_id)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return lio_fail(LIO_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    HIPCHK(hipSetDevice(device_id));
    (void)hipGetLastError();
    return LIO_OK;
}

// enqueues the whole build of one descriptor on `s`
int sc_build(const unsigned char* d_rec, size_t stride, size_t xyz_off, size_t n, const lio_sc_config& cfg, unsigned* table, float* desc,
             float* rkey, double* skey, hipStream_t s)
{
    const int cells = cfg.num_rings * cfg.num_sectors;
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)table, (int)lio_f2ord(SC_NO_POINT), (size_t)cells, s));
    if (n) {
        const LioScGeom g = { cfg.num_rings, cfg.num_sectors, cfg.max_radius, cfg.lidar_height };
        size_t n_wg = (n + SC_FOLD_PTS - 1) / SC_FOLD_PTS;
        if (n_wg > SC_FOLD_MAX_WG) n_wg = SC_FOLD_MAX_WG;
        hipLaunchKernelGGL(k_sc_fold, dim3((unsigned)n_wg), dim3(256), 0, s, d_rec, stride, xyz_off, (int)n, g, table);
    }
    hipLaunchKernelGGL(k_sc_finish, dim3(1), dim3(256), 0, s, table, cfg.num_rings, cfg.num_sectors, desc, rkey, skey);
    return LIO_OK;
}

int sc_search_radius(const lio_sc_config& c) { return (int)round(0.5 * c.search_ratio * (double)c.num_sectors); }   // SC:123

template <typename T>
int sc_grow(LioDevBuf<T>& b, size_t per, size_t used, size_t ncap)
{
    LioDevBuf<T> nb;
    HIPCHK(nb.grow(ncap * per, 1.0, 0));
    if (used) HIPCHK(hipMemcpy(nb, b, used * per * sizeof(T), hipMemcpyDeviceToDevice));
    b = std::move(nb);                                                 // (frees the old block)
    return LIO_OK;
}
}  // namespace

extern "C" int lio_sc_make(int32_t device_id, const void* cloud, size_t n, size_t stride, const lio_sc_config* cfg, float* desc, float* ring_key,
                           double* sector_key)
try {
    if (n && !cloud) return lio_fail(LIO_ERR_ARG, "null cloud");
    if (stride < 12 || (stride & 3)) return lio_fail(LIO_ERR_ARG, "stride must be >= 12 and a multiple of 4");
    if (n > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    int rc = lio_sc_check_config(cfg);
    if (rc != LIO_OK) return rc;
    if ((rc = sc_device(device_id)) != LIO_OK) return rc;
    const size_t cells = (size_t)cfg->num_rings * cfg->num_sectors, R = (size_t)cfg->num_rings, S = (size_t)cfg->num_sectors;
    hipStream_t s = nullptr;
    LioTemp raw, table, d_desc, d_rkey, d_skey;
    HIPCHK(table.alloc(cells * sizeof(unsigned)));
    HIPCHK(d_desc.alloc(cells * sizeof(float)));
    HIPCHK(d_rkey.alloc(R * sizeof(float)));
    HIPCHK(d_skey.alloc(S * sizeof(double)));
    if (n) {
        HIPCHK(raw.alloc(n * stride));
        HIPCHK(hipMemcpyAsync(raw.p, cloud, n * stride, hipMemcpyHostToDevice, s));
    }
    if ((rc = sc_build(raw.as<unsigned char>(), stride, 0, n, *cfg, table.as<unsigned>(), d_desc.as<float>(), d_rkey.as<float>(),
                       d_skey.as<double>(), s)) != LIO_OK) return rc;
    if (desc) HIPCHK(hipMemcpyAsync(desc, d_desc.p, cells * sizeof(float), hipMemcpyDeviceToHost, s));
    if (ring_key) HIPCHK(hipMemcpyAsync(ring_key, d_rkey.p, R * sizeof(float), hipMemcpyDeviceToHost, s));
    if (sector_key) HIPCHK(hipMemcpyAsync(sector_key, d_skey.p, S * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_sc_distance(int32_t device_id, const float* desc_a, const float* desc_b, const lio_sc_config* cfg, double* dist, int32_t* align)
try {
    if (!desc_a || !desc_b || !dist || !align) return lio_fail(LIO_ERR_ARG, "null argument");
    int rc = lio_sc_check_config(cfg);
    if (rc != LIO_OK) return rc;
    if ((rc = sc_device(device_id)) != LIO_OK) return rc;
    const size_t cells = (size_t)cfg->num_rings * cfg->num_sectors;
    hipStream_t s = nullptr;
    LioTemp d_desc, d_out;
    HIPCHK(d_desc.alloc(2 * cells * sizeof(float)));
    HIPCHK(d_out.alloc(2 * sizeof(double)));
    HIPCHK(hipMemcpyAsync(d_desc.p, desc_a, cells * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_desc.as<float>() + cells, desc_b, cells * sizeof(float), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_sc_distance, dim3(1), dim3(256), 0, s, d_desc.as<float>(), d_desc.as<float>(), (const int32_t*)nullptr, 1,
                       cfg->num_rings, cfg->num_sectors, sc_search_radius(*cfg), d_out.as<double>(), (int32_t*)(d_out.as<double>() + 1));
    struct { double d; int32_t a, pad; } h;
    HIPCHK(hipMemcpyAsync(&h, d_out.p, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    *dist = h.d; *align = h.a;
    return LIO_OK;
} LIO_CATCH

int lio_sc_store_append(LioScStore& sc, const unsigned char* d_rec, size_t stride, size_t xyz_off, size_t n, const lio_sc_config* cfg,
                        hipStream_t s, int32_t* id_out)
{
    lio_sc_config c;
    if (cfg) {
        c = *cfg;
    } else {
        lio_sc_default_config(&c);
        if (sc.count) { c.num_rings = sc.rings; c.num_sectors = sc.sectors; c.max_radius = sc.max_radius; c.lidar_height = sc.lidar_height; }
    }
    int rc = lio_sc_check_config(&c);
    if (rc != LIO_OK) return rc;
    if (sc.count && (c.num_rings != sc.rings || c.num_sectors != sc.sectors || c.max_radius != sc.max_radius || c.lidar_height != sc.lidar_height))
        return lio_fail(LIO_ERR_ARG, "the descriptors of one store share the geometry of the first (num_rings, num_sectors, max_radius, lidar_height)");
    if (n > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    if (sc.count >= 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "descriptor store is full");
    const size_t cells = (size_t)c.num_rings * c.num_sectors, R = (size_t)c.num_rings, S = (size_t)c.num_sectors;
    // grow geometrically, keep the resident descriptors.  The first descriptor always sizes the storage anew: the row sizes
    // are its geometry's, and a first append that failed may have left storage sized for another one.
    if (!sc.count || sc.count + 1 > sc.cap) {
        const size_t ncap = sc.count ? sc.cap * 2 : 256;
        HIPCHK(hipDeviceSynchronize());
        if ((rc = sc_grow(sc.desc, cells, sc.count, ncap)) != LIO_OK) return rc;
        if ((rc = sc_grow(sc.rkey, R, sc.count, ncap)) != LIO_OK) return rc;
        if ((rc = sc_grow(sc.skey, S, sc.count, ncap)) != LIO_OK) return rc;
        if ((rc = sc_grow(sc.keys, 1, 0, ncap)) != LIO_OK) return rc;
        sc.cap = ncap;
    }
    HIPCHK(sc.table.grow(LIO_SC_MAX_CELLS, 1.0, 0));
    if ((rc = sc_build(d_rec, stride, xyz_off, n, c, sc.table, sc.desc + sc.count * cells, sc.rkey + sc.count * R, sc.skey + sc.count * S, s)) != LIO_OK)
        return rc;
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (!sc.count) { sc.rings = c.num_rings; sc.sectors = c.num_sectors; sc.max_radius = c.max_radius; sc.lidar_height = c.lidar_height; }
    if (id_out) *id_out = (int32_t)sc.count;
    ++sc.count;
    return LIO_OK;
}

int lio_sc_store_get(const LioScStore& sc, int id, float* desc, float* ring_key, double* sector_key)
{
    if (id < 0 || (size_t)id >= sc.count) return lio_fail(LIO_ERR_ARG, "no such descriptor");
    const size_t cells = (size_t)sc.rings * sc.sectors, R = (size_t)sc.rings, S = (size_t)sc.sectors, k = (size_t)id;
    if (desc) HIPCHK(hipMemcpy(desc, sc.desc + k * cells, cells * sizeof(float), hipMemcpyDeviceToHost));
    if (ring_key) HIPCHK(hipMemcpy(ring_key, sc.rkey + k * R, R * sizeof(float), hipMemcpyDeviceToHost));
    if (sector_key) HIPCHK(hipMemcpy(sector_key, sc.skey + k * S, S * sizeof(double), hipMemcpyDeviceToHost));
    return LIO_OK;
}

int lio_sc_store_detect(LioScStore& sc, const lio_sc_config* cfg, lio_sc_result* res, hipStream_t s)
{
    int rc = lio_sc_check_config(cfg);
    if (rc != LIO_OK) return rc;
    if (sc.count && (cfg->num_rings != sc.rings || cfg->num_sectors != sc.sectors))
        return lio_fail(LIO_ERR_ARG, "num_rings / num_sectors differ from the store's descriptors");
    memset(res, 0, sizeof(*res));
    res->loop_id = -1;
    res->min_dist = 10000000.0;                                        // SC:284
    if ((long long)sc.count < (long long)cfg->num_exclude_recent + 1) return LIO_OK;           // SC:263-267
    if (sc.counter % cfg->tree_period == 0 || sc.prefix < 1) sc.prefix = (int)sc.count - cfg->num_exclude_recent;   // SC:270-281
    ++sc.counter;
    const int prefix = sc.prefix;                                      // (>= 1: set by a call that passed SC:263, and count only grows)
    const int n_cand = cfg->num_candidates < prefix ? cfg->num_candidates : prefix;
    const size_t cells = (size_t)sc.rings * sc.sectors;
    const int query = (int)sc.count - 1;
    HIPCHK(sc.d_res.alloc(sizeof(LioScCand)));
    LioScCand* d = sc.d_res.as<LioScCand>();
    hipLaunchKernelGGL(k_sc_ring_topk, dim3(1), dim3(256), 0, s, (const float*)sc.rkey, sc.rings, prefix, query, n_cand,
                       (unsigned long long*)sc.keys, d);
    hipLaunchKernelGGL(k_sc_distance, dim3((unsigned)n_cand), dim3(256), 0, s, (const float*)(sc.desc + (size_t)query * cells),
                       (const float*)sc.desc, (const int32_t*)d->idx, 0, sc.rings, sc.sectors, sc_search_radius(*cfg), d->dist, d->align);
    LioScCand h;
    HIPCHK(hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    res->n_searched = prefix;
    res->n_candidates = n_cand;
    double min_dist = 10000000.0;
    int nn_align = 0, nn_idx = 0;
    for (int k = 0; k < n_cand; ++k) {                                 // SC:302-317
        res->cand_idx[k] = h.idx[k]; res->cand_ring_d2[k] = h.d2[k]; res->cand_dist[k] = h.dist[k]; res->cand_align[k] = h.align[k];
        if (h.dist[k] < min_dist) { min_dist = h.dist[k]; nn_align = h.align[k]; nn_idx = h.idx[k]; }
    }
    res->min_dist = min_dist; res->align = nn_align; res->nn_idx = nn_idx;
    if (min_dist < cfg->dist_thres) res->loop_id = nn_idx;             // SC:323-326
    const float deg = (float)((double)nn_align * (360.0 / (double)sc.sectors));   // nn_align * PC_UNIT_SECTORANGLE as deg2rad's float
    res->yaw_diff_rad = (float)((double)deg * M_PI / 180.0);           // SC:17-20, SC:339
    return LIO_OK;
}

// ------------------------------------------------ Scan Context loop detection (performSCLoopClosure MO:1163-1269)
// The entry points on the keyframe store, whose descriptor k belongs to keyframe k, and on the cloud a handle has staged.
extern "C" int lio_kf_store_sc_add(lio_kf_store* s, const void* cloud, size_t n, size_t stride, const lio_sc_config* cfg, int32_t* id_out)
try {
    if (!s || (n && !cloud)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (stride < 12 || (stride & 3)) return lio_fail(LIO_ERR_ARG, "stride must be >= 12 and a multiple of 4");
    if (n > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    int rc = lio_check_device(s->device_id);
    if (rc != LIO_OK) return rc;
    LioTemp raw;
    if (n) {
        HIPCHK(raw.alloc(n * stride));
        HIPCHK(hipMemcpyAsync(raw.p, cloud, n * stride, hipMemcpyDefault, nullptr));
    }
    return lio_sc_store_append(s->sc, raw.as<unsigned char>(), stride, 0, n, cfg, nullptr, id_out);
} LIO_CATCH

extern "C" int lio_kf_store_sc_add_device(lio_kf_store* s, const void* d_cloud, size_t n, size_t stride, const lio_sc_config* cfg, int32_t* id_out)
try {
    if (!s || (n && !d_cloud)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (stride < 12 || (stride & 3)) return lio_fail(LIO_ERR_ARG, "stride must be >= 12 and a multiple of 4");
    if ((uintptr_t)d_cloud & 3) return lio_fail(LIO_ERR_ARG, "d_cloud must be aligned to 4 bytes");      // k_sc_fold reads it as floats
    int rc = lio_check_device(s->device_id);
    if (rc != LIO_OK) return rc;
    if (n) HIPCHK(hipDeviceSynchronize());               // the producer of d_cloud may have used any stream
    return lio_sc_store_append(s->sc, (const unsigned char*)d_cloud, stride, 0, n, cfg, nullptr, id_out);
} LIO_CATCH

// thisRawCloudKeyFrame of MO:2149-2156 is cloud_info.cloud_deskewed: the cloud lio_s2m_register_raw has just turned into
// float4 records on the handle (before the voxel filter).  Read where it lies, on the stream that wrote it.
extern "C" int lio_kf_store_sc_add_from_handle(lio_kf_store* s, lio_s2m_handle* h, const lio_sc_config* cfg, int32_t* id_out)
try {
    if (!s || !h) return lio_fail(LIO_ERR_ARG, "null argument");
    if (h->cfg.device_id != s->device_id) return lio_fail(LIO_ERR_ARG, "the handle and the keyframe store live on different devices");
    if (h->multi || !h->raw_ws || !h->raw_ws->has_raw) return lio_fail(LIO_ERR_ARG, "the handle holds no cloud staged by lio_s2m_register_raw");
    int rc = lio_check_device(s->device_id);
    if (rc != LIO_OK) return rc;
    LioRawWs* w = h->raw_ws;
    return lio_sc_store_append(s->sc, w->xyzi.as<unsigned char>(), sizeof(float4), 0, w->n_raw, cfg, w->aux, id_out);
} LIO_CATCH

extern "C" int lio_kf_store_sc_count(const lio_kf_store* s)
try {
    return s ? (int)s->sc.count : 0;
} LIO_CATCH

extern "C" int lio_kf_store_sc_geometry(const lio_kf_store* s, int32_t* num_rings, int32_t* num_sectors)
try {
    if (!s || !num_rings || !num_sectors) return lio_fail(LIO_ERR_ARG, "null argument");
    *num_rings = s->sc.count ? s->sc.rings : 0;
    *num_sectors = s->sc.count ? s->sc.sectors : 0;
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_kf_store_sc_get(lio_kf_store* s, int32_t id, float* desc, float* ring_key, double* sector_key)
try {
    if (!s) return lio_fail(LIO_ERR_ARG, "null argument");
    int rc = lio_check_device(s->device_id);
    if (rc != LIO_OK) return rc;
    return lio_sc_store_get(s->sc, id, desc, ring_key, sector_key);
} LIO_CATCH

extern "C" int lio_kf_store_sc_detect(lio_kf_store* s, const lio_sc_config* cfg, lio_sc_result* res)
try {
    if (!s || !res) return lio_fail(LIO_ERR_ARG, "null argument");
    int rc = lio_check_device(s->device_id);
    if (rc != LIO_OK) return rc;
    rc = lio_sc_store_detect(s->sc, cfg, res, nullptr);
    res->status = rc;
    return rc;
} LIO_CATCH
