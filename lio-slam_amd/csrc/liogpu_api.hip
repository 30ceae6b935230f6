// liogpu_api.hip -- the base of the C ABI in include/liogpu.h: the error plumbing, the life cycle of a scan-to-map handle,
// the host / device memory helpers and the profile.  The handle's map is in lio_s2m_map.hip, its batch in lio_s2m_upload.hip,
// the Gauss-Newton loop and the registrations in lio_s2m_run.hip.  MO = mapOptmization.cpp of the reference (liorf).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <exception>
#include <memory>

#include "lio_gridplan.h"
#include "lio_handle.h"
#include "lio_multi.h"

static thread_local char g_last_error[512];   // (a fixed buffer: recording an allocation failure allocates nothing)

int lio_fail(int code, const char* what, hipError_t e)
{
    if (e != hipSuccess) snprintf(g_last_error, sizeof(g_last_error), "%s: %s", what, hipGetErrorString(e));
    else snprintf(g_last_error, sizeof(g_last_error), "%s", what);
    return code;
}

// LIO_CATCH: what the library can throw is std::bad_alloc or std::length_error from a container or `new` -- out of
// host memory or a size beyond it -- hence LIO_ERR_CAPACITY.
int lio_fail_exception(void)
{
    char buf[256];
    try {
        throw;
    } catch (const std::exception& e) {
        snprintf(buf, sizeof(buf), "C++ exception: %s", e.what());
    } catch (...) {
        snprintf(buf, sizeof(buf), "C++ exception of an unknown type");
    }
    return lio_fail(LIO_ERR_CAPACITY, buf);
}

extern "C" int lio_version(void) { return LIO_VERSION; }
extern "C" const char* lio_last_error(void) { return g_last_error; }

extern "C" void lio_s2m_default_config(lio_s2m_config* c)
{
    memset(c, 0, sizeof(*c));
    c->k = 5;                 // MO:1631
    c->max_sq_dist = 1.0f;    // MO:1641
    c->plane_tol = 0.2;       // MO:1662
    c->weight = 0.9;          // MO:1671
    c->min_s = 0.1;           // MO:1679
    c->min_corr = 50;         // MO:1722
    c->max_iters = 30;        // MO:1848
    c->eig_thresh = 100.0f;   // MO:1796
    c->conv_deg = 0.05;       // MO:1833
    c->conv_cm = 0.05;        // MO:1833
    c->min_scan_pts = 30;     // MO:1844
    c->jacobian_mode = 0;
    c->force_all_iters = 0;
    c->device_id = 0;
    c->cell_size = 0.0f;
    c->max_batch = 1;
    c->max_scan_pts = 0;
    c->record_corr_iter = -1;
    c->kernel_variant = 0;
    c->profile = 0;
    c->lookahead = -1;
    c->use_lds = 0;
    c->cell_div = 2;
    c->xcd_remap = 1;
    c->tile_size = 0.0f;
    c->use_graph = 0;
    c->sort_batch = 1;
    c->graph_iters = 4;
    c->sort_scan = 1;
    c->nn_cache = 1;
    c->pipeline = 0;
    c->n_devices = 1;
    for (int i = 0; i < 8; ++i) c->device_ids[i] = i;
    c->x_sub = 0;
    c->tight_rows = 0;
}

void lio_consts_from_config(const lio_s2m_config& g, LioConsts& c)
{
    c.plane_tol = g.plane_tol; c.weight = g.weight; c.min_s = g.min_s;
    c.plane_tol_f = lio_threshold_f32(g.plane_tol); c.min_s_f = lio_threshold_f32(g.min_s);
    c.conv_deg = g.conv_deg; c.conv_cm = g.conv_cm;
    c.max_sq_dist = g.max_sq_dist; c.eig_thresh = g.eig_thresh;
    c.gate_reach = lio_gate_reach(g.max_sq_dist);
    c.min_corr = g.min_corr; c.max_iters = g.max_iters;
    c.jac_exact = g.jacobian_mode ? 1 : 0; c.force_all = g.force_all_iters ? 1 : 0;
    c.record_iter = g.record_corr_iter; c.min_scan_pts = g.min_scan_pts;
}

static void lio_fill_consts(lio_s2m_handle* h) { lio_consts_from_config(h->cfg, h->c); }

static int lio_s2m_init_resources(lio_s2m_handle* h)
{
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (int i = 0; i < LIO_MAX_ITERS; ++i) {
        HIPCHK(hipEventCreate(&h->ev_beg[i]));
        HIPCHK(hipEventCreate(&h->ev_end[i]));
        HIPCHK(hipEventCreateWithFlags(&h->ev_chk[i], hipEventDisableTiming));
    }
    HIPCHK(h->h_active.grow(LIO_MAX_ITERS, LIO_MAX_ITERS));
    HIPCHK(hipEventCreate(&h->ev_map[0]));
    HIPCHK(hipEventCreate(&h->ev_map[1]));
    HIPCHK(hipEventCreate(&h->ev_mapl[0]));
    HIPCHK(hipEventCreate(&h->ev_mapl[1]));
    HIPCHK(h->d_bbox.grow(6, 1.0, 0));
    HIPCHK(h->d_active.grow(1, 1.0, 0));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->cfg.device_id) == hipSuccess) h->n_cu = prop.multiProcessorCount;
    (void)hipGetLastError();
    return LIO_OK;
}

extern "C" int lio_s2m_create(const lio_s2m_config* cfg, lio_s2m_handle** out)
try {
    if (!cfg || !out) return lio_fail(LIO_ERR_ARG, "null argument");
    if (cfg->k != 5) return lio_fail(LIO_ERR_ARG, "only k = 5 is supported (MO:1631)");
    if (cfg->max_iters < 1 || cfg->max_iters > LIO_MAX_ITERS) return lio_fail(LIO_ERR_ARG, "max_iters out of range");
    if (!(cfg->max_sq_dist > 0.0f)) return lio_fail(LIO_ERR_ARG, "max_sq_dist must be positive");
    if (cfg->x_sub != 0 && cfg->x_sub != 1 && cfg->x_sub != 2 && cfg->x_sub != 4 && cfg->x_sub != 8)
        return lio_fail(LIO_ERR_ARG, "cfg.x_sub must be 0 (auto), 1, 2, 4 or 8");
    if (cfg->tight_rows < -1 || cfg->tight_rows > LIO_TB_MAX) return lio_fail(LIO_ERR_ARG, "cfg.tight_rows must be -1 (none), 0 (auto) or 1..3 tables");
    if (cfg->pipeline != 0 && cfg->pipeline != 1 && cfg->pipeline != 4)
        return lio_fail(LIO_ERR_ARG, "cfg.pipeline must be 0 (auto), 1 (one launch per iteration) or 4 (one-launch loop)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return lio_fail(LIO_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return lio_fail(LIO_ERR_ARG, "device_id out of range");
    if (cfg->n_devices > 1) {                           // in-library multi-GPU: a front handle + one child per listed device (lio_multi.hip)
        const int rc = lio_multi_create(cfg, out);
        if (rc == LIO_OK) lio_fill_consts(*out);
        return rc;
    }
    HIPCHK(hipSetDevice(cfg->device_id));
    if (cfg->cell_size > 0.0f && cfg->cell_size < lio_gate_cell_min(*cfg))   // (before division by cell_div)
        return lio_fail(LIO_ERR_ARG, "cell_size must be >= sqrt(max_sq_dist)*1.001 for an exact 27-cell search");
    std::unique_ptr<lio_s2m_handle> h(new lio_s2m_handle());   // (releases whatever had been created if a step fails)
    h->cfg = *cfg;
    lio_fill_consts(h.get());
    h->shard.axis = -1;
    // the plain instantiation of k_s2m_iterate (lio_launch_iterate) unless LIO_PLAIN_KERNEL=0 in the environment: kept per
    // handle, so one process can hold both kinds for A/B runs
    { const char* e = getenv("LIO_PLAIN_KERNEL"); h->plain_kernel = !(e && *e && atoi(e) == 0); }
    // the looped form of the plain kernel from launch LIO_TAIL_FROM of a run on (-1: never), on LIO_TAIL_WGS workgroups
    { const char* e = getenv("LIO_TAIL_FROM"); if (e && *e) h->tail_from = atoi(e) < 0 ? -1 : atoi(e); }
    { const char* e = getenv("LIO_TAIL_WGS"); if (e && *e) h->tail_wgs = atoi(e); }
    h->tail_wgs = h->tail_wgs < 8 ? 8 : ((h->tail_wgs + 7) & ~7);
    const int rc = lio_s2m_init_resources(h.get());
    if (rc != LIO_OK) return rc;
    *out = h.release();
    return LIO_OK;
} LIO_CATCH

extern "C" void lio_s2m_destroy(lio_s2m_handle* h)
{
    if (!h) return;
    if (h->multi) { lio_multi_destroy(h); return; }
    (void)hipSetDevice(h->cfg.device_id);
    (void)hipStreamSynchronize(h->stream);
    delete h;
}

lio_s2m_handle::~lio_s2m_handle()
{
    delete multi;                                           // (a multi-device front holds nothing else)
    lio_s2m_destroy(corner);
    lio_raw_ws_free(raw_ws);
    for (int i = 0; i < LIO_MAX_ITERS; ++i) {               // (a handle whose creation failed half-way holds nulls)
        if (ev_beg[i]) (void)hipEventDestroy(ev_beg[i]);
        if (ev_end[i]) (void)hipEventDestroy(ev_end[i]);
        if (ev_chk[i]) (void)hipEventDestroy(ev_chk[i]);
    }
    for (hipEvent_t e : { ev_map[0], ev_map[1], ev_mapl[0], ev_mapl[1] }) if (e) (void)hipEventDestroy(e);
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    if (graph) (void)hipGraphDestroy(graph);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

extern "C" int lio_s2m_set_stream(lio_s2m_handle* h, void* hip_stream)
try {
    if (h && h->multi) return lio_refuse_multi();
    if (!h) return lio_fail(LIO_ERR_ARG, "null handle");
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->own_stream && h->stream) HIPCHK(hipStreamDestroy(h->stream));
    h->stream = (hipStream_t)hip_stream;
    h->own_stream = false;
    h->graph_dirty = true;
    if (h->corner) return lio_s2m_set_stream(h->corner, hip_stream);
    return LIO_OK;
} LIO_CATCH

extern "C" void* lio_host_alloc(size_t bytes)
{
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
extern "C" void lio_host_free(void* p) { if (p) (void)hipHostFree(p); }

// Device memory for callers that keep their clouds in HBM between calls (every entry point that takes `scans` / `data`
// reads memory of the handle's own device in place).
extern "C" void* lio_device_alloc(int32_t device_id, size_t bytes)
{
    void* p = nullptr;
    if (hipSetDevice(device_id) != hipSuccess || hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
extern "C" void lio_device_free(int32_t device_id, void* p)
{
    if (p && hipSetDevice(device_id) == hipSuccess) (void)hipFree(p);
}
extern "C" int lio_device_upload(int32_t device_id, void* dst, const void* src, size_t bytes)
try {
    if (!dst || (!src && bytes)) return lio_fail(LIO_ERR_ARG, "null pointer");
    HIPCHK(hipSetDevice(device_id));
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return LIO_OK;
} LIO_CATCH
extern "C" int lio_host_register(void* p, size_t bytes)
try {
    if (!p || !bytes) return lio_fail(LIO_ERR_ARG, "null range");
    HIPCHK(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return LIO_OK;
} LIO_CATCH
extern "C" int lio_host_unregister(void* p)
try {
    if (!p) return lio_fail(LIO_ERR_ARG, "null pointer");
    HIPCHK(hipHostUnregister(p));
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_s2m_get_profile(lio_s2m_handle* h, lio_s2m_profile* out)
try {
    if (!h || !out) return lio_fail(LIO_ERR_ARG, "null argument");
    if (h->multi) h->prof.n_map = (int64_t)h->n_map;
    if (h->map_timing_pending) {
        HIPCHK(hipSetDevice(h->cfg.device_id));
        HIPCHK(hipEventSynchronize(h->ev_mapl[1]));
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, h->ev_mapl[0], h->ev_mapl[1]));
        h->prof.map_build_ms = ms;
        h->map_timing_pending = false;
    }
    *out = h->prof;
    return LIO_OK;
} LIO_CATCH
