// lio_globalmap.hip -- the last readers of surfCloudKeyFrames move onto the resident keyframe store:
//   lio_kf_store_global_map    publishGlobalMap  MO:992-1041  (selection of lio_mapbuild.hip without the recent suffix, K6, K7)
//   lio_kf_store_export_map    saveMapService    MO:935-962   (k_export_chunk: every keyframe under its stored pose, streamed out)
//   lio_kf_store_get_keyframe  the read-back of one keyframe, as stored or under a pose
//   lio_s2m_registered_cloud   publishFrames     MO:2330-2345 (K6 over a cloud the handle still has staged)
//   lio_kf_store_occupancy_grid  the draft ogmGeneration.cpp on the cloud the export leaves on the device (lio_ogm.hip)
// MO = the reference's src/liorf/src/mapOptmization.cpp.  -ffp-contract=off.
//
// All four leave the store and the handle as they found them: they work in LioGlobalWs (on the store) or in the pub_*
// members of LioRawWs (on the handle), on private non-blocking streams, and are complete when they return.  They never
// touch the store's world / ds / vws / nws / d_kf / d_poses / d_chunks: an installed map can alias st->ds, and the nearby
// selection owns the rest.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <string.h>
#include <algorithm>
#include <vector>

#include "lio_handle.h"
#include "lio_kfstore.h"
#include "lio_ogm.h"

#define LIO_EXPORT_DEFAULT_CHUNK (1 << 22)
#define LIO_EXPORT_LDS_DWORDS 16          // records of up to 64 bytes are assembled in LDS and leave as 16-byte stores

struct LioGlobalWs {
    ~LioGlobalWs()
    {
        for (hipEvent_t e : { ev[0], ev[1], ev_tab }) if (e) (void)hipEventDestroy(e);
        for (hipStream_t q : { s, s2 }) if (q) (void)hipStreamDestroy(q);
    }
    hipStream_t s = nullptr, s2 = nullptr;           // s: everything; s2: the odd chunks of the export
    hipEvent_t ev[2] = { nullptr, nullptr }, ev_tab = nullptr;
    // global map: the selection's buffers, the world-frame sum, K7
    LioVoxWs<LioDevBytes> nws, vws;
    LioDevBytes nb_pts, nb_cent, nb_cid, nb_ids, nb_meta, d_kf, d_poses, d_chunks, world, ds;
    LioPinned<unsigned char> h_meta;                 // LioNbMeta, then the ids
    // export / read-back: one descriptor, one pose and one prefix offset per keyframe, and the two staging chunks
    LioDevBytes x_kf, x_poses, x_first;
    LioPinned<unsigned char> h_tab;                  // their host image on its way up (pinned: an early return leaves no
                                                     // asynchronous copy reading memory that is gone)
    LioPinned<unsigned char> h_chunk[2];
};

void lio_global_ws_free(LioGlobalWs* w) { delete w; }

// One thread per output point g0 + j of the concatenation "every keyframe 0 .. n_kf-1 in store order": finds the point's
// keyframe by a binary search over the prefix offsets (first[k] <= g < first[k + 1]; empty keyframes are stepped over
// because the search keeps the LAST k whose offset is <= g), applies that keyframe's 3x4 transform -- filled by
// k_kf_transforms, and the expression is K6's, so the bits are K6's -- and writes either a float4 (AOS = false: the input
// of the filtered copy) or an out_stride-byte PointXYZI-compatible record (x, y, z, 1, intensity, zeros) of the chunk that
// starts at g0.  Loads: 16 bytes per lane from the store.  Stores: a workgroup's 256 records are contiguous, so they are
// assembled in LDS and written as coalesced 16-byte words whatever the stride (the target is pinned host memory: narrow
// strided stores would each cross the link on their own); records wider than 64 bytes are written field by field.
// XFORM = false: `store` already holds the concatenation in the world frame (the input of the filtered copy): point g is
// copied, no table is read -- so that a call that makes both clouds transforms every point once.
template <bool AOS, bool XFORM>
__global__ __launch_bounds__(256) void k_export_chunk(const float4* __restrict__ store, const LioKfDesc* __restrict__ kf,
                                                      const int* __restrict__ first /* [n_kf + 1] */, int n_kf, int g0, int m,
                                                      unsigned char* __restrict__ out, int stride)
{
    __shared__ uint4 s_rec[256 * LIO_EXPORT_LDS_DWORDS / 4];
    const int j = blockIdx.x * 256 + (int)threadIdx.x;
    const bool live = j < m;
    float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live && !XFORM) q = store[g0 + j];
    if (live && XFORM) {
        const int g = g0 + j;
        int lo = 0, hi = n_kf;                        // first[lo] <= g < first[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (first[mid] <= g) lo = mid; else hi = mid;
        }
        const LioKfDesc d = kf[lo];
        const float4 p = store[d.src + (g - d.first)];
        q = make_float4(d.T[0] * p.x + d.T[1] * p.y + d.T[2]  * p.z + d.T[3],
                        d.T[4] * p.x + d.T[5] * p.y + d.T[6]  * p.z + d.T[7],
                        d.T[8] * p.x + d.T[9] * p.y + d.T[10] * p.z + d.T[11], p.w);   // MO:861-864
    }
    if (!AOS) {
        if (live) reinterpret_cast<float4*>(out)[j] = q;
        return;
    }
    const int W = stride >> 2;                        // dwords per record, >= 5
    if (W > LIO_EXPORT_LDS_DWORDS) {
        if (!live) return;
        float* o = reinterpret_cast<float*>(out + (size_t)j * (size_t)stride);
        o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = 1.0f; o[4] = q.w;
        for (int c = 5; c < W; ++c) o[c] = 0.0f;
        return;
    }
    float* s_f = reinterpret_cast<float*>(s_rec);
    if (live) {
        float* r = s_f + (int)threadIdx.x * W;
        r[0] = q.x; r[1] = q.y; r[2] = q.z; r[3] = 1.0f; r[4] = q.w;
        for (int c = 5; c < W; ++c) r[c] = 0.0f;
    }
    __syncthreads();
    const int blk0 = blockIdx.x * 256;                // (workgroup-uniform from here on)
    const int cnt = min(256, m - blk0);
    if (cnt <= 0) return;
    const int n_dw = cnt * W, n_16 = n_dw >> 2;
    unsigned char* base = out + (size_t)blk0 * (size_t)stride;       // 256 * stride is a multiple of 16: aligned as `out` is
    uint4* o16 = reinterpret_cast<uint4*>(base);
    for (int c = threadIdx.x; c < n_16; c += 256) o16[c] = s_rec[c];
    const int tail = n_dw & 3;                        // (only the last workgroup of a chunk can have one)
    if ((int)threadIdx.x < tail) reinterpret_cast<float*>(base)[n_16 * 4 + threadIdx.x] = s_f[n_16 * 4 + threadIdx.x];
}

namespace {

int global_ws(lio_kf_store* st, LioGlobalWs** out)
{
    if (!st->gws) st->gws = new LioGlobalWs();
    LioGlobalWs* g = st->gws;
    if (!g->s) HIPCHK(hipStreamCreateWithFlags(&g->s, hipStreamNonBlocking));
    if (!g->s2) HIPCHK(hipStreamCreateWithFlags(&g->s2, hipStreamNonBlocking));
    for (hipEvent_t* e : { &g->ev[0], &g->ev[1], &g->ev_tab })
        if (!*e) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    *out = g;
    return LIO_OK;
}

bool stride_ok(size_t stride) { return stride >= 20 && !(stride & 3) && stride <= (size_t)1 << 20; }

// descriptors, poses and prefix offsets of the keyframes [id0, id0 + n) under `pose` (null: each under its stored pose) on
// the device, T filled: what k_export_chunk reads.  *total = their points.  The host image is built in the pinned stage; complete when this returns.
int export_tables(lio_kf_store* st, LioGlobalWs* g, int id0, int n, const float* pose, size_t* total)
{
    const size_t b_kf = sizeof(LioKfDesc) * (size_t)n, b_poses = sizeof(float) * 6 * (size_t)n, b_first = sizeof(int) * ((size_t)n + 1);
    HIPCHK(g->h_tab.grow(b_kf + b_poses + b_first, (b_kf + b_poses + b_first) * 2 + 256));   // (idle: every call ends complete)
    LioKfDesc* kf = reinterpret_cast<LioKfDesc*>(g->h_tab.p);
    float* poses = reinterpret_cast<float*>(g->h_tab.p + b_kf);
    int* first = reinterpret_cast<int*>(g->h_tab.p + b_kf + b_poses);
    size_t sum = 0;
    for (int k = 0; k < n; ++k) {
        const size_t id = (size_t)id0 + (size_t)k;
        kf[(size_t)k] = lio_kf_desc(st, id, sum);
        if (pose) memcpy(poses + (size_t)k * 6, pose, 6 * sizeof(float));
        else lio_kf_stored_pose(st, id, poses + (size_t)k * 6);
        first[(size_t)k] = (int)sum;
        sum += st->cnt[id];
    }
    first[(size_t)n] = (int)sum;
    *total = sum;
    HIPCHK(g->x_kf.alloc(sizeof(LioKfDesc) * (size_t)n));
    HIPCHK(g->x_poses.alloc(sizeof(float) * 6 * (size_t)n));
    HIPCHK(g->x_first.alloc(sizeof(int) * ((size_t)n + 1)));
    HIPCHK(hipMemcpyAsync(g->x_kf.p, kf, b_kf, hipMemcpyHostToDevice, g->s));
    HIPCHK(hipMemcpyAsync(g->x_poses.p, poses, b_poses, hipMemcpyHostToDevice, g->s));
    HIPCHK(hipMemcpyAsync(g->x_first.p, first, b_first, hipMemcpyHostToDevice, g->s));
    lio_kf_transforms(g->x_kf.as<LioKfDesc>(), g->x_poses.as<float>(), n, g->s);
    HIPCHK(hipStreamSynchronize(g->s));
    HIPCHK(hipGetLastError());
    return LIO_OK;
}

// the whole concatenation as float4 into `dst` (a device buffer of `total` float4) on g->s
void export_world(lio_kf_store* st, LioGlobalWs* g, int n_kf, size_t total, float4* dst)
{
    if (!total) return;
    hipLaunchKernelGGL((k_export_chunk<false, true>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, g->s, st->d_pts, g->x_kf.as<LioKfDesc>(),
                       g->x_first.as<int>(), n_kf, 0, (int)total, reinterpret_cast<unsigned char*>(dst), 16);
}

}  // namespace

extern "C" void lio_global_map_default_config(lio_global_map_config* cfg)
{
    if (!cfg) return;
    cfg->search_radius = 1000.0f;    // globalMapVisualizationSearchRadius, all 12 yaml files
    cfg->pose_density = 10.0f;       // globalMapVisualizationPoseDensity
    cfg->leaf = 1.0f;                // globalMapVisualizationLeafSize
}

// publishGlobalMap MO:992-1041.  The key-pose table: this call may upload its dirty range on its own stream.  That is safe
// against a selection on a handle's stream because (1) calls on one store are not re-entrant, (2) every kernel of
// lio_assemble_map_nearby that reads the table (k_nb_select .. k_nb_compact) has completed at that call's one wait, before
// it returns -- what is still in flight on the handle's stream afterwards (K6, K7, the grid build) reads the copies in
// d_kf / d_poses, not the table -- and (3) this call ends with waits behind everything it queued, so the next selection,
// on whatever stream, finds the table complete and the dirty range empty.  The pinned stage of the upload is idle for the
// same reason (lio_kf_store_set_poses writes host arrays only).
extern "C" int lio_kf_store_global_map(lio_kf_store* st, const lio_global_map_config* cfg, int32_t* ids_out, int32_t ids_cap, int32_t* n_ids,
                                       void* out, size_t out_stride, size_t out_cap, size_t* n_out, lio_global_map_info* info)
try {
    if (!st || !cfg || ids_cap < 0) return lio_fail(LIO_ERR_ARG, "null argument");
    if (out && !stride_ok(out_stride)) return lio_fail(LIO_ERR_ARG, "output stride must be >= 20 and a multiple of 4");
    const float R = cfg->search_radius;
    if (!(R > 0.0f) || !std::isfinite(R) || !(cfg->pose_density > 0.0f) || !std::isfinite(cfg->pose_density) || !(cfg->leaf > 0.0f) ||
        !std::isfinite(cfg->leaf))
        return lio_fail(LIO_ERR_ARG, "search_radius, pose_density and leaf must be positive and finite");
    if (n_ids) *n_ids = 0;
    if (n_out) *n_out = 0;
    if (info) memset(info, 0, sizeof(*info));
    int rc = lio_check_device(st->device_id);
    if (rc != LIO_OK) return rc;
    const int N = (int)st->off.size();
    if (N == 0) return LIO_OK;                       // MO:997
    if (st->n_posed != (size_t)N) return lio_fail(LIO_ERR_ARG, "a keyframe has no pose (lio_kf_store_set_poses)");
    LioGlobalWs* g = nullptr;
    if ((rc = global_ws(st, &g)) != LIO_OK) return rc;
    hipStream_t s = g->s;
    if ((rc = lio_kf_upload_pose_tab(st, s)) != LIO_OK) return rc;
    HIPCHK(g->h_meta.grow(sizeof(LioNbMeta) + sizeof(int) * (size_t)N, sizeof(LioNbMeta) + sizeof(int) * 2 * (size_t)N + 4096));
    LioNbMeta* hm = (LioNbMeta*)g->h_meta.p;
    LioNbBufs nb = { g->nws, g->nb_pts, g->nb_cent, g->nb_cid, g->nb_ids, g->nb_meta, g->d_kf, g->d_poses };
    if ((rc = lio_nb_select(st, nb, R, cfg->pose_density, false, 0.0, 0.0, hm, s)) != LIO_OK) return rc;
    const int n_sel = hm->n_ids, n_chunks = hm->n_chunks;
    const unsigned long long total = hm->total;
    if (n_ids) *n_ids = n_sel;
    if (info) info->n_keyframes = n_sel;
    if (ids_out && ids_cap < n_sel) return lio_fail(LIO_ERR_ARG, "ids_cap is smaller than the selected list (*n_ids)");
    if (total > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "too many points");
    if (info) info->n_summed = (int)total;
    int* h_ids = (int*)(hm + 1);                     // (without the recent suffix the list holds at most N entries)
    if (ids_out && n_sel) HIPCHK(hipMemcpyAsync(h_ids, g->nb_ids.p, (size_t)n_sel * sizeof(int), hipMemcpyDeviceToHost, s));
    // K6 over the kept list, duplicates included, then K7 at the leaf (both wait: the ids are complete behind them)
    HIPCHK(g->d_chunks.alloc(sizeof(int2) * (size_t)(n_chunks ? n_chunks : 1)));
    HIPCHK(g->world.alloc(sizeof(float4) * (size_t)total));
    lio_nb_chunks(g->d_kf.as<LioKfDesc>(), n_sel, g->d_chunks.as<int2>(), s);
    lio_kf_sum_launch(st, g->d_kf.as<LioKfDesc>(), g->d_poses.as<float>(), g->d_chunks.as<int2>(), n_sel, n_chunks, g->world.as<float4>(), s);
    int no = 0;
    rc = lio_voxel_grid_device(g->world.as<float4>(), (int)total, cfg->leaf, g->ds, &no, s, g->vws, nullptr);
    if (rc < 0) { (void)hipStreamSynchronize(s); return rc; }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (ids_out && n_sel) memcpy(ids_out, h_ids, (size_t)n_sel * sizeof(int));
    if (info) { info->n_out = no; info->voxel_passthrough = rc == 1 ? 1 : 0; }
    if (n_out) *n_out = (size_t)no;
    if (out && (size_t)no > out_cap) return lio_fail(LIO_ERR_ARG, "out holds fewer records than the global map (*n_out)");
    const int rc2 = lio_copy_out(g->ds.as<float4>(), no, out, out_stride, s);
    if (rc2 < 0) return rc2;
    return LIO_OK;
} LIO_CATCH

// saveMapService MO:935-962.  The unfiltered cloud never exists on the device: k_export_chunk writes chunk k straight into
// pinned staging buffer k & 1 -- the kernel IS the transfer -- on stream k & 1, and while it runs the host copies chunk
// k - 1 out of the other buffer into the caller's cloud.  Buffer b is written again by chunk k + 2, which is launched only
// after the host copy of chunk k has returned; completion is tracked with one event per buffer, nothing waits for the device
// as a whole.  Device memory: 92 bytes per keyframe (a 64-byte descriptor, a 24-byte pose, a 4-byte offset) before the allocator's
// slack, whatever the chunk size.
extern "C" int lio_kf_store_export_map(lio_kf_store* st, const lio_export_config* cfg, void* out_full, size_t full_stride, size_t full_cap,
                                       size_t* n_full, void* out_ds, size_t ds_stride, size_t ds_cap, size_t* n_ds, int32_t* voxel_passthrough)
try {
    if (!st || !cfg) return lio_fail(LIO_ERR_ARG, "null argument");
    if ((out_full && !stride_ok(full_stride)) || (out_ds && !stride_ok(ds_stride)))
        return lio_fail(LIO_ERR_ARG, "output strides must be >= 20 and multiples of 4");
    if (!(cfg->resolution >= 0.0f) || !std::isfinite(cfg->resolution)) return lio_fail(LIO_ERR_ARG, "resolution must be finite and not negative");
    if (cfg->chunk_points != 0 && (cfg->chunk_points < 256 || cfg->chunk_points > (1 << 26)))
        return lio_fail(LIO_ERR_ARG, "chunk_points must be 0 or in [256, 1 << 26]");
    if (n_full) *n_full = 0;
    if (n_ds) *n_ds = 0;
    if (voxel_passthrough) *voxel_passthrough = 0;
    int rc = lio_check_device(st->device_id);
    if (rc != LIO_OK) return rc;
    const int N = (int)st->off.size();
    if (N == 0) return LIO_OK;
    if (st->n_posed != (size_t)N) return lio_fail(LIO_ERR_ARG, "a keyframe has no pose (lio_kf_store_set_poses)");
    LioGlobalWs* g = nullptr;
    if ((rc = global_ws(st, &g)) != LIO_OK) return rc;
    size_t total = 0;
    if ((rc = export_tables(st, g, 0, N, nullptr, &total)) != LIO_OK) return rc;
    if (n_full) *n_full = total;
    const bool filtered = cfg->resolution != 0.0f;   // MO:943
    int no = 0;
    if (filtered && total) {
        // PCL's filter is a global sort: the filtered copy needs the whole world-frame cloud on the device
        HIPCHK(g->world.alloc(sizeof(float4) * total));
        export_world(st, g, N, total, g->world.as<float4>());
        rc = lio_voxel_grid_device(g->world.as<float4>(), (int)total, cfg->resolution, g->ds, &no, g->s, g->vws, nullptr);
        if (rc < 0) { (void)hipStreamSynchronize(g->s); return rc; }
        HIPCHK(hipStreamSynchronize(g->s));
        HIPCHK(hipGetLastError());
        if (voxel_passthrough) *voxel_passthrough = rc == 1 ? 1 : 0;
    }
    if (n_ds) *n_ds = (size_t)no;
    if ((out_full && total > full_cap) || (filtered && out_ds && (size_t)no > ds_cap))
        return lio_fail(LIO_ERR_ARG, "an output holds fewer records than its cloud (*n_full, *n_ds)");
    if (filtered && out_ds && (rc = lio_copy_out(g->ds.as<float4>(), no, out_ds, ds_stride, g->s)) < 0) return rc;
    if (!out_full || !total) return LIO_OK;
    // ---- the unfiltered cloud, chunk by chunk
    const size_t cp = std::min<size_t>(cfg->chunk_points ? (size_t)cfg->chunk_points : (size_t)LIO_EXPORT_DEFAULT_CHUNK, total);
    const size_t n_chunks = (total + cp - 1) / cp;
    for (int b = 0; b < (n_chunks > 1 ? 2 : 1); ++b)
        HIPCHK(g->h_chunk[b].grow(cp * full_stride, cp * full_stride + 256));
    // (with a filtered copy the world-frame cloud is on the device already: the chunks are cut from it, not computed again)
    const bool from_world = filtered;
    const float4* src = from_world ? g->world.as<float4>() : (const float4*)st->d_pts;
    hipStream_t q[2] = { g->s, g->s2 };
    HIPCHK(hipEventRecord(g->ev_tab, g->s));         // (the tables were written on s; complete already, this keeps the order explicit)
    HIPCHK(hipStreamWaitEvent(g->s2, g->ev_tab, 0));
    unsigned char* dst = (unsigned char*)out_full;
    hipError_t err = hipSuccess;
    for (size_t k = 0; k <= n_chunks && err == hipSuccess; ++k) {
        const int b = (int)(k & 1);
        if (k < n_chunks) {
            const size_t g0 = k * cp, m = std::min(cp, total - g0);
            if (from_world)
                hipLaunchKernelGGL((k_export_chunk<true, false>), dim3((unsigned)((m + 255) / 256)), dim3(256), 0, q[b], src, g->x_kf.as<LioKfDesc>(),
                                   g->x_first.as<int>(), N, (int)g0, (int)m, g->h_chunk[b].p, (int)full_stride);
            else
                hipLaunchKernelGGL((k_export_chunk<true, true>), dim3((unsigned)((m + 255) / 256)), dim3(256), 0, q[b], src, g->x_kf.as<LioKfDesc>(),
                                   g->x_first.as<int>(), N, (int)g0, (int)m, g->h_chunk[b].p, (int)full_stride);
            err = hipEventRecord(g->ev[b], q[b]);
        }
        if (k >= 1 && err == hipSuccess) {           // chunk k - 1: wait for its kernel, copy it out while chunk k runs
            const size_t g0 = (k - 1) * cp, m = std::min(cp, total - g0);
            err = hipEventSynchronize(g->ev[b ^ 1]);
            if (err == hipSuccess) memcpy(dst + g0 * full_stride, g->h_chunk[b ^ 1].p, m * full_stride);
        }
    }
    if (err != hipSuccess) { (void)hipStreamSynchronize(g->s); (void)hipStreamSynchronize(g->s2); }
    HIPCHK(err);
    HIPCHK(hipGetLastError());
    return LIO_OK;
} LIO_CATCH

// The fork's draft ogmGeneration.cpp on the cloud it would load from GlobalMap.pcd: the export's world-frame sum
// (map_resolution 0) or its filtered copy, where lio_kf_store_export_map leaves them -- g->world, g->ds -- then the chain of
// lio_ogm.hip on g->s.  Only the grid and the info cross to the host.
extern "C" int lio_kf_store_occupancy_grid(lio_kf_store* st, float map_resolution, const lio_ogm_config* cfg, int8_t* grid, size_t grid_cap,
                                           size_t* n_map, lio_ogm_info* info)
try {
    lio_ogm_info local;
    if (!info) info = &local;
    memset(info, 0, sizeof(*info));
    if (n_map) *n_map = 0;
    if (!st || !cfg) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!(map_resolution >= 0.0f) || !std::isfinite(map_resolution)) return lio_fail(LIO_ERR_ARG, "map_resolution must be finite and not negative");
    int rc = lio_ogm_check(cfg);
    if (rc != LIO_OK) return rc;
    if ((rc = lio_check_device(st->device_id)) != LIO_OK) return rc;
    const int N = (int)st->off.size();
    if (N == 0) return LIO_OK;
    if (st->n_posed != (size_t)N) return lio_fail(LIO_ERR_ARG, "a keyframe has no pose (lio_kf_store_set_poses)");
    LioGlobalWs* g = nullptr;
    if ((rc = global_ws(st, &g)) != LIO_OK) return rc;
    size_t total = 0;
    if ((rc = export_tables(st, g, 0, N, nullptr, &total)) != LIO_OK) return rc;
    if (total > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "too many points");
    const float4* cloud = nullptr;
    int n_cloud = (int)total;
    if (total) {
        HIPCHK(g->world.alloc(sizeof(float4) * total));
        export_world(st, g, N, total, g->world.as<float4>());
        cloud = g->world.as<float4>();
        if (map_resolution != 0.0f) {                 // MO:943
            int no = 0;
            rc = lio_voxel_grid_device(g->world.as<float4>(), (int)total, map_resolution, g->ds, &no, g->s, g->vws, nullptr);
            if (rc < 0) { (void)hipStreamSynchronize(g->s); return rc; }
            cloud = g->ds.as<float4>(); n_cloud = no;
        }
    }
    if (n_map) *n_map = (size_t)n_cloud;
    rc = lio_ogm_device(cloud, n_cloud, *cfg, grid, grid_cap, info, g->s, lio_ogm_times_wanted());
    (void)hipStreamSynchronize(g->s);                 // complete on return, whatever the chain returned
    if (rc == LIO_OK) HIPCHK(hipGetLastError());
    return rc;
} LIO_CATCH

extern "C" int lio_kf_store_get_keyframe(lio_kf_store* st, int32_t id, const float* pose, void* out, size_t out_stride, size_t out_cap,
                                         size_t* n_out)
try {
    if (!st) return lio_fail(LIO_ERR_ARG, "null argument");
    if (id < 0 || (size_t)id >= st->off.size()) return lio_fail(LIO_ERR_ARG, "unknown keyframe id");
    if (out && !stride_ok(out_stride)) return lio_fail(LIO_ERR_ARG, "output stride must be >= 20 and a multiple of 4");
    if (pose)
        for (int j = 0; j < 6; ++j) if (!std::isfinite(pose[j])) return lio_fail(LIO_ERR_ARG, "non-finite pose");
    const size_t n = st->cnt[(size_t)id];
    if (n_out) *n_out = n;
    if (out && n > out_cap) return lio_fail(LIO_ERR_ARG, "out holds fewer records than the keyframe (*n_out)");
    if (!out || !n) return LIO_OK;
    int rc = lio_check_device(st->device_id);
    if (rc != LIO_OK) return rc;
    LioGlobalWs* g = nullptr;
    if ((rc = global_ws(st, &g)) != LIO_OK) return rc;
    // (every lio_kf_store_add* has waited for its write of d_pts before it returned)
    if (!pose) {
        rc = lio_copy_out(st->d_pts + st->off[(size_t)id], (int)n, out, out_stride, g->s);
        return rc < 0 ? rc : LIO_OK;
    }
    size_t total = 0;
    if ((rc = export_tables(st, g, id, 1, pose, &total)) != LIO_OK) return rc;
    HIPCHK(g->world.alloc(sizeof(float4) * total));
    export_world(st, g, 1, total, g->world.as<float4>());
    if ((rc = lio_copy_out(g->world.as<float4>(), (int)total, out, out_stride, g->s)) < 0) return rc;
    HIPCHK(hipGetLastError());
    return LIO_OK;
} LIO_CATCH

// publishFrames MO:2330-2345: cloud_registered = transformPointCloud(laserCloudSurfLastDS, final pose), cloud_registered_raw
// the same of cloud_deskewed.  Both clouds are still staged on the handle; the read is ordered behind the stream that wrote
// them (the handle's for the registered scan, the auxiliary one of lio_s2m_register_raw for the whole cloud) by an event.
extern "C" int lio_s2m_registered_cloud(lio_s2m_handle* h, int32_t which, const float pose[6], void* out, size_t out_stride, size_t out_cap,
                                        size_t* n_out)
try {
    if (!h || !pose) return lio_fail(LIO_ERR_ARG, "null argument");
    if (which != LIO_STAGED_DS && which != LIO_STAGED_RAW) return lio_fail(LIO_ERR_ARG, "which must be LIO_STAGED_DS or LIO_STAGED_RAW");
    if (h->multi) return lio_fail(LIO_ERR_ARG, "lio_s2m_registered_cloud needs a single-device handle");
    if (out && !stride_ok(out_stride)) return lio_fail(LIO_ERR_ARG, "output stride must be >= 20 and a multiple of 4");
    for (int j = 0; j < 6; ++j) if (!std::isfinite(pose[j])) return lio_fail(LIO_ERR_ARG, "non-finite pose");
    if (n_out) *n_out = 0;
    const unsigned char* rec = nullptr;
    size_t n = 0, stride = sizeof(float4), xyz_off = 0;
    int dev = h->cfg.device_id, int_off = 12;
    hipStream_t producer = nullptr;
    if (which == LIO_STAGED_DS) {
        const int rc = lio_s2m_staged_scan(h, 0, &rec, &n, &stride, &xyz_off, &int_off, &dev, &producer);
        if (rc != LIO_OK) return rc;
    } else {
        if (!h->raw_ws || !h->raw_ws->has_raw) return lio_fail(LIO_ERR_ARG, "the handle holds no cloud staged by lio_s2m_register_raw");
        rec = h->raw_ws->xyzi.as<unsigned char>(); n = h->raw_ws->n_raw; producer = h->raw_ws->aux;
    }
    if (n > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    if (n_out) *n_out = n;
    if (out && n > out_cap) return lio_fail(LIO_ERR_ARG, "out holds fewer records than the staged cloud (*n_out)");
    if (!out || !n) return LIO_OK;
    int rc = lio_check_device(dev);
    if (rc != LIO_OK) return rc;
    if (!h->raw_ws) h->raw_ws = new LioRawWs();
    LioRawWs* w = h->raw_ws;
    if (!w->pub) HIPCHK(hipStreamCreateWithFlags(&w->pub, hipStreamNonBlocking));
    if (!w->ev_pub) HIPCHK(hipEventCreateWithFlags(&w->ev_pub, hipEventDisableTiming));
    hipStream_t s = w->pub;
    HIPCHK(hipEventRecord(w->ev_pub, producer));
    HIPCHK(hipStreamWaitEvent(s, w->ev_pub, 0));
    HIPCHK(w->pub_world.alloc(sizeof(float4) * n));
    HIPCHK(w->pub_kf.alloc(sizeof(LioKfDesc) + 6 * sizeof(float) + 2 * sizeof(int)));
    // one "keyframe" of n points under `pose`: descriptor, pose, prefix offsets (0, n) in one small buffer
    // (built in pinned memory kept on the handle: an early return leaves no asynchronous copy reading a dead stack frame)
    struct PubTab { LioKfDesc d; float pose[6]; int first[2]; };
    HIPCHK(w->pub_tab.grow(sizeof(PubTab), sizeof(PubTab)));
    PubTab& tab = *reinterpret_cast<PubTab*>(w->pub_tab.p);
    tab.d.src = 0; tab.d.first = 0; tab.d.n = (int)n; tab.d.pad = 0;
    for (int j = 0; j < 12; ++j) tab.d.T[j] = 0.0f;
    for (int j = 0; j < 6; ++j) tab.pose[j] = pose[j];
    tab.first[0] = 0; tab.first[1] = (int)n;
    HIPCHK(hipMemcpyAsync(w->pub_kf.p, &tab, sizeof(tab), hipMemcpyHostToDevice, s));
    LioKfDesc* d_kf = w->pub_kf.as<LioKfDesc>();
    const float* d_pose = reinterpret_cast<const float*>(w->pub_kf.as<unsigned char>() + offsetof(PubTab, pose));
    const int* d_first = reinterpret_cast<const int*>(w->pub_kf.as<unsigned char>() + offsetof(PubTab, first));
    lio_kf_transforms(d_kf, d_pose, 1, s);
    const float4* src = reinterpret_cast<const float4*>(rec);       // the whole staged cloud is float4 (x, y, z, intensity) already
    if (which == LIO_STAGED_DS) {                                   // the staged scan: records as uploaded
        HIPCHK(w->pub_xyzi.alloc(sizeof(float4) * n));
        lio_rec_to_xyzi4(rec, stride, xyz_off, int_off, (int)n, w->pub_xyzi.as<float4>(), s);
        src = w->pub_xyzi.as<float4>();
    }
    hipLaunchKernelGGL((k_export_chunk<false, true>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, d_kf, d_first, 1, 0,
                       (int)n, w->pub_world.as<unsigned char>(), 16);
    if ((rc = lio_copy_out(w->pub_world.as<float4>(), (int)n, out, out_stride, s)) < 0) return rc;   // (waits for `s`)
    HIPCHK(hipGetLastError());
    return LIO_OK;
} LIO_CATCH
