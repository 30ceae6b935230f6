// lio_kfstore.h -- the resident keyframe store (lio_kfstore.hip) and what its readers share: the descriptors of K6, the
// key-pose table, the keyframe sum, and the cloud lio_s2m_register_raw keeps staged on the handle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#include "../../include/liogpu.h"
#include "lio_cloud.h"
#include "lio_pool.h"
#include "lio_sc.h"

struct LioKfDesc {       // one selected keyframe
    int src;             // first point of the keyframe in the resident store
    int first;           // first point in the concatenated world-frame cloud
    int n;
    int pad;
    float T[12];         // pclPointToAffine3f of its pose (MO:856), filled on the device
};

struct LioKfSum {        // the host tables of one keyframe sum (below): descriptors, the 256-point chunks of K6, poses, points
    std::vector<LioKfDesc> kf; std::vector<int2> chunks; std::vector<float> poses;
    size_t total = 0;
};

struct LioPoseTab { const float *x, *y, *z, *roll, *pitch, *yaw; const double* t; const int *off, *cnt; };
struct LioNbMeta { int n_sel, recent_fail; unsigned box[6]; int n_ids, n_chunks; unsigned long long total; };

struct LioGlobalWs;                                  // lio_globalmap.hip: the workspace of the global map and the export
void lio_global_ws_free(LioGlobalWs* w);

// surfCloudKeyFrames (MO:128): every keyframe cloud is uploaded ONCE (MO:2138-2142) and stays in
// HBM; assembling the local map for a scan only needs the selected ids and their current poses.
struct lio_kf_store {
    ~lio_kf_store()                                  // (the buffers: on the device lio_kf_store_destroy sets)
    {
        if (ev_ids) (void)hipEventDestroy(ev_ids);
        lio_global_ws_free(gws);
    }
    int device_id = 0;
    LioDevBuf<float4> d_pts;
    size_t used = 0;
    std::vector<size_t> off, cnt;
    // workspace of lio_assemble_map_resident when the map is installed in a handle (kept between calls)
    LioVoxWs<LioDevBytes> vws;
    LioDevBytes world, ds, d_kf, d_poses, d_chunks, blk_box;
    LioKfSum v_sum;
    // key-pose table = cloudKeyPoses6D (x, y, z, roll, pitch, yaw, time): host copy written by lio_kf_store_set_poses (never
    // blocks), device SoA next to off / cnt uploaded -- the dirty range only -- on the stream of the next selection
    std::vector<float> px, py, pz, proll, ppitch, pyaw;
    std::vector<double> ptime;
    std::vector<unsigned char> has_pose, has_time;
    size_t n_posed = 0, dirty_lo = SIZE_MAX, dirty_hi = 0, tab_cap = 0;
    LioDevBytes d_tab;                               // [tab_cap] x 6 float, [tab_cap] double, [tab_cap] x 2 int
    LioPinned<unsigned char> h_stage;                // the dirty range on its way up, then (n_ids, total), then ids
    // workspace of lio_assemble_map_nearby's selection
    LioVoxWs<LioDevBytes> nws;
    LioDevBytes nb_pts, nb_cent, nb_cid, nb_ids, nb_meta;
    hipEvent_t ev_ids = nullptr;
    LioScStore sc;                                   // the Scan Context descriptors (lio_sc.hip), descriptor k = keyframe k
    LioGlobalWs* gws = nullptr;                      // lio_kf_store_global_map / _export_map / _get_keyframe (lio_globalmap.hip)
};

// Staged cloud and voxel-filter workspace of lio_s2m_register_raw, kept on the handle from one callback to the next.
struct LioRawWs {
    ~LioRawWs()
    {
        if (ev_in) (void)hipEventDestroy(ev_in);
        if (ev_done) (void)hipEventDestroy(ev_done);
        if (ev_pub) (void)hipEventDestroy(ev_pub);
        if (aux) (void)hipStreamDestroy(aux);
        if (pub) (void)hipStreamDestroy(pub);
    }
    LioDevBytes raw, xyzi, ds;
    LioVoxWs<LioDevBytes> vws;
    // the upload and the voxel filter of the sweep run on a stream of their own: they do not depend on the local map, whose
    // assembly (lio_assemble_map_resident: K6 + K7 + grid build, ~0.25 ms of small kernels) is usually still in flight on the
    // handle's stream when the node calls lio_s2m_register_raw -- the two chains overlap on the GPU, and the filter's host
    // waits (bounding box, voxel count) no longer wait for the map as well
    hipStream_t aux = nullptr;
    hipEvent_t ev_in = nullptr, ev_done = nullptr;
    size_t n_raw = 0;                                // points of the whole cloud in `xyzi` (written on `aux`)
    bool has_raw = false;
    // lio_s2m_registered_cloud (lio_globalmap.hip): its own stream and buffers, so that it leaves the staged clouds alone
    hipStream_t pub = nullptr;
    hipEvent_t ev_pub = nullptr;
    LioDevBytes pub_xyzi, pub_world, pub_kf;
    LioPinned<unsigned char> pub_tab;                // the host image of pub_kf on its way up
};

// the dirty range of the key-pose table (and off / cnt) to the device, on stream `s`, through the store's pinned stage
int lio_kf_upload_pose_tab(lio_kf_store* st, hipStream_t s);
LioPoseTab lio_kf_pose_tab(lio_kf_store* st);        // the columns of the uploaded table

// ---- the keyframe sum: keyframes ids[k] under poses p[k], concatenated in the world frame (K6, MO:849-868)
LioKfDesc lio_kf_desc(const lio_kf_store* st, size_t id, size_t first);     // T zeroed: k_kf_transforms fills it
void lio_kf_stored_pose(const lio_kf_store* st, size_t id, float pose[6]);  // [roll, pitch, yaw, x, y, z]
// The tables over ids[0 .. n), all ids of the store; with pose_ids, t.poses = the stored pose of pose_ids[k] for keyframe k.
void lio_kf_sum_tables(const lio_kf_store* st, const int32_t* ids, const int32_t* pose_ids, int n, LioKfSum& t);
// t.kf, t.chunks and `poses` to the device on `s`; the host arrays must outlive the copies.  B: LioTemp or LioDevBytes.
template <class B> int lio_kf_sum_upload(const LioKfSum& t, const float* poses, B& d_kf, B& d_poses, B& d_chunks, hipStream_t s);
void lio_kf_transforms(LioKfDesc* d_kf, const float* d_poses, int n_kf, hipStream_t s);                // k_kf_transforms
// k_kf_transforms, then K6 into dst on `s`; nothing waits
void lio_kf_sum_launch(const lio_kf_store* st, LioKfDesc* d_kf, const float* d_poses, const int2* d_chunks, int n_sel, int n_chunks, float4* dst, hipStream_t s);

// ---- lio_mapbuild.hip: the selection of the surrounding keyframes, which the global map (lio_globalmap.hip) shares
// The buffers one selection works in: lio_assemble_map_nearby passes the store's, the global map its own.
struct LioNbBufs {
    LioVoxWs<LioDevBytes>& ws;
    LioDevBytes &pts, &cent, &cid, &ids, &meta, &d_kf, &d_poses;
};
// k_nb_select .. k_nb_compact on stream `s` over the uploaded key-pose table, then ONE wait for *hm (pinned): n_ids, n_chunks
// and total of the kept list, whose descriptors (T not yet filled), poses and ids lie in b.d_kf, b.d_poses and b.ids.
// recent = false leaves the suffix of MO:1544-1551 out (publishGlobalMap has none) and reads no key-pose time.
int lio_nb_select(lio_kf_store* st, LioNbBufs& b, float R, float density, bool recent, double time_cur, double window, LioNbMeta* hm,
                  hipStream_t s);
// the 256-point chunks of K6 for the kept list
void lio_nb_chunks(const LioKfDesc* kf, int n_sel, int2* chunks, hipStream_t s);
