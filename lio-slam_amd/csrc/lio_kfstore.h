// lio_kfstore.h -- what lio_globalmap.hip shares with lio_mapbuild.hip: the resident keyframe store, the descriptors of K6,
// the workspace of K7, the staged cloud of lio_s2m_register_raw, and the launches of lio_mapbuild.hip's kernels that the
// global map and the map export reuse (the selection k_nb_select .. k_nb_compact, K6, K7, the record conversions).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#include "../../include/liogpu.h"
#include "lio_pool.h"
#include "lio_sc.h"

struct LioKfDesc {       // one selected keyframe
    int src;             // first point of the keyframe in the resident store
    int first;           // first point in the concatenated world-frame cloud
    int n;
    int pad;
    float T[12];         // pclPointToAffine3f of its pose (MO:856), filled on the device
};

// B: LioTemp (pool temporaries, recycled when the call returns) or LioDevBytes (a workspace kept from one call to the next,
// so that nothing has to be waited for before the call returns)
template <class B> struct LioVoxWs { B bbox, large, pairs_a, pairs_b, hist, blk_heads, seg_start, d_no, row_total; };

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
    std::vector<LioKfDesc> v_kf;
    std::vector<int2> v_chunks;
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

// ---- lio_mapbuild.hip, for lio_globalmap.hip
int lio_mb_check_device(int device_id);
// the dirty range of the key-pose table (and off / cnt) to the device, on stream `s`, through the store's pinned stage
int lio_mb_upload_pose_tab(lio_kf_store* st, hipStream_t s);

// The buffers one selection works in: lio_assemble_map_nearby passes the store's, the global map its own.
struct LioNbBufs {
    LioVoxWs<LioDevBytes>& ws;
    LioDevBytes &pts, &cent, &cid, &ids, &meta, &d_kf, &d_poses;
};
// k_nb_select .. k_nb_compact on stream `s` over the uploaded key-pose table, then ONE wait for *hm (pinned): n_ids, n_chunks
// and total of the kept list, whose descriptors (T not yet filled), poses and ids lie in b.d_kf, b.d_poses and b.ids.
// recent = false leaves the suffix of MO:1544-1551 out (publishGlobalMap has none) and reads no key-pose time.
int lio_mb_select(lio_kf_store* st, LioNbBufs& b, float R, float density, bool recent, double time_cur, double window, LioNbMeta* hm,
                  hipStream_t s);
void lio_mb_launch_nb_chunks(const LioKfDesc* kf, int n_sel, int2* chunks, hipStream_t s);
void lio_mb_launch_kf_transforms(LioKfDesc* kf, const float* poses, int n_kf, hipStream_t s);          // k_kf_transforms
void lio_mb_launch_transform_clouds(const float4* store, const LioKfDesc* kf, const int2* chunks, int n_chunks, float4* dst,
                                    hipStream_t s);                                                    // K6
void lio_mb_launch_rec_to_xyzi4(const unsigned char* src, size_t stride, size_t xyz_off, int int_off, int n, float4* dst, hipStream_t s);
// K7 with a workspace kept between calls; LIO_OK, 1 for PCL's pass-through, < 0 on error.  Complete when it returns.
int lio_mb_voxel_grid(const float4* d_in, int n, float leaf, LioDevBytes& out, int* n_out, hipStream_t s, LioVoxWs<LioDevBytes>& ws);
// n float4 (x, y, z, intensity) -> PointXYZI-compatible host records; waits for `s`
int lio_mb_copy_out(const float4* d_pts, int n, void* out, size_t out_stride, hipStream_t s);
