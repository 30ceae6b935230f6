// lio_handle.h -- the opaque handle behind include/liogpu.h, and what the files that implement its scan-to-map entries
// (liogpu_api.hip, lio_s2m_map.hip, lio_s2m_upload.hip, lio_s2m_run.hip) offer one another and the files that work on a
// handle (lio_multi.hip, lio_mapbuild.hip, lio_kfstore.hip, lio_globalmap.hip, lio_debug_math.hip).  Host-side only; the
// error plumbing and the buffer types it is built from are in lio_pool.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/liogpu.h"
#include "lio_kernels.h"
#include "lio_pool.h"
#include "lio_types.h"

void lio_raw_ws_free(struct LioRawWs* ws);                 // lio_mapbuild.hip

// What one upload is told by its caller.  Nothing of it outlives the call.
enum { LIO_WAIT_STREAM = 0, LIO_WAIT_COPY = 1, LIO_WAIT_NONE = 2 };   // what the call waits for before it returns
struct LioUploadOpts {
    size_t xyz_off = 0;           // byte offset of x inside a record
    int int_off = -2;             // FLOAT32 intensity: -1 none, -2 PCL convention (byte 16 of a record of >= 20 bytes with x at byte 0)
    const float* pose = nullptr;  // one scan only: the guess rides inside the state upload
    int wait = LIO_WAIT_STREAM;   // LIO_WAIT_STREAM | LIO_WAIT_COPY (H2D only) | LIO_WAIT_NONE
};

// ---- liogpu_api.hip
void lio_consts_from_config(const lio_s2m_config& g, LioConsts& c);

// ---- lio_s2m_map.hip, for the map builders and the keyframe store
int lio_s2m_set_map_device_xyzi(lio_s2m_handle* h, const float4* d_xyzi, size_t n);
int lio_s2m_set_map_device_bbox(lio_s2m_handle* h, const float4* d_xyzi, size_t n, const float box[6]);
hipStream_t lio_s2m_stream_of(lio_s2m_handle* h);
bool lio_s2m_takes_device_map(const lio_s2m_handle* h);

// ---- lio_s2m_upload.hip: the public entries of the same names with what they read as arguments
// (`wait` of the last two: LIO_WAIT_STREAM or LIO_WAIT_NONE)
int lio_s2m_upload(lio_s2m_handle* h, int32_t n_scans, const void* const* scans, const size_t* n_pts, size_t stride, const LioUploadOpts& o);
int lio_s2m_upload_corners(lio_s2m_handle* h, int32_t n_scans, const void* const* scans, const size_t* n_pts, size_t stride, int wait);
int lio_s2m_set_poses(lio_s2m_handle* h, const float* poses, int wait);
int lio_ensure_soa(lio_s2m_handle* h);
// the staged records of batch slot `scan` as they were uploaded
int lio_s2m_staged_scan(lio_s2m_handle* h, int scan, const unsigned char** d_rec, size_t* n, size_t* stride, size_t* xyz_off, int* int_off,
                        int* device_id, hipStream_t* stream);

// ---- lio_s2m_run.hip
bool lio_persist_eligible(const lio_s2m_handle* h, bool allow_one_launch);
int lio_pc2_check_xyz(const lio_pc2_layout* L);
// lio_s2m_register on records laid out as `o` says (its pose and wait are set inside)
int lio_s2m_register_opts(lio_s2m_handle* h, const void* scan, size_t n, size_t stride, float pose[6], lio_s2m_result* res, LioUploadOpts o);

// What a captured chunk of GN launches depends on.  Built zeroed and compared as bytes: padding takes part, as in run_P.
struct LioGraphKey {
    int chunk, blocks, ppt;
    bool plain;                       // the plain_kernel switch
    int tail_from, tail_wgs;
    int blocks_c;                     // workgroups of the corner launch; -1 = none, and params_c stays zero
    LioIterParams params, params_c;   // arguments of the surface and of the corner launch
};

// Owns everything it points to except `map_src` and a stream installed by lio_s2m_set_stream (own_stream == false); the
// destructor releases it on the current device, which lio_s2m_destroy sets.
struct lio_s2m_handle {
    ~lio_s2m_handle();                // liogpu_api.hip
    lio_s2m_config cfg;
    LioConsts c;
    hipStream_t stream = nullptr;
    bool own_stream = true;

    // ---- resident local map (laserCloudSurfFromMapDS, MO:149) ----
    bool has_map = false;
    size_t n_map = 0;
    LioDevBuf<float> d_mx, d_my, d_mz;
    LioDevBuf<float4> d_map4, d_sorted, d_nbr_pts;
    LioDevBuf<int> d_cell_of, d_cell_count, d_cell_start, d_tile_sums, d_nbr_start;
    LioDevBuf<int> d_nbr_slot;                 // [n_map][(2k+1)^2] place of every replica inside its row-cell list
    LioDevBuf<unsigned> d_bbox;
    LioDevBuf<unsigned char> d_stage;          // the resident batch's records as uploaded
    LioDevBuf<unsigned char> d_map_stage;      // lio_s2m_set_map's upload (its own buffer: the batch's staged records stay
                                               // valid -- the one-launch loop and lio_kf_store_add_from_handle read them
                                               // after a new map)
    LioGrid grid{};

    // ---- resident scan batch (laserCloudSurfLastDS, MO:138) ----
    int n_scans = 0;
    size_t total_pts = 0;
    LioDevBuf<float> d_sx, d_sy, d_sz;
    LioDevBuf<LioScanState> d_state;
    std::vector<LioScanState> h_state;
    std::vector<LioBlockDesc> v_blocks, v_prep;      // launch descriptors (kept alive for async H2D)
    std::vector<LioScanTiles> v_tiles;
    std::vector<LioBlockDesc> v_blocks_sorted;       // v_blocks re-ordered by scan position (sort_batch)
    std::vector<int> v_order, v_first, v_first_orig;
    LioDevBuf<float> d_poses;
    bool pose_in_state = false;       // the initial guess went up inside the state (LioUploadOpts::pose): the next k_s2m_init_state
                                      // takes it from there (and copies it to d_poses)
    LioDevBuf<float> d_summary;       // [n_scans][10] compact results (lio_s2m_batch_results without `results`)
    LioPinned<float> h_summary;
    bool host_state_stale = false;    // h_state misses device-side updates (matP ...) since a summary-only read
    LioDevBuf<LioBlockDesc> d_blocks;
    int n_blocks = 0, ppt = 1, max_blk = 1;
    LioDevBuf<double> d_partials;
    LioDevBuf<unsigned> d_arrive;
    bool poses_set = false, ran = false;
    // upload-time tile sort of the scans
    LioDevBuf<LioScanTiles> d_tiles;
    LioDevBuf<LioBlockDesc> d_prep_blocks;
    LioDevBuf<int> d_key_of, d_key_count, d_key_start, d_key_tiles, d_tmp_idx, d_perm;
    LioDevBuf<float> d_block_box;     // map sharding: per-workgroup bounding boxes (cull)
    bool has_block_box = false;
    LioDevBuf<unsigned char> d_blk_skip;
    LioDevBuf<int> d_big_list;        // tiles with more than LIO_TILE_CAP points (+ their count in the last slot)
    LioDevBuf<unsigned> d_scan_bbox;  // [n_scans][6] ordered-uint bounding boxes
    LioPinned<unsigned> h_scan_bbox;  // its host mirror
    bool sorted = false;
    const unsigned char* last_stage = nullptr;   // the records of the resident batch as uploaded (d_stage, or the caller's device buffer)
    size_t last_stride = 0, last_xyz_off = 0;
    int last_int_off = -1;               // byte offset of their FLOAT32 intensity, -1 = none (lio_kf_store_add_from_handle)
    struct LioRawWs* raw_ws = nullptr;   // lio_s2m_register_raw: staged cloud + voxel-filter workspace (lio_mapbuild.hip)
    int persist_fallbacks = 0;           // one-launch loops that timed out and were re-run through the launch loop
    unsigned persist_spin_max = 0;       // polls before a waiting workgroup gives up (0 = default, LIO_PERSIST_SPIN_MAX in the environment)
    int persist_withhold = -1;           // test hook (lio_s2m_debug_persist_spin)
    lio_s2m_handle* map_src = nullptr;   // lio_s2m_share_map: the handle whose resident map this one searches
    unsigned long long map_epoch = 0;    // bumped by every set_map
    LioDevBuf<float> d_nn_cache;         // [total_pts] squared 5th-neighbour distance of the previous GN iteration
    LioDevBuf<long long> d_stamps;
    // one-launch loop (cfg.pipeline = 4, k_s2m_persist): per-scan generation numbers
    LioDevBuf<unsigned> d_gen;        // [2][d_gen.cap / 2]: generation numbers, then the speculation states
    LioDevBuf<double> d_spec_sums;    // sums of the first solve of every scan (roll-back of the speculation)
    unsigned gen_epoch = 0;           // grows by 128 per run: generation numbers are never cleared
    int n_cu = 0;                     // compute units of the device: every workgroup of a one-launch loop must be resident
    bool run_persist = false;
    bool soa_valid = true;            // d_sx/d_sy/d_sz hold the resident batch (false: a one-launch batch still only staged as records)
    // hipGraph-captured chunk of GN iterations (cfg.use_graph)
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    bool graph_dirty = true;
    LioGraphKey graph_key{};          // what the cached graph was captured under
    int units_this_run = 0, unit_iters = 1;
    bool plain_kernel = true;         // LIO_PLAIN_KERNEL=0 in the environment at lio_s2m_create: always the general k_s2m_iterate (A/B runs)
    int iterate_variant = 0;          // instantiation of the last run's surface launches (lio_s2m_kernel_variant)
    // Looped form of the plain kernel for the late launches of a run (k_s2m_iterate_tail), read from the environment at lio_s2m_create:
    int tail_from = LIO_TAIL_FROM_DEFAULT;   // LIO_TAIL_FROM: launches whose index within the run is >= this take it; -1 = never, 0 = all
    int tail_wgs = LIO_TAIL_WGS_DEFAULT;     // LIO_TAIL_WGS: its grid, a multiple of 8 (>= 8)
    int graph_n_full = 0, graph_n_looped = 0;       // surface launches of each form in the cached graph
    int run_n_full = 0, run_n_looped = 0;           // ... enqueued by the last run (lio_s2m_launch_forms)

    // correspondence record (debug / parity)
    LioDevBuf<unsigned char> d_rec_flag;
    LioDevBuf<float> d_rec_coeff;
    LioDevBuf<int> d_rec_nn;

    // in-library multi-GPU mode (cfg.n_devices > 1): this handle is only a front; see struct LioMulti
    struct LioMulti* multi = nullptr;

    // resumable launch loop (lio_s2m_batch_run / lio_run_continue)
    bool run_pending = false, run_graph = false, run_has_c = false;
    int run_next = 0, run_units = 0, run_look = 0;
    LioIterParams run_P, run_Pc;

    // sharding
    LioShard shard{};
    float gorigin[3] = {0, 0, 0};
    int gdims[3] = {0, 0, 0};
    bool has_global = false;
    int block_rank = 0, block_world = 1;   // scan-range sharding
    int plan_ranks = 0, plan_rank = 0, plan_halo = 1, plan_bounds[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // lio_s2m_set_shard_plan

    // EXTENSION: point-to-line residuals.  `corner` is a child handle that owns the corner
    // map (its grid and neighbourhood rows) and the batch of edge points; its association launch writes
    // into THIS handle's per-scan partial sums and state.
    lio_s2m_handle* corner = nullptr;
    bool corner_active = false;       // a corner batch matching the current surf batch is resident

    // profiling
    hipEvent_t ev_beg[LIO_MAX_ITERS] = {}, ev_end[LIO_MAX_ITERS] = {}, ev_chk[LIO_MAX_ITERS] = {};
    hipEvent_t ev_map[2] = {};
    hipEvent_t ev_mapl[2] = {};        // asynchronous map installation (lio_s2m_set_map_device_bbox): build time resolved on demand; [1] = "map ready"
    bool map_timing_pending = false;
    LioPinned<int> h_active;          // active-scan count after each launch
    lio_s2m_profile prof{};
    int launches_this_run = 0;
    LioDevBuf<int> d_active;
};

// the handle whose resident map h searches (a sibling's after lio_s2m_share_map)
static inline const lio_s2m_handle* lio_map_of(const lio_s2m_handle* h) { return h->map_src ? h->map_src : h; }

// Head of every entry that enqueues on a handle: its device made current, and stale codes left by other HIP users of this
// thread (e.g. hipErrorNotReady) dropped.
static inline int lio_enter(const lio_s2m_handle* h)
{
    HIPCHK(hipSetDevice(h->cfg.device_id));
    (void)hipGetLastError();
    return LIO_OK;
}

static inline int lio_refuse_multi(void)
{
    return lio_fail(LIO_ERR_ARG, "not available on a multi-device handle (cfg.n_devices > 1 shards inside the library)");
}
