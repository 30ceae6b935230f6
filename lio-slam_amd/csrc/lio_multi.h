// lio_multi.h -- in-library multi-GPU mode (lio_multi.hip), called by the scan-to-map entry points (liogpu_api.hip,
// lio_s2m_map.hip, lio_s2m_upload.hip, lio_s2m_run.hip) for handles created with cfg.n_devices > 1.
#pragma once
#include <memory>
#include <vector>

#include "lio_handle.h"

// One device of a multi-device handle: its child handle and what the exchange keeps for it (lio_multi.hip).
struct LioMultiChild {
    ~LioMultiChild();
    lio_s2m_handle* h = nullptr;
    LioDevBuf<double> d_part;                         // its partial sums [n_scans][LIO_SUMS]
    LioDevBuf<double> d_gather;                       // [2 parities][n_dev slots][slot_scans][LIO_SUMS]
    LioDevBuf<double> d_tot;                          // (host exchange only)
    LioPinned<double> h_part;                         // (host exchange only) its partial sums on the host
    hipEvent_t ev_pub[LIO_MAX_ITERS] = {};            // its publish of each iteration
    std::vector<int> shard_idx;                       // caller's map index of every point of its shard
};

// The state of a handle created with cfg.n_devices > 1 (lio_s2m_handle::multi).  The destructor releases every child with
// its device current.
struct LioMulti {
    ~LioMulti();
    std::vector<std::unique_ptr<LioMultiChild>> dev;
    LioPinned<double> h_tot;                          // (host exchange only)
    int join_device = 0;
    hipStream_t join_stream = nullptr;                // four devices and more: ONE stream waits for all publish events of an iteration
    hipEvent_t ev_all[LIO_MAX_ITERS] = {};            // ... and records "everybody has published" for every device to wait on
    size_t slot_scans = 0;                            // scans a gather slot holds
    std::vector<unsigned char> gather;                // host staging of one shard's records
    int n_scans = 0;
    int exchange = 0;                                 // 0 = peer stores from a kernel, 1 = hipMemcpyPeerAsync, 2 = through the host (round 2)
    bool peer_ok = true;
    // diagnostics of the last run (lio_s2m_profile.multi_*)
    int stream_syncs = 0, event_waits = 0, iterations = 0;
};

int  lio_multi_create(const lio_s2m_config* cfg, lio_s2m_handle** out);
void lio_multi_destroy(lio_s2m_handle* h);
int  lio_multi_set_map(lio_s2m_handle* h, const void* pts, size_t n, size_t stride);
int  lio_multi_upload(lio_s2m_handle* h, int32_t n_scans, const void* const* scans, const size_t* n_pts, size_t stride, const LioUploadOpts& o);
int  lio_multi_set_poses(lio_s2m_handle* h, const float* poses);
int  lio_multi_set_degeneracy(lio_s2m_handle* h, int32_t scan, const float matP[36], int32_t is_degenerate);
int  lio_multi_run(lio_s2m_handle* h);
int  lio_multi_sync(lio_s2m_handle* h);
int  lio_multi_results(lio_s2m_handle* h, float* poses, lio_s2m_result* results);
int  lio_multi_get_correspondences(lio_s2m_handle* h, int32_t scan, uint8_t* flag, float* coeff4, int32_t* nn_idx5);

// lio_s2m_run.hip: lio_s2m_batch_iter_apply for sums that arrive as `n_slots` partial tables of `slot_stride` doubles each
// (one per device, added in slot order inside the solving kernel).
int  lio_s2m_iter_apply_slots(lio_s2m_handle* h, const double* d_slots, size_t slot_stride, int n_slots);
