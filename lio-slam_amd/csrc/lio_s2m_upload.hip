// lio_s2m_upload.hip -- the resident scan batch of a scan-to-map handle (include/liogpu.h): the upload with its tile sort,
// the corner batch of the point-to-line extension, the initial poses and the persistent degeneracy members.  What a
// caller wants of one upload (record layout, a pose to carry, how far to wait) is an argument, LioUploadOpts; the handle
// keeps only what describes the batch that is resident.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "lio_gridplan.h"
#include "lio_handle.h"
#include "lio_multi.h"
#include "lio_wg.h"

// The SoA copy of the resident batch, for the paths that read it, if the upload skipped it.
int lio_ensure_soa(lio_s2m_handle* h)
{
    if (h->soa_valid || !h->total_pts) return LIO_OK;
    lio_launch_aos_to_soa(h->last_stage + h->last_xyz_off, h->last_stride, (int)h->total_pts, h->d_sx, h->d_sy, h->d_sz, nullptr, h->stream);
    h->soa_valid = true;
    HIPCHK(hipGetLastError());
    return LIO_OK;
}

// The steps of lio_s2m_upload, in the order it takes them.

// The buffers every batch needs, sized for n_scans scans of tt points in all.
static int lio_upload_reserve(lio_s2m_handle* h, int n_scans, size_t tt, size_t stride)
{
    HIPCHK(h->d_sx.grow(tt));
    HIPCHK(h->d_sy.grow(tt));
    HIPCHK(h->d_sz.grow(tt));
    HIPCHK(h->d_stage.grow(tt * stride));
    HIPCHK(h->d_state.grow((size_t)n_scans));
    HIPCHK(h->d_poses.grow((size_t)n_scans * 6));
    // every launch leaves the counters at zero (the last workgroup of a scan re-arms it): clear at allocation only
    bool fresh = false;
    HIPCHK(h->d_arrive.grow((size_t)n_scans, 1.25, 64, false, &fresh));
    if (fresh) HIPCHK(hipMemsetAsync(h->d_arrive, 0, h->d_arrive.cap * sizeof(unsigned), h->stream));
    if (h->cfg.nn_cache && !h->cfg.use_lds) HIPCHK(h->d_nn_cache.grow(tt));
    return LIO_OK;
}

// Layout, on the host alone: the per-scan states (h_state), the workgroup list (v_blocks, with where each scan's
// workgroups start in it, v_first_orig) and the most workgroups any scan has (max_blk).  `pose`: see LioUploadOpts.
static void lio_upload_layout(lio_s2m_handle* h, int n_scans, const size_t* n_pts, const float* pose)
{
    // launch geometry: one workgroup = LIO_BLOCK * ppt consecutive points of one scan
    int ppt = h->cfg.kernel_variant;
    if (ppt != 1 && ppt != 2 && ppt != 4) ppt = 1;       // auto: one point per thread measured fastest at every batch size tried
    h->ppt = ppt;
    const size_t per_blk = (size_t)LIO_BLOCK * ppt;
    std::vector<LioBlockDesc>& blocks = h->v_blocks;
    blocks.clear();
    int max_blk = 1;
    const size_t old_scans = h->h_state.size();
    h->h_state.resize((size_t)n_scans);
    size_t off = 0;
    for (int s = 0; s < n_scans; ++s) {
        LioScanState& st = h->h_state[s];
        if ((size_t)s >= old_scans) memset(&st, 0, sizeof(st));   // keep matP / is_degenerate of live slots
        st.n_pts = (int)n_pts[s];
        st.offset = (int)off;
        if (pose && n_scans == 1) memcpy(st.pose, pose, sizeof(float) * 6);
        st.c_n_pts = 0;                // a corner batch has to be uploaded again after every surf batch
        st.c_offset = 0;
        st.done = 1;
        const int nb = (int)((n_pts[s] + per_blk - 1) / per_blk);
        // scan-range sharding ("replicate the map, shard the scan"): this rank takes one
        // block_world-th of the workgroups of every scan; the per-scan sums are all-reduced by the caller
        // a contiguous range of the (tile-sorted) workgroups, rotated from scan to scan so that no rank
        // always gets the same part of the sweep
        const int bw = h->block_world > 1 ? h->block_world : 1, br = h->block_world > 1 ? h->block_rank : 0;
        const int part = (br + s) % bw;
        const int b0 = (int)((long long)nb * part / bw), b1 = (int)((long long)nb * (part + 1) / bw);
        const int nb_local = b1 - b0;
        if (nb_local > max_blk) max_blk = nb_local;
        for (int b = b0; b < b1; ++b) blocks.push_back({ s, (int)(b * per_blk), b - b0, nb_local });
        off += n_pts[s];
    }
    h->v_first_orig.assign((size_t)n_scans + 1, 0);
    for (const LioBlockDesc& b : blocks) h->v_first_orig[b.scan + 1]++;
    for (int s = 0; s < n_scans; ++s) h->v_first_orig[s + 1] += h->v_first_orig[s];
    h->n_scans = n_scans;
    h->total_pts = off;
    h->n_blocks = (int)blocks.size();
    h->max_blk = max_blk;
}

// The caller's records as they are.  A batch that is one contiguous block in the caller's memory -- what a
// streaming front end keeps in a pinned ring -- goes to the device in ONE copy; pageable or scattered scans are
// copied one by one; a contiguous batch that already lives in THIS device's memory is not copied at all: the
// sort kernels read it in place (it must stay valid until the next lio_s2m_batch_sync / _results).
// *stage: where the records are on the device; *host_copy: the caller's (host) buffers are in flight, borrowed until the
// copy is done.
static int lio_upload_copy(lio_s2m_handle* h, int n_scans, const void* const* scans, const size_t* n_pts, size_t stride,
                           const unsigned char** stage, bool* host_copy)
{
    const size_t total = h->total_pts;
    *stage = h->d_stage;
    *host_copy = false;
    bool contiguous = true;
    for (int s = 0; s + 1 < n_scans && contiguous; ++s)
        contiguous = (const unsigned char*)scans[s + 1] == (const unsigned char*)scans[s] + n_pts[s] * stride;
    bool in_place = false;
    if (contiguous && total) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, scans[0]) == hipSuccess)
            in_place = at.type == hipMemoryTypeDevice && at.device == h->cfg.device_id;
        (void)hipGetLastError();                     // (pageable host memory is reported as an error)
    }
    if (in_place) {
        *stage = (const unsigned char*)scans[0];
    } else if (contiguous && total) {
        HIPCHK(hipMemcpyAsync(h->d_stage, scans[0], total * stride, hipMemcpyDefault, h->stream));
        *host_copy = true;
    } else {
        *host_copy = true;
        size_t o = 0;
        for (int s = 0; s < n_scans; ++s) {
            if (n_pts[s])
                HIPCHK(hipMemcpyAsync(h->d_stage + o * stride, scans[s], n_pts[s] * stride, hipMemcpyDefault, h->stream));
            o += n_pts[s];
        }
    }
    return LIO_OK;
}

// The tables of the launches on the device: the diagnostic records cleared, the workgroup list and the states copied up.
static int lio_upload_tables(lio_s2m_handle* h)
{
    const std::vector<LioBlockDesc>& blocks = h->v_blocks;
    const int n_scans = h->n_scans;
    const size_t tt = h->total_pts ? h->total_pts : 1;
    HIPCHK(h->d_blocks.grow(blocks.size() ? blocks.size() : 1));
    HIPCHK(h->d_partials.grow((size_t)n_scans * h->max_blk * LIO_SUMS));
    if (h->cfg.profile == 2) {
        HIPCHK(h->d_stamps.grow(blocks.size() * (LIO_BLOCK / 64) * 8 + 8));
        HIPCHK(hipMemsetAsync(h->d_stamps, 0, (blocks.size() * (LIO_BLOCK / 64) * 8 + 8) * sizeof(long long), h->stream));
    }
    if (h->cfg.record_corr_iter >= 0) {
        HIPCHK(h->d_rec_flag.grow(tt));
        HIPCHK(h->d_rec_coeff.grow(tt * 4));
        HIPCHK(h->d_rec_nn.grow(tt * 5));
        HIPCHK(hipMemsetAsync(h->d_rec_flag, 0, tt, h->stream));
        HIPCHK(hipMemsetAsync(h->d_rec_coeff, 0, tt * 4 * sizeof(float), h->stream));
        HIPCHK(hipMemsetAsync(h->d_rec_nn, 0xff, tt * 5 * sizeof(int), h->stream));
    }
    if (!blocks.empty())
        HIPCHK(hipMemcpyAsync(h->d_blocks, blocks.data(), blocks.size() * sizeof(LioBlockDesc),
                              hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_state, h->h_state.data(), (size_t)n_scans * sizeof(LioScanState),
                          hipMemcpyHostToDevice, h->stream));
    return LIO_OK;
}

// The tile sort of the scans' points (x at `stage`) into d_sx / d_sy / d_sz, with its permutation in d_perm: sets h->sorted.
// max_n: the points of the largest scan.
static int lio_upload_sort(lio_s2m_handle* h, const unsigned char* stage, size_t stride, const size_t* n_pts, size_t max_n)
{
    const int n_scans = h->n_scans;
    const size_t total = h->total_pts, tt = total ? total : 1;
    std::vector<LioScanTiles>& tiles = h->v_tiles;
    std::vector<LioBlockDesc>& prep = h->v_prep;
    tiles.clear(); prep.clear();
    h->sorted = false;
    // the tile sort pays for itself on batches; a lone small scan skips its eight launches
    const bool want_sort = total && (h->cfg.sort_scan >= 2 || (h->cfg.sort_scan == 1 && total >= 65536));
    // (up to 16383 points: the key (tile id << 14) | index of a 16384th point in tile 262143 would be the 0xffffffff that marks
    // an empty slot of k_scan_sort_radix)
    if (want_sort && max_n < 16384 && h->cfg.sort_scan != 3) {
        // every scan fits one workgroup's LDS: bounding box, tile keys, sort and gather in ONE launch, nothing read back
        HIPCHK(h->d_perm.grow(tt));
        lio_launch_scan_sort_lds(stage, stride, h->d_state, n_scans, (int)max_n, h->cfg.tile_size > 0.0f ? h->cfg.tile_size : 4.0f,
                                 h->shard.axis, h->d_perm, h->d_sx, h->d_sy, h->d_sz, h->stream);
        h->sorted = true;
    } else if (want_sort) {
        // scan-local tile grids from the scans' bounding boxes, reduced on the device (the caller's memory is
        // never read by the host: it may be pinned, pageable or device memory)
        for (int s = 0; s < n_scans; ++s) {
            const int nb1 = (int)((n_pts[s] + LIO_BLOCK - 1) / LIO_BLOCK);
            for (int b = 0; b < nb1; ++b) prep.push_back({ s, b * LIO_BLOCK, b, nb1 });
        }
        HIPCHK(h->d_prep_blocks.grow(prep.size()));
        HIPCHK(h->d_scan_bbox.grow((size_t)n_scans * 6));
        HIPCHK(h->h_scan_bbox.grow((size_t)n_scans * 6, (size_t)n_scans * 6 + 64));
        for (int s = 0; s < n_scans; ++s)
            lio_ord_box_clear(&h->h_scan_bbox[s * 6]);
        HIPCHK(hipMemcpyAsync(h->d_scan_bbox, h->h_scan_bbox, (size_t)n_scans * 6 * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_prep_blocks, prep.data(), prep.size() * sizeof(LioBlockDesc), hipMemcpyHostToDevice, h->stream));
        lio_launch_scan_bbox(stage, stride, h->d_prep_blocks, (int)prep.size(), h->d_state, h->d_scan_bbox, h->stream);
        HIPCHK(hipMemcpyAsync(h->h_scan_bbox, h->d_scan_bbox, (size_t)n_scans * 6 * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));          // (this handle's stream only: a sibling handle keeps computing)
        tiles.resize((size_t)n_scans);
        long long n_keys = 0;
        for (int s = 0; s < n_scans; ++s) {
            float mn[3], mx[3];
            for (int a = 0; a < 3; ++a) {
                const unsigned lo = h->h_scan_bbox[s * 6 + a], hi = h->h_scan_bbox[s * 6 + 3 + a];
                const bool none = lo == LIO_ORD_NO_MIN;
                mn[a] = none ? 0.0f : lio_ord2f(lo);
                mx[a] = none ? 0.0f : lio_ord2f(hi);
            }
            LioScanTiles t = lio_plan_scan_tiles(mn, mx, h->cfg.tile_size > 0.0f ? h->cfg.tile_size : 4.0f, h->shard.axis);
            t.key_offset = (int)n_keys;
            tiles[s] = t;
            n_keys += (long long)t.ntx * t.nty * t.ntz;
        }
        if (n_keys < 0x7fffffffLL - 1024) {
            HIPCHK(h->d_tiles.grow((size_t)n_scans));
            HIPCHK(h->d_key_of.grow(tt));
            HIPCHK(h->d_big_list.grow(tt / 1024 + 2));
            HIPCHK(h->d_tmp_idx.grow(tt));
            HIPCHK(h->d_perm.grow(tt));
            HIPCHK(h->d_key_count.grow((size_t)n_keys));
            HIPCHK(h->d_key_start.grow((size_t)n_keys + 1));
            HIPCHK(h->d_key_tiles.grow((size_t)lio_scan_tiles((int)n_keys) + 1));
            HIPCHK(hipMemcpyAsync(h->d_tiles, tiles.data(), tiles.size() * sizeof(LioScanTiles), hipMemcpyHostToDevice, h->stream));
            lio_launch_scan_tile_sort(stage, stride, (int)total, h->d_prep_blocks, (int)prep.size(), h->d_state,
                                      h->d_tiles, (int)n_keys, h->d_key_of, h->d_key_count, h->d_key_start,
                                      h->d_key_tiles, h->d_tmp_idx, h->d_perm, h->d_big_list, h->d_big_list + (h->d_big_list.cap - 1),
                                      h->d_sx, h->d_sy, h->d_sz, h->stream);
            h->sorted = true;
        }
    }
    return LIO_OK;
}

// The tail: the SoA copy of an unsorted batch (or its skip), the workgroup boxes of a sharded map, and the wait.
static int lio_upload_tail(lio_s2m_handle* h, const unsigned char* stage, size_t stride, int wait)
{
    const size_t total = h->total_pts, tt = total ? total : 1;
    h->soa_valid = true;
    if (total && !h->sorted) {
        // a batch the one-launch loop will take (lio_persist_eligible) reads its points once, from the records: no AoS -> SoA launch
        if (lio_persist_eligible(h, true)) h->soa_valid = false;
        else lio_launch_aos_to_soa(stage, stride, (int)total, h->d_sx, h->d_sy, h->d_sz, nullptr, h->stream);
    }
    h->has_block_box = false;
    if (h->shard.axis >= 0 && h->ppt == 1 && h->n_blocks > 0) {
        // map sharding: the box of every workgroup's points, for the cull at the head of k_s2m_iterate
        HIPCHK(h->d_block_box.grow((tt / LIO_BLOCK + (size_t)h->n_scans + 2) * 6));
        HIPCHK(h->d_blk_skip.grow((size_t)h->n_blocks));
        lio_launch_block_boxes(h->d_blocks, h->n_blocks, h->d_state, h->d_sx, h->d_sy, h->d_sz, h->d_block_box, h->stream);
        h->has_block_box = true;
    }
    if (wait == LIO_WAIT_STREAM) HIPCHK(hipStreamSynchronize(h->stream));   // the caller's scans are borrowed only for this call
    HIPCHK(hipGetLastError());
    return LIO_OK;
}

// lio_s2m_batch_upload (include/liogpu.h) with the record layout, a pose to carry and the wait as arguments: the checks, the
// host copy of the states brought up to date, then the steps above.  Buffers grow and work is enqueued in this order only.
int lio_s2m_upload(lio_s2m_handle* h, int32_t n_scans, const void* const* scans, const size_t* n_pts, size_t stride, const LioUploadOpts& o)
{
    if (!h || !scans || !n_pts) return lio_fail(LIO_ERR_ARG, "null argument");
    if (n_scans < 1) return lio_fail(LIO_ERR_ARG, "n_scans must be >= 1");
    if (stride < 12 || (stride & 3)) return lio_fail(LIO_ERR_ARG, "stride_bytes must be >= 12 and a multiple of 4");
    if (h->multi) return lio_multi_upload(h, n_scans, scans, n_pts, stride, o);
    int rc = lio_enter(h);
    if (rc != LIO_OK) return rc;
    size_t total = 0, max_n = 0;
    for (int s = 0; s < n_scans; ++s) {
        if (n_pts[s] && !scans[s]) return lio_fail(LIO_ERR_ARG, "null scan pointer");
        total += n_pts[s];
        if (n_pts[s] > max_n) max_n = n_pts[s];
    }
    if (total > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "batch too large");
    h->run_pending = false;            // (a run whose results were never fetched is abandoned)
    if (h->host_state_stale && h->n_scans > 0 && h->d_state) {
        // the persistent members (matP / isDegenerate, MO:176-177) live in the device copy: bring the host copy
        // up to date before it is edited and uploaded again
        HIPCHK(hipMemcpyAsync(h->h_state.data(), h->d_state, (size_t)h->n_scans * sizeof(LioScanState),
                              hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    h->host_state_stale = false;
    if ((rc = lio_upload_reserve(h, n_scans, total ? total : 1, stride)) != LIO_OK) return rc;
    lio_upload_layout(h, n_scans, n_pts, o.pose);
    const unsigned char* stage = nullptr;
    bool host_copy = false;
    if ((rc = lio_upload_copy(h, n_scans, scans, n_pts, stride, &stage, &host_copy)) != LIO_OK) return rc;
    if (host_copy && o.wait == LIO_WAIT_COPY) {
        HIPCHK(hipEventRecord(h->ev_map[0], h->stream));   // (async upload: wait for the H2D only, the sort stays in flight)
        HIPCHK(hipEventSynchronize(h->ev_map[0]));
    }
    h->last_stage = stage; h->last_stride = stride; h->last_xyz_off = o.xyz_off;
    h->last_int_off = o.int_off != -2 ? o.int_off : ((o.xyz_off == 0 && stride >= 20) ? 16 : -1);
    stage += o.xyz_off;                                  // (x, y, z are read at +0, +4, +8 from here; xyz_off + 12 <= stride)
    if ((rc = lio_upload_tables(h)) != LIO_OK) return rc;
    if ((rc = lio_upload_sort(h, stage, stride, n_pts, max_n)) != LIO_OK) return rc;
    if ((rc = lio_upload_tail(h, stage, stride, o.wait)) != LIO_OK) return rc;
    h->poses_set = false;
    h->pose_in_state = o.pose != nullptr && n_scans == 1;
    h->ran = false;
    h->graph_dirty = true;
    h->corner_active = false;
    return LIO_OK;
}

extern "C" int lio_s2m_batch_upload(lio_s2m_handle* h, int32_t n_scans, const void* const* scans,
                                    const size_t* n_pts, size_t stride)
try {
    return lio_s2m_upload(h, n_scans, scans, n_pts, stride, LioUploadOpts());
} LIO_CATCH

extern "C" int lio_s2m_batch_upload_async(lio_s2m_handle* h, int32_t n_scans, const void* const* scans,
                                          const size_t* n_pts, size_t stride)
try {
    if (!h) return lio_fail(LIO_ERR_ARG, "null handle");
    LioUploadOpts o;
    o.wait = LIO_WAIT_COPY;
    return lio_s2m_upload(h, n_scans, scans, n_pts, stride, o);
} LIO_CATCH

// ------------------------------------------------- corner residuals (extension)
extern "C" int lio_s2m_set_corner_map(lio_s2m_handle* h, const void* pts, size_t n, size_t stride)
try {
    if (!h) return lio_fail(LIO_ERR_ARG, "null handle");
    if (h->multi) return lio_fail(LIO_ERR_ARG, "the corner extension is not available on a multi-device handle");
    if (const int rc = lio_enter(h); rc != LIO_OK) return rc;
    if (!h->corner) {
        lio_s2m_config cc = h->cfg;
        cc.kernel_variant = 1;         // edge sets are small: one point per thread, candidates from global memory
        cc.use_lds = 0;
        cc.profile = 0;
        cc.use_graph = 0;
        cc.pipeline = 1;               // the edge launch is the fused kernel's CORNER instantiation
        int rc = lio_s2m_create(&cc, &h->corner);
        if (rc != LIO_OK) return rc;
        if ((rc = lio_s2m_set_stream(h->corner, h->stream)) != LIO_OK) return rc;
    }
    h->corner_active = false;
    h->graph_dirty = true;
    return lio_s2m_set_map(h->corner, pts, n, stride);
} LIO_CATCH

int lio_s2m_upload_corners(lio_s2m_handle* h, int32_t n_scans, const void* const* scans, const size_t* n_pts, size_t stride, int wait)
{
    if (!h || !scans || !n_pts) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!h->corner || !h->corner->has_map) return lio_fail(LIO_ERR_NO_MAP, "set_corner_map has not been called");
    if (h->n_scans < 1 || n_scans != h->n_scans)
        return lio_fail(LIO_ERR_ARG, "upload the surf batch first; the corner batch must have the same number of scans");
    lio_s2m_handle* ch = h->corner;
    ch->block_rank = h->block_rank;
    ch->block_world = h->block_world;
    LioUploadOpts o;
    o.wait = wait;
    int rc = lio_s2m_upload(ch, n_scans, scans, n_pts, stride, o);
    if (rc != LIO_OK) return rc;
    // One arrival counter and one partial-sum table per scan serve both launches: the scan's corner
    // chunks are numbered after its surf chunks (combineOptimizationCoeffs appends one list to the other).
    int max_blk = 1;
    for (LioBlockDesc& b : h->v_blocks) {
        const int ns = h->v_first_orig[b.scan + 1] - h->v_first_orig[b.scan];
        const int nc = ch->v_first_orig[b.scan + 1] - ch->v_first_orig[b.scan];
        b.n_blk = ns + nc;
        if (b.n_blk > max_blk) max_blk = b.n_blk;
    }
    for (LioBlockDesc& b : ch->v_blocks) {
        const int ns = h->v_first_orig[b.scan + 1] - h->v_first_orig[b.scan];
        const int nc = ch->v_first_orig[b.scan + 1] - ch->v_first_orig[b.scan];
        b.blk += ns;
        b.n_blk = ns + nc;
        if (b.n_blk > max_blk) max_blk = b.n_blk;
    }
    h->max_blk = max_blk;
    HIPCHK(h->d_partials.grow((size_t)n_scans * max_blk * LIO_SUMS));
    if (!h->v_blocks.empty())
        HIPCHK(hipMemcpyAsync(h->d_blocks, h->v_blocks.data(), h->v_blocks.size() * sizeof(LioBlockDesc),
                              hipMemcpyHostToDevice, h->stream));
    if (!ch->v_blocks.empty())
        HIPCHK(hipMemcpyAsync(ch->d_blocks, ch->v_blocks.data(), ch->v_blocks.size() * sizeof(LioBlockDesc),
                              hipMemcpyHostToDevice, h->stream));
    for (int s = 0; s < n_scans; ++s) {
        h->h_state[s].c_n_pts = ch->h_state[s].n_pts;
        h->h_state[s].c_offset = ch->h_state[s].offset;
    }
    HIPCHK(hipMemcpyAsync(h->d_state, h->h_state.data(), (size_t)n_scans * sizeof(LioScanState),
                          hipMemcpyHostToDevice, h->stream));
    if (wait == LIO_WAIT_STREAM) HIPCHK(hipStreamSynchronize(h->stream));
    h->corner_active = true;
    h->poses_set = false;             // (the workgroup list was rewritten: batch_set_poses re-orders it)
    h->graph_dirty = true;
    return LIO_OK;
}

extern "C" int lio_s2m_batch_upload_corners(lio_s2m_handle* h, int32_t n_scans, const void* const* scans,
                                            const size_t* n_pts, size_t stride)
try {
    return lio_s2m_upload_corners(h, n_scans, scans, n_pts, stride, LIO_WAIT_STREAM);
} LIO_CATCH

int lio_s2m_set_poses(lio_s2m_handle* h, const float* poses, int wait)
{
    if (!h || !poses) return lio_fail(LIO_ERR_ARG, "null argument");
    if (h->n_scans < 1) return lio_fail(LIO_ERR_ARG, "no batch uploaded");
    if (h->multi) return lio_multi_set_poses(h, poses);
    if (const int rc = lio_enter(h); rc != LIO_OK) return rc;
    h->run_pending = false;           // (a run whose results were never fetched is abandoned)
    h->pose_in_state = false;
    HIPCHK(hipMemcpyAsync(h->d_poses, poses, (size_t)h->n_scans * 6 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (h->cfg.sort_batch && h->n_scans > 8 && !h->v_blocks.empty()) {
        // Locality only: order the workgroup list by where the scans ARE (position along the map's
        // longest axis).  Together with the XCD-aware workgroup order every XCD then streams the
        // map rows of one stretch of the trajectory, which fit its private 4 MB L2.
        const LioGrid& mg = lio_map_of(h)->grid;
        const float ext[3] = { (float)mg.nx, (float)mg.ny, (float)mg.nz };
        const int ax = (ext[0] >= ext[1] && ext[0] >= ext[2]) ? 0 : (ext[1] >= ext[2] ? 1 : 2);
        std::vector<int>& order = h->v_order;
        order.resize((size_t)h->n_scans);
        for (int s = 0; s < h->n_scans; ++s) order[s] = s;
        std::stable_sort(order.begin(), order.end(),
                         [&](int a, int b) { return poses[a * 6 + 3 + ax] < poses[b * 6 + 3 + ax]; });
        // v_blocks is grouped by scan in upload order: gather the groups in the new order
        std::vector<int>& first = h->v_first;
        first.assign((size_t)h->n_scans + 1, 0);
        for (const LioBlockDesc& b : h->v_blocks) first[b.scan + 1]++;
        for (int s = 0; s < h->n_scans; ++s) first[s + 1] += first[s];
        std::vector<LioBlockDesc>& sorted = h->v_blocks_sorted;
        sorted.clear();
        sorted.reserve(h->v_blocks.size());
        // (v_blocks itself stays in scan order so that the grouping survives repeated calls)
        for (int k = 0; k < h->n_scans; ++k) {
            const int s = order[k];
            // blocks of scan s are the ones whose .scan == s; they are contiguous in the ORIGINAL list
            for (int i = h->v_first_orig[s]; i < h->v_first_orig[s + 1]; ++i) sorted.push_back(h->v_blocks[i]);
        }
        HIPCHK(hipMemcpyAsync(h->d_blocks, sorted.data(), sorted.size() * sizeof(LioBlockDesc), hipMemcpyHostToDevice, h->stream));
    }
    if (wait == LIO_WAIT_STREAM) HIPCHK(hipStreamSynchronize(h->stream));
    h->poses_set = true;
    return LIO_OK;
}

extern "C" int lio_s2m_batch_set_poses(lio_s2m_handle* h, const float* poses)
try {
    return lio_s2m_set_poses(h, poses, LIO_WAIT_STREAM);
} LIO_CATCH

extern "C" int lio_s2m_set_degeneracy(lio_s2m_handle* h, int32_t scan, const float matP[36], int32_t is_degenerate)
try {
    if (!h || !matP) return lio_fail(LIO_ERR_ARG, "null argument");
    if (scan < 0 || scan >= h->n_scans) return lio_fail(LIO_ERR_ARG, "scan slot out of range");
    if (h->multi) return lio_multi_set_degeneracy(h, scan, matP, is_degenerate);
    if (const int rc = lio_enter(h); rc != LIO_OK) return rc;
    LioScanState& st = h->h_state[scan];
    memcpy(st.matP, matP, sizeof(float) * 36);
    st.is_degenerate = is_degenerate;
    char* base = (char*)(h->d_state + scan);
    HIPCHK(hipMemcpyAsync(base + offsetof(LioScanState, matP), st.matP, sizeof(float) * 36, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(base + offsetof(LioScanState, is_degenerate), &st.is_degenerate, sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return LIO_OK;
} LIO_CATCH

// Internal (lio_handle.h): the staged records of batch slot `scan` as they were uploaded.
int lio_s2m_staged_scan(lio_s2m_handle* h, int scan, const unsigned char** d_rec, size_t* n, size_t* stride, size_t* xyz_off, int* int_off,
                        int* device_id, hipStream_t* stream)
{
    if (!h || scan < 0 || scan >= h->n_scans || !h->last_stage) return lio_fail(LIO_ERR_ARG, "no such resident scan");
    const LioScanState& st = h->h_state[scan];
    *d_rec = h->last_stage + (size_t)st.offset * h->last_stride;
    *n = (size_t)st.n_pts; *stride = h->last_stride; *xyz_off = h->last_xyz_off; *int_off = h->last_int_off;
    *device_id = h->cfg.device_id; *stream = h->stream;
    return LIO_OK;
}
