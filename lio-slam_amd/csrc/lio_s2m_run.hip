// lio_s2m_run.hip -- the Gauss-Newton loop of a scan-to-map handle (include/liogpu.h) on the batch that is resident: the
// launch loop (resumable, optionally as replays of a captured graph), the whole loop as one launch, the iteration-wise
// entries of the sharded modes, the results, and the registrations that chain upload, poses, run and results in one call.
// MO = mapOptmization.cpp of the reference (liorf).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "lio_handle.h"
#include "lio_multi.h"

// The whole Gauss-Newton loop as one launch (k_s2m_persist, lio_persist.hip): possible when every workgroup of the batch is
// resident at once and the batch uses nothing but the default surf association; measured faster than the launch loop
// for every batch that fits (0.17 against 0.25 ms for a lone registration).  cfg.pipeline = 4 takes
// it for up to one workgroup per compute unit; auto (0) for up to half of that -- a lone registration is ~26 workgroups
// at the default 0.4 m scan leaf, 76 / 111 at the reference's 0.2 / 0.15 m leaves (6-8 % faster there than the launch loop,
// profiles/r03_callback_leaf_sizes.txt) --, so that two handles doing so at the same time still fit the device together (a
// workgroup that waits at its scan's barrier keeps its slot; the polls are bounded, and a launch that cannot make progress
// is re-run through the launch loop inside lio_s2m_batch_results: a few milliseconds, never an error).
// Auto steps aside for an explicit cfg.use_graph and for the diagnostic phase clock of the launch loop (cfg.profile = 2).
// `allow_one_launch` is false for that re-run alone: the launch loop, whatever cfg.pipeline says.
bool lio_persist_eligible(const lio_s2m_handle* h, bool allow_one_launch)
{
    int limit = 0;
    if (h->cfg.pipeline == 4) limit = h->n_cu;
    else if (h->cfg.pipeline == 0 && !h->cfg.use_graph && h->cfg.profile != 2) limit = h->n_cu / 2;
    return limit > 0 && allow_one_launch && !h->cfg.use_lds && h->ppt == 1 && h->shard.axis < 0 &&
           h->block_world == 1 && h->n_blocks > 0 && h->n_blocks + h->n_scans <= limit;      // (+ one helper workgroup per scan)
}

// Polls before a workgroup of the one-launch loop stops waiting for its scan's solve.  A poll is a short sleep plus one
// L2-bypassing load (~1-2 us): the default of 4096 bounds a stalled launch to a few milliseconds, after which the host re-runs
// the registration through the launch loop (lio_s2m_batch_results).  A healthy solve is answered within ~50 us.
static unsigned lio_persist_spin_max(const lio_s2m_handle* h)
{
    if (h->persist_spin_max) return h->persist_spin_max;
    static const unsigned env = [] { const char* e = getenv("LIO_PERSIST_SPIN_MAX"); const long v = e ? atol(e) : 0; return v > 0 ? (unsigned)v : 4096u; }();
    return env;
}

static void lio_fill_params(lio_s2m_handle* h, LioIterParams& P, double* sums_out)
{
    const lio_s2m_handle* m = lio_map_of(h);       // (a sibling's resident map after lio_s2m_share_map)
    P.grid = m->grid;
    P.shard = h->shard;
    P.c = h->c;
    P.map_sorted = m->d_sorted;
    P.map_xyz4 = m->d_map4;
    P.cell_start = m->d_cell_start;
    P.nbr_pts = m->d_nbr_pts;
    P.nbr_start = m->d_nbr_start;
    P.sx = h->d_sx; P.sy = h->d_sy; P.sz = h->d_sz;
    P.perm = h->sorted ? h->d_perm : nullptr;
    P.state = h->d_state;
    P.blocks = h->d_blocks;
    P.partials = h->d_partials;
    P.arrive = h->d_arrive;
    P.max_blk = h->max_blk;
    P.xcd_remap = h->cfg.xcd_remap;
    P.n_active = h->d_active;
    P.sums_out = sums_out;
    const bool rec = h->cfg.record_corr_iter >= 0;
    P.rec_flag = rec ? h->d_rec_flag : nullptr;
    P.rec_coeff = rec ? h->d_rec_coeff : nullptr;
    P.rec_nn = rec ? h->d_rec_nn : nullptr;
    P.stamps = (h->cfg.profile == 2) ? h->d_stamps : nullptr;
    P.d5_cache = (h->cfg.nn_cache && !h->cfg.use_lds) ? h->d_nn_cache : nullptr;
    P.blk_skip = (h->shard.axis >= 0 && h->has_block_box && sums_out != nullptr && !h->cfg.use_lds && h->ppt == 1) ? h->d_blk_skip : nullptr;
    // With a sharded map the workgroups a rank keeps belong to the scans near its slab, and the batch's workgroups are
    // ordered by scan position: a contiguous stretch of the list, i.e. ONE OR TWO of the eight XCDs under the XCD-aware
    // order (measured: 0.82 ms against 0.47 ms for the same launch).  Deal them round-robin instead.
    if (P.blk_skip) P.xcd_remap = 0;
}

// Arguments of the corner launch: the child's map, grid, edge points and workgroup list; everything
// that is per scan (state, partial sums, arrival counters, active count) is the parent's.
static void lio_fill_params_corner(lio_s2m_handle* h, LioIterParams& Pc, double* sums_out)
{
    lio_fill_params(h->corner, Pc, sums_out);
    Pc.shard = h->shard;
    Pc.state = h->d_state;
    Pc.partials = h->d_partials;
    Pc.arrive = h->d_arrive;
    Pc.max_blk = h->max_blk;
    Pc.n_active = h->d_active;
    Pc.stamps = nullptr;
}

// One Gauss-Newton iteration of the batch: cornerOptimization (if a corner batch is resident), then
// surfOptimization MO:1618-1687; the workgroup that arrives last on a scan's counter runs
// LMOptimization MO:1702-1837 for it.
// `index`: the launch's position within the run (0-based); from h->tail_from on, a launch that qualifies for the plain
// instantiation takes its looped form.  Returns whether it did.
static bool lio_launch_gn(lio_s2m_handle* h, const LioIterParams& P, const LioIterParams* Pc, int index)
{
    if (Pc) lio_launch_iterate(*Pc, h->corner->n_blocks, 1, false, h->stream, true);
    // (a run with a corner batch keeps the general surface kernel: that path is as it was)
    const int tail_wgs = (h->tail_from >= 0 && index >= h->tail_from) ? h->tail_wgs : 0;
    bool looped = false;
    h->iterate_variant = lio_launch_iterate(P, h->n_blocks, h->ppt, h->cfg.use_lds != 0, h->stream, false, h->plain_kernel && !Pc, tail_wgs, &looped);
    return looped;
}

extern "C" int lio_s2m_batch_begin(lio_s2m_handle* h)
try {
    if (h && h->multi) return lio_refuse_multi();
    if (!h) return lio_fail(LIO_ERR_ARG, "null handle");
    if (!lio_map_of(h)->has_map) return lio_fail(LIO_ERR_NO_MAP, "set_map has not been called");
    if (h->n_scans < 1 || !h->poses_set) return lio_fail(LIO_ERR_ARG, "batch_upload and batch_set_poses first");
    if (const int rc = lio_enter(h); rc != LIO_OK) return rc;
    if (h->map_src && h->map_epoch != h->map_src->map_epoch) {      // the shared map was replaced since the last run
        h->map_epoch = h->map_src->map_epoch;
        h->graph_dirty = true;
        HIPCHK(hipStreamWaitEvent(h->stream, h->map_src->ev_mapl[1], 0));   // (its build may still be in flight on the owner's stream)
    }
    lio_launch_init_state(h->d_state, h->n_scans, h->d_poses, h->pose_in_state, h->c, h->d_active, h->stream);
    h->pose_in_state = false;          // (d_poses holds the guess from now on)
    // search-bound cache: iteration 0 never reads it and rewrites the entry of every point it processes; entries
    // of points it does not process (owned by another rank) could date from an earlier run -> drop them
    // (0xff bytes = NaN, which fails the `>= 0` validity test like -1 does)
    if (h->cfg.nn_cache && !h->cfg.use_lds && h->d_nn_cache && h->shard.axis >= 0)
        HIPCHK(hipMemsetAsync(h->d_nn_cache, 0xff, (h->total_pts ? h->total_pts : 1) * sizeof(float), h->stream));
    if (h->corner_active && h->corner->d_nn_cache && h->shard.axis >= 0)
        HIPCHK(hipMemsetAsync(h->corner->d_nn_cache, 0xff, (h->corner->total_pts ? h->corner->total_pts : 1) * sizeof(float), h->stream));
    h->launches_this_run = 0;
    h->units_this_run = 0;
    h->unit_iters = 1;
    h->iterate_variant = 0;             // (set by the first k_s2m_iterate launch of the run; a one-launch loop leaves 0)
    h->run_n_full = h->run_n_looped = 0;
    h->ran = true;
    return LIO_OK;
} LIO_CATCH

// (Re)capture `chunk` consecutive GN-iteration launches into a hipGraph.  Every launch has the
// same arguments -- all per-iteration state lives in device memory -- so one executable graph
// serves the whole loop; scans that are done turn their workgroups into immediate exits.
static int lio_graph_prepare(lio_s2m_handle* h, const LioIterParams& P, const LioIterParams* Pc, int chunk)
{
    // the cached graph stays valid as long as the kernel arguments and the launch geometry are the same
    LioGraphKey key;
    memset(&key, 0, sizeof(key));
    key.chunk = chunk; key.blocks = h->n_blocks; key.ppt = h->ppt; key.plain = h->plain_kernel;
    key.tail_from = h->tail_from; key.tail_wgs = h->tail_wgs;
    key.blocks_c = Pc ? h->corner->n_blocks : -1;
    memcpy(&key.params, &P, sizeof(P));
    if (Pc) memcpy(&key.params_c, Pc, sizeof(P));
    if (h->graph_exec && memcmp(&h->graph_key, &key, sizeof(key)) == 0) return LIO_OK;
    if (h->graph_exec) { HIPCHK(hipGraphExecDestroy(h->graph_exec)); h->graph_exec = nullptr; }
    if (h->graph) { HIPCHK(hipGraphDestroy(h->graph)); h->graph = nullptr; }
    HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    // (every unit of a run replays this graph: the position in the chunk stands for the index within the run.  A launch of a
    // later unit is then full-grid where its index alone would make it looped; both forms compute the same)
    h->graph_n_full = h->graph_n_looped = 0;
    for (int i = 0; i < chunk; ++i) {
        if (lio_launch_gn(h, P, Pc, i)) h->graph_n_looped++;
        else h->graph_n_full++;
    }
    HIPCHK(hipStreamEndCapture(h->stream, &h->graph));
    HIPCHK(hipGraphInstantiate(&h->graph_exec, h->graph, nullptr, nullptr, 0));
    memcpy(&h->graph_key, &key, sizeof(key));          // (stored as it is compared: with its padding)
    h->graph_dirty = false;
    return LIO_OK;
}

// The GN loop (MO:1848-1859) as a resumable launch loop.  After every launch unit (one launch, or one replay of a
// captured chunk of `graph_iters` launches) the count of still-iterating scans is copied to pinned memory; unit u
// is only enqueued once the count after unit u-1-lookahead is known to be non-zero (lookahead 0 never enqueues an
// empty launch; larger values keep the queue fed for small batches).  `blocking == false` (lio_s2m_batch_run)
// enqueues what can be enqueued WITHOUT waiting for the device and returns -- the caller is free to upload the
// next batch on a sibling handle --; lio_s2m_batch_sync / _results resume the loop with `blocking == true`.
static int lio_run_continue(lio_s2m_handle* h, bool blocking)
{
    if (!h->run_pending) return LIO_OK;
    const bool prof = h->cfg.profile != 0;
    const LioIterParams* Pc = h->run_has_c ? &h->run_Pc : nullptr;
    while (h->run_next < h->run_units && h->run_next < LIO_MAX_ITERS) {          // MO:1848
        const int u = h->run_next;
        const int chk = u - 1 - h->run_look;
        if (chk >= 0) {
            if (blocking) {
                HIPCHK(hipEventSynchronize(h->ev_chk[chk]));
            } else {
                const hipError_t q = hipEventQuery(h->ev_chk[chk]);
                if (q == hipErrorNotReady) { (void)hipGetLastError(); return LIO_OK; }   // resumed by sync / results
                HIPCHK(q);
            }
            if (h->h_active[chk] == 0) break;
        }
        if (prof) HIPCHK(hipEventRecord(h->ev_beg[u], h->stream));
        if (h->run_persist) {
            lio_launch_persist(h->run_P, h->n_blocks, h->d_gen, h->gen_epoch, h->soa_valid ? nullptr : h->last_stage + h->last_xyz_off,
                               h->last_stride, h->n_scans, getenv("LIO_NO_SPEC") ? nullptr : h->d_gen + h->n_scans, h->d_spec_sums, h->d_poses,
                               lio_persist_spin_max(h), h->persist_withhold, h->stream);
        } else if (h->run_graph) {
            HIPCHK(hipGraphLaunch(h->graph_exec, h->stream));
            h->run_n_full += h->graph_n_full; h->run_n_looped += h->graph_n_looped;
        } else if (lio_launch_gn(h, h->run_P, Pc, u)) h->run_n_looped++;
        else h->run_n_full++;
        if (prof) HIPCHK(hipEventRecord(h->ev_end[u], h->stream));
        if (!h->run_persist) HIPCHK(hipMemcpyAsync(&h->h_active[u], h->d_active, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipEventRecord(h->ev_chk[u], h->stream));
        h->run_next = u + 1;
        h->units_this_run = u + 1;
        h->launches_this_run = (u + 1) * h->unit_iters;
    }
    h->run_pending = false;
    HIPCHK(hipGetLastError());
    return LIO_OK;
}

// lio_s2m_batch_run with its two choices as arguments.  `blocking`: drive the loop to its end before returning (a lone
// registration has nothing to overlap with) instead of enqueueing what can be enqueued without waiting for the device.
// `allow_one_launch`: see lio_persist_eligible.
static int lio_s2m_run(lio_s2m_handle* h, bool blocking, bool allow_one_launch)
{
    if (h && h->multi) return lio_multi_run(h);
    int rc = lio_s2m_batch_begin(h);
    if (rc != LIO_OK) return rc;
    LioIterParams& P = h->run_P;
    memset(&P, 0, sizeof(P));          // (padding bytes take part in the graph-cache comparison)
    lio_fill_params(h, P, nullptr);
    memset(&h->run_Pc, 0, sizeof(h->run_Pc));
    h->run_has_c = h->corner_active && h->corner->n_blocks > 0;
    if (h->run_has_c) lio_fill_params_corner(h, h->run_Pc, nullptr);
    int look = h->cfg.lookahead;
    if (look < 0) look = (h->total_pts >= 200000) ? 0 : 2;
    // use_graph: a unit is one replay of a captured chunk of `graph_iters` iterations
    h->run_persist = lio_persist_eligible(h, allow_one_launch) && !h->run_has_c;        // (see lio_persist_eligible)
    if (!h->run_persist && (rc = lio_ensure_soa(h)) != LIO_OK) return rc;
    const bool graph = !h->run_persist && h->cfg.use_graph != 0 && h->cfg.profile != 2 && h->cfg.record_corr_iter < 0 && h->n_blocks > 0;
    int chunk = 1;
    if (graph) {
        chunk = h->cfg.graph_iters > 0 ? h->cfg.graph_iters : 4;
        if (chunk > h->cfg.max_iters) chunk = h->cfg.max_iters;
        if ((rc = lio_graph_prepare(h, P, h->run_has_c ? &h->run_Pc : nullptr, chunk)) != LIO_OK) return rc;
        if (h->cfg.lookahead < 0) look = 0;              // a chunk already is a run-ahead of `chunk` launches
    }
    if (h->run_persist) {
        bool fresh = false;
        HIPCHK(h->d_gen.grow((size_t)h->n_scans * 2, 1.25, 64, false, &fresh));
        if (fresh) {
            HIPCHK(hipMemsetAsync(h->d_gen, 0, h->d_gen.cap * sizeof(unsigned), h->stream));   // (fresh generation numbers / speculation states)
            h->gen_epoch = 0;
        }
        HIPCHK(h->d_spec_sums.grow((size_t)h->n_scans * LIO_SUMS));
        h->gen_epoch += 128;
        chunk = h->cfg.max_iters;                        // one unit = the whole loop
    }
    // (a replayed graph launches nothing through lio_launch_gn: the same pure function of P and the switch says what it holds)
    if (!h->run_persist)
        h->iterate_variant = lio_iterate_variant(P, h->ppt, h->cfg.use_lds != 0, false, h->plain_kernel && !h->run_has_c);
    h->run_graph = graph;
    h->run_look = look;
    h->run_units = (h->cfg.max_iters + chunk - 1) / chunk;
    h->run_next = 0;
    h->unit_iters = h->run_persist ? 1 : chunk;
    h->units_this_run = 0;
    h->launches_this_run = 0;
    h->run_pending = true;
    return lio_run_continue(h, blocking);
}

extern "C" int lio_s2m_batch_run(lio_s2m_handle* h)
try {
    return lio_s2m_run(h, false, true);
} LIO_CATCH

extern "C" int lio_s2m_kernel_variant(const lio_s2m_handle* h)
try {
    if (!h) return lio_fail(LIO_ERR_ARG, "null handle");
    if (h->multi) return 0;            // (the devices' handles publish their sums: always the general instantiation)
    return h->iterate_variant;
} LIO_CATCH

// Surface launches of the last run by form: *n_full with one workgroup per entry of the block list (k_s2m_iterate), *n_looped
// with the looped form of the plain instantiation (k_s2m_iterate_tail).  A one-launch loop (k_s2m_persist) counts as neither.
extern "C" int lio_s2m_launch_forms(const lio_s2m_handle* h, int32_t* n_full, int32_t* n_looped)
try {
    if (!h || !n_full || !n_looped) return lio_fail(LIO_ERR_ARG, "null argument");
    *n_full = h->multi ? 0 : h->run_n_full;            // (the devices' handles publish their sums: never looped, not counted here)
    *n_looped = h->multi ? 0 : h->run_n_looped;
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_s2m_batch_iter_partial(lio_s2m_handle* h, double* d_sums)
try {
    if (!h || !d_sums) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!h->ran) return lio_fail(LIO_ERR_ARG, "batch_begin first");
    if (const int rc = lio_enter(h); rc != LIO_OK) return rc;
    { const int rcs = lio_ensure_soa(h); if (rcs != LIO_OK) return rcs; }
    LioIterParams P;
    lio_fill_params(h, P, d_sums);
    HIPCHK(hipMemsetAsync(d_sums, 0, (size_t)h->n_scans * LIO_SUMS * sizeof(double), h->stream));
    const int it = h->launches_this_run;
    const bool prof = h->cfg.profile != 0 && it < LIO_MAX_ITERS;
    if (prof) HIPCHK(hipEventRecord(h->ev_beg[it], h->stream));
    LioIterParams Pcs;
    const bool with_corners = h->corner_active && h->corner->n_blocks > 0;
    if (with_corners) lio_fill_params_corner(h, Pcs, d_sums);
    if (P.blk_skip && !getenv("LIO_NO_CULL")) {
        lio_launch_shard_cull(P, h->plan_ranks, h->plan_rank, h->plan_halo, h->plan_bounds, h->d_block_box, h->n_blocks, h->d_blk_skip,
                              h->stream);
        if (getenv("LIO_CULL_STATS")) {                  // diagnostics only (synchronises)
            std::vector<unsigned char> sk((size_t)h->n_blocks);
            HIPCHK(hipMemcpyAsync(sk.data(), h->d_blk_skip, sk.size(), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            size_t c = 0, c2 = 0;
            for (unsigned char v : sk) { c += (v == 1); c2 += (v == 2); }
            fprintf(stderr, "[liogpu] shard cull: %zu of %d workgroups skipped, %zu wholly owned (iteration %d)\n", c, h->n_blocks, c2, it);
        }
    } else {
        P.blk_skip = nullptr;
    }
    if (lio_launch_gn(h, P, with_corners ? &Pcs : nullptr, it)) h->run_n_looped++;     // (never: a launch that publishes its sums is not plain)
    else h->run_n_full++;
    if (prof) HIPCHK(hipEventRecord(h->ev_end[it], h->stream));
    h->launches_this_run++;
    h->units_this_run = h->launches_this_run;
    HIPCHK(hipGetLastError());
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_s2m_batch_iter_apply(lio_s2m_handle* h, const double* d_sums)
try {
    return lio_s2m_iter_apply_slots(h, d_sums, 0, 1);
} LIO_CATCH

int lio_s2m_iter_apply_slots(lio_s2m_handle* h, const double* d_sums, size_t slot_stride, int n_slots)
{
    if (!h || !d_sums || n_slots < 1) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!h->ran || h->launches_this_run < 1) return lio_fail(LIO_ERR_ARG, "batch_iter_partial first");
    if (const int rc = lio_enter(h); rc != LIO_OK) return rc;
    lio_launch_apply(h->d_state, h->n_scans, d_sums, slot_stride, n_slots, h->c, h->d_active, h->stream);
    // publish the number of still-iterating scans after this iteration (see lio_s2m_batch_poll_active)
    const int it = h->launches_this_run - 1;
    if (it < LIO_MAX_ITERS) {
        HIPCHK(hipMemcpyAsync(&h->h_active[it], h->d_active, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipEventRecord(h->ev_chk[it], h->stream));
    }
    HIPCHK(hipGetLastError());
    return LIO_OK;
}

extern "C" int lio_s2m_batch_poll_active(lio_s2m_handle* h, int32_t iteration, int32_t* n_active)
try {
    if (!h || !n_active) return lio_fail(LIO_ERR_ARG, "null argument");
    if (iteration < 0 || iteration >= h->launches_this_run || iteration >= LIO_MAX_ITERS)
        return lio_fail(LIO_ERR_ARG, "iteration has not been applied");
    HIPCHK(hipEventSynchronize(h->ev_chk[iteration]));
    *n_active = h->h_active[iteration];
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_s2m_batch_n_active(lio_s2m_handle* h, int32_t* n_active)
try {
    if (!h || !n_active) return lio_fail(LIO_ERR_ARG, "null argument");
    if (const int rc = lio_enter(h); rc != LIO_OK) return rc;
    HIPCHK(hipMemcpyAsync(&h->h_active[0], h->d_active, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *n_active = h->h_active[0];
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_s2m_batch_sync(lio_s2m_handle* h)
try {
    if (!h) return lio_fail(LIO_ERR_ARG, "null handle");
    if (h->multi) return lio_multi_sync(h);
    if (const int rc = lio_enter(h); rc != LIO_OK) return rc;
    { const int rcc = lio_run_continue(h, true); if (rcc != LIO_OK) return rcc; }
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    return LIO_OK;
} LIO_CATCH

// The run's part of the profile, from the states lio_s2m_batch_results has just read.
static void lio_results_profile(lio_s2m_handle* h, int64_t point_iters)
{
    h->prof.point_iters = point_iters;
    h->prof.n_launches = h->launches_this_run;
    for (int i = 0; i < LIO_MAX_ITERS; ++i) { h->prof.launch_ms[i] = 0.0f; h->prof.launch_active[i] = 0; }
    // launch_ms[u] = device time of launch unit u (one launch, or one graph replay of unit_iters
    // launches); launch_active[u] = scans that took part in the unit's first launch
    const int n_units = h->units_this_run > 0 ? h->units_this_run : h->launches_this_run;
    for (int u = 0; u < n_units && u < LIO_MAX_ITERS; ++u) {
        int act = 0;
        for (int s = 0; s < h->n_scans; ++s) {
            const LioScanState& st = h->h_state[s];
            const int ran = st.status == 1 ? 0 : (st.status == 2 ? 1 : st.iter);
            if (u * h->unit_iters < ran) ++act;
        }
        h->prof.launch_active[u] = act;
        if (h->cfg.profile && h->units_this_run > 0) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, h->ev_beg[u], h->ev_end[u]) != hipSuccess) ms = -1.0f;
            h->prof.launch_ms[u] = ms;
        }
    }
    h->prof.n_units = n_units;
    h->prof.unit_iters = h->unit_iters;
    h->prof.pipeline = h->run_persist ? 4 : 1;
    h->prof.persist_fallbacks = h->persist_fallbacks;
}

extern "C" int lio_s2m_batch_results(lio_s2m_handle* h, float* poses, lio_s2m_result* results)
try {
    if (!h) return lio_fail(LIO_ERR_ARG, "null handle");
    if (h->multi) return lio_multi_results(h, poses, results);
    if (!h->ran) return lio_fail(LIO_ERR_ARG, "nothing has been run");
    if (const int rc = lio_enter(h); rc != LIO_OK) return rc;
    { const int rcc = lio_run_continue(h, true); if (rcc != LIO_OK) return rcc; }
    if (results) {
        HIPCHK(hipMemcpyAsync(h->h_state.data(), h->d_state, (size_t)h->n_scans * sizeof(LioScanState),
                              hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->host_state_stale = false;
    } else {
        // poses only: 40 bytes per scan through a pinned buffer instead of the whole state (1.5 KB per scan)
        const size_t need = (size_t)h->n_scans * 10;
        HIPCHK(h->d_summary.grow(need));
        HIPCHK(h->h_summary.grow(need, need + 64));
        h->host_state_stale = true;
        lio_launch_pack_summary(h->d_state, h->n_scans, h->d_summary, h->stream);
        HIPCHK(hipMemcpyAsync(h->h_summary, h->d_summary, need * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (int s = 0; s < h->n_scans; ++s) {
            LioScanState& st = h->h_state[s];
            const float* o = h->h_summary + (size_t)s * 10;
            memcpy(st.pose, o, sizeof(float) * 6);
            memcpy(&st.iter, o + 6, 4); memcpy(&st.status, o + 7, 4);
            st.done = (st.status & 0x100) ? 0 : 1;
            st.status &= 0xff;
            memcpy(&st.converged, o + 8, 4); memcpy(&st.is_degenerate, o + 9, 4);
        }
    }
    HIPCHK(hipGetLastError());
    if (h->run_persist) {
        // Every scan leaves a one-launch loop done; one that did not gave up waiting at its barrier (bounded polls): its
        // workgroups were not all resident (another client holds compute units) or never arrived.  Recover inside this
        // call: clear the arrival counters the aborted launch left armed (every later run on this handle would otherwise
        // find its "last workgroup" one arrival early -- round-2 advisor finding), and run the same registrations through
        // the launch loop from the saved initial guesses (d_poses).  What the aborted launch may already have written into
        // the persistent members (isDegenerate / matP of a first solve) is what the launch loop's first solve computes from
        // the same sums, bit for bit, so nothing else needs restoring.
        bool incomplete = false;
        for (int s = 0; s < h->n_scans; ++s) incomplete = incomplete || !h->h_state[s].done;
        if (incomplete) {
            h->persist_fallbacks++;
            h->prof.persist_fallbacks = h->persist_fallbacks;
            HIPCHK(hipMemsetAsync(h->d_arrive, 0, h->d_arrive.cap * sizeof(unsigned), h->stream));
            h->poses_set = true; h->pose_in_state = false;           // (k_s2m_init_state left the guesses in d_poses)
            int rc = lio_s2m_run(h, true, false);
            if (rc == LIO_OK) rc = lio_s2m_batch_results(h, poses, results);
            return rc;
        }
    }
    int64_t pit = 0;
    for (int s = 0; s < h->n_scans; ++s) {
        const LioScanState& st = h->h_state[s];
        if (poses) memcpy(poses + (size_t)s * 6, st.pose, sizeof(float) * 6);
        // a "< 50 correspondences" scan was fast-forwarded: it did its work once
        pit += (int64_t)(st.n_pts + st.c_n_pts) * (st.status == 2 ? 1 : st.iter) * (st.status == 1 ? 0 : 1);
        if (results) {
            lio_s2m_result& r = results[s];
            memset(&r, 0, sizeof(r));
            r.status = st.status;
            r.iters = st.status == 1 ? 0 : st.iter;
            r.converged = st.converged;
            r.is_degenerate = st.is_degenerate;
            r.n_corr_last = st.n_corr_last;
            memcpy(r.n_corr_iter, st.n_corr_iter, sizeof(r.n_corr_iter));
            memcpy(r.matP, st.matP, sizeof(r.matP));
            memcpy(r.AtA, st.AtA, sizeof(r.AtA));
            memcpy(r.AtB, st.AtB, sizeof(r.AtB));
            memcpy(r.pose_iter, st.pose_iter, sizeof(r.pose_iter));
        }
    }
    lio_results_profile(h, pit);
    return LIO_OK;
} LIO_CATCH

// One registration: upload, optional corner upload, poses and the GN loop chained on the stream; the only host wait is
// for the results (the caller's buffers stay valid for the whole call).  Returns the scan's status.
static int lio_register_chain(lio_s2m_handle* h, const void* corner_scan, size_t n_corner, const void* surf_scan, size_t n_surf,
                              size_t stride, float pose[6], lio_s2m_result* res, const LioUploadOpts& o)
{
    const void* scans[1] = { surf_scan };
    const void* cscans[1] = { corner_scan };
    size_t np[1] = { n_surf }, ncp[1] = { n_corner };
    int rc = lio_s2m_upload(h, 1, scans, np, stride, o);
    if (rc == LIO_OK && n_corner) rc = lio_s2m_upload_corners(h, 1, cscans, ncp, stride, LIO_WAIT_NONE);
    if (rc == LIO_OK) {
        if (h->pose_in_state) h->poses_set = true;
        else rc = lio_s2m_set_poses(h, pose, LIO_WAIT_NONE);
    }
    if (rc == LIO_OK) rc = lio_s2m_run(h, true, true);
    if (rc != LIO_OK) { (void)hipStreamSynchronize(h->stream); return rc; }
    lio_s2m_result local;
    if ((rc = lio_s2m_batch_results(h, pose, res ? res : &local)) != LIO_OK) return rc;
    return (res ? res : &local)->status;
}

int lio_s2m_register_opts(lio_s2m_handle* h, const void* scan, size_t n, size_t stride, float pose[6], lio_s2m_result* res, LioUploadOpts o)
{
    if (!h || !pose) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!lio_map_of(h)->has_map) return lio_fail(LIO_ERR_NO_MAP, "set_map has not been called");
    o.pose = h->multi ? nullptr : pose;                  // one host-to-device copy less: the guess rides with the state
    o.wait = LIO_WAIT_NONE;
    return lio_register_chain(h, nullptr, 0, scan, n, stride, pose, res, o);
}

extern "C" int lio_s2m_register(lio_s2m_handle* h, const void* scan, size_t n, size_t stride,
                                float pose[6], lio_s2m_result* res)
try {
    return lio_s2m_register_opts(h, scan, n, stride, pose, res, LioUploadOpts());
} LIO_CATCH

extern "C" int lio_s2m_register_cs(lio_s2m_handle* h, const void* corner_scan, size_t n_corner,
                                   const void* surf_scan, size_t n_surf, size_t stride,
                                   float pose[6], lio_s2m_result* res)
try {
    if (!h || !pose) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!h->has_map) return lio_fail(LIO_ERR_NO_MAP, "set_map has not been called");
    if (n_corner && (!h->corner || !h->corner->has_map)) return lio_fail(LIO_ERR_NO_MAP, "set_corner_map has not been called");
    LioUploadOpts o;
    o.wait = LIO_WAIT_NONE;                              // (no pose: here the guess goes up through set_poses)
    return lio_register_chain(h, corner_scan, n_corner, surf_scan, n_surf, stride, pose, res, o);
} LIO_CATCH

// Field offsets of a PointCloud2 come off the wire: every comparison is written so that it cannot wrap (off + 12 > step
// passes for off = 0xfffffff4 in 32-bit arithmetic -- round-2 advisor finding).
int lio_pc2_check_xyz(const lio_pc2_layout* L)
{
    if (!L) return lio_fail(LIO_ERR_ARG, "null layout");
    const uint32_t st = L->point_step;
    if (st < 12 || (st & 3) || (L->off_x & 3) || L->off_x > st - 12)
        return lio_fail(LIO_ERR_ARG, "x, y, z must be three consecutive FLOAT32 fields inside the record");
    if (L->off_intensity >= 0 && ((L->off_intensity & 3) || (uint32_t)L->off_intensity > st - 4))
        return lio_fail(LIO_ERR_ARG, "intensity must be a FLOAT32 field inside the record");
    return LIO_OK;
}

// lio_s2m_register on a sensor_msgs/PointCloud2 `data` blob (cloud_info.cloud_deskewed, cloud_info.msg:27): what
// pcl::fromROSMsg(msgIn->cloud_deskewed, *laserCloudSurfLast) MO:440 + scan2MapOptimization do, without the copy
// into a pcl::PointCloud.  x, y, z are read in place at layout->off_x.
extern "C" int lio_s2m_register_pc2(lio_s2m_handle* h, const void* data, size_t n_points, const lio_pc2_layout* layout,
                                    float pose[6], lio_s2m_result* res)
try {
    if (!h || !layout || !pose) return lio_fail(LIO_ERR_ARG, "null argument");
    if (lio_pc2_check_xyz(layout) != LIO_OK) return LIO_ERR_ARG;
    bool pinned = false;
    if (layout->pin_host && data && n_points) {
        HIPCHK(hipSetDevice(h->cfg.device_id));
        pinned = hipHostRegister(const_cast<void*>(data), n_points * layout->point_step, hipHostRegisterDefault) == hipSuccess;
        (void)hipGetLastError();
    }
    LioUploadOpts o;
    o.xyz_off = layout->off_x;
    o.int_off = layout->off_intensity >= 0 ? layout->off_intensity : -1;
    const int rc = lio_s2m_register_opts(h, data, n_points, layout->point_step, pose, res, o);
    if (pinned) (void)hipHostUnregister(const_cast<void*>(data));
    return rc;
} LIO_CATCH

extern "C" int lio_s2m_get_correspondences(lio_s2m_handle* h, int32_t scan, uint8_t* flag,
                                           float* coeff4, int32_t* nn_idx5)
try {
    if (!h) return lio_fail(LIO_ERR_ARG, "null handle");
    if (h->cfg.record_corr_iter < 0) return lio_fail(LIO_ERR_ARG, "record_corr_iter was not set at create time");
    if (scan < 0 || scan >= h->n_scans) return lio_fail(LIO_ERR_ARG, "scan slot out of range");
    if (h->multi) return lio_multi_get_correspondences(h, scan, flag, coeff4, nn_idx5);
    if (const int rc = lio_enter(h); rc != LIO_OK) return rc;
    { const int rcc = lio_run_continue(h, true); if (rcc != LIO_OK) return rcc; }   // (a run started by batch_run may still be pending)
    const size_t off = (size_t)h->h_state[scan].offset, n = (size_t)h->h_state[scan].n_pts;
    if (n == 0) return LIO_OK;
    if (flag) HIPCHK(hipMemcpyAsync(flag, h->d_rec_flag + off, n, hipMemcpyDeviceToHost, h->stream));
    if (coeff4) HIPCHK(hipMemcpyAsync(coeff4, h->d_rec_coeff + off * 4, n * 4 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (nn_idx5) HIPCHK(hipMemcpyAsync(nn_idx5, h->d_rec_nn + off * 5, n * 5 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_s2m_get_corner_correspondences(lio_s2m_handle* h, int32_t scan, uint8_t* flag,
                                                  float* coeff4, int32_t* nn_idx5)
try {
    if (!h) return lio_fail(LIO_ERR_ARG, "null handle");
    if (!h->corner || !h->corner_active) return lio_fail(LIO_ERR_ARG, "no corner batch is resident");
    return lio_s2m_get_correspondences(h->corner, scan, flag, coeff4, nn_idx5);
} LIO_CATCH
