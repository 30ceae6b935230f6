/*
 * liogpu.h -- C ABI of the MI355X-native scan-to-map registration path.
 *
 * Drop-in boundary for the hot path of the reference's mapping node
 * (src/liorf/src/mapOptmization.cpp = MO, imageProjection.cpp = IP,
 * featureExtraction.cpp = FE, include/utility.h = UT).  The reference has no
 * FFI/plugin interface of its own; the seam is cut where the member-state
 * crossing is narrowest.  Plain pointers and sizes only; all
 * device memory is owned by the opaque handle.  Nothing here throws or aborts:
 * every entry point returns an int status (0 ok, >0 soft condition that the
 * reference also treats as "skip", <0 hard HIP/argument error).  A C++
 * exception inside the library (host memory exhausted) is caught at the entry
 * point and returned as LIO_ERR_CAPACITY; a handle it interrupted is still
 * safe to destroy, but need not be usable.
 *
 * Point clouds cross the edge in the caller's layout: `stride_bytes` between
 * points, float x,y,z at byte offsets 0,4,8 (pcl::PointXYZI: stride 32, UT:65;
 * a packed float[3] array: stride 12).
 */
#ifndef LIOGPU_H
#define LIOGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIO_VERSION 102
#define LIO_MAX_ITERS 32

/* status codes */
enum {
    LIO_OK               = 0,
    LIO_TOO_FEW_POINTS   = 1,   /* N_s <= 30, MO:1844 / MO:1862-1864: pose unchanged     */
    LIO_TOO_FEW_CORR     = 2,   /* last iteration had < 50 correspondences, MO:1721-1724 */
    LIO_ERR_ARG          = -1,
    LIO_ERR_HIP          = -2,
    LIO_ERR_CAPACITY     = -3,
    LIO_ERR_NO_MAP       = -4,
    LIO_ERR_NO_DEVICE    = -5
};

/* Constants of the scan-to-map loop; the caller fills them from the untouched
 * ParamServer (UT:72-367) or keeps the defaults, which are the literals
 * hard-coded in MO. */
typedef struct lio_s2m_config {
    int32_t k;               /* 5     neighbours, MO:1631 (only 5 is supported)            */
    float   max_sq_dist;     /* 1.0   gate on the 5th neighbour, MO:1641                   */
    double  plane_tol;       /* 0.2   MO:1662 (double literal in the reference)            */
    double  weight;          /* 0.9   MO:1671 (double literal)                             */
    double  min_s;           /* 0.1   MO:1679 (double literal)                             */
    int32_t min_corr;        /* 50    MO:1722                                              */
    int32_t max_iters;       /* 30    MO:1848 (<= LIO_MAX_ITERS)                           */
    float   eig_thresh;      /* 100   MO:1796                                              */
    double  conv_deg;        /* 0.05  MO:1833                                              */
    double  conv_cm;         /* 0.05  MO:1833                                              */
    int32_t min_scan_pts;    /* 30    MO:1844 (N_s must exceed it)                         */
    int32_t jacobian_mode;   /* 0 = reference (MO:1764 as written), 1 = exact derivative   */
    int32_t force_all_iters; /* 1 = ignore the convergence break MO:1857-1858              */
    int32_t device_id;       /* HIP device ordinal                                         */
    float   cell_size;       /* search radius covered by the grid neighbourhood, metres;
                                0 = sqrt(max_sq_dist)*1.001.  Cell edge = cell_size/cell_div */
    int32_t max_batch;       /* hint: scans per batch (buffers grow on demand; may be 0); also decides x_sub = auto */
    int32_t max_scan_pts;    /* hint: points per scan (buffers grow on demand; may be 0)    */
    int32_t record_corr_iter;/* iteration whose correspondences are kept for
                                lio_s2m_get_correspondences (-1 = none)                    */
    int32_t kernel_variant;  /* scan points per thread: 0 = auto (1), or 1 / 2 / 4 (A/B testing)   */
    int32_t profile;         /* 1 = bracket every GN-iteration launch with HIP events      */
    int32_t lookahead;       /* GN launches enqueued ahead of the convergence check;
                                0 = never enqueue an empty launch, -1 = auto               */
    int32_t use_lds;         /* 1 = stage the workgroup's map region through LDS (measured 2.5x slower);
                                0 (default) = stream the replicated neighbourhood rows     */
    int32_t sort_scan;       /* 1 = re-order scans by tiles at upload when the batch has >= 65536
                                points (default), 2 = always, 0 = never, 3 = always and by the
                                multi-kernel counting sort even when every scan fits the one-launch
                                LDS sort (A/B and tests); results are reported in the caller's
                                order either way                                            */
    int32_t cell_div;        /* k: cells per search radius (1..3, default 2); the candidate
                                scan visits (2k+1)^3 cells, map rows are replicated (2k+1)^2 x */
    int32_t xcd_remap;       /* 1 (default) = XCD-aware workgroup order (L2 locality only)  */
    float   tile_size;       /* edge of the upload-time sort tiles in metres (0 = 4 m)      */
    int32_t use_graph;       /* 1 = replay a hipGraph of `graph_iters` captured GN iterations
                                per unit of the launch loop (BASELINE config 5); ignored when
                                record_corr_iter or the diagnostic profile=2 is set        */
    int32_t graph_iters;     /* iterations per captured chunk (default 4)                   */
    int32_t sort_batch;      /* 1 (default) = order the workgroups of a batch by the scans'
                                positions (L2 locality only; results are unaffected)       */
    int32_t nn_cache;        /* 1 (default) = from the second GN iteration on, bound each point's
                                search by the distances to its previous 5 neighbours (exact:
                                the candidate run shrinks, the result does not change)      */
    int32_t pipeline;        /* how the Gauss-Newton loop MO:1848-1859 is issued; results are identical for every value.
                                0 = auto: one launch per iteration (k_s2m_iterate), or -- for a batch of at most half
                                a workgroup per compute unit, e.g. a lone registration, unless use_graph or profile = 2
                                is set -- the whole loop as ONE launch (k_s2m_persist: per-scan barrier between
                                iterations; 0.17 against 0.25 ms per registration on MI355X); 1 = always one launch per
                                iteration; 4 = the one-launch loop for every batch of at most one workgroup per compute
                                unit.  Other values are refused (2, 3 and 5 were per-point-cache experiments of round 2,
                                measured slower or equal and removed: DESIGN.md appendix)                                */
    int32_t n_devices;       /* 1 (default) = the single device `device_id`.  > 1: in-library multi-GPU -- the local
                                map is cut into slabs (+ a halo of 16 cells, i.e. ~16 m of extra map per side and
                                device) over device_ids[0..n_devices), every
                                registration's points are processed by the device owning their map cell and the
                                6x6 JtJ / 6x1 Jtr / N_c are summed across the devices once per GN iteration
                                (the join of the OpenMP loop MO:1622-1686); set_map / register / batch_* work
                                unchanged on such a handle, so a patched node needs no other change              */
    int32_t device_ids[8];   /* HIP device ordinals of the multi-GPU mode (an ordinal may repeat)               */
    int32_t x_sub;           /* the replicated neighbourhood rows are bucketed along x this many times finer than the
                                cells (1, 2, 4, 8): a query's candidate run is cut to [x(q - R), x(q + R)] at that
                                resolution -- 20 % fewer candidates at 4, -6 % per launch, +5 % registrations/s on the
                                512-scan batches (same results: the search stays exact) -- at the price of a 4x longer
                                bucket table, +0.08 ms per map build.  0 = auto: 4 for a handle set up for batches
                                (max_batch >= 8: the map is built once and searched by many scans), 1 for a node's handle
                                (the map is rebuilt for every scan; a lone registration is latency-bound and gains nothing) */
    int32_t tight_rows;      /* further sets of neighbourhood rows over the same points with 3x3 cells of 0.6 / 0.3 / 0.15 x
                                the gate radius (+36 % map memory and build time each): a query whose search bound -- the
                                previous iteration's fifth neighbour plus its own movement -- is at most a table's cell walks
                                that table's row: a (1.8 m)^2 / (0.9 m)^2 / (0.45 m)^2 cross-section instead of (2.5 m)^2 at
                                the 1 m gate; same results.  -3 % per launch on the 512-scan batches of the default 0.5 m map
                                (one table), 2.1x the registrations/s on a 0.1 m map (three).  1..3 = that many tables, -1 =
                                none, 0 = auto: none for a node's handle (max_batch < 8), else one table plus the finer ones
                                the map's point density has queries for (lio_s2m_profile.map_tight_tables says how many)  */
} lio_s2m_config;

/* What scan2MapOptimization leaves behind (MO:1817-1822 pose is returned in
 * place; MO:176-177 isDegenerate/matP; the rest is diagnostics). */
typedef struct lio_s2m_result {
    int32_t status;
    int32_t iters;             /* loop bodies executed (<= max_iters)                    */
    int32_t converged;         /* LMOptimization returned true, MO:1833-1835             */
    int32_t is_degenerate;     /* MO:176 -> odometry_incremental covariance[0], MO:2309  */
    int32_t n_corr_last;       /* N_c of the last executed iteration                     */
    int32_t n_corr_iter[LIO_MAX_ITERS];
    float   matP[36];          /* row-major, MO:177/1807                                 */
    float   AtA[36];           /* last normal matrix, row-major, MO:1782                 */
    float   AtB[6];            /* MO:1783                                                */
    float   pose_iter[LIO_MAX_ITERS][6]; /* pose after each iteration                    */
} lio_s2m_result;

typedef struct lio_s2m_profile {
    float   map_build_ms;      /* last set_map: H2D excluded, grid build kernels only     */
    float   map_upload_ms;     /* last set_map: wall time of staging + H2D                */
    int32_t n_launches;        /* GN-iteration launches of the last run                   */
    int32_t n_units;           /* launch units: single launches, or graph replays          */
    int32_t unit_iters;        /* launches per unit (1, or cfg.graph_iters)                */
    float   launch_ms[LIO_MAX_ITERS]; /* device time of each unit (profile=1)            */
    int32_t launch_active[LIO_MAX_ITERS]; /* scans in the first launch of each unit       */
    int64_t point_iters;       /* scan points processed by active scans over the run      */
    int64_t n_map;             /* resident map points                                     */
    int64_t n_cells;           /* grid cells                                              */
    int32_t pipeline;          /* what the last run used: 1 = one launch per iteration, 4 = one-launch loop */
    int32_t multi_iterations;  /* in-library multi-GPU mode (cfg.n_devices > 1), last run: GN iterations enqueued,        */
    int32_t multi_stream_syncs;/* ... stream / device synchronisations issued inside the loop (0 with the device-side
                                  exchange) and                                                                        */
    int32_t multi_event_waits; /* ... waits for a convergence count (an event wait, `lookahead` iterations behind)      */
    int32_t multi_exchange;    /* ... 0 = peer stores from a kernel, 1 = hipMemcpyPeerAsync, 2 = through host memory    */
    int32_t persist_fallbacks; /* one-launch loops of this handle that timed out at a barrier and were re-run through the
                                  launch loop inside the same call (cumulative; see lio_s2m_batch_results)              */
    int32_t map_x_sub;         /* last set_map: x subdivision of the row buckets in effect (cfg.x_sub)                  */
    int32_t map_tight_tables;  /* ... tight row tables built (cfg.tight_rows)                                            */
    int32_t map_first_try;     /* ... the tight table a query without a search bound tries before the full search (its
                                  index, 0 = the widest; -1: none -- the full search at once)                            */
    float   map_pts_per_cell;  /* ... map points per occupied grid cell, the density estimate behind the automatic choice
                                  of map_tight_tables (0: not measured)                                                  */
} lio_s2m_profile;

typedef struct lio_s2m_handle lio_s2m_handle;

int  lio_version(void);
void lio_s2m_default_config(lio_s2m_config *cfg);
const char *lio_last_error(void);

int  lio_s2m_create(const lio_s2m_config *cfg, lio_s2m_handle **out);
void lio_s2m_destroy(lio_s2m_handle *h);

/* Replaces kdtreeSurfFromMap->setInputCloud(laserCloudSurfFromMapDS), MO:1846:
 * copies the local map to the device as SoA and builds the hash grid. */
int  lio_s2m_set_map(lio_s2m_handle *h, const void *pts, size_t n, size_t stride_bytes);

/* Replaces the loop MO:1848-1859 for one scan (laserCloudSurfLastDS, MO:138).
 * pose = transformTobeMapped [roll,pitch,yaw,x,y,z] (MO:171), in/out.
 * matP / isDegenerate persist on the handle between calls like the members
 * MO:176-177.  Synchronous. */
int  lio_s2m_register(lio_s2m_handle *h, const void *scan, size_t n, size_t stride_bytes,
                      float pose[6], lio_s2m_result *res);

/* Batched form (BASELINE config 5): many scans against the same resident map,
 * every scan its own pose / matP / convergence.  upload -> set_poses -> run
 * (asynchronous on the handle's stream) -> results (synchronises). */
int  lio_s2m_batch_upload(lio_s2m_handle *h, int32_t n_scans, const void *const *scans,
                          const size_t *n_pts, size_t stride_bytes);
int  lio_s2m_batch_set_poses(lio_s2m_handle *h, const float *poses /* n_scans x 6 */);
int  lio_s2m_batch_run(lio_s2m_handle *h);
int  lio_s2m_batch_sync(lio_s2m_handle *h);
int  lio_s2m_batch_results(lio_s2m_handle *h, float *poses /* n_scans x 6 */,
                           lio_s2m_result *results /* n_scans, may be NULL */);

/* ---- streaming: upload batch k+1 while batch k iterates (SURVEY 8d puts the per-scan H2D inside the metric;
 * the reference analogue is one cloud_info message arriving per callback, MO:432-476).
 * lio_s2m_share_map: handle `h` searches `map_owner`'s resident map (no copy); it keeps its own HIP stream,
 * scan buffers and per-scan state, so several handles form a software pipeline -- two a double buffer:
 *     run(A) ... upload_async(B, next batch) ... results(A) ... run(B) ... upload_async(A, ...) ...
 * THREE (two batches in flight ahead of the one whose results are awaited) measured 16 % faster than two: the host's
 * preparation of the next upload then never leaves the GPU alone with the last, nearly empty launches of a batch
 * (more than three streams oversubscribe the runtime's four hardware queues).
 * upload_async returns once the scans' H2D copies are DONE on h's stream (the caller's buffers are free
 * again) while the tile sort is still in flight; set_poses/run/results queue behind it.  Copies are true DMA
 * only from pinned memory: lio_host_alloc / lio_host_register (hipHostMalloc / hipHostRegister).  A batch laid
 * out contiguously (scans[s+1] == scans[s] + n_pts[s]*stride) goes in one copy.  scans[] may also be DEVICE
 * pointers (inputs already resident in HBM, e.g. the output of lio_deskew kept on the device).
 * The owner must outlive the sharer; call lio_s2m_set_map on the owner only while both streams are idle. */
int   lio_s2m_share_map(lio_s2m_handle *h, lio_s2m_handle *map_owner);
int   lio_s2m_batch_upload_async(lio_s2m_handle *h, int32_t n_scans, const void *const *scans,
                                 const size_t *n_pts, size_t stride_bytes);
void *lio_host_alloc(size_t bytes);
void  lio_host_free(void *p);
int   lio_host_register(void *p, size_t bytes);
int   lio_host_unregister(void *p);
/* Device memory for callers that keep clouds in HBM between calls (memory of the handle's own device is read in place by
 * lio_s2m_batch_upload*, lio_s2m_register_raw, lio_kf_store_add_device).  lio_device_upload is a synchronous H2D copy. */
void *lio_device_alloc(int32_t device_id, size_t bytes);
void  lio_device_free(int32_t device_id, void *p);
int   lio_device_upload(int32_t device_id, void *dst, const void *src, size_t bytes);

/* Persistent members MO:176-177 for batch slot `scan` (slot 0 = lio_s2m_register). */
int  lio_s2m_set_degeneracy(lio_s2m_handle *h, int32_t scan, const float matP[36], int32_t is_degenerate);

/* Association of iteration cfg.record_corr_iter for batch slot `scan`
 * (laserCloudOriSurfFlag / coeffSelSurfVec, MO:143-145, plus the 5 neighbour
 * indices into the caller's map order).  Arrays sized by that scan's N_s. */
int  lio_s2m_get_correspondences(lio_s2m_handle *h, int32_t scan, uint8_t *flag,
                                 float *coeff4, int32_t *nn_idx5);

/* ---- EXTENSION beyond this reference: point-to-line ("corner") residuals ------------------
 * BASELINE.json's north_star names cornerOptimization, which this fork removed (its
 * scan2MapOptimization MO:1839-1865 is surf-only).  These entry points
 * add the cornerOptimization of upstream LIO-SAM (kdtreeCornerFromMap 5-NN, 3x3 covariance,
 * cv::eigen, lambda0 > 3*lambda1, point-to-line distance) to the same Gauss-Newton loop:
 * corner rows are appended to the surf rows exactly as upstream's combineOptimizationCoeffs
 * does, and LMOptimization MO:1702-1837 is shared.  There is no reference oracle for them
 * in /root/reference (parity unpinned: checked against oracle/lio_oracle.c lo_scan2map_cs
 * only).  Without a corner batch every other entry point behaves exactly as before.
 *
 * set_corner_map          : kdtreeCornerFromMap->setInputCloud(laserCloudCornerFromMapDS)
 * batch_upload_corners    : the scans' edge points (laserCloudCornerLastDS); call after
 *                           lio_s2m_batch_upload with the same n_scans and before
 *                           lio_s2m_batch_set_poses; n_pts[s] may be 0
 * register_cs             : lio_s2m_register with both clouds
 * get_corner_correspondences : as lio_s2m_get_correspondences, for the edge points */
int  lio_s2m_set_corner_map(lio_s2m_handle *h, const void *pts, size_t n, size_t stride_bytes);
int  lio_s2m_batch_upload_corners(lio_s2m_handle *h, int32_t n_scans, const void *const *scans,
                                  const size_t *n_pts, size_t stride_bytes);
int  lio_s2m_register_cs(lio_s2m_handle *h, const void *corner_scan, size_t n_corner,
                         const void *surf_scan, size_t n_surf, size_t stride_bytes,
                         float pose[6], lio_s2m_result *res);
int  lio_s2m_get_corner_correspondences(lio_s2m_handle *h, int32_t scan, uint8_t *flag,
                                        float *coeff4, int32_t *nn_idx5);

int  lio_s2m_get_profile(lio_s2m_handle *h, lio_s2m_profile *out);
/* Which instantiation of the Gauss-Newton kernel the surface launches of the last run used: bit 0 = the plain one (one
 * device, no map sharding, no correspondence record, no phase clock, no corner batch; LIO_PLAIN_KERNEL=0 in the environment
 * when the handle is created forces the general one), bits 8.. = the waves per SIMD it was compiled for.  0 before any run
 * and after a one-launch loop; negative = error. */
int  lio_s2m_kernel_variant(const lio_s2m_handle *h);
/* How many surface launches of the last run had one workgroup per entry of the block list (*n_full) and how many were the
 * looped form of the plain kernel on a fixed grid (*n_looped), which launches take from index LIO_TAIL_FROM of a run on
 * (environment, read when the handle is created: -1 = never, 0 = every launch; LIO_TAIL_WGS = its workgroups, a multiple of
 * 8).  Both forms compute the same bytes.  A one-launch loop and a multi-device front handle report 0 / 0. */
int  lio_s2m_launch_forms(const lio_s2m_handle *h, int32_t *n_full, int32_t *n_looped);
/* Test hook for the one-launch loop (cfg.pipeline 0 / 4): spin_max = polls before a workgroup waiting at its scan's barrier
 * gives up (0 = default: 4096, a few milliseconds; LIO_PERSIST_SPIN_MAX in the environment), withhold_wg = index of an
 * association workgroup that never arrives (-1 = none).  A launch that times out is re-run through the launch loop inside
 * lio_s2m_batch_results / lio_s2m_register and counted in lio_s2m_profile.persist_fallbacks; results are the same. */
int  lio_s2m_debug_persist_spin(lio_s2m_handle *h, int32_t spin_max, int32_t withhold_wg);

/* Test hook: the device plane fit of the association (MO:1648-1666: 5x3 colPivHouseholderQr solve against -1, unit normal
 * and offset, plane test against plane_tol) on n neighbour sets, sets[n][5][3] in host memory.  out[n][8]: the raw bits of
 * X0[0..2], pa, pb, pc, pd, then planeValid (0 / 1). */
int  lio_debug_plane_fit(int32_t device_id, const float *sets, size_t n, double plane_tol, uint32_t *out);
/* Test hook: the serial Gauss-Newton step that ends every launch (MO:1784-1833 from the reduced sums onward and the loop
 * control MO:1848-1859: QR solve; on iteration 0 the eigen-decomposition, the degeneracy rule, matV.inv() * matV2; the
 * projection, the pose update, the convergence test) on n independent cases, one wave each, every case with a scan state of its
 * own.  It runs the source function of the library's kernels as compiled into the hook's kernel.
 * cfg: NULL = the defaults.  Per case i: sums[28 i ..] = the 21 upper-triangle entries of JtJ (row by row), the 6 of Jtr and the
 * correspondence count, in fp64 as the reduction leaves them; pose[6 i ..] the incoming pose; iter[i] the iteration number (0 ..
 * LIO_MAX_ITERS - 1); is_degenerate[i] and matP[36 i ..] the stored members MO:176-177.  For the whole call, the speculation
 * arguments of the one-launch loop: deg_override >= 0 takes the place of the stored is_degenerate (iterations > 0);
 * skip_eigen != 0: iteration 0 without the eigen-decomposition (matP / is_degenerate left alone, the non-degenerate update);
 * hold_if_done != 0: a step that would end the registration changes nothing it decides and returns 2.
 * out[i]: the state after the step, layout below (109 words of 4 bytes, no padding); T / trig are rewritten only when done == 0.
 * NON-FINITE POLICY: a sum that is not finite (as fp64 or as the fp32 the step converts it to), a count outside [0, 2^31) and a
 * non-finite pose are LIO_ERR_ARG before any launch.  The wave-parallel pivot search is defined for finite matrices only -- a
 * NaN compares unequal to the maximum it produced, and the search would then index lanes the serial code never reads; the
 * library keeps non-finite values out of the sums at the association (tests/test_gpu_nonfinite.py). */
typedef struct lio_debug_gn_record {
    float   pose[6];         /* word   0 */
    float   matP[36];        /* word   6 */
    float   AtA[36];         /* word  42 */
    float   AtB[6];          /* word  78 */
    float   T[12];           /* word  84 */
    float   trig[6];         /* word  96 */
    int32_t iter;            /* word 102 */
    int32_t done;            /* word 103 */
    int32_t status;          /* word 104 */
    int32_t converged;       /* word 105 */
    int32_t is_degenerate;   /* word 106 */
    int32_t n_corr_last;     /* word 107 */
    int32_t ret;             /* word 108: what the step returned (0, or 2 when held) */
} lio_debug_gn_record;
int  lio_debug_gn_step(int32_t device_id, const lio_s2m_config *cfg, size_t n, const double *sums, const float *pose,
                       const int32_t *iter, const int32_t *is_degenerate, const float *matP, int32_t deg_override,
                       int32_t skip_eigen, int32_t hold_if_done, lio_debug_gn_record *out);
/* Test hook: the line fit of the corner association (upstream cornerOptimization after the 5-NN gate: centroid, covariance,
 * cv::eigen 3x3, line iff e0 > 3 e1, point-to-line distance and gradient, s = 1 - weight |ld2|, accept iff s > min_s) on n cases,
 * one per thread: sets[n][5][3] = the five neighbours in the caller's order, pts[n][3] = the transformed points.  out[n][5]: the
 * raw bits of the four coefficients, then the accept flag (0 / 1).  Non-finite inputs are allowed (the code is serial). */
int  lio_debug_corner_fit(int32_t device_id, const float *sets, const float *pts, size_t n, double weight, double min_s, uint32_t *out);
/* Test hook: the association's fast fp32 operations against the device's plain operators, bit for bit.  op 0: square root,
 * op 1: x / 5, op 2: sqrtf(sqrtf(r2)) of the scan point (x, 0, 0) as the association takes it, its guard riding on the plane fit's
 * (a fixed neighbour set; raw ignored); raw != 0: the fast instruction sequence without its range guard (equal to the plain operator on the guarded
 * range only), raw == 0: the guarded entry point (equal everywhere).  Operands: the bit patterns patterns[0..count), or with
 * patterns NULL first, first + 1, ... (count <= 2^32; <= 2^27 with patterns or values).  *n_diff: results that differ from the
 * plain operator (two NaNs are equal); first_diff[8]: up to eight such patterns, *n_first of them; values (may be NULL): the
 * result bits. */
int  lio_debug_fast_f32_ops(int32_t device_id, int32_t op, int32_t raw, const uint32_t *patterns, uint64_t first, uint64_t count,
                            uint32_t *values, uint64_t *n_diff, uint32_t *first_diff, int32_t *n_first);
/* Test hook (host only): the largest float not above t.  The surface association compares fp32 values against this in place
 * of the double plane_tol / min_s: (double)v > t exactly when v > lio_debug_threshold_f32(t). */
float lio_debug_threshold_f32(double t);
/* Test hook (host only): the search grid lio_s2m_set_map would lay out for cfg over n map points in the box [mn, mx] --
 * the same override parser (LIO_X_SUB, LIO_TIGHT, LIO_TRY) and the same two planning steps, no device.  occupied = the
 * grid cells that hold a point (negative: not counted); caller_box != 0: the box came from the caller, as for a map
 * assembled on the device (that path counts no cells).  Arrays of 3: one entry per tight row table, reach descending,
 * tb_reach < 0 = no such table. */
typedef struct lio_grid_plan_info {
    float   origin[3], inv_cell;
    int32_t nx, ny, nz, n_cells, k, xs, nxf;
    float   inv_cell_x;
    int32_t tb_row0[3], tb_ny[3], tb_nz[3];
    float   tb_oy[3], tb_oz[3], tb_inv_cell[3], tb_reach[3];
    int32_t tb_try;
    float   tb_try_b2[3];
    float   cell;              /* edge of the main grid's cells after grow_steps growths by 1.5 */
    int32_t n_tb, grow_steps, want_occupancy;
    float   pts_per_cell;
    int64_t buckets;           /* row buckets of the main grid and of every table */
} lio_grid_plan_info;
int  lio_debug_grid_plan(const lio_s2m_config *cfg, const float mn[3], const float mx[3], size_t n, int32_t occupied,
                         int32_t caller_box, lio_grid_plan_info *out);
/* Diagnostic (cfg.profile == 2): per-wave phase clock of the last GN launch,
 * n_blocks x 4 x 8 cycle counters; returns n_blocks.  Not for production. */
int  lio_s2m_debug_stamps(lio_s2m_handle *h, long long *out, size_t cap_entries);
/* Test hook: the order the upload-time tile sort gave the resident batch.  Waits for the handle's stream and returns the
 * batch's total point count (all scans), or a negative LIO_ERR_*.  *sorted (may be NULL): 1 when the batch was tile-sorted.
 * With perm / xyz non-NULL and cap_points >= that count: perm[j] = the caller's (batch-wide) index of the record at sorted
 * position j (copied only when sorted), xyz = the SoA the Gauss-Newton loop reads as three runs of `count` floats -- all x,
 * all y, all z -- (copied only when the upload filled it).  perm == NULL, xyz == NULL, cap_points == 0 asks for the count.
 * A null handle, a multi-device handle and a capacity below the count are LIO_ERR_ARG. */
int  lio_s2m_debug_scan_order(lio_s2m_handle *h, int32_t *perm, float *xyz, size_t cap_points, int32_t *sorted);
/* Test hook (host only): the scan-local tile grid the upload lays over a scan whose finite coordinates span [mn, mx], asked
 * for tiles of edge `tile`, under shard axis -1 (unsharded), 0, 1 or 2.  out_i = tiles along x, y, z and the key strides of
 * x, y, z; out_f = the grid's origin and 1 / (the edge after doubling). */
int  lio_debug_scan_tile_plan(const float mn[3], const float mx[3], float tile, int32_t shard_axis, int32_t out_i[6], float out_f[4]);

/* Multi-GPU hooks (one process per GPU; the caller owns the collective).
 * The map given to set_map is this rank's shard INCLUDING a halo of one cell;
 * lio_s2m_set_shard restricts which transformed scan points this rank owns
 * (owner-computes): cells whose index along `axis` lies in [lo, hi) of the
 * GLOBAL grid described by origin/dims.  iter_partial leaves per-scan sums
 * (n_scans x 32 doubles: 21 upper JtJ, 6 Jtr, N_c, pad) in a device buffer;
 * the caller all-reduces it and iter_apply solves + updates every scan. */
int  lio_s2m_set_stream(lio_s2m_handle *h, void *hip_stream);
int  lio_s2m_set_global_grid(lio_s2m_handle *h, const float origin[3], const int32_t dims[3]);
int  lio_s2m_set_shard(lio_s2m_handle *h, int32_t axis, int32_t lo, int32_t hi);
/* The whole slab plan instead of this rank's range: rank r of n_ranks owns cells [bounds[r], bounds[r+1]) and holds the
 * map of [bounds[r] - halo_cells, bounds[r+1] + halo_cells).  With halo_cells > 1 a workgroup of scan points (256
 * consecutive points of the tile-sorted scan) whose extent fits the held region of the rank owning its middle is
 * processed WHOLLY by that rank and skipped by all others; longer workgroups keep per-point ownership.  Same results;
 * no wave runs for a handful of owned lanes.  Every rank must be given identical bounds and halo. */
int  lio_s2m_set_shard_plan(lio_s2m_handle *h, int32_t axis, int32_t n_ranks, int32_t rank, const int32_t *bounds,
                            int32_t halo_cells);
/* Alternative partition: the map is replicated, every rank processes each world-th
 * workgroup of every scan (call before lio_s2m_batch_upload); same iter_partial / all-reduce /
 * iter_apply protocol.  No halo, no ownership tests, perfectly balanced. */
int  lio_s2m_set_scan_shard(lio_s2m_handle *h, int32_t rank, int32_t world);
int  lio_s2m_batch_begin(lio_s2m_handle *h);
int  lio_s2m_batch_iter_partial(lio_s2m_handle *h, double *d_sums /* device, n_scans x 32 */);
int  lio_s2m_batch_iter_apply(lio_s2m_handle *h, const double *d_sums);
int  lio_s2m_batch_n_active(lio_s2m_handle *h, int32_t *n_active);
/* Scans still iterating after applied iteration `iteration` (0-based); waits only for that
 * iteration, so the caller can keep later iterations enqueued. */
int  lio_s2m_batch_poll_active(lio_s2m_handle *h, int32_t iteration, int32_t *n_active);

/* transformUpdate + constraintTransformation, MO:1867-1907 (host, fp64 slerp). */
void lio_transform_update(float pose[6], int32_t imu_available, int32_t imu_type,
                          float imu_roll_init, float imu_pitch_init, float imu_rpy_weight,
                          float rotation_tollerance, float z_tollerance);

/* ------------------------------------------------------------------ deskew */
/* Filters of projectPointCloud IP:577-615, keys UT:275-285. */
typedef struct lio_deskew_config {
    int32_t N_SCAN;
    int32_t downsampleRate;
    int32_t point_filter_num;
    float   lidarMinFront, lidarMinBack, lidarMinLeft, lidarMinRight;
    float   lidarMaxRange;
    float   lidarMaxIntensity;
    int32_t deskew_flag;      /* -1 = cloud has no per-point time field, IP:547 */
    int32_t device_id;
} lio_deskew_config;

void lio_deskew_default_config(lio_deskew_config *cfg);

/* imuDeskewInfo, IP:359-418 (host, fp64): integrates the gyro over the sweep.
 * Tables have room for 2000 entries (queueLength, IP:62).  Returns
 * imuPointerCur (> 0 <=> cloudInfo.imuAvailable). */
int  lio_imu_deskew_info(const double *stamp, const double *gyro_x, const double *gyro_y,
                         const double *gyro_z, int32_t n_imu,
                         double time_scan_cur, double time_scan_end,
                         double *imuTime, double *imuRotX, double *imuRotY, double *imuRotZ);

/* projectPointCloud + deskewPoint, IP:545-615, on the device.
 * pts: PointXYZIRT records (IP:4-15): float x,y,z @0,4,8; float intensity @16;
 * uint16 ring @20; float time @24; stride 32.  out: pcl::PointXYZI-compatible
 * records (x,y,z @0,4,8, intensity @16) with `out_stride_bytes` (>= 20),
 * input order preserved.  Returns status; *n_out = survivors. */
int  lio_deskew(const lio_deskew_config *cfg, const void *pts, size_t n, size_t stride_bytes,
                double time_scan_cur,
                const double *imuTime, const double *imuRotX, const double *imuRotY,
                const double *imuRotZ, int32_t imuPointerCur,
                void *out, size_t out_stride_bytes, size_t *n_out);

/* ---- cloud_info wire path: sensor_msgs/PointCloud2 blobs read in place ----------------------
 * The reference moves every cloud through pcl::fromROSMsg / pcl::moveFromROSMsg (MO:440, IP:226-232) and
 * pcl::toROSMsg (publishCloud UT:369-379); cloud_info.cloud_deskewed is such a blob (cloud_info.msg:27).  These
 * entry points take the message's `data` pointer, `width*height` and the byte offsets of its `fields` directly.
 * Constraints: little-endian (is_bigendian == 0); x, y, z are three consecutive FLOAT32 fields; intensity FLOAT32.
 * ring / time variants cover the four sensor layouts cachePointCloud converts on the host (IP:226-285). */
enum { LIO_PC2_UINT8 = 2, LIO_PC2_UINT16 = 4, LIO_PC2_INT32 = 5 };            /* sensor_msgs/PointField datatype codes */
enum { LIO_PC2_TIME_F32_SECONDS = 0,   /* Velodyne / Livox "time": float seconds from the sweep start          */
       LIO_PC2_TIME_U32_NS      = 1,   /* Ouster "t": dst.time = src.t * 1e-9f, IP:243                          */
       LIO_PC2_TIME_U32_RAW     = 2,   /* Mulran "t": dst.time = static_cast<float>(src.t), IP:262              */
       LIO_PC2_TIME_F64_STAMP   = 3 }; /* Robosense "timestamp": src.timestamp - points[0].timestamp, IP:269-281 */
typedef struct lio_pc2_layout {
    uint32_t point_step;      /* bytes per point (PointCloud2.point_step)                               */
    uint32_t off_x;           /* byte offset of x; y and z follow at +4, +8                              */
    int32_t  off_intensity;   /* FLOAT32, -1 = no such field (intensity reads as 0)                       */
    int32_t  off_ring;        /* deskew only; the reference refuses clouds without it, IP:313-329         */
    int32_t  ring_type;       /* LIO_PC2_UINT8 / LIO_PC2_UINT16 / LIO_PC2_INT32                           */
    int32_t  off_time;        /* deskew only; -1 = no per-point time (deskewFlag = -1, IP:341-356)        */
    int32_t  time_type;       /* LIO_PC2_TIME_*                                                           */
    int32_t  pin_host;        /* 1 = hipHostRegister the blob for the duration of the call (the caller
                                 allows its pages to be pinned): the H2D copy is then a true DMA         */
} lio_pc2_layout;

/* lio_s2m_register on the blob of cloud_info.cloud_deskewed (or any PointCloud2 with xyz): replaces
 * pcl::fromROSMsg MO:440 + the loop MO:1848-1859.  Only off_x / point_step / pin_host of the layout are used. */
int  lio_s2m_register_pc2(lio_s2m_handle *h, const void *data, size_t n_points, const lio_pc2_layout *layout,
                          float pose[6], lio_s2m_result *res);
/* One mapping callback on the device: downsampleCurrentScan MO:1605-1611 (`downSizeFilterSurf.filter`, leaf =
 * mappingSurfLeafSize) + scan2MapOptimization MO:1839-1865 on the blob of cloud_info.cloud_deskewed (MO:440), without a host
 * round trip in between: one H2D copy of the blob (true DMA with layout->pin_host or lio_host_alloc memory; none when
 * `data` already is memory of the handle's device), the voxel filter on the handle's stream with its workspace kept on
 * the handle, the Gauss-Newton loop on the filter's output where it lies.  Bit-identical to lio_voxel_grid followed by
 * lio_s2m_register on its output (including PCL's pass-through when the leaf overflows the voxel index: the function
 * then still registers the unfiltered cloud, as the reference does).  off_x / off_intensity / point_step / pin_host of the
 * layout are used.  ds_out (may be NULL): receives laserCloudSurfLastDS as PointXYZI-compatible records, room for
 * n_points; *n_ds (may be NULL) = its size.  The filtered cloud stays staged on the handle: lio_kf_store_add_from_handle
 * (h, 0) makes it a keyframe (MO:2136-2142) without a copy through the host. */
int  lio_s2m_register_raw(lio_s2m_handle *h, const void *data, size_t n_points, const lio_pc2_layout *layout, float leaf,
                          float pose[6], lio_s2m_result *res, void *ds_out, size_t ds_out_stride, size_t *n_ds);
/* lio_deskew on the raw driver message (IP:214-232 + IP:577-615).  out: PointXYZI-compatible records as for lio_deskew. */
int  lio_deskew_pc2(const lio_deskew_config *cfg, const void *data, size_t n_points, const lio_pc2_layout *layout,
                    double time_scan_cur,
                    const double *imuTime, const double *imuRotX, const double *imuRotY,
                    const double *imuRotZ, int32_t imuPointerCur,
                    void *out, size_t out_stride_bytes, size_t *n_out);

/* ---- EXTENSION beyond this reference: the range-image build -------------------------------
 * BASELINE.json's north_star names "imageProjection's deskew/range-image build"; this fork's
 * projectPointCloud IP:577-615 no longer builds one and nothing in the fork fills
 * startRingIndex / endRingIndex / pointColInd / pointRange (MSG:4-8), which its own
 * featureExtraction.cpp reads.  lio_range_image is projectPointCloud +
 * cloudExtraction of upstream LIO-SAM (Velodyne/Ouster column rule, first point per range-image
 * cell wins) with this fork's deskewPoint IP:545-575, i.e. the producer lio_extract_features
 * needs.  No reference oracle exists for it (parity unpinned; checked against
 * oracle/lio_oracle.c lo_range_image only).
 * pts: PointXYZIRT records as for lio_deskew.  out: PointXYZI-compatible records, room for
 * N_SCAN * Horizon_SCAN; pointColInd / pointRange the same; startRingIndex / endRingIndex:
 * N_SCAN entries.  *n_out = points kept (ring-major, ascending column). */
typedef struct lio_range_image_config {
    int32_t N_SCAN, Horizon_SCAN, downsampleRate;
    float   lidarMinRange, lidarMaxRange;
    int32_t deskew_flag;     /* -1 = no per-point time field */
    int32_t device_id;
} lio_range_image_config;
void lio_range_image_default_config(lio_range_image_config *cfg);
int  lio_range_image(const lio_range_image_config *cfg, const void *pts, size_t n, size_t stride_bytes,
                     double time_scan_cur,
                     const double *imuTime, const double *imuRotX, const double *imuRotY,
                     const double *imuRotZ, int32_t imuPointerCur,
                     void *out, size_t out_stride_bytes, size_t *n_out,
                     int32_t *startRingIndex, int32_t *endRingIndex,
                     int32_t *pointColInd, float *pointRange);

/* calculateSmoothness, FE:81-101: curvature[i] for i in [5, n-5), also zeroes
 * neighbor_picked / label there (either may be NULL).  Host pointers. */
int  lio_curvature(int32_t device_id, const float *range, size_t n, float *curvature,
                   int32_t *neighbor_picked, int32_t *label);

/* The rest of FeatureExtraction::laserCloudInfoHandler FE:67-79: calculateSmoothness FE:81-101,
 * markOccludedPoints FE:103-139 and extractFeatures FE:141-238 on the device, consuming the
 * cloud_info arrays (MSG:4-8) as the reference does.
 * cloud: extractedCloud records (x,y,z @0,4,8, intensity @16), n points, ring-major.
 * startRingIndex/endRingIndex: cfg->N_SCAN entries.  Rings must own disjoint, ascending index
 * windows [start-5, end+4] (what upstream's cloudExtraction produces: start = first + 4,
 * end = last - 5, so a ring's window is the ring and the cell before it); a window holds at most
 * 4096 cells, i.e. 4096 points per ring (LIO_ERR_CAPACITY beyond); columns must fit int16.
 * A ring reads and writes neighbor_picked / label inside its own window only.
 * corner_out: room for 120 * N_SCAN records (FE:171: <= 20 per sector); surface_out: room for n.
 * Records have `stride_bytes` / `out_stride_bytes` (>= 20, multiples of 4); of an output record
 * only x, y, z and intensity are meaningful: its other bytes are left as they were or set to zero.
 * curvature / neighbor_picked / label (each n entries, may be NULL) receive cloudCurvature,
 * cloudNeighborPicked and cloudLabel as the reference leaves them after the handler.
 * Defined here where the reference is not (see oracle/lio_oracle.c lo_extract_features): the
 * flag arrays start from zero for every scan, equal curvatures keep ascending point index
 * (std::sort FE:162 leaves their order open), and a suppression walk FE:178-193 stops at the
 * array boundary instead of indexing pointColInd[-1]. */
typedef struct lio_feature_config {
    int32_t N_SCAN;          /* UT:164 */
    float   edgeThreshold;   /* UT:186, 1.0 in the yaml configs */
    float   surfThreshold;   /* UT:187, 0.1 */
    float   surfLeafSize;    /* mappingSurfLeafSize FE:56 */
    int32_t device_id;
} lio_feature_config;
void lio_feature_default_config(lio_feature_config *cfg);
int  lio_extract_features(const lio_feature_config *cfg, const void *cloud, size_t n, size_t stride_bytes,
                          const int32_t *startRingIndex, const int32_t *endRingIndex,
                          const int32_t *pointColInd, const float *pointRange,
                          void *corner_out, size_t *n_corner, void *surface_out, size_t *n_surface,
                          size_t out_stride_bytes, float *curvature, int32_t *neighbor_picked, int32_t *label);

/* ------------------------------------------------ local-map assembly (feeders) */
/* pcl::VoxelGrid<PointXYZI>::filter as used by downsampleCurrentScan MO:1605-1611
 * (downSizeFilterSurf, leaf = mappingSurfLeafSize) and MO:1581-1583: centroid per
 * voxel (x, y, z and intensity), output in ascending voxel index.  Records: x,y,z
 * @0,4,8 and intensity @16.  Returns LIO_OK, or 1 when PCL would pass the cloud
 * through unfiltered ("Leaf size is too small", voxel index overflow). */
int  lio_voxel_grid(int32_t device_id, const void *pts, size_t n, size_t stride_bytes, float leaf,
                    void *out, size_t out_stride_bytes, size_t *n_out);

/* extractCloud MO:1556-1588: laserCloudSurfFromMap = sum over the nearby keyframes of
 * transformPointCloud(surfCloudKeyFrames[i], cloudKeyPoses6D[i]) (MO:849-868), then
 * VoxelGrid(surroundingKeyframeMapLeafSize) -> laserCloudSurfFromMapDS.  poses are
 * [roll,pitch,yaw,x,y,z] per keyframe.  If h != NULL the result becomes h's resident map
 * (replaces lio_s2m_set_map, no round trip through the host); `out` (may be NULL) receives
 * the downsampled map as PointXYZI-compatible records. */
int  lio_assemble_map(lio_s2m_handle *h, int32_t device_id, int32_t n_keyframes, const void *const *clouds,
                      const size_t *n_pts, size_t stride_bytes, const float *poses, float leaf,
                      void *out, size_t out_stride_bytes, size_t *n_out);

/* Device-resident keyframe store = surfCloudKeyFrames (MO:128): every keyframe cloud is
 * uploaded once when it is saved (MO:2138-2142); lio_assemble_map_resident then builds the local
 * map of a scan from keyframe ids + their current poses (cloudKeyPoses6D) without touching the
 * host clouds again.  ids index the store in insertion order. */
typedef struct lio_kf_store lio_kf_store;
int  lio_kf_store_create(int32_t device_id, lio_kf_store **out);
void lio_kf_store_destroy(lio_kf_store *s);
int  lio_kf_store_add(lio_kf_store *s, const void *cloud, size_t n, size_t stride_bytes, int32_t *id_out);
int  lio_kf_store_count(const lio_kf_store *s);
/* Points of keyframe `id` (0 for an id the store does not hold): what a caller adds up to size `out` of
 * lio_assemble_map_resident. */
size_t lio_kf_store_points(const lio_kf_store *s, int32_t id);
/* The same from DEVICE memory (x,y,z @0,4,8, intensity @16 when stride >= 20, else 0): no host round trip. */
int  lio_kf_store_add_device(lio_kf_store *s, const void *d_cloud, size_t n, size_t stride_bytes, int32_t *id_out);
/* saveKeyFramesAndFactor MO:2136-2142 (`pcl::copyPointCloud(*laserCloudSurfLastDS, *thisSurfKeyFrame);
 * surfCloudKeyFrames.push_back(thisSurfKeyFrame)`): appends the scan that batch slot `scan` of `h` has just
 * registered (its records are still staged on the device) as a keyframe -- no D2H, no H2D. */
int  lio_kf_store_add_from_handle(lio_kf_store *s, lio_s2m_handle *h, int32_t scan, int32_t *id_out);
/* `out` (may be NULL) needs room for the SUM of the selected keyframes' points: the filter's output is at most that many,
 * and exactly that many when the leaf overflows PCL's voxel index (or the clouds hold non-finite coordinates) and the
 * input is passed through, as pcl::VoxelGrid does.  The same holds for `out` of lio_assemble_map (sum of n_pts). */
int  lio_assemble_map_resident(lio_s2m_handle *h, lio_kf_store *s, int32_t n_selected, const int32_t *ids,
                               const float *poses, float leaf, void *out, size_t out_stride_bytes, size_t *n_out);

/* ------------------------------------------------ surrounding keyframes (extractNearby MO:1519-1551) */
typedef struct lio_nearby_config {
    float  search_radius;    /* surroundingKeyframeSearchRadius, UT:316 default 50.0                  */
    float  pose_density;     /* surroundingKeyframeDensity, UT:314 default 1.0 (the shipped yamls: 2.0) */
    double recent_window_s;  /* the literal 10.0 of MO:1547                                            */
} lio_nearby_config;
void lio_nearby_default_config(lio_nearby_config *cfg);

/* cloudKeyPoses6D[first .. first+n) of keyframes the store already holds: [roll,pitch,yaw,x,y,z] per keyframe (the order
 * of transformTobeMapped) and its time (PointTypePose.time).  saveKeyFramesAndFactor MO:2107-2120 sets one, correctPoses
 * MO:2184-2196 rewrites all of them.  times == NULL keeps the stored times (LIO_ERR_ARG for a keyframe that has none yet);
 * non-finite values -> LIO_ERR_ARG.  Host only: never waits, and work already queued keeps the poses it was given; the
 * next lio_assemble_map_nearby uploads what changed on its own stream. */
int  lio_kf_store_set_poses(lio_kf_store *s, int32_t first, int32_t n, const float *poses, const double *times);

/* extractSurroundingKeyFrames MO:1590-1603 + extractCloud MO:1556-1588 in one call: the keyframes are selected on the
 * device from the stored poses (radius search around the last key pose, VoxelGrid at pose_density, nearest-pose relabel,
 * the keyframes younger than recent_window_s before time_cur, the radius recheck of MO:1562; DESIGN.md states the tie and
 * boundary conventions), then the map is assembled exactly as lio_assemble_map_resident does with those ids and their
 * stored poses, for the same handle kinds (h may be NULL).  ids_out (may be NULL) receives the selected list in order,
 * duplicates included; *n_ids its length.  `out` (may be NULL) holds out_cap records; a larger map -> LIO_ERR_ARG with the
 * needed count in *n_out (the handle's map is installed all the same).  An empty store: LIO_OK, *n_ids = 0, the handle's
 * map untouched (MO:1592-1593).  LIO_ERR_ARG when a keyframe has no pose, when the store and the handle live on different
 * devices, and when ids_out is given with ids_cap < *n_ids (*n_ids is the needed count; nothing is built). */
int  lio_assemble_map_nearby(lio_s2m_handle *h, lio_kf_store *s, const lio_nearby_config *cfg, double time_cur, float leaf,
                             int32_t *ids_out, int32_t ids_cap, int32_t *n_ids, void *out, size_t out_stride_bytes,
                             size_t out_cap, size_t *n_out);

/* ------------------------------------------------ loop-closure registration (performRSLoopClosure MO:1098-1143) */
/* pcl::IterativeClosestPoint<PointType, PointType> as MO:1110-1124 sets it up (no rejectors: setRANSACIterations(0) adds
 * none; TransformationEstimationSVD; DefaultConvergenceCriteria), its getFitnessScore and the corrected pose MO:1136-1143,
 * on the device.  DESIGN.md section 2 states what is defined here where PCL is not a function of its inputs (ties, the
 * order of sums, the thresholds below: parity unpinned, restated from memory).  Out-of-range values are refused with
 * LIO_ERR_ARG, never clamped. */
#define LIO_ICP_MAX_ITERS 1000
enum {                                  /* lio_icp_result.state = DefaultConvergenceCriteria::ConvergenceState */
    LIO_ICP_NOT_CONVERGED      = 0,
    LIO_ICP_ITERATIONS         = 1,
    LIO_ICP_TRANSFORM          = 2,
    LIO_ICP_ABS_MSE            = 3,
    LIO_ICP_REL_MSE            = 4,
    LIO_ICP_NO_CORRESPONDENCES = 5
};
typedef struct lio_icp_config {
    double  max_corr_dist;      /* 30.0     setMaxCorrespondenceDistance: historyKeyframeSearchRadius * 2, MO:1112 (yaml: 15.0) */
    double  transform_eps;      /* 1e-6     setTransformationEpsilon MO:1114: bound on |t_step|^2                                 */
    double  fitness_eps;        /* 1e-6     setEuclideanFitnessEpsilon MO:1115: bound on |mse - mse_prev| (ABS_MSE)               */
    double  rel_mse_eps;        /* 1e-5     bound on |mse - mse_prev| / mse_prev (REL_MSE); PCL 1.10 default                      */
    double  rotation_threshold; /* 0.99999  bound on cos(angle of the step) = 0.5 (trace R - 1); PCL 1.10 default                 */
    double  fitness_max;        /* 0.3      historyKeyframeFitnessScore UT:324: accepted = converged && fitness <= fitness_max    */
    int32_t max_iters;          /* 100      setMaximumIterations MO:1113 (<= LIO_ICP_MAX_ITERS)                                   */
    int32_t min_corr;           /* 3        fewer correspondences end the loop unconverged; PCL 1.10 default                      */
    int32_t max_similar;        /* 0        consecutive "similar" iterations before a threshold counts; PCL 1.10 default          */
    int32_t min_source_points;  /* 300      MO:1104 (lio_kf_store_loop_icp only)                                                  */
    int32_t min_target_points;  /* 1000     MO:1104                                                                               */
    int32_t lookahead;          /* iterations enqueued ahead of the look at the done flag; 0 = auto (4)                           */
} lio_icp_config;

typedef struct lio_icp_result {
    int32_t status;             /* what the call returned                                                                   */
    int32_t converged;          /* icp.hasConverged()                                                                       */
    int32_t state;              /* LIO_ICP_*                                                                                */
    int32_t iters;              /* nr_iterations_                                                                           */
    int32_t n_corr_last;        /* correspondences of the last executed iteration                                           */
    int32_t accepted;           /* converged && fitness <= fitness_max, MO:1124                                             */
    int32_t n_source, n_target; /* points of the two clouds that were aligned                                               */
    int32_t n_launches;         /* kernel launches of the loop and the fitness pass (those that exited at once included)    */
    int32_t pad;
    double  fitness;            /* icp.getFitnessScore(); DBL_MAX when no source point found a neighbour                    */
    float   T[16];              /* icp.getFinalTransformation(), row-major                                                  */
    float   pose_corrected[6];  /* [roll,pitch,yaw,x,y,z] of T * tWrong, MO:1140-1143 (lio_kf_store_loop_icp only, else 0)  */
} lio_icp_result;

/* Optional clouds of lio_kf_store_loop_icp: the two submaps (cureKeyframeCloud, prevKeyframeCloud) and closed_cloud
 * (MO:1131), PointXYZI-compatible records of `stride` bytes.  A null pointer skips that cloud; cap_* = records it holds;
 * n_* = records needed (written always).  A cloud that does not fit: LIO_ERR_ARG with the needed counts, nothing aligned. */
typedef struct lio_icp_clouds {
    void  *source, *target, *closed;
    size_t cap_source, cap_target, cap_closed;
    size_t n_source, n_target, n_closed;
    size_t stride;
} lio_icp_clouds;

void lio_icp_default_config(lio_icp_config *cfg);
/* icp.setInputSource(source); icp.setInputTarget(target); icp.align(unused, guess); icp.getFitnessScore() on two host
 * clouds (x,y,z @0,4,8; strides >= 12, multiples of 4).  guess: 16 floats row-major, or NULL for the identity (a non-finite
 * entry: LIO_ERR_ARG).  Which points take part: a TARGET point when all three of its coordinates are at most 1e15 in magnitude
 * (the bound of the cell sort; NaN, inf and larger finite values leave the point out, and the grid's box takes each axis from
 * the coordinates within the bound on that axis); a SOURCE point when its coordinates are finite, before and after it is
 * transformed.  A source point beyond 1e15 is searched like any other: its squared distance is huge or overflows to inf, so it
 * fails every gate, and the fitness score counts it only while that distance is finite.  An empty cloud, or a target without
 * a point that takes part: LIO_OK, state NO_CORRESPONDENCES, converged 0, T = guess. */
int  lio_icp_align(int32_t device_id, const void *source, size_t n_source, size_t source_stride,
                   const void *target, size_t n_target, size_t target_stride,
                   const lio_icp_config *cfg, const float *guess, lio_icp_result *result);
/* MO:1098-1143 in one call, from the resident clouds and the stored poses (lio_kf_store_set_poses): the source submap is
 * keyframe key_cur, the target submap the keyframes key_pre - search_num .. key_pre + search_num that the store holds
 * (loopFindNearKeyframes MO:1360-1383: transform, sum, VoxelGrid at `leaf` = loopClosureICPSurfLeafSize; the same K6 + K7
 * code as lio_assemble_map_resident, bit for bit).  pose_index = -1: every keyframe under its own pose; >= 0: every
 * keyframe under the pose of that one keyframe.  Fewer than min_source_points / min_target_points (MO:1104): returns
 * LIO_TOO_FEW_POINTS, nothing aligned.  Then the alignment, the fitness score and pose_corrected.  Neither submap visits
 * the host unless `clouds` (may be NULL) asks for it. */
int  lio_kf_store_loop_icp(lio_kf_store *s, int32_t key_cur, int32_t key_pre, int32_t search_num, int32_t pose_index,
                           float leaf, const lio_icp_config *cfg, lio_icp_result *result, lio_icp_clouds *clouds);
/* detectLoopClosureDistance MO:1271-1304 over the stored poses (host only): the key poses with d2 < radius^2 around the
 * last one, ordered by (d2, index); the first whose |time - time_cur| > time_diff is *key_pre, *key_cur = the last key.
 * Returns 1 when found, 0 when none is or when it is the last key itself (the loopIndexContainer lookup MO:1277 stays with
 * the caller), LIO_ERR_ARG when a keyframe has no pose or time. */
int  lio_kf_store_detect_loop(lio_kf_store *s, float radius, double time_diff, double time_cur, int32_t *key_cur, int32_t *key_pre);
/* Test hook: lio_icp_align that also returns, per executed iteration k < *n_trace, the step transformation (steps[k][16]),
 * the number of correspondences and their mean squared distance, and the correspondence (target index, -1 = none) of every
 * source point at iteration rec_iter (-1 = none).  Arrays of cfg->max_iters entries; corr of n_source; any may be NULL. */
int  lio_icp_debug_trace(int32_t device_id, const void *source, size_t n_source, size_t source_stride,
                         const void *target, size_t n_target, size_t target_stride,
                         const lio_icp_config *cfg, const float *guess, int32_t rec_iter, lio_icp_result *result,
                         float *steps, int32_t *n_corr, double *mse, int32_t *corr, int32_t *n_trace);
/* Test hook, read-only: the search grid an alignment lays over `target`, by the very code the alignment runs (the box, the
 * trial grid of 64 cells along the longest side, the edge for four points per occupied cell).  any = 0: no target point
 * within the coordinate bound, every other field 0.  occupied = -1: the box is a point and no trial grid is laid (edge 1). */
typedef struct lio_icp_grid_info {
    float   origin[3];          /* the box's minimum corner = the corner of cell (0, 0, 0) */
    float   edge, inv_cell;     /* cell edge and the factor the cell formula multiplies with */
    int32_t nx, ny, nz, n_cells;
    int32_t occupied;           /* occupied cells of the trial grid */
    int32_t any;
} lio_icp_grid_info;
int  lio_icp_debug_grid(int32_t device_id, const void *target, size_t n_target, size_t target_stride, lio_icp_grid_info *out);

/* ------------------------------------------------ Scan Context loop detection (performSCLoopClosure MO:1163-1269) */
/* SCManager (Scancontext.cpp, "SC:") on the device: makeScancontext + the two keys of every keyframe, kept next to the
 * resident keyframes (descriptor k = keyframe k), and detectLoopClosureID over them.  DESIGN.md section 4c states what is
 * defined here where Eigen and nanoflann are not functions of their inputs (every sum in ascending index order, an exact
 * brute-force ring-key search ordered by (distance, index); parity unpinned).  Out-of-range values are refused with
 * LIO_ERR_ARG, never clamped. */
#define LIO_SC_MAX_CELLS      4096   /* num_rings * num_sectors: what the kernels' LDS layout holds */
#define LIO_SC_MAX_DIM        256    /* num_rings and num_sectors, each                              */
#define LIO_SC_MAX_CANDIDATES 16
typedef struct lio_sc_config {
    double  max_radius;          /* 80.0  PC_MAX_RADIUS: points with sqrtf(x^2 + y^2) beyond it are dropped       */
    double  lidar_height;        /* 2.0   LIDAR_HEIGHT, added to z                                                 */
    double  search_ratio;        /* 0.1   SEARCH_RATIO: shifts within round(0.5 ratio S) of the sector-key shift, [0, 1] */
    double  dist_thres;          /* 0.3   SC_DIST_THRES: a loop when min_dist < dist_thres                         */
    int32_t num_rings;           /* 20    PC_NUM_RING   (<= LIO_SC_MAX_DIM; rings * sectors <= LIO_SC_MAX_CELLS)   */
    int32_t num_sectors;         /* 60    PC_NUM_SECTOR                                                            */
    int32_t num_exclude_recent;  /* 30    NUM_EXCLUDE_RECENT                                                       */
    int32_t num_candidates;      /* 3     NUM_CANDIDATES_FROM_TREE (1 .. LIO_SC_MAX_CANDIDATES)                    */
    int32_t tree_period;         /* 10    TREE_MAKING_PERIOD_ (>= 1)                                               */
    int32_t pad;
} lio_sc_config;

typedef struct lio_sc_result {
    int32_t status;              /* what the call returned                                                          */
    int32_t loop_id;             /* detectLoopClosureID().first: the matched descriptor, -1 = no loop               */
    int32_t align;               /* nn_align: the sector shift of the best candidate                                */
    int32_t nn_idx;              /* the best candidate whether or not it passed the threshold                       */
    int32_t n_searched;          /* descriptors [0, n_searched) were searched: the prefix of the last rebuild       */
    int32_t n_candidates;        /* min(num_candidates, n_searched) entries of the arrays below are set             */
    float   yaw_diff_rad;        /* detectLoopClosureID().second = deg2rad(align * 360 / num_sectors)               */
    int32_t pad;
    double  min_dist;            /* distance of nn_idx; 1e7 when nothing was compared                               */
    int32_t cand_idx[LIO_SC_MAX_CANDIDATES];      /* candidates in (ring-key distance, index) order                 */
    float   cand_ring_d2[LIO_SC_MAX_CANDIDATES];  /* their squared ring-key distances (fp32)                        */
    double  cand_dist[LIO_SC_MAX_CANDIDATES];     /* distanceBtnScanContext().first; 1e7 = no common non-zero column  */
    int32_t cand_align[LIO_SC_MAX_CANDIDATES];    /* distanceBtnScanContext().second                                */
} lio_sc_result;

void lio_sc_default_config(lio_sc_config *cfg);
/* makeScancontext + makeRingkey / makeSectorkeyFromScancontext (SC:151-227) of one host cloud (x,y,z @0,4,8; stride >= 12,
 * a multiple of 4): desc[num_rings * num_sectors] ring-major, ring_key[num_rings] (the float of polarcontext_invkeys_mat_),
 * sector_key[num_sectors]; any may be NULL.  Non-finite points and points with x == 0 and y == 0 are skipped.  An empty
 * cloud: all zeros, LIO_OK. */
int  lio_sc_make(int32_t device_id, const void *cloud, size_t n, size_t stride_bytes, const lio_sc_config *cfg,
                 float *desc, float *ring_key, double *sector_key);
/* makeAndSaveScancontextAndKeys (MO:2149-2156 with SINGLE_SCAN_FULL): appends the descriptor of the next keyframe, from a
 * host cloud, from device memory (x,y,z @0,4,8; stride >= 12, pointer and stride multiples of 4), or from the whole cloud that h's last lio_s2m_register_raw
 * staged on the device -- no copy at all.  cfg == NULL: the geometry of the store's first descriptor (the defaults for the
 * first one); a geometry that differs from the first descriptor's -> LIO_ERR_ARG.  id_out may be NULL. */
int  lio_kf_store_sc_add(lio_kf_store *s, const void *cloud, size_t n, size_t stride_bytes, const lio_sc_config *cfg, int32_t *id_out);
int  lio_kf_store_sc_add_device(lio_kf_store *s, const void *d_cloud, size_t n, size_t stride_bytes, const lio_sc_config *cfg,
                                int32_t *id_out);
int  lio_kf_store_sc_add_from_handle(lio_kf_store *s, lio_s2m_handle *h, const lio_sc_config *cfg, int32_t *id_out);
int  lio_kf_store_sc_count(const lio_kf_store *s);
/* num_rings / num_sectors of the store's descriptors (those of the first one); 0, 0 while it holds none. */
int  lio_kf_store_sc_geometry(const lio_kf_store *s, int32_t *num_rings, int32_t *num_sectors);
/* Descriptor `id` and its keys, sized as for lio_sc_make with the store's geometry (lio_kf_store_sc_geometry); any may be NULL. */
int  lio_kf_store_sc_get(lio_kf_store *s, int32_t id, float *desc, float *ring_key, double *sector_key);
/* detectLoopClosureID (SC:253-344): the query is the last descriptor.  Fewer than num_exclude_recent + 1 descriptors: LIO_OK,
 * loop_id -1, yaw 0, nothing searched and the period counter untouched.  Otherwise the searchable prefix is refreshed to
 * count - num_exclude_recent when the store's counter is a multiple of tree_period (a stale prefix in between is reference
 * behaviour), the counter is incremented, and the num_candidates nearest ring keys of the prefix are compared.  The result
 * feeds lio_kf_store_loop_icp(s, count - 1, loop_id, search_num, 0, ...) -- pose_index = 0 is loop_index = 0 of MO:1193-1194.
 * cfg's num_rings / num_sectors must be the store's. */
int  lio_kf_store_sc_detect(lio_kf_store *s, const lio_sc_config *cfg, lio_sc_result *result);
/* Test hook: distanceBtnScanContext (SC:116-148) of two host descriptors (desc_a = _sc1, the query). */
int  lio_sc_distance(int32_t device_id, const float *desc_a, const float *desc_b, const lio_sc_config *cfg, double *dist, int32_t *align);

/* ------------------------------------------------ planning local map (publishLocalMap MO:2442-2541) */
/* pcl::StatisticalOutlierRemoval<PointXYZI> as MO:293-294 sets it up and MO:2513-2514 runs it (sor.setMeanK,
 * sor.setStddevMulThresh, sor.filter), on the device.  DESIGN.md section 4d states the conventions (parity unpinned,
 * restated from memory): for every point the mean_k + 1 smallest fp32 squared distances to all points of the cloud, the
 * point itself included, the smallest dropped; dist_i = the fp64 mean of their square roots, rounded to float; a point
 * stays iff dist_i <= mean + stddev_mul * stddev of all dist_i.  Input order and intensity are kept.  Records: x,y,z
 * @0,4,8, intensity @16 when stride >= 20 (else 0); out records are PointXYZI (out_stride >= 20); `out` (may be NULL: count
 * only) holds n records.  Points with a non-finite coordinate (or one beyond 1e15 m, which the search grid leaves out) are
 * dropped and not counted.  mean_dist (may be NULL): n floats, dist_i per input point, NaN for a dropped one.  stats (may
 * be NULL): mean, stddev, threshold.  Returns LIO_OK, or 1 when the cloud has at most mean_k such points and is passed
 * through (dist_i = 0, stats = 0, 0, +inf).  mean_k outside [1, 32] or a non-finite stddev_mul -> LIO_ERR_ARG. */
int  lio_sor_filter(int32_t device_id, const void *pts, size_t n, size_t stride_bytes, int32_t mean_k, float stddev_mul,
                    void *out, size_t out_stride_bytes, size_t *n_out, float *mean_dist, double stats[3]);

/* Test hook, read-only: the search grid lio_sor_filter lays over the cloud at `mean_k`, by the very code the filter runs (the
 * box of the coordinates within 1e15 m, the trial grid, the edge for (mean_k + 1) / 3 points per occupied cell).  any = 0: no
 * participating point on some axis, the grid is one empty cell at the origin (edge 1).  occupied = -1: no trial grid was laid.
 * An empty cloud: LIO_OK, every field 0 but occupied = -1.  mean_k outside [1, 32] -> LIO_ERR_ARG. */
int  lio_sor_debug_grid(int32_t device_id, const void *pts, size_t n, size_t stride_bytes, int32_t mean_k, lio_icp_grid_info *out);

typedef struct lio_local_map_config {
    int32_t n_keyframes;      /* localMapKeyFramesNumber  UT:219  30   */
    float   front, left, back, right; /* localMapFront .. localMapRight UT:220-223  70, 40, 20, 40 */
    int32_t remove_outliers;  /* useRemovingOutliers      UT:227  1    */
    int32_t mean_k;           /* meanK                    UT:228  10   */
    float   stddev_mul;       /* stddevThreshold          UT:229  1.0  */
    int32_t downsample;       /* useDownSamplingLocalMap  UT:224  1    */
    float   leaf;             /* localMappingSurfLeafSize UT:226  0.01 */
} lio_local_map_config;
typedef struct lio_local_map_info {
    int32_t first_keyframe, n_keyframes;            /* startPoseNum MO:2462 and how many keyframes were summed */
    int32_t n_summed, n_cropped, n_inliers, n_out;  /* points after each stage */
    int32_t voxel_passthrough;                      /* 1: pcl::VoxelGrid would not filter (voxel index overflow) */
    int32_t pad;
    double  sor_mean, sor_stddev, sor_threshold;    /* 0, 0, 0 when remove_outliers is off */
} lio_local_map_info;
void lio_local_map_default_config(lio_local_map_config *cfg);
/* MO:2447-2540 in one call, from the resident store: the keyframes max(0, count - n_keyframes) .. count - 1 summed under
 * their stored poses (MO:2462-2466, the kernels of lio_assemble_map_resident), moved into the yaw-aligned vehicle frame of
 * `pose` = transformTobeMapped (MO:2474-2489: yaw, x, y, z are used; roll and pitch are not undone) and cropped to
 * -left <= x <= right, -back <= y <= front (MO:2502-2506, limits inclusive), filtered as lio_sor_filter when
 * remove_outliers, voxel-filtered as lio_voxel_grid when downsample.  At the default leaf the voxel index overflows and
 * PCL passes the cloud through: info->voxel_passthrough says so, it is no error.  `out` (may be NULL: count only) holds
 * out_cap PointXYZI records; a larger result -> LIO_ERR_ARG with the needed count in *n_out.  An empty store: LIO_OK,
 * *n_out = 0 (MO:2444).  LIO_ERR_ARG for a summed keyframe without a pose, a non-finite pose and an out-of-range config
 * (n_keyframes < 1, limits not finite or crossing, flags other than 0 / 1, mean_k, stddev_mul, leaf).  info may be NULL. */
int  lio_kf_store_local_map(lio_kf_store *s, const lio_local_map_config *cfg, const float pose[6],
                            void *out, size_t out_stride_bytes, size_t out_cap, size_t *n_out, lio_local_map_info *info);

/* ------------------------------------------------ planning height map (grid_map_pcl's loader as the fork rewrote it) */
/* The only subscriber of liorf/mapping/map_4planning, grid_map_pcl_loader_node.cpp:39-76: every local map becomes the
 * "elevation" layer of /height_map.  DESIGN.md section 4e states the conventions (parity unpinned: PCL, Eigen and grid_map
 * are restated, not linked).  The defaults are config/parameters.yaml's. */
typedef struct lio_height_map_config {
    float   roll, pitch;          /* thisPoseRoll / thisPosePitch, radians, as the node stores them (float) */
    int32_t level_and_ego_filter; /* 1: GridMapPclLoader.cpp:80-85 (level by R1, ego-vehicle height filter, R2) */
    int32_t remove_outliers;      /* outlier_removal.is_remove_outliers  1 */
    int32_t mean_k;               /* outlier_removal.mean_K              10 */
    float   stddev_mul;           /* outlier_removal.stddev_threshold    1.0 */
    int32_t downsample;           /* downsampling.is_downsample_cloud    0 */
    float   voxel[3];             /* downsampling.voxel_size             0.1 0.1 0.1; the three must be equal when downsample */
    double  resolution;           /* grid_map.resolution                 0.2 */
    int32_t min_points_per_cell, max_points_per_cell;   /* grid_map.min/max_num_points_per_cell  1, 1000000000 */
    int32_t use_cluster;          /* cluster_extraction.use_cluster      0 */
    float   cluster_tolerance;    /* cluster_extraction.cluster_tolerance 1.0 */
    int32_t cluster_min_points, cluster_max_points;     /* cluster_extraction.min/max_num_points  1, 1000000000 */
    int32_t use_max_height;       /* cluster_extraction.use_max_height_as_cell_elevation  0 */
    int32_t fill_holes;           /* 0: the reference as written (its hole-filling pass changes nothing); 1: labelled extension */
} lio_height_map_config;
typedef struct lio_height_map_info {
    int32_t rows, cols;             /* grid_map size(0) (along x), size(1) (along y) */
    double  length[2], position[2]; /* grid_map length_, position_ */
    int32_t n_in;                   /* points given */
    int32_t n_inliers;              /* after the outlier filter (points with a non-finite coordinate are gone from here on) */
    int32_t n_filtered;             /* after the voxel filter and the ego filter: the points the grid is laid around */
    int32_t n_binned;               /* of those, the points inside a cell (an index equal to the size is the reference's spare row) */
    int32_t n_valid_cells;          /* cells with an elevation before the hole filling */
    int32_t n_filled_cells;         /* cells the hole filling gave one (0 when fill_holes is 0) */
    int32_t voxel_passthrough, pad; /* 1: pcl::VoxelGrid would not filter (voxel index overflow) */
} lio_height_map_info;
void lio_height_map_default_config(lio_height_map_config *cfg);
/* helpers.cpp:97-105 on n host records (x,y,z @0,4,8; the loader's cloud is PointXYZ), in the reference's order: the outlier
 * filter of lio_sor_filter when remove_outliers; lio_voxel_grid when downsample; R1 = Rx(-roll) Ry(-pitch), the ego filter
 * of PointcloudProcessor.cpp:39-55 on the levelled point, R2 = Rx(roll) Ry(pitch) on what it keeps (R2 is not R1's inverse:
 * reproduced as written); the geometry from the cloud's box; every point to its cell; per cell with min_points_per_cell <=
 * count <= max_points_per_cell either the fp64 mean of z in input order or, with use_cluster, the min (max) over the
 * connected components under cluster_tolerance of that mean; the hole filling.  `grid`: column-major rows x cols floats
 * (grid_map::Matrix), NaN = no elevation; NULL = the geometry only (the counts behind n_filtered stay 0).  More cells than
 * grid_cap -> LIO_ERR_ARG with rows and cols filled in.  An empty cloud, and a cloud whose box has no extent along x or y
 * (where the reference asserts): LIO_OK with rows or cols 0.  Points with a non-finite coordinate (or one beyond 1e15 m) are
 * dropped.  fill_holes = 1: every NaN cell with four valid cells in rows [r-5, r+5) x cols [c-5, c+5) becomes the mean of the
 * four nearest, found by the cascade of GridMapPclLoader.cpp:225-249 on the layer before the pass.  LIO_ERR_ARG, never a
 * clamp, for resolution < 1e-4 (the reference throws), flags other than 0 / 1, non-finite angles, mean_k / stddev_mul as
 * lio_sor_filter, unequal or non-positive voxel sizes when downsample, negative counts, a negative or non-finite tolerance. */
int  lio_height_map(int32_t device_id, const void *pts, size_t n, size_t stride_bytes, const lio_height_map_config *cfg,
                    float *grid, size_t grid_cap, lio_height_map_info *info);
/* lio_kf_store_local_map's stages, then the chain above on the device cloud they leave: nothing goes to the host in between,
 * only the grid crosses.  lm_info (may be NULL) = what lio_kf_store_local_map reports for the same arguments.  An empty
 * store or an empty local map: LIO_OK, rows = cols = 0.  Replaces cloudMapInfoHandler, grid_map_pcl_loader_node.cpp:47-54.
 * This call and the four lio_kf_store_* planning calls below are one chain with different stages behind the height map: on
 * any return other than for a null argument the infos are zeroed or filled. */
int  lio_kf_store_height_map(lio_kf_store *s, const lio_local_map_config *lm, const float pose[6],
                             const lio_height_map_config *cfg, float *grid, size_t grid_cap,
                             lio_local_map_info *lm_info, lio_height_map_info *info);

/* ------------------------------------------------ terrain layers (grid_map_filters' demo chain behind the height map) */
/* grid_map_demos/config/filters_demo_filter_chain.yaml on the elevation grid: elevation -> smooth (MeanInRadiusFilter) ->
 * surface normals (NormalVectorsFilter) -> slope -> roughness (MathExpressionFilter) -> edges
 * (SlidingWindowMathExpressionFilter) -> traversability -> its two ThresholdFilters.  The input grid stands for the
 * chain's `elevation_inpainted`: OpenCV's inpaint is not reproduced, fill_holes = 1 of the height map is the labelled
 * substitute (lio_median_fill below is the reference tree's own inpainting filter, restated exactly).  DESIGN.md section 4g states the conventions (parity unpinned: Eigen, EigenLab and grid_map are restated, not
 * linked).  The defaults are the yaml's literal values, which are tuned for a 0.02 m grid: at the loader's 0.2 m resolution
 * a node scales the three lengths (normal_radius, smooth_radius, edge_window_length) accordingly, by 10. */
enum { LIO_TERRAIN_SMOOTH = 0, LIO_TERRAIN_NORMAL_X, LIO_TERRAIN_NORMAL_Y, LIO_TERRAIN_NORMAL_Z,
       LIO_TERRAIN_SLOPE, LIO_TERRAIN_ROUGHNESS, LIO_TERRAIN_EDGES, LIO_TERRAIN_TRAVERSABILITY,
       LIO_TERRAIN_N_LAYERS };
typedef struct lio_terrain_config {
    int32_t  normal_method;       /* 0 area (NormalVectorsFilter.cpp:195-251), 1 raster (:304-394)            */
    int32_t  normal_axis;         /* normal_vector_positive_axis: 0 x, 1 y, 2 z                    2          */
    double   normal_radius;       /* surface_normals.radius                                        0.05       */
    double   smooth_radius;       /* mean_in_radius.radius                                         0.06       */
    int32_t  edge_window_size;    /* window_size; 0 = derive from edge_window_length               0          */
    double   edge_window_length;  /* edge_detection.window_length                                  0.05       */
    float    slope_critical, roughness_critical;   /* the 0.6 and 0.1 of the traversability expression       */
    float    slope_weight, roughness_weight;       /* 0.5, 0.5                                                */
    uint32_t layers;              /* bit i set: layer i is copied out; default all                            */
} lio_terrain_config;
typedef struct lio_terrain_info {
    int32_t rows, cols, n_valid_cells;      /* finite cells of the input layer                                */
    int32_t normal_method_used;             /* 1 when area fell back to raster (radius <= 0, as :39-51 do)    */
    int32_t n_normal_cells, n_few_points, n_degenerate;   /* normals written; nPoints < 3; eigenvalue(1) <= 1e-8 */
    int32_t edge_window_size;               /* the odd size used                                              */
} lio_terrain_info;
void lio_terrain_default_config(lio_terrain_config *cfg);
/* The chain on a host grid of rows x cols floats, column-major (grid_map::Matrix), NaN = no elevation; `length` and
 * `position` are lio_height_map_info's; length[a] must equal size[a] * resolution.  `layers` (may be NULL: the
 * counts only) receives the layers whose bit is set in cfg->layers, in enum order, each rows x cols floats, column-major,
 * NaN = no value; layers_cap counts floats.  Fewer than (set bits) x rows x cols -> LIO_ERR_ARG with rows and cols
 * filled in.  rows or cols 0: LIO_OK, nothing written.  Stage by stage:
 *  - smooth, every cell: (float)(fp64 sum of the finite input values in the circle of smooth_radius / their count), NaN for
 *    none.  A cell belongs to a circle iff dx dx + dy dy <= radius radius on the fp64 cell centres of GridMapMath.cpp:130-145,
 *    visited in SubmapIterator order over the window of CircleIterator::findSubmapParameters;
 *  - normals, area: from the fp64 sums of (x, y, z) and their products over the circle of normal_radius, the eigenvector of
 *    the smallest eigenvalue of the covariance by SelfAdjointEigenSolver::computeDirect; UnitZ for fewer than 3 points or
 *    eigenvalue(1) <= 1e-8; written where the centre cell is finite.  normal_radius <= 0 falls back to raster
 *    (normal_method_used = 1).  Raster: the five-cell stencil on interior cells, also for a NaN centre between two valid
 *    neighbours; none on a grid of fewer than 3 rows or columns.  Both are flipped towards normal_axis;
 *  - slope = acosf(normal_z), roughness = fabsf(input - smooth);
 *  - edges, every cell: the standard deviation of slope over the window of edge_window_size cells (odd; 0: derived from
 *    edge_window_length as round(length / resolution), plus 1 when even), cropped at the borders, float, column-major;
 *  - traversability = w_s (1 - slope / s_crit) + w_r (1 - roughness / r_crit) in float, then !(t >= 0) -> 0 and
 *    !(t <= 1) -> 1 as the two ThresholdFilters do: a cell without slope or roughness ends at 0, not NaN.
 * LIO_ERR_ARG, never a clamp: non-finite or negative radii, window length, criticals or weights; resolution < 1e-4 or
 * non-finite geometry; a method or axis out of range; an even or negative edge_window_size; bits beyond the eight layers;
 * a radius or half-window above 32 cells (the limit of the kernels' LDS tile halo). */
int  lio_terrain_layers(int32_t device_id, const float *elevation, int32_t rows, int32_t cols, double resolution,
                        const double length[2], const double position[2], const lio_terrain_config *cfg,
                        float *layers, size_t layers_cap, lio_terrain_info *info);
/* lio_kf_store_height_map's chain (same arguments, same grid bytes; `grid` may be NULL), then the chain above on the
 * device grid it leaves: only the elevation grid (when grid != NULL) and the requested layers cross to the host.  hm->
 * resolution is the grid's.  An empty store or an empty local map: LIO_OK, rows = cols = 0.  Complete on return.  What
 * would follow cloudMapInfoHandler in a planning node. */
int  lio_kf_store_terrain_map(lio_kf_store *s, const lio_local_map_config *lm, const float pose[6],
                              const lio_height_map_config *hm, const lio_terrain_config *cfg,
                              float *grid, size_t grid_cap, float *layers, size_t layers_cap,
                              lio_local_map_info *lm_info, lio_height_map_info *hm_info, lio_terrain_info *info);

/* ------------------------------------------------ global map, map export, read-back (the last readers of surfCloudKeyFrames) */
/* With the four calls below the store is the only owner of the keyframe clouds: a node needs no host copy of one to
 * visualise, save or publish.  Rules that hold for all four:
 *  - they leave the store and the handle as they found them -- they work in buffers of their own, kept between calls, on
 *    private non-blocking streams; the map installed in a handle and the buffers of lio_assemble_map_nearby are not touched;
 *  - they are complete when they return;
 *  - calls on one store remain non-re-entrant: the node holds `mtx` around them, as MO:1010 does;
 *  - lio_kf_store_global_map may upload the dirty range of the key-pose table (lio_kf_store_set_poses) on its own stream.
 * DESIGN.md section 4f states the conventions (parity unpinned). */
typedef struct lio_global_map_config {
    float search_radius;   /* globalMapVisualizationSearchRadius  1000.0 */
    float pose_density;    /* globalMapVisualizationPoseDensity   10.0   */
    float leaf;            /* globalMapVisualizationLeafSize      1.0    */
} lio_global_map_config;
typedef struct lio_global_map_info {
    int32_t n_keyframes, n_summed, n_out, voxel_passthrough;   /* kept list (duplicates included), its points, the map, 1: the
                                                                * cloud filter's index overflows and the sum passes through */
} lio_global_map_info;
void lio_global_map_default_config(lio_global_map_config *cfg);
/* publishGlobalMap MO:992-1041: lio_assemble_map_nearby with h == NULL, without the recent-keyframe suffix of MO:1544-1551
 * and without reading a key-pose time: the radius set around the last key pose (d2 < (float)((double)R * R), ordered by
 * (d2, i)), VoxelGrid at pose_density over (x, y, z, intensity = i) -- passed through when the voxel index overflows --,
 * every centroid relabelled to its nearest key pose over all of them (ties to the lowest index), the recheck
 * pointDistance > R of MO:1030 on the centroid's own coordinates, then the kept keyframes (duplicates included) under their
 * stored poses, summed and voxel-filtered at `leaf`.  ids_out (may be NULL) receives the kept list, *n_ids its length; `out`
 * (may be NULL: count only) holds out_cap PointXYZI records.  An empty store (MO:997): LIO_OK, *n_ids = 0, *n_out = 0.
 * LIO_ERR_ARG for a keyframe without a pose, a non-finite or non-positive radius, density or leaf, ids_cap < *n_ids (the
 * needed count is returned, nothing is built) and out_cap < *n_out (the needed count is returned).  info may be NULL. */
int  lio_kf_store_global_map(lio_kf_store *s, const lio_global_map_config *cfg,
                             int32_t *ids_out, int32_t ids_cap, int32_t *n_ids,
                             void *out, size_t out_stride_bytes, size_t out_cap,
                             size_t *n_out, lio_global_map_info *info);

typedef struct lio_export_config {
    float   resolution;    /* save_map.srv `resolution`; 0 = no filtered copy (MO:943) */
    int32_t chunk_points;  /* points per transfer chunk of the unfiltered cloud; 0 = default (1 << 22) */
} lio_export_config;
/* saveMapService MO:935-962.  out_full receives globalSurfCloud: every keyframe 0 .. count - 1 in store order under its
 * stored pose, always the sum of the keyframe sizes (GlobalMap.pcd; SurfMap.pcd when resolution is 0).  It is never
 * materialised on the device: one kernel finds each point's keyframe, transforms it and writes chunk_points records at a
 * time straight into one of two pinned staging buffers, and the host copies one chunk out while the next is written.  Device
 * memory of this path: 92 bytes per keyframe (descriptor 64, pose 24, offset 4) plus the allocator's slack, whatever chunk_points is; pinned host memory: two chunks.  out_ds is written
 * only when resolution != 0: lio_voxel_grid of that cloud at `resolution` (passed through on index overflow, reported in
 * *voxel_passthrough).  The filtered copy DOES need the whole world-frame cloud on the device (16 bytes per point plus the
 * sort's workspace): PCL's filter is a global sort.  Either output may be NULL: its count alone is returned.  LIO_ERR_ARG
 * for a negative or non-finite resolution, chunk_points outside [256, 1 << 26] unless 0, a keyframe without a pose, and
 * caps that are too small (*n_full and *n_ds hold the needed counts; nothing is written). */
int  lio_kf_store_export_map(lio_kf_store *s, const lio_export_config *cfg,
                             void *out_full, size_t full_stride_bytes, size_t full_cap, size_t *n_full,
                             void *out_ds, size_t ds_stride_bytes, size_t ds_cap, size_t *n_ds,
                             int32_t *voxel_passthrough);

/* Keyframe `id` back from the store: bit for bit as stored (pose == NULL, lidar frame), or transformPointCloud of it under
 * pose = [roll,pitch,yaw,x,y,z].  `out` may be NULL (count only).  LIO_ERR_ARG for an unknown id, a non-finite pose and
 * out_cap < *n_out. */
int  lio_kf_store_get_keyframe(lio_kf_store *s, int32_t id, const float *pose,
                               void *out, size_t out_stride_bytes, size_t out_cap, size_t *n_out);

/* publishFrames MO:2330-2345: transformPointCloud of a cloud the handle still has staged, under the final pose.
 * LIO_STAGED_DS: the scan of batch slot 0 (laserCloudSurfLastDS -> cloud_registered); LIO_STAGED_RAW: the whole cloud of the
 * last lio_s2m_register_raw (cloud_deskewed -> cloud_registered_raw).  Ordered behind the stream that wrote the staged cloud.
 * LIO_ERR_ARG when nothing of that kind is staged, for a multi-device handle, a non-finite pose and out_cap < *n_out. */
enum { LIO_STAGED_DS = 0, LIO_STAGED_RAW = 1 };
int  lio_s2m_registered_cloud(lio_s2m_handle *h, int32_t which, const float pose[6],
                              void *out, size_t out_stride_bytes, size_t out_cap, size_t *n_out);

/* ------------------------------------------------ occupancy grid for a planner (the fork's draft ogmGeneration.cpp, OG) */
/* src/liorf/src/ogmGeneration.tar.xz holds the draft of the node that turns the saved map into a nav_msgs/OccupancyGrid:
 * pcl::PassThrough on z (OG:74-93), pcl::RadiusOutlierRemoval (OG:96-112), SetMapTopicMsg (OG:115-188).  The draft does not
 * compile as archived; its three stages and their parameters are reproduced on the device.  DESIGN.md section 4h states the
 * conventions (parity unpinned: PCL and FLANN are restated, not linked). */
/* pcl::RadiusOutlierRemoval: a point stays iff k_i > min_neighbors, k_i = the points j of the cloud, the point itself and
 * its duplicates included, with d2 < r2; d2 = ((dx dx) + dy dy) + dz dz in fp32 without contraction (FLANN L2_Simple),
 * r2 = (float)((double)radius * radius), the comparison strict (the radius search's, as lio_kf_store_global_map's).  Records
 * as for lio_sor_filter: x,y,z @0,4,8, intensity @16 when stride >= 20 (else 0); out records are PointXYZI (out_stride >=
 * 20); `out` (may be NULL: count only) holds n records.  Input order and intensity are kept.  Points with a non-finite
 * coordinate (or one beyond 1e15 m, which the search grid leaves out) are dropped and are nobody's neighbour.  A cloud of at
 * most min_neighbors such points loses all of them: there is no pass-through here.  n_neighbors (may be NULL): n ints, the
 * exact k_i per input point, -1 for a dropped one; with NULL a lane may stop counting once k_i > min_neighbors -- the kept
 * set is the same.  radius not finite or <= 0, min_neighbors < 0 -> LIO_ERR_ARG, nothing is clamped. */
int  lio_radius_filter(int32_t device_id, const void *pts, size_t n, size_t stride_bytes, float radius, int32_t min_neighbors,
                       void *out, size_t out_stride_bytes, size_t *n_out, int32_t *n_neighbors);

typedef struct lio_ogm_config {
    float   z_min, z_max;      /* thre_z_min, thre_z_max     OG:205-206  0.2, 2.0                                    */
    int32_t z_negative;        /* flag_pass_through          OG:207      0; 1 keeps the outside of [z_min, z_max]   */
    int32_t remove_outliers;   /* 1: OG:227 runs the filter unconditionally; 0 = the commented-out call of OG:230   */
    float   radius;            /* thre_radius                OG:208      0.5                                         */
    int32_t min_neighbors;     /* thres_point_count          OG:210      10                                          */
    double  resolution;        /* map_resolution             OG:209      0.05                                        */
    int32_t whole_box;         /* 0: as written; 1: labelled extension -- the box over every point, the last row filled */
} lio_ogm_config;
typedef struct lio_ogm_info {
    int32_t width, height;     /* cells along x and y (nav_msgs/MapMetaData)                                          */
    double  origin[2];         /* x_min, y_min                                                                        */
    int32_t n_in, n_slice, n_inliers, n_binned, n_occupied, pad;   /* points given, after the slice, after the filter,
                                                                    * points that marked a cell, cells of value 100   */
} lio_ogm_info;
void lio_ogm_default_config(lio_ogm_config *cfg);
/* The draft's chain on a host cloud (records as above; intensity is not read).  Stage by stage:
 *  - slice: pcl::PassThrough<PointXYZ> on z: points with a non-finite coordinate go first, then z_min <= z <= z_max stays
 *    (both limits inclusive; z_negative = 1 keeps the others instead);
 *  - filter: lio_radius_filter on what the slice left, when remove_outliers;
 *  - raster as written (whole_box = 0): the box in fp64 over the points 0 .. n - 2 of the filtered cloud (the loop of OG:139
 *    stops one short; a one-point cloud has that point as its box); width = (int)((x_max - x_min) / resolution), height
 *    likewise; i = (int)(((double)x - x_min) / resolution), j likewise, toward zero; a point is skipped iff i < 0 ||
 *    i >= width || j < 0 || j >= height - 1 (OG:181: the last row is never filled); grid[i + j * width] = 100, every other
 *    cell 0, row-major as the message is;
 *  - raster, whole_box = 1 (extension): the box over every point, and the test is j >= height.
 * `grid` (may be NULL: geometry and counts only) holds grid_cap cells.  More cells than grid_cap -> LIO_ERR_ARG with width,
 * height and origin filled in; more than 2^31 - 1 cells -> LIO_ERR_CAPACITY.  width or height 0, or an empty cloud at any
 * stage: LIO_OK, the dimensions reported, nothing written.  LIO_ERR_ARG before any device is touched, never a clamp:
 * resolution < 1e-4 or not finite, limits not finite or z_min > z_max, flags other than 0 / 1, and lio_radius_filter's
 * refusals when remove_outliers.  info may be NULL.  Replaces the main() of the draft up to the message. */
int  lio_occupancy_grid(int32_t device_id, const void *pts, size_t n, size_t stride_bytes, const lio_ogm_config *cfg,
                        int8_t *grid, size_t grid_cap, lio_ogm_info *info);
/* The same chain on the cloud the draft would load from GlobalMap.pcd, where lio_kf_store_export_map leaves it on the
 * device: map_resolution (save_map.srv `resolution`) 0 = every keyframe under its stored pose, summed; any other value =
 * that cloud through lio_voxel_grid at map_resolution.  *n_map (may be NULL) = its points.  Only the grid and the info cross
 * to the host.  The rules stated above lio_global_map_config hold: the store and the handles are left as found, the result
 * is complete on return, calls on one store remain non-re-entrant.  An empty store: LIO_OK, width = height = 0.  A keyframe
 * without a pose, a negative or non-finite map_resolution: LIO_ERR_ARG. */
int  lio_kf_store_occupancy_grid(lio_kf_store *s, float map_resolution, const lio_ogm_config *cfg,
                                 int8_t *grid, size_t grid_cap, size_t *n_map, lio_ogm_info *info);
/* Measurement hook (tools/ogm_cost.py): enable != 0 makes the calling thread's following chains record their stage
 * boundaries as HIP events; ms (may be NULL) receives the last such chain's slice, grid build, search, compaction, raster and
 * grid copy, in milliseconds. */
int  lio_ogm_debug_stage_ms(int32_t enable, float ms[6]);

/* ------------------------------------------------ signed distance field (grid_map_sdf behind the height map) */
/* src/grid_map/grid_map_sdf: the query a planner makes of the terrain -- how far a body point is from it and in which
 * direction it lies.  SignedDistanceField (the 3-D field over the `elevation` layer with its three derivatives),
 * SignedDistance2d (the planar field of an occupancy grid), Gridmap3dLookup (nearest node, first-order extrapolation).
 * DESIGN.md section 4i states the conventions.  The arithmetic is the reference's fp32 text, serial sweep included; its own
 * tests hold it to an N^2 definition within 1e-4 (distance from a cell centre to the border of the nearest cell column of
 * the other class, the height difference as third component), and so do this repository's. */
typedef struct lio_sdf lio_sdf;
typedef struct lio_sdf_config {
    double  min_height, max_height;  /* the field's band; NaN = the finite cells' minimum / maximum; max < min: LIO_ERR_ARG  */
    int32_t nan_policy;              /* 0: a layer with a non-finite cell is refused (LIO_ERR_ARG, info.n_nan filled in; the
                                      * reference warns that its result is invalid); 1: labelled extension -- such a cell
                                      * reads as the smallest finite elevation                                                */
    int32_t pad;
} lio_sdf_config;
typedef struct lio_sdf_info {
    int32_t rows, cols, layers;      /* the 3-D grid: size(0) along x, size(1) along y, numZLayers = max(ceil(band / res), 2) */
    int32_t n_nan;                   /* non-finite cells of the elevation layer                                              */
    double  origin[3], resolution;   /* the centre of cell (0, 0) and the band's lower end: node (0, 0, 0)                    */
    float   layer_min, layer_max;    /* minCoeff / maxCoeff of the layer (finite cells): they pick each layer's branch        */
    int32_t n_all_obstacle, n_all_free, n_mixed;   /* layers below the minimum, above the maximum, between                   */
    int32_t pad;
} lio_sdf_info;
#define LIO_SDF_NODE_LIMIT (1 << 25)   /* rows x cols x layers above it: LIO_ERR_CAPACITY (16 bytes a node)                  */
void lio_sdf_default_config(lio_sdf_config *cfg);           /* NaN, NaN, 0 */
/* The object owns the resident field (rows x cols x layers nodes of 16 bytes, plus 4 bytes a node of distances) and the
 * workspace of the build, both reused between builds and grown, never shrunk.  The workspace of a build is 24 bytes x rows x
 * cols x slab (8 of intermediate distances, 16 of the lines' lower bounds), slab = the layers swept at once: at most 32, fewer
 * until that product fits 128 MiB, at least 1 -- so at most max(128 MiB, 24 bytes x rows x cols), for any aspect of the grid. */
int  lio_sdf_create(int32_t device_id, lio_sdf **out);
void lio_sdf_destroy(lio_sdf *sdf);
/* SignedDistanceField's constructor on a host grid, column-major rows x cols floats (grid_map::Matrix); `length` and
 * `position` are lio_height_map_info's.  Layer z lies at float(min_height) + z * resolution (formed in float as the reference
 * forms it); per layer the two Euclidean distance transforms of SignedDistance2d.cpp in pixel units, combined to
 * resolution * (to_obstacle - to_free), or one of them alone where the layer lies wholly below or above the terrain; then the
 * central differences (one-sided at the six faces) along x, y with -resolution and along z with +resolution.  The previous
 * field of the object is replaced; after a failure the object holds none.  LIO_ERR_ARG before any device is touched, never a
 * clamp: rows or cols < 2 (the reference asserts), non-finite length or position, resolution < 1e-4 or not finite,
 * length[a] != size[a] * resolution, max_height < min_height, a nan_policy other than 0 / 1, rows or cols >= 2^24.
 * LIO_ERR_ARG after the layer was read: a non-finite cell under nan_policy 0, no finite cell at all.  More than
 * LIO_SDF_NODE_LIMIT nodes: LIO_ERR_CAPACITY with info filled in (before any device is touched where 2 layers already exceed it).  info may be NULL.  Complete on return. */
int  lio_sdf_build(lio_sdf *sdf, const float *elevation, int32_t rows, int32_t cols, double resolution,
                   const double length[2], const double position[2], const lio_sdf_config *cfg, lio_sdf_info *info);
/* lio_kf_store_height_map's chain (same arguments, same grid bytes; `grid` may be NULL), then the build above on the device
 * grid it leaves: nothing else crosses to the host.  hm->resolution is the field's.  An empty store or an empty local map:
 * LIO_OK, rows = cols = 0, the object holds no field.  A store and an sdf on different devices: LIO_ERR_ARG.  The rules stated
 * above lio_global_map_config hold: the store is left as found, the result is complete on return, calls on one store and on
 * one sdf remain non-re-entrant.  What a planning node calls after cloudMapInfoHandler. */
int  lio_kf_store_sdf(lio_kf_store *s, const lio_local_map_config *lm, const float pose[6],
                      const lio_height_map_config *hm, const lio_sdf_config *cfg, float *grid, size_t grid_cap,
                      lio_sdf *sdf, lio_local_map_info *lm_info, lio_height_map_info *hm_info, lio_sdf_info *info);
/* The field in the reference's data_ order: {distance, dx, dy, dz} as four floats at ((z * cols + col) * rows + row) * 4.
 * cap_floats < 4 x rows x cols x layers, or no field: LIO_ERR_ARG. */
int  lio_sdf_nodes(lio_sdf *sdf, float *nodes, size_t cap_floats);
/* valueAndDerivative for n positions (x, y, z as doubles): the nearest node by std::round, clamped to the grid on all six
 * sides in double, value = distance + derivative . (position - node position) in double, summed x, y, z.  `derivative` (n x 3,
 * may be NULL) receives the node's.  n = 0: LIO_OK.  No field: LIO_ERR_ARG. */
int  lio_sdf_query(lio_sdf *sdf, const double *positions, size_t n, double *value, double *derivative);
/* signedDistanceFromOccupancy on a nav_msgs/OccupancyGrid.data as lio_occupancy_grid writes it: the row-major message is
 * read as the column-major width x height matrix, a cell is an obstacle iff its value >= occupied_min (100 is what the draft
 * writes besides 0).  out: width x height floats in the grid's layout, resolution * (pixels to the nearest obstacle - pixels
 * to the nearest free cell); +INF everywhere without an obstacle, -INF everywhere without free space.  The same sweeps as the
 * field's, with the offsets 0 / INF and one layer.  LIO_ERR_ARG: width or height < 1 or >= 2^24, more than 2^31 - 1 cells,
 * resolution < 1e-4 or not finite. */
int  lio_occupancy_sdf(int32_t device_id, const int8_t *grid, int32_t width, int32_t height, float resolution,
                       int32_t occupied_min, float *out);
/* The device memory the object holds now, in bytes: the field (nodes and distances) and the build's workspace.  Either may be NULL. */
int  lio_sdf_memory(lio_sdf *sdf, size_t *field_bytes, size_t *workspace_bytes);
/* Measurement hook (tools/sdf_cost.py): enable != 0 makes the calling thread's following builds record their stage
 * boundaries as HIP events; ms (may be NULL) receives the last such build's layer statistics with their host wait, column
 * sweeps, row sweeps and node stencil, in milliseconds (a build's allocations fall between the first and the second). */
int  lio_sdf_debug_stage_ms(int32_t enable, float ms[4]);

/* ------------------------------------------------ median fill (grid_map_filters' MedianFillFilter behind the height map) */
/* grid_map_filters/src/MedianFillFilter.cpp (plugin gridMapFilters/MedianFillFilter): the inpainting filter of the reference
 * tree that can be restated exactly -- a validity mask, 3 x 3 morphology on it, and the median of the finite values in a square
 * window for every hole the mask marks.  Every operation is a selection or a comparison, so the result equals the
 * restatement (tests/median_fill_restate.py) bit for bit; parity is against that restatement, OpenCV and grid_map are not
 * linked, and the reference's own test case (median_fill_filter_test.cpp) pins one input.  It is what SignedDistanceField.cpp:
 * 46-51 asks for ("Apply inpainting first") and what may stand for the terrain chain's `elevation_inpainted`.  DESIGN.md
 * section 4j states the conventions.  The defaults are the constructor's (:24-25). */
typedef struct lio_median_fill_config {
    double  fill_hole_radius;               /* the window of a hole, metres                                   0.05 */
    double  existing_value_radius;          /* the window of a finite cell when filter_existing_values        0.0  */
    int32_t filter_existing_values;         /* 1: masked finite cells become their window's median            0    */
    int32_t num_erode_dilation_iterations;  /* N of fillHoles, 0 .. 15                                        4    */
} lio_median_fill_config;
typedef struct lio_median_fill_info {
    int32_t rows, cols;
    int32_t fill_radius_cells, existing_radius_cells;   /* static_cast<size_t>(radius / resolution): truncated, 0.6 / 0.2 = 2 */
    int32_t n_nan_in;                       /* non-finite cells of the input (+-inf is a hole like NaN)                 */
    int32_t n_mask;                         /* non-zero cells of the fill mask                                         */
    int32_t n_filled;                       /* non-finite in, finite out                                               */
    int32_t n_filtered;                     /* finite cells that went through the median (filter_existing_values)      */
    int32_t n_nan_out;                      /* non-finite cells of the output                                          */
    int32_t pad;
} lio_median_fill_info;
void lio_median_fill_default_config(lio_median_fill_config *cfg);
/* update() on a host grid of rows x cols floats, column-major (grid_map::Matrix).  Stage by stage, as written there:
 *  - validity: std::isfinite;
 *  - cleaned mask (:212-224): dilate(erode(valid)) with the 3 x 3 rectangle -- the first dilate / erode pair is overwritten
 *    by the third call, one opening survives;
 *  - fill mask (:226-239): max(N, 1) dilations, then N erosions (one dilation is unconditional: N = 0 dilates once and never
 *    erodes).  Cells outside the grid take no part in any minimum or maximum (OpenCV's default border);
 *  - per cell (:132-145): input not finite and mask != 0 -> the median over [r - R, r + R] x [c - R, c + R] clamped into the
 *    grid, R = fill_radius_cells; else filter_existing_values and mask != 0 -> the median with existing_radius_cells; else
 *    the input's bits (NaN payloads and infinities pass through);
 *  - the median (:153-186): the element at sorted position n / 2 of the n finite values (the upper median for even n), the
 *    quiet NaN 0x7fc00000 for n = 0; -0 sorts below +0 (a convention: std::nth_element leaves it open).
 * mask_in (may be NULL): the fill mask of a previous run, rows x cols floats, used as it is (non-zero = fill); none is
 * computed and cleaned_mask is left alone.  filled: the output layer.  fill_mask, cleaned_mask (each may be NULL): the masks
 * as 0.0f / 1.0f; cleaned_mask is the filter's debug layer.  rows or cols 0: LIO_OK, nothing written.  LIO_ERR_ARG before any
 * device is touched, never a clamp: negative or non-finite radii, resolution < 1e-4 or not finite, a flag other than 0 / 1,
 * N < 0 or N > 15 (the mask kernel's halo 2 + max(N, 1) + N is at most 32 cells), a radius above 32 cells, null arguments.
 * More than 2^31 - 1024 cells: LIO_ERR_CAPACITY. */
int  lio_median_fill(int32_t device_id, const float *elevation, int32_t rows, int32_t cols, double resolution,
                     const lio_median_fill_config *cfg, const float *mask_in, float *filled, float *fill_mask,
                     float *cleaned_mask, lio_median_fill_info *info);

/* The host buffers of lio_kf_store_planning_map, each with its capacity in floats and each skipped when NULL. */
typedef struct lio_planning_map_buffers {
    float *grid;      size_t grid_cap;       /* the raw elevation grid: lio_kf_store_height_map's bytes   */
    float *filled;    size_t filled_cap;     /* the filled grid (fill given)                              */
    float *fill_mask; size_t fill_mask_cap;  /* its fill mask (fill given)                                */
    float *layers;    size_t layers_cap;     /* the terrain layers as lio_terrain_layers lays them out    */
} lio_planning_map_buffers;
/* One chain for a planning node: lio_kf_store_height_map's stages run once, then on the device grid they leave
 *  - fill != NULL: lio_median_fill (no mask_in);
 *  - terrain != NULL: lio_terrain_layers on the filled grid (on the raw grid without fill);
 *  - sdf != NULL (sdf_cfg then too): lio_sdf_build on the same grid; sdf_info->n_nan counts that grid.
 * Every info (each may be NULL) is filled as the stand-alone call fills it; the stages run in this order on the null stream
 * and all are complete on return, so a refusal of the field (holes left under nan_policy 0) still leaves the grids and the
 * layers written.  With fill, terrain and sdf all NULL the call is lio_kf_store_height_map.  An empty store or an empty local
 * map: LIO_OK, rows = cols = 0.  A store and an sdf on different devices: LIO_ERR_ARG.  A buffer smaller than rows x cols
 * (layers: times the requested layers): LIO_ERR_ARG with rows and cols filled in.  The configurations are refused as their
 * own calls refuse them, before any device is touched. */
int  lio_kf_store_planning_map(lio_kf_store *s, const lio_local_map_config *lm, const float pose[6],
                               const lio_height_map_config *hm, const lio_median_fill_config *fill,
                               const lio_terrain_config *terrain, lio_sdf *sdf, const lio_sdf_config *sdf_cfg,
                               const lio_planning_map_buffers *out, lio_local_map_info *lm_info,
                               lio_height_map_info *hm_info, lio_median_fill_info *fill_info,
                               lio_terrain_info *terrain_info, lio_sdf_info *sdf_info);

/* ------------------------------------------------ resident planning layers, sampled on the device (GridMap::atPosition) */
/* grid_map_core's GridMap::atPosition with its four InterpolationMethods (GridMap.cpp:161-210, :777-846,
 * CubicInterpolation.cpp): what a planner asks of the elevation grid and the terrain layers, once per trajectory point and
 * footprint corner.  The layers stay on the device in a lio_grid; only positions go up and values come down.  DESIGN.md
 * section 4k states the conventions.  Every operation is fp64 in the reference's order on taps widened from float; parity is
 * against the restatement (tests/grid_sample_restate.py), with the reference's own test values on top (parity unpinned:
 * Eigen and grid_map are restated, not linked). */
typedef struct lio_grid lio_grid;
#define LIO_GRID_MAX_LAYERS 16
enum { LIO_GRID_NEAREST = 0, LIO_GRID_LINEAR = 1, LIO_GRID_CUBIC_CONVOLUTION = 2, LIO_GRID_CUBIC = 3,   /* InterpolationMethods, TypeDefs.hpp:39-44 */
       LIO_GRID_OUTSIDE = 255 };                                                                       /* method used: the position is not in the map */
/* the layers lio_kf_store_planning_grid leaves: the raw grid, the filled grid, then the terrain layers in their enum order */
enum { LIO_GRID_LAYER_ELEVATION = 0, LIO_GRID_LAYER_FILLED = 1, LIO_GRID_LAYER_TERRAIN = 2 };
typedef struct lio_grid_sample_config {
    int32_t method;               /* LIO_GRID_NEAREST .. LIO_GRID_CUBIC                                        0 */
    int32_t border_mode;          /* 0: tap indices wrap and fail as the reference's do; 1: labelled extension --
                                   * every tap index of the three interpolating methods clamped into the grid  0 */
} lio_grid_sample_config;
typedef struct lio_grid_sample_info {
    int64_t n_outside;            /* (layer, position) pairs answered LIO_GRID_OUTSIDE: the positions outside x the layers */
    int64_t n_method[4];          /* pairs per method used; with n_outside they sum to n_layers x n             */
} lio_grid_sample_info;
typedef struct lio_grid_desc {
    int32_t  rows, cols;          /* 0, 0: the object holds no layer                                            */
    double   resolution, length[2], position[2];
    uint32_t layer_mask;          /* bit k set: layer k is present                                              */
    int32_t  pad;
} lio_grid_desc;                 /* what lio_grid_info reports */
void lio_grid_sample_default_config(lio_grid_sample_config *cfg);   /* nearest, 0 */
/* The object owns up to LIO_GRID_MAX_LAYERS column-major rows x cols float layers on one device, each kept between calls and
 * grown, never shrunk.  Calls on one object are non-re-entrant.  Destroying NULL does nothing. */
int  lio_grid_create(int32_t device_id, lio_grid **out);
void lio_grid_destroy(lio_grid *g);
/* Uploads n_layers host layers, laid out layer after layer, each rows x cols floats, column-major (grid_map::Matrix), as
 * layers 0 .. n_layers - 1; what the object held is replaced.  `length` and `position` are the grid map's.  LIO_ERR_ARG
 * before any device is touched, never a clamp: null arguments, n_layers outside 1 .. 16, rows or cols < 1 or >= 2^24,
 * non-finite length or position, resolution < 1e-4 or not finite, length[a] != size[a] * resolution.  More than 2^31 - 1024
 * cells a layer: LIO_ERR_CAPACITY.  Complete on return. */
int  lio_grid_set_layers(lio_grid *g, const float *layers, int32_t n_layers, int32_t rows, int32_t cols, double resolution,
                         const double length[2], const double position[2]);
/* Layer `layer` to the host.  An absent layer, or cap_floats < rows x cols: LIO_ERR_ARG. */
int  lio_grid_get_layer(lio_grid *g, int32_t layer, float *out, size_t cap_floats);
/* The geometry and the layers present.  Never touches a device. */
int  lio_grid_info(lio_grid *g, lio_grid_desc *info);
/* The device memory the object holds now, in bytes. */
int  lio_grid_memory(lio_grid *g, size_t *bytes);
/* atPosition for n positions (x, y as doubles, pair after pair) on the n_layers layers named by layer_ids, in that order:
 * values[k * n + q] is layer layer_ids[k] at position q, method_used (may be NULL) the same for the method that produced it,
 * 0 .. 3 in the reference's enum order, or LIO_GRID_OUTSIDE.  The position's cell, the taps and the normalised coordinates
 * are formed once per position; the taps are gathered and the fall-back chain of GridMap.cpp:161-204 runs per layer:
 *  - outside: the position fails checkIfPositionWithinMap (GridMapMath.cpp:162-172: above the high edge or at or below the
 *    low edge of either axis; non-finite), or its index does.  Nothing is read, the value is the quiet NaN 0x7fc00000.  A
 *    labelled deviation: the reference throws there (its linear step can "succeed" on wrapped cells by accident);
 *  - nearest: the cell's bits, NaN payloads and infinities included;
 *  - linear (GridMap.cpp:777-846): the four taps around the position, each tested through its column-major linear index
 *    alone, so a row index of `rows` reads row 0 of the next column and -1 the last row of the column before -- for positions
 *    inside the map, reproduced as written; a tap whose linear index is negative or >= rows x cols fails and the query falls
 *    back to nearest (the reference lets rows x cols itself pass and reads one float past the buffer: labelled deviation).
 *    No finiteness test: a non-finite tap gives NaN with method used = linear;
 *  - cubic convolution (CubicInterpolation.cpp:44-135) and bicubic (:150-432): 16 taps, resp. 4 corners with their central
 *    differences; indices are bound as unsigned, so an index below 0 goes to the last row or column, as written; a result
 *    that is not finite falls back to linear, and linear to nearest;
 *  - border_mode 1: every tap index of the three interpolating methods is formed in int and clamped into the grid; no wrap,
 *    no linear-index test, nothing else changed.
 * info (may be NULL): the counts of the call.  n = 0: LIO_OK.  LIO_ERR_ARG: null arguments, an object without layers,
 * n_layers < 1 or > 16, an absent or repeated layer id, a method outside 0 .. 3, a border mode outside 0 / 1.  More than
 * 2^27 positions: LIO_ERR_CAPACITY.  Complete on return, one host wait per call. */
int  lio_grid_sample(lio_grid *g, const int32_t *layer_ids, int32_t n_layers, const lio_grid_sample_config *cfg,
                     const double *positions, size_t n, float *values, uint8_t *method_used, lio_grid_sample_info *info);
/* lio_kf_store_planning_map (same arguments, same bytes in every buffer and info), which also leaves its grids in grid_out
 * by device-to-device copy: layer 0 the raw elevation grid, layer 1 the filled grid (with fill), layers 2 .. 9 the eight
 * terrain layers in enum order (with terrain; all eight, whatever terrain->layers copies to the host).  The geometry is
 * hm_info's.  grid_out == NULL: lio_kf_store_planning_map.  An empty store or an empty map leaves the object without
 * layers, and so does a failure of the fill, of the terrain layers or of a copy into the object; a refusal of the field
 * leaves them in place.  A store and a grid on different devices: LIO_ERR_ARG. */
int  lio_kf_store_planning_grid(lio_kf_store *s, const lio_local_map_config *lm, const float pose[6],
                                const lio_height_map_config *hm, const lio_median_fill_config *fill,
                                const lio_terrain_config *terrain, lio_sdf *sdf, const lio_sdf_config *sdf_cfg,
                                const lio_planning_map_buffers *out, lio_local_map_info *lm_info,
                                lio_height_map_info *hm_info, lio_median_fill_info *fill_info,
                                lio_terrain_info *terrain_info, lio_sdf_info *sdf_info, lio_grid *grid_out);
/* Measurement hook (tools/grid_sample_cost.py): enable != 0 makes the calling thread's following sampling calls record their
 * stage boundaries as HIP events; ms (may be NULL) receives the last such call's positions up, kernel and values down, in
 * milliseconds. */
int  lio_grid_debug_stage_ms(int32_t enable, float ms[3]);

/* ------------------------------------------------ resident planning layers, reduced over regions (grid_map's iterators) */
/* grid_map_core's LineIterator, CircleIterator, EllipseIterator and PolygonIterator (src/iterators/) on a lio_grid: the cells
 * a region covers, and per requested layer the reduction a planner would loop for (is this footprint free of cells below a
 * traversability threshold, the worst slope under a swath).  Only regions go up and one record per (layer, region) comes
 * down.  DESIGN.md section 4l states the conventions; parity is against the restatement (tests/grid_region_restate.py) with
 * the reference's own test sequences on top (parity unpinned).
 *  - circle   p = (cx, cy, r): window by findSubmapParameters, member when dx dx + dy dy <= r r on the cell's centre;
 *  - ellipse  p = (cx, cy, lx, ly, rotation): the lengths are full axes (EllipseIterator.cpp:17-28, :74-97); sin and cos of
 *             the rotation are taken on the host (libm);
 *  - polygon  n_vertices (x, y) pairs from first_vertex of `vertices`: window from the vertex extremes, member by
 *             Polygon::isInside (even-odd);
 *  - line     p = (x0, y0, x1, y1): both ends limited to the map by getIndexLimitedToMapRange, Bresenham between them.
 * Cells come in the iterator's order: SubmapIterator's (row index outer, column index inner) for the three area kinds, start
 * to end for the line.  The status is per region and never fails the call: OK; EMPTY (no cell: a line whose constructor
 * throws, an area that misses every centre); INVALID (nothing is read, 0 cells: a non-finite parameter or vertex, r < 0, an
 * ellipse length not > 0, a line end whose walk exceeds LIO_REGION_MAX_WALK steps -- a labelled deviation, the reference
 * keeps walking). */
enum { LIO_REGION_LINE = 0, LIO_REGION_CIRCLE = 1, LIO_REGION_ELLIPSE = 2, LIO_REGION_POLYGON = 3 };
enum { LIO_REGION_OK = 0, LIO_REGION_EMPTY = 1, LIO_REGION_INVALID = 2 };
#define LIO_REGION_MAX_VERTICES 64
#define LIO_REGION_MAX_WALK 4096
typedef struct lio_grid_region {
    int32_t kind, n_vertices;     /* LIO_REGION_*; n_vertices and first_vertex: polygons only                   */
    int64_t first_vertex;
    double  p[5];                 /* the kind's parameters, the rest ignored                                    */
} lio_grid_region;
typedef struct lio_grid_region_config {
    float   threshold;            /* n_below counts finite member cells with value < threshold (float)      0.5 */
    int32_t pad;
} lio_grid_region_config;
typedef struct lio_grid_region_stat {
    double  sum;                  /* fp64 over the finite member cells, in the fixed order below                */
    float   min, max;             /* over the finite member cells, -0.0 < +0.0; none: the quiet NaN 0x7fc00000  */
    int32_t n_finite, n_below;
} lio_grid_region_stat;
typedef struct lio_grid_region_info {
    int64_t n_ok, n_empty, n_invalid, n_cells;     /* regions per status; cells over all regions                */
} lio_grid_region_info;
void lio_grid_region_default_config(lio_grid_region_config *cfg);   /* threshold 0.5 */
/* stats[k * n + q]: layer layer_ids[k] over region q.  n_cells[q] (may be NULL): the region's cells, status[q] (may be NULL)
 * its status, info (may be NULL) the counts of the call.  The sum's order is part of the interface: number the window's
 * cells column-major (row fastest; a line's cells by their place on it); partial p of 64 adds the finite member cells of
 * number = p (mod 64), ascending, from +0.0; then for s = 32, 16, .. 1: part[k] += part[k + s], k < s; sum = part[0].
 * n = 0: LIO_OK.  LIO_ERR_ARG before any device is touched: null arguments, a non-finite threshold, n_layers outside 1 .. 16,
 * a layer id outside 0 .. 15, repeated or absent, a kind outside the enum, a polygon with fewer than 3 or more than
 * LIO_REGION_MAX_VERTICES vertices or whose vertices leave [0, n_vertices), an object without layers.  More than 2^24
 * regions: LIO_ERR_CAPACITY.  Complete on return, one host wait per call; the layers are only read. */
int  lio_grid_region_reduce(lio_grid *g, const int32_t *layer_ids, int32_t n_layers, const lio_grid_region_config *cfg,
                            const lio_grid_region *regions, size_t n, const double *vertices, size_t n_vertices,
                            lio_grid_region_stat *stats, int32_t *n_cells, uint8_t *status, lio_grid_region_info *info);
/* The cells themselves: cells[offsets[q] .. offsets[q + 1]) are region q's, as column-major linear indices col * rows + row,
 * in the iterator's order; offsets has n + 1 entries.  Reads no layer.  status and info may be NULL.  cap_cells smaller than
 * offsets[n]: LIO_ERR_CAPACITY with offsets filled (offsets[n] tells the need) and cells untouched; so are more than
 * 2^31 - 1 cells in one call.  The other refusals are lio_grid_region_reduce's.  Complete on return; two host waits: the
 * sizes, then exactly offsets[n] cells. */
int  lio_grid_region_cells(lio_grid *g, const lio_grid_region *regions, size_t n, const double *vertices, size_t n_vertices,
                           int64_t *offsets, int32_t *cells, size_t cap_cells, uint8_t *status, lio_grid_region_info *info);
/* Measurement hook (tools/grid_region_cost.py), as lio_grid_debug_stage_ms: the last lio_grid_region_reduce of the calling
 * thread as regions up, plan kernel, reduce kernel and results down, in milliseconds. */
int  lio_grid_region_debug_stage_ms(int32_t enable, float ms[4]);

/* ------------------------------------------------ resident planning layers into another frame, and out as an occupancy grid */
/* grid_map's GridMap::getTransformedMap (GridMap.cpp:332-436) from one lio_grid into another on the same device, and
 * GridMapRosConverter::toOccupancyGrid (GridMapRosConverter.cpp:329-365) on one resident layer: the planning grid moved into a
 * yaw-aligned vehicle frame and a layer handed to a nav_msgs/OccupancyGrid consumer without the layers crossing PCIe.
 * DESIGN.md section 4m states the conventions; parity is against the restatement (tests/grid_transform_restate.py) with the
 * reference's own test values on top (parity unpinned).
 *  - new geometry   on the host in fp64: the corners position +- 0.5 length at z = 0 in the order (+, +), (+, -), (-, +),
 *                   (-, -), each transformed, summed from zero in that order and multiplied by 0.25 (the centre); the largest
 *                   fabs(corner - centre) per axis by fmax, doubled; setGeometry: size = (int)round(length / resolution),
 *                   length = size * resolution, position = the centre;
 *  - transform * p  ((R_i0 x + R_i1 y) + R_i2 z) + t_i per component, fp64, no contraction;
 *  - visit order    source cells by column-major linear index ascending; a cell whose height is not finite is skipped; with
 *                   sample_ratio > 0 five samples, the centre then x - l, x + l, y - l, y + l with l = resolution *
 *                   sample_ratio, otherwise the centre alone; a sample whose getIndex on the new map fails is dropped;
 *  - the rule       a sample is skipped when the new cell's height is not NaN and, widened to double, greater than the
 *                   sample's fp64 z; otherwise the new cell's height becomes (float)z and every other layer takes the source
 *                   cell's bits, NaN included.  Cells nothing reaches are the quiet NaN 0x7fc00000 in every layer.
 * The result is the serial loop's bit for bit, on every run (integer atomics only).  The structs are declared apart from their
 * typedefs; they are the same types. */
struct lio_grid_transform_info {
    int32_t rows, cols;           /* the new grid                                                               */
    double  length[2], position[2];
    int64_t n_source_cells;       /* cells with a finite height (getPosition3 succeeded)                        */
    int64_t n_samples_outside;    /* samples whose getIndex on the new map failed                               */
    int64_t n_cells_written;      /* new cells that received a value                                            */
};
typedef struct lio_grid_transform_info lio_grid_transform_info;
struct lio_grid_occupancy_desc {
    uint32_t width, height;       /* rows, cols (info.width = getSize()(0), info.height = getSize()(1))         */
    float    resolution;          /* the double narrowed to float, as the message field does                    */
    int32_t  pad;
    double   origin[2];           /* position - 0.5 length                                                      */
};
typedef struct lio_grid_occupancy_desc lio_grid_occupancy_desc;
/* 5 x source cells is the largest visit number + 1 and must fit 31 bits of the winner's key */
#define LIO_GRID_TRANSFORM_MAX_SOURCE_CELLS 429496729
/* Afterwards dst holds every layer src holds, under the same ids, in the new geometry; what dst held is replaced (after a
 * failure past the refusals it holds none); src is only read.  transform: the rows of [R | t].  info may be NULL.
 * LIO_ERR_ARG before any device is touched and with dst untouched: null src, dst or transform, src == dst, grids on
 * different devices, src without layers, height_layer absent, a non-finite transform entry or sample_ratio, a new size below
 * 1 on either axis (the reference asserts there), and a z row so large that a transformed height could overflow fp64 (a
 * labelled deviation: the reference would store NaN).  LIO_ERR_CAPACITY, dst untouched as well: a new axis >= 2^24, more than
 * 2^31 - 1024 new cells, more than LIO_GRID_TRANSFORM_MAX_SOURCE_CELLS source cells.  Complete on return, one host wait per
 * call (the counters). */
int  lio_grid_transform(lio_grid *src, const double transform[12], int32_t height_layer, double sample_ratio, lio_grid *dst,
                        lio_grid_transform_info *info);
/* Layer `layer` as the cells of a nav_msgs/OccupancyGrid; only the int8 cells come down.  In float, as written:
 * value = (v - data_min) / (data_max - data_min); NaN gives -1, otherwise 0 + min(max(0, value), 1) * 100, converted to int8_t
 * by truncation.  The cell of column-major linear index col * rows + row goes to data[n - 1 - index], n = rows x cols.
 * data_min == data_max is not refused: the division's infinities clamp and its NaN gives -1.  desc may be NULL.  LIO_ERR_ARG:
 * a null grid or data, an absent layer, cap_cells < rows x cols (data untouched), a non-finite data_min or data_max.
 * Complete on return, one host wait per call. */
int  lio_grid_to_occupancy(lio_grid *g, int32_t layer, float data_min, float data_max, int8_t *data, size_t cap_cells,
                           lio_grid_occupancy_desc *desc);
/* Measurement hook (tools/grid_transform_cost.py), as lio_grid_debug_stage_ms: the last lio_grid_transform of the calling
 * thread as keys cleared, scatter kernel, gather kernel with the counters down, in milliseconds. */
int  lio_grid_transform_debug_stage_ms(int32_t enable, float ms[3]);

/* ------------------------------------------------ resident planning layers cropped, moved, extended and merged on the device */
/* grid_map's GridMap::getSubmap (GridMap.cpp:282-330), move (:442-507), extendToInclude (:554-627) and addDataFrom (:514-552)
 * on lio_grid objects of one device: a persistent map that grows as the vehicle drives, a window of it, a map that follows the
 * vehicle, without a layer crossing PCIe.  DESIGN.md section 4n states the conventions; parity is against the restatement
 * (tests/grid_geom_restate.py) with the reference's own test values on top (parity unpinned).  A lio_grid keeps startIndex 0:
 * every result is the reference's after convertToDefaultStartIndex (:677-707).  All geometry is decided on the host in fp64,
 * in the order the source writes it:
 *  - submap   getSubmapInformation (GridMapMath.cpp:287-341): both corners position +- 0.5 length through
 *             boundPositionToRange and getIndexFromPosition, size = bottom right - top left + 1, length = size * resolution,
 *             position = the top-left cell's centre + 0.5 resolution - 0.5 length, and getIndexFromPosition of the requested
 *             position in the submap, whose failure (a requested centre outside the map) fails the call;
 *  - move     getIndexShiftFromPositionShift (:183-196): per axis v = (position - map position) / resolution, index shift =
 *             -(int)(v + 0.5 * (v > 0 ? 1 : -1)); the map's position moves by (double)(-index shift) * resolution; new cell
 *             (r, c) takes old cell (r + shift0, c + shift1) where that exists, the quiet NaN 0x7fc00000 elsewhere;
 *  - extend   the four corner comparisons and their half differences, setGeometry (size = (int)round(length / resolution)),
 *             the alignment by fmod, the `< resolution / 2` branch and the parity correction by copysign; then every new cell
 *             takes its centre, isInside and getIndex on the old geometry, and the old cell's bits (the quiet NaN elsewhere);
 *  - add      after the extension (if asked for) and after the layers this map lacks were added as NaN: per cell, valid =
 *             every basic layer finite (no basic layer: never valid); a valid cell is skipped unless overwrite; the cell's
 *             centre, isInside and getIndex on `other`; each listed layer takes other's bits where they are finite.
 * Labelled deviations: where isInside holds and getIndex fails (a centre within an ulp of the low edge) the reference reads
 * past the buffer; such a cell is skipped and counted in n_index_outside.  A bounded submap corner whose index still falls
 * outside is brought back to the last cell, where the reference fails.  |v| >= 2^30 or a non-finite v in move is LIO_ERR_ARG
 * (the reference's cast is undefined).  Layers are matched by id, as the reference matches them by name.  Every result is the
 * serial loop's bit for bit (no cell reads another cell of the map it writes).  The structs are declared apart from their
 * typedefs; they are the same types. */
struct lio_grid_submap_info {
    int32_t success;              /* getSubmap's isSuccess; 0: dst holds no layers                              */
    int32_t rows, cols, pad;
    double  length[2], position[2];
    int32_t top_left[2];          /* the submap's first cell in src                                             */
    int32_t requested_index[2];   /* the requested position's cell in the submap                                */
};
typedef struct lio_grid_submap_info lio_grid_submap_info;
struct lio_grid_move_info {
    int32_t moved, pad;           /* move's return value: the index shift is not (0, 0)                         */
    int32_t index_shift[2];
    double  position[2];          /* the map's position afterwards (aligned to the cells)                       */
    int64_t n_cells_cleared;      /* cells per layer that became NaN                                            */
};
typedef struct lio_grid_move_info lio_grid_move_info;
struct lio_grid_extend_info {
    int32_t resized, rows, cols, pad;              /* the geometry afterwards                                   */
    double  length[2], position[2];
    int64_t n_cells_kept;         /* new cells that took an old cell                                            */
    int64_t n_index_outside;      /* isInside held, getIndex failed: skipped (the labelled deviation)           */
};
typedef struct lio_grid_extend_info lio_grid_extend_info;
struct lio_grid_add_info {
    int32_t resized, rows, cols, pad;              /* the geometry afterwards                                   */
    double  length[2], position[2];
    int64_t n_cells_skipped_valid;                 /* valid and not overwrite                                   */
    int64_t n_cells_outside_other;                 /* the centre is not inside `other`                          */
    int64_t n_index_outside;      /* as above, on the old map (the extension) or on `other`                     */
    int64_t n_values_copied;      /* finite values taken from `other`, over all layers                          */
};
typedef struct lio_grid_add_info lio_grid_add_info;
/* Refusals common to the four: LIO_ERR_ARG before any device is touched and with every object untouched for a null argument,
 * src == dst or g == other, grids on different devices, a source (src, other, or the g that is moved, extended or added to)
 * without layers, a non-finite position or length, a negative length, a flag outside 0 / 1.  LIO_ERR_CAPACITY, untouched as
 * well: a new axis >= 2^24, more than 2^31 - 1024 new cells.  Every call is complete on return with one host wait (the
 * counters); info may be NULL; src and other are only read.
 *
 * getSubmap: dst then holds every layer src holds, under the same ids, cropped; what it held is replaced.  A requested centre
 * outside the map is not an error: LIO_OK, info->success = 0, dst without layers. */
int  lio_grid_submap(lio_grid *src, const double position[2], const double length[2], lio_grid *dst, lio_grid_submap_info *info);
/* move, in place: every layer of g is shifted through a second buffer from the library's pool, which then takes the layer's
 * place (the old one goes back to the pool).  An index shift of (0, 0) launches nothing; the position still takes the aligned
 * shift, as written. */
int  lio_grid_move(lio_grid *g, const double position[2], lio_grid_move_info *info);
/* extendToInclude.  Nothing to extend: LIO_OK, info->resized = 0, nothing touched.  `other` may have any resolution: the
 * reference reads its corners only, and the new map keeps g's resolution and is aligned with g's cells.  (With differing
 * resolutions there is nothing else to align: none is refused for it; a g without layers has no geometry to extend and is.) */
int  lio_grid_extend_to_include(lio_grid *g, lio_grid *other, lio_grid_extend_info *info);
/* addDataFrom(other, extend, overwrite, copyAllLayers, layers).  n_layers = 0: every layer `other` holds.  An id g lacks is
 * added, NaN-filled.  basic_mask (bit k: layer k) stands for basicLayers_ and may be 0.  With extend and a resize, extension
 * and addition are one launch; otherwise the addition works in place.  Further LIO_ERR_ARG: n_layers outside 0 .. 16, an id
 * outside 0 .. 15, repeated or absent from `other`, a basic_mask bit for a layer g does not hold. */
int  lio_grid_add_data_from(lio_grid *g, lio_grid *other, int32_t extend, int32_t overwrite, const int32_t *layer_ids,
                            int32_t n_layers, uint32_t basic_mask, lio_grid_add_info *info);
/* Measurement hook (tools/grid_geom_cost.py), as lio_grid_debug_stage_ms: the kernel of the calling thread's last call of the
 * four, in milliseconds (0 where none was launched). */
int  lio_grid_geom_debug_kernel_ms(int32_t enable, float *ms);

/* ------------------------------------------------ resident planning layers out as images, clouds and grid cells, and in again */
/* grid_map_cv's GridMapCvConverter (toImage, addLayerFromImage, addColorLayerFromImage, initializeFromImage) and
 * GridMapRosConverter's toPointCloud (both), toGridCells and fromOccupancyGrid on resident objects: what a node publishes
 * comes down in the format it is published in, and a costmap or a mask that arrives as an image or an occupancy grid becomes a
 * layer beside the terrain layers.  DESIGN.md section 4o states the conventions and the labelled deviations; parity is
 * against the restatement (tests/grid_convert_restate.py) with the reference's own test values on top (parity unpinned).
 * Layers are column-major rows x cols with start index 0: GridMapIterator's linear order is the storage order.  Images are
 * row-major rows x cols x channels, tightly packed, image row = grid row, image column = grid column, little-endian elements.
 * Every call is complete on return on the null stream; info may be NULL; the four to_* calls only read their object.
 * LIO_ERR_ARG is returned before any device is touched wherever that is possible, never a clamp. */
#define LIO_IMAGE_8U  0
#define LIO_IMAGE_16U 1
#define LIO_IMAGE_32F 2
struct lio_grid_image_info {
    int32_t rows, cols;
    float   lower, upper;         /* the bounds used (the layer's finite extremes when both arguments were NaN)  */
    int64_t n_pixels;             /* pixels that received a value                                               */
    int64_t n_clamped_low;        /* cells below lower                                                          */
    int64_t n_clamped_high;       /* cells above upper                                                          */
    int64_t n_nonfinite;          /* cells whose clamped value is not finite: the pixel is zero in every channel */
};
typedef struct lio_grid_image_info lio_grid_image_info;
struct lio_grid_from_image_info {
    int32_t rows, cols;
    int32_t geometry_set, pad;    /* 1: the grid held no layers and took its geometry from the call             */
    int64_t n_cells_set;          /* cells that received a value                                                */
    int64_t n_cells_transparent;  /* cells whose alpha is below the threshold: NaN                              */
};
typedef struct lio_grid_from_image_info lio_grid_from_image_info;
struct lio_grid_from_occupancy_info {
    int32_t rows, cols;           /* width, height                                                              */
    int32_t geometry_replaced, pad;   /* 1: setGeometry ran, every other layer reads NaN at the new size        */
    double  length[2], position[2];
    int64_t n_unknown;            /* cells of -1: NaN                                                           */
};
typedef struct lio_grid_from_occupancy_info lio_grid_from_occupancy_info;
/* toImage<Type, NChannels> (GridMapCvConverter.hpp:173-247) of layer `layer`: channels 1, 3 or 4, depth LIO_IMAGE_*.  Per
 * cell in float, as written: v = x < lower ? lower : (x > upper ? upper : x) (a NaN stays NaN); a non-finite v leaves the
 * pixel zero in every channel, alpha included; otherwise (Type)(((v - lower) / (upper - lower)) * (float)max) by truncation,
 * max = 255, 65535 or 1.0f, repeated in three channels when there are at least 3, and max in the last of 4.  lower and upper
 * both NaN: the layer's minCoeffOfFinites / maxCoeffOfFinites (the same on every run).  image holds cap_bytes bytes; fewer
 * than rows x cols x channels x element size: LIO_ERR_ARG, image untouched.  Also LIO_ERR_ARG (the reference divides by zero
 * and casts NaN there): !(upper > lower), a non-finite upper - lower, one bound NaN alone, automatic bounds on a layer without
 * a finite cell or whose extremes are equal.  Two host waits with automatic bounds (the bounds decide the refusal), else one. */
int  lio_grid_to_image(lio_grid *g, int32_t layer, int32_t channels, int32_t depth, float lower, float upper, void *image,
                       size_t cap_bytes, lio_grid_image_info *info);
/* addLayerFromImage<Type, NChannels> (:58-119) into layer `layer`: replaced when present, the other layers untouched.  A
 * cell whose alpha (the last of 4 channels) is below (Type)(alpha_threshold * max) stays NaN; otherwise it is
 * lower + (upper - lower) * ((float)v / max), v the single channel or, for 3 and 4 channels, the grey value
 * (c0 * 1868 + c1 * 9617 + c2 * 4899 + 8192) >> 14 (cvtColor's BGR2GRAY as published, unpinned; equal channels return the
 * channel exactly).  A grid that holds layers must have the image's size; one that holds none takes rows, cols, resolution
 * and position as initializeFromImage does (length = resolution * size).  LIO_ERR_ARG: channels other than 1, 3, 4 (the
 * reference reads 2 channels as garbage), 32F with more than one channel, alpha_threshold outside [0, 1], a size that does
 * not match, on an empty grid what lio_grid_set_layers refuses of a geometry. */
int  lio_grid_add_layer_from_image(lio_grid *g, int32_t layer, const void *image, int32_t rows, int32_t cols, int32_t channels,
                                   int32_t depth, float lower, float upper, double alpha_threshold, double resolution,
                                   const double position[2], lio_grid_from_image_info *info);
/* addColorLayerFromImage<unsigned char, NChannels> (:128-159): 8U with 3 or 4 channels; the cell is the word
 * (c0 << 16) + (c1 << 8) + c2 read as a float (colorVectorToValue).  As written, with 4 channels c0 and c2 are swapped first
 * (cvtColor BGRA2RGB), with 3 they are not.  Geometry as above. */
int  lio_grid_add_color_layer_from_image(lio_grid *g, int32_t layer, const void *image, int32_t rows, int32_t cols,
                                         int32_t channels, int32_t depth, double resolution, const double position[2],
                                         lio_grid_from_image_info *info);
/* fromOccupancyGrid (GridMapRosConverter.cpp:283-327) into layer `layer`: cell i (column-major linear index) takes
 * data[n - 1 - i], -1 as NaN; length = (double)resolution * (width, height), position = origin + 0.5 * length.  Where size,
 * resolution, length or position differ from the grid's (or it holds no layers) the geometry is replaced and every layer it
 * held reads NaN at the new size (setGeometry's clearAll).  LIO_ERR_ARG: width * height != n, width or height below 1 or at
 * or above 2^24, a resolution below 1e-4 or not finite, a non-finite origin.  With lio_grid_to_occupancy(layer, 0, 100)
 * this is the reference's round trip. */
int  lio_grid_from_occupancy(lio_grid *g, int32_t layer, const int8_t *data, size_t n, uint32_t width, uint32_t height,
                             float resolution, const double origin[2], lio_grid_from_occupancy_info *info);
/* toPointCloud (:124-223).  layer_ids: the distinct layers whose fields a point carries, in this order: point_layer gives
 * x, y, z, every other layer one float; *n_fields (may be NULL) receives their number F.  point_layer need not be listed.
 * basic_mask (bit k: layer k) stands for basicLayers_; 0: no validity test.  A cell stays iff every basic layer and the
 * point layer are finite there; x and y are getPositionFromIndex's doubles narrowed to float, z the point layer's value,
 * the other fields the layers' words unchanged.  Survivors keep the iterator's order.  points holds cap_points records of F
 * floats; *n_out receives the count.  More survivors than cap_points: LIO_ERR_CAPACITY, *n_out set, points untouched.
 * LIO_ERR_ARG: n_layers outside 1 .. 16, an id repeated or absent, an absent point_layer, a basic_mask bit of an absent layer. */
int  lio_grid_to_point_cloud(lio_grid *g, int32_t point_layer, const int32_t *layer_ids, int32_t n_layers, uint32_t basic_mask,
                             float *points, size_t cap_points, size_t *n_out, int32_t *n_fields);
/* toGridCells (:367-388): the centres, as pairs of doubles in the iterator's order, of the cells of `layer` that are finite
 * and >= lower && <= upper, compared in float.  Capacity as above.  A NaN bound is LIO_ERR_ARG. */
int  lio_grid_to_grid_cells(lio_grid *g, int32_t layer, float lower, float upper, double *cells, size_t cap_cells, size_t *n_out);
/* toPointCloud(SignedDistanceField) (:225-281) over filterPoints (SignedDistanceField.cpp:186-196): every decimation-th node
 * along z, then y, then x (x fastest) whose distance lies in [lower, upper] (a NaN bound: none on that side) as
 * {x, y, z, intensity}: nodePosition's doubles narrowed to float and the distance.  Only the kept nodes come down.  Capacity
 * as above.  LIO_ERR_ARG: no field in the object, decimation below 1. */
int  lio_sdf_to_point_cloud(lio_sdf *sdf, int32_t decimation, float lower, float upper, float *points, size_t cap_points,
                            size_t *n_out);
/* Measurement hook (tools/grid_convert_cost.py), as lio_grid_debug_stage_ms: the calling thread's last call of the seven as
 * its first stage (the extremes; count and scan; the image up), its second (the image kernel; emit; the ingest kernel) and the
 * result down, in milliseconds (0 for a stage that did not run).  use_tiled != 0 makes the image entries of the calling thread
 * launch their LDS-tiled kernels instead of the direct ones they run by default, for comparison (the same bytes). */
int  lio_grid_convert_debug_stage_ms(int32_t enable, int32_t use_tiled, float ms[3]);

/* ------------------------------------------------ resident planning layers filtered into new layers (grid_map_filters) */
/* grid_map_filters' MinInRadiusFilter, MeanInRadiusFilter, SlidingWindowMathExpressionFilter, CurvatureFilter,
 * ThresholdFilter, DuplicationFilter and DeletionFilter on a lio_grid: a layer derived from one the object holds, wherever
 * that layer came from (the planning chain, lio_grid_add_data_from, lio_grid_move, an image, an occupancy grid), without it
 * crossing PCIe.  DESIGN.md section 4p states the conventions and the labelled deviations; parity is against the restatement
 * (tests/grid_filter_restate.py) with the reference's own test values on top (parity unpinned).  All arithmetic is IEEE basic
 * operations in the reference's order; every word equals the serial loops'.
 *
 * Common to the four filters: out_layer is any id in 0 .. 15; the call replaces what that layer held (the reference's
 * mapOut.add(output_layer) overwrites with NaN), so a cell the filter does not write is the quiet NaN 0x7fc00000.  info may be
 * NULL: n_visited counts the cells the reference's loop evaluates, n_written the cells that receive a value, n_changed the cells
 * the threshold sets.  Complete on return with one host wait.  A failure leaves the object's layer set as it was.  LIO_ERR_ARG,
 * never a clamp, the arguments checked before the object is read: a null g, an object without layers, an absent input layer, a
 * layer id outside 0 .. 15, an op, a mode or a flag out of range, a non-finite or negative radius or length, a radius or a
 * half-window above 32 cells. */
enum { LIO_GF_MIN = 0, LIO_GF_MEAN = 1 };                                               /* radius op */
enum { LIO_GW_INSIDE = 0, LIO_GW_CROP = 1, LIO_GW_EMPTY = 2, LIO_GW_EDGE_MEAN = 3 };    /* SlidingWindowIterator::EdgeHandling, in its order */
enum { LIO_GW_SUM = 0, LIO_GW_MEAN_OF_FINITES, LIO_GW_MIN_OF_FINITES, LIO_GW_MAX_OF_FINITES,
       LIO_GW_NUMBER_OF_FINITES, LIO_GW_STDDEV, LIO_GW_WEIGHTED_SUM };                  /* window op */
struct lio_grid_filter_info {
    int32_t rows, cols;
    int32_t window_size;          /* the window used, in cells (0: not a window filter)                          */
    int32_t pad;
    int64_t n_visited, n_written, n_changed;
};
typedef struct lio_grid_filter_info lio_grid_filter_info;
/* MinInRadiusFilter (op LIO_GF_MIN) and MeanInRadiusFilter (LIO_GF_MEAN).  The circle is CircleIterator's around the cell's
 * own centre: fp64 centres, member when dx dx + dy dy <= radius radius, the window of findSubmapParameters, SubmapIterator's
 * order; a member counts when it is finite.  Mean: every cell; (float)(fp64 serial sum / count), written where the count is
 * not 0 -- the arithmetic of LIO_TERRAIN_SMOOTH.  Min: where the centre is finite; the first finite member initialises, a
 * later one replaces it only when it is smaller (of +0 and -0 the first seen stays).  radius = 0: the cell alone.
 * out_layer == in_layer: LIO_ERR_ARG (a labelled deviation: the reference clears its own input there and returns NaN). */
int  lio_grid_filter_radius(lio_grid *g, int32_t in_layer, int32_t out_layer, int32_t op, double radius, lio_grid_filter_info *info);
/* SlidingWindowMathExpressionFilter with one of seven expressions over SlidingWindowIterator::getData().  window_size >= 1 is
 * used as given (even: LIO_ERR_ARG, the reference throws); window_size == 0 derives it from window_length as setWindowLength
 * does: (size_t)round(window_length / resolution), plus 1 when even.  The window matrix W is the block clipped to the map
 * (INSIDE, CROP) or the full size x size matrix, pre-filled with NaN (EMPTY) or with the clipped block's meanOfFinites()
 * (EDGE_MEAN).  Every reduction is serial, column-major over W, the first coefficient initialises (Eigen's default redux on a
 * functor without a packet form):
 *   SUM sumOfFinites(W); MEAN_OF_FINITES sumOfFinites / numberOfFinites in float; MIN_ / MAX_OF_FINITES the functors of
 *   FunctorsPlugin.hpp as written; NUMBER_OF_FINITES counts x == x (an infinity counts), as a float;
 *   STDDEV sqrt(sumOfFinites(square(W - meanOfFinites(W))) ./ numberOfFinites(W)) (with CROP: LIO_TERRAIN_EDGES);
 *   WEIGHTED_SUM sumOfFinites(K .* W), weights = K, size x size floats, column-major, K(a, b) against W(a, b), each product
 *   rounded to float.  weights must be NULL for every other op.  With CROP and a window above 1 the sizes disagree at the border
 *   (EigenLab throws): LIO_ERR_ARG.
 * CROP, EMPTY and EDGE_MEAN visit every cell.  INSIDE visits the cells whose whole window fits; with a size derived from the
 * length it also reproduces the iterator's two setup() calls (the first with the filter's default size 3): a derived size of 1
 * never visits column 0 and cell (0, 1), and a grid with fewer than 3 rows or columns is not visited at all.  The reference
 * reads compute_empty_cells and never uses it: there is no such argument.  out_layer == in_layer is allowed and computes from
 * the old values. */
int  lio_grid_filter_window(lio_grid *g, int32_t in_layer, int32_t out_layer, int32_t op, int32_t edge_handling,
                            int32_t window_size, double window_length, const float *weights, lio_grid_filter_info *info);
/* CurvatureFilter.  L2 = (float)(resolution * resolution); per finite cell D = (float)(((double)(left + right) / 2.0 -
 * (double)centre) / (double)L2) along the columns, E the same along the rows, the neighbour sum a float addition, a neighbour
 * the map lacks replaced by the cell itself; a D or E that is not finite becomes 0; the value is (float)(-2.0 * (double)(D + E)).
 * Cells that are not finite stay NaN.  out_layer == in_layer: LIO_ERR_ARG, as for the radius filters. */
int  lio_grid_filter_curvature(lio_grid *g, int32_t in_layer, int32_t out_layer, lio_grid_filter_info *info);
/* ThresholdFilter, in place on out_layer, which must exist and may be condition_layer: upper == 0 sets the cells where
 * !((double)condition >= threshold), upper == 1 where !((double)condition <= threshold), to the bits of (float)set_to.  A NaN
 * threshold or set_to is allowed, as there. */
int  lio_grid_filter_threshold(lio_grid *g, int32_t condition_layer, int32_t out_layer, int32_t upper, double threshold,
                               double set_to, lio_grid_filter_info *info);
/* DuplicationFilter: out_layer becomes a copy of in_layer, device to device. */
int  lio_grid_duplicate_layer(lio_grid *g, int32_t in_layer, int32_t out_layer);
/* DeletionFilter: the listed layers leave the object (their memory stays with it).  LIO_ERR_ARG: n_layers outside 1 .. 16, an
 * id outside 0 .. 15 or repeated, and (a labelled deviation: the reference logs it) a listed layer the object does not hold.
 * An object left without a layer is as lio_grid_create left it. */
int  lio_grid_delete_layers(lio_grid *g, const int32_t *layer_ids, int32_t n_layers);
/* Measurement hook (tools/grid_filter_cost.py), as lio_grid_geom_debug_kernel_ms: the kernel of the calling thread's last call
 * of the six, in milliseconds (0 where none was launched). */
int  lio_grid_filter_debug_kernel_ms(int32_t enable, float *ms);

/* ------------------------------------------------ a layer from several by an expression (grid_map_filters' MathExpressionFilter) */
/* An EigenLab expression (Parser<Eigen::MatrixXf>) over the layers of a lio_grid, stored as a layer of the same object.  The
 * text is compiled on the host by a port of the parser's chunk passes (split into chunks, negations, powers, products, sums,
 * functions -- in that order, each left to right) into a postfix program, which the device interprets one lane per cell;
 * DESIGN.md section 4q states the conventions and the labelled deviations, parity is against the restatement
 * (tests/grid_expression_restate.py; parity unpinned).  A value is a full layer or a scalar.
 *   + - .+ .-            layer with layer, layer with scalar, scalar with layer
 *   * / .* ./            with a scalar on either side; .* ./ also layer with layer
 *   ^ .^                 with a scalar on either side; .^ also layer with layer
 *   -x                   x * -1, before powers: -a^2 is (-a)^2
 *   abs sqrt square      float; square is x * x
 *   cwiseMin(a, b)       b < a ? b : a;  cwiseMax(a, b): a < b ? b : a, also on a NaN (Eigen's scalar path)
 *   acos                 acosf, the call behind LIO_TERRAIN_SLOPE
 *   exp log sin cos tan asin, and pow: the fp64 function on the widened argument, narrowed once; log10 is that log times
 *                        (float)(1.0 / log(10)), a float product
 *   sumOfFinites meanOfFinites minOfFinites maxOfFinites numberOfFinites
 *                        of a layer-valued argument: one scalar for the whole map, serial in memory order (column-major), the
 *                        first coefficient initialises, FunctorsPlugin.hpp's functors; numberOfFinites counts x == x.  Of a
 *                        scalar argument: the value, x == x ? 1 : 0, their quotient.
 * names[k] is the variable that stands for layer layer_ids[k]: at most 16 names of [A-Za-z0-9_], not empty, not starting with a
 * digit, each once; ids in 0 .. 15.  A name that is also a function's is the layer.  A listed layer that the object lacks is
 * refused only when the expression reads it.  out_layer may be a layer the expression reads: the result is computed from the old
 * values.  A failure leaves the object's layer set as it was.
 * LIO_ERR_ARG, decided before the object or a device is touched, lio_last_error naming the construct: matrix literals [..],
 * ranges with ':', index groups name(..), assignment, * / ^ between two layers, trace norm size transpose conjugate adjoint zeros
 * ones eye prod, sum mean min max absmax (their order is the Eigen build's), a second (dimension) argument, an unknown name, a
 * function without '(', a missing bracket, an empty expression, what does not reduce to one value (a leading '+'), a scalar
 * result.  LIO_ERR_CAPACITY: an expression above 1024 bytes, 128 ops, a stack of 16 or 8 map-wide reductions. */
struct lio_grid_expression_info {
    int32_t  rows, cols;
    int32_t  n_ops, n_passes;     /* ops over all passes; passes = reductions + 1 */
    uint32_t layers_read;         /* bit k: layer k is read                        */
    int32_t  stack_depth;
    int64_t  n_finite;            /* finite cells of the result (0 from _check)    */
};
typedef struct lio_grid_expression_info lio_grid_expression_info;
/* compile only: no grid, no device (rows = cols = 0) */
int  lio_grid_expression_check(const char *expression, const char *const *names, const int32_t *layer_ids,
                               int32_t n_names, lio_grid_expression_info *info);
int  lio_grid_filter_expression(lio_grid *g, const char *expression, const char *const *names,
                                const int32_t *layer_ids, int32_t n_names, int32_t out_layer,
                                lio_grid_expression_info *info);
/* The same program through the same header text on the host, serially.  layers: n_names layers of rows x cols, column-major,
 * in the order of names; out: rows x cols. */
int  lio_debug_grid_expression_host(const char *expression, const char *const *names, int32_t n_names,
                                    const float *layers, int32_t rows, int32_t cols, float *out);
/* Measurement hook (tools/grid_expression_cost.py): the reduction passes and the storing pass of the calling thread's last
 * lio_grid_filter_expression, in milliseconds. */
int  lio_grid_expression_debug_kernel_ms(int32_t enable, float ms[2]);

#ifdef __cplusplus
}
#endif
#endif /* LIOGPU_H */
