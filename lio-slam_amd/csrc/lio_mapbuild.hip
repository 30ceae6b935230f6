// lio_mapbuild.hip -- the feeders of the registration path:
//   extractCloud = sum of K6 (lio_kfstore.hip) over the nearby keyframes, then K7 (lio_cloud.hip)   MO:1556-1588
//   extractNearby, the selection of those keyframes on the device (lio_nb_select)                   MO:1519-1551
//   downsampleCurrentScan + scan2MapOptimization as one chain (lio_s2m_register_raw)                MO:1605-1611
// MO = the reference's src/liorf/src/mapOptmization.cpp.  -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <string.h>
#include <vector>

#include "lio_handle.h"
#include "lio_kfstore.h"
#include "lio_wg.h"

// K6 with getMinMax3D folded in: the bounding box of the transformed cloud (what the voxel filter starts with) is
// accumulated while the points are written, one set of atomics per workgroup -- no separate pass over the 1.3 M points.
__global__ __launch_bounds__(256) void k_transform_clouds_bbox(const float4* __restrict__ store, const LioKfDesc* __restrict__ kf,
                                                               const int2* __restrict__ chunks /* (kf, first) */,
                                                               float4* __restrict__ dst, float* __restrict__ blk_box /* [grid][6] */)
{
    const int2 c = chunks[blockIdx.x];
    const LioKfDesc d = kf[c.x];
    const int li = c.y + (int)threadIdx.x;
    float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    if (li < d.n) {
        const float4 p = store[d.src + li];
        const float4 q = make_float4(d.T[0] * p.x + d.T[1] * p.y + d.T[2]  * p.z + d.T[3],
                                     d.T[4] * p.x + d.T[5] * p.y + d.T[6]  * p.z + d.T[7],
                                     d.T[8] * p.x + d.T[9] * p.y + d.T[10] * p.z + d.T[11], p.w);   // MO:861-864
        dst[d.first + li] = q;
        mn[0] = mx[0] = q.x; mn[1] = mx[1] = q.y; mn[2] = mx[2] = q.z;
    }
    __shared__ LioWgBoxLds<4> s_box;
    float lo, hi;
    lio_wg_box(mn, mx, s_box, lo, hi);
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        blk_box[(size_t)blockIdx.x * 6 + a] = lo;            // (+inf / -inf for an empty chunk)
        blk_box[(size_t)blockIdx.x * 6 + 3 + a] = hi;
    }
}

// the per-workgroup boxes of k_transform_clouds_bbox -> one box, in k_vox_bbox's order-preserving encoding (one workgroup;
// ~5 000 workgroups hammering six words with atomics cost 124 us, this costs 3)
__global__ __launch_bounds__(256) void k_bbox_reduce(const float* __restrict__ blk_box, int n_blk, unsigned* __restrict__ bbox)
{
    float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int i = threadIdx.x; i < n_blk; i += 256)
#pragma unroll
        for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], blk_box[(size_t)i * 6 + a]); mx[a] = fmaxf(mx[a], blk_box[(size_t)i * 6 + 3 + a]); }
    __shared__ LioWgBoxLds<4> s_box;
    float lo, hi;
    lio_wg_box(mn, mx, s_box, lo, hi);
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        bbox[a] = lo <= hi ? lio_f2ord(lo) : LIO_ORD_NO_MIN;
        bbox[3 + a] = lo <= hi ? lio_f2ord(hi) : LIO_ORD_NO_MAX;
    }
}

// K6 + K7 from selection descriptors already on the device -- src / first / n of every selected keyframe (d_kf, T filled
// here), its pose (d_poses, [roll,pitch,yaw,x,y,z]) and the 256-point chunks of K6 (d_chunks) -- then the map into `h`:
// the common tail of lio_assemble_map_resident and lio_assemble_map_nearby.  `s` is h's stream on the node path, else the
// null stream.
static int assemble_tail(lio_s2m_handle* h, lio_kf_store* st, int n_sel, size_t total, int n_chunks, LioKfDesc* d_kf,
                         const float* d_poses, const int2* d_chunks, hipStream_t s, float leaf, void* out, size_t out_stride, size_t out_cap,
                         size_t* n_out)
{
    int rc, no = 0;
    LioTemp world, ds;
    const float4* map = nullptr;
    if (lio_s2m_takes_device_map(h)) {
        lio_kf_transforms(d_kf, d_poses, n_sel, s);
        HIPCHK(st->world.alloc(total * sizeof(float4)));
        HIPCHK(st->vws.bbox.alloc(6 * sizeof(unsigned)));
        HIPCHK(st->blk_box.alloc(sizeof(float) * 6 * (n_chunks ? n_chunks : 1)));
        if (n_chunks)
            hipLaunchKernelGGL(k_transform_clouds_bbox, dim3((unsigned)n_chunks), dim3(256), 0, s, st->d_pts, d_kf, d_chunks,
                               st->world.as<float4>(), st->blk_box.as<float>());
        hipLaunchKernelGGL(k_bbox_reduce, dim3(1), dim3(256), 0, s, st->blk_box.as<float>(), n_chunks, st->vws.bbox.as<unsigned>());
        float box[6];
        rc = lio_voxel_grid_device<LioDevBytes>(st->world.as<float4>(), (int)total, leaf, st->ds, &no, s, st->vws, box, true);
        if (rc < 0) return rc;
        const int rc3 = lio_s2m_set_map_device_bbox(h, st->ds.as<float4>(), (size_t)no, box);
        if (rc3 != LIO_OK) return rc3;
        map = st->ds.as<float4>();
    } else {
        HIPCHK(world.alloc(total * sizeof(float4)));
        lio_kf_sum_launch(st, d_kf, d_poses, d_chunks, n_sel, n_chunks, world.as<float4>(), s);
        HIPCHK(hipStreamSynchronize(s));   // (the descriptors may be pool temporaries or host arrays of the caller)
        rc = lio_voxel_grid_device(world.as<float4>(), (int)total, leaf, ds, &no, s);
        if (rc < 0) return rc;
        if (h) {                           // (a multi-device or map-sharing handle: through the generic path)
            const int rc3 = lio_s2m_set_map_device_xyzi(h, ds.as<float4>(), (size_t)no);
            if (rc3 != LIO_OK) return rc3;
        }
        map = ds.as<float4>();
    }
    if (out && (size_t)no > out_cap) { if (n_out) *n_out = (size_t)no; return lio_fail(LIO_ERR_ARG, "out holds fewer records than the map (*n_out)"); }
    const int rc2 = lio_copy_out(map, no, out, out_stride, s);
    if (rc2 < 0) return rc2;
    if (n_out) *n_out = (size_t)no;
    return rc;
}

extern "C" int lio_assemble_map_resident(lio_s2m_handle* h, lio_kf_store* st, int32_t n_sel, const int32_t* ids,
                                         const float* poses, float leaf, void* out, size_t out_stride, size_t* n_out)
try {
    if (!st || n_sel < 0 || (n_sel && (!ids || !poses))) return lio_fail(LIO_ERR_ARG, "null argument");
    if ((out && (out_stride < 20 || (out_stride & 3))) || !(leaf > 0.0f))
        return lio_fail(LIO_ERR_ARG, "output stride must be >= 20 and a multiple of 4, leaf > 0");
    int rc = lio_check_device(st->device_id);
    if (rc != LIO_OK) return rc;
    for (int k = 0; k < n_sel; ++k)
        if (ids[k] < 0 || (size_t)ids[k] >= st->off.size()) return lio_fail(LIO_ERR_ARG, "unknown keyframe id");
    LioKfSum t;
    lio_kf_sum_tables(st, ids, nullptr, n_sel, t);
    if (t.total > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "too many points");
    if (n_out) *n_out = 0;
    const int n_chunks = (int)t.chunks.size();
    if (lio_s2m_takes_device_map(h)) {
        // The node path (MO:1556-1588 straight into the resident map of `h`): everything on the handle's stream, the
        // temporaries kept in the store, the map's grid laid over the bounding box the voxel filter measured anyway, and no
        // wait at the end -- the registration that follows is ordered behind the build.  The two waits left are the voxel
        // filter's (bounding box, then the number of occupied voxels: both size what comes next).
        hipStream_t s = lio_s2m_stream_of(h);
        std::swap(st->v_sum, t);           // (host arrays of the asynchronous copies live in the store)
        if ((rc = lio_kf_sum_upload(st->v_sum, poses, st->d_kf, st->d_poses, st->d_chunks, s)) != LIO_OK) return rc;
        // (`poses` is consumed by the voxel filter's first wait, which follows its copy on the same stream)
        return assemble_tail(h, st, n_sel, st->v_sum.total, n_chunks, st->d_kf.as<LioKfDesc>(), st->d_poses.as<float>(), st->d_chunks.as<int2>(),
                             s, leaf, out, out_stride, SIZE_MAX, n_out);
    }
    hipStream_t s = nullptr;
    LioTemp d_kf, d_poses, d_chunks;
    if ((rc = lio_kf_sum_upload(t, poses, d_kf, d_poses, d_chunks, s)) != LIO_OK) return rc;
    return assemble_tail(h, st, n_sel, t.total, n_chunks, d_kf.as<LioKfDesc>(), d_poses.as<float>(), d_chunks.as<int2>(), s, leaf, out,
                         out_stride, SIZE_MAX, n_out);
} LIO_CATCH

// One-shot form: host keyframe clouds in, map out (uploads into a temporary store).
extern "C" int lio_assemble_map(lio_s2m_handle* h, int32_t device_id, int32_t n_kf, const void* const* clouds,
                                const size_t* n_pts, size_t stride, const float* poses, float leaf,
                                void* out, size_t out_stride, size_t* n_out)
try {
    if (!clouds || !n_pts || !poses || n_kf < 0) return lio_fail(LIO_ERR_ARG, "null argument");
    std::vector<int32_t> ids((size_t)n_kf);
    lio_kf_store* st = nullptr;
    int rc = lio_kf_store_create(device_id, &st);
    if (rc != LIO_OK) return rc;
    for (int k = 0; k < n_kf && rc == LIO_OK; ++k) rc = lio_kf_store_add(st, clouds[k], n_pts[k], stride, &ids[k]);
    if (rc == LIO_OK) rc = lio_assemble_map_resident(h, st, n_kf, ids.data(), poses, leaf, out, out_stride, n_out);
    lio_kf_store_destroy(st);
    return rc;
} LIO_CATCH

// ------------------------------------------------ surrounding keyframes on the device (extractNearby MO:1519-1551 + MO:1562)
// cloudKeyPoses6D lives in the store (lio_kf_store_set_poses); lio_assemble_map_nearby selects the keyframes of the local
// map from it and hands the selection to the tail of lio_assemble_map_resident without the ids crossing to the host:
//   k_nb_select    radius test around the last key pose (d2 < r2), the start of the recent suffix, the box of the hits
//   sort           the hits by (d2, i): the stable radix sort of lio_voxsort.h on (d2 bits, i) pairs, misses keyed last
//   k_nb_voxkeys   pcl::VoxelGrid at surroundingKeyframeDensity over the sorted hits (lio_voxsort.h: grid, keys, sort,
//   + centroids    in-order centroids) -> surroundingKeyPosesDS
//   k_nb_relabel   nearest key pose of every centroid, brute force over all N, ties to the lowest index
//   k_nb_compact   centroids, then the recent keyframes newest first, minus those beyond the radius (MO:1562); prefix sums
//                  over cnt[id] and its 256-point chunks -> LioKfDesc records, poses, ids
// One host wait: (n_ids, total points, chunks), which sizes the world-frame cloud.  DESIGN.md has the conventions.

__global__ void k_nb_init(LioNbMeta* m)
{
    m->n_sel = 0; m->recent_fail = -1;
    lio_ord_box_clear(m->box);
    m->n_ids = 0; m->n_chunks = 0; m->total = 0ull;
}

// one thread per key pose: d2 to the last one, the radius flag (strict <, as FLANN's RadiusResultSet), the newest keyframe
// that fails the recent test (atomic max: the suffix after it is what MO:1544-1551 appends), the box of the hits
// RECENT = false: no recent suffix (publishGlobalMap MO:992-1041 has none) -- the key-pose times are not read and every
// keyframe "fails" the recent test, so that the suffix k_nb_compact appends is empty
template <bool RECENT>
__global__ __launch_bounds__(256) void k_nb_select(LioPoseTab tab, int n, float r2, double time_cur, double window,
                                                   uint2* __restrict__ pairs, LioNbMeta* __restrict__ m)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const float lx = tab.x[n - 1], ly = tab.y[n - 1], lz = tab.z[n - 1];
    bool sel = false;
    int fail = -1;
    float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    if (i < n) {
        const float x = tab.x[i], y = tab.y[i], z = tab.z[i];
        const float dx = x - lx, dy = y - ly, dz = z - lz;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        sel = d2 < r2;
        if (!RECENT) fail = i;
        else if (!(time_cur - tab.t[i] < window)) fail = i;
        pairs[i] = make_uint2(sel ? __float_as_uint(d2) : 0xffffffffu, (unsigned)i);
        if (sel) { mn[0] = mx[0] = x; mn[1] = mx[1] = y; mn[2] = mx[2] = z; }
    }
    const int n_hit = __popcll(__ballot(sel));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) fail = max(fail, __shfl_xor(fail, off));
    lio_wave_box(mn, mx);
    if ((threadIdx.x & 63) == 0) {
        if (n_hit) {
            atomicAdd(&m->n_sel, n_hit);
            for (int a = 0; a < 3; ++a) { atomicMin(&m->box[a], lio_f2ord(mn[a])); atomicMax(&m->box[3 + a], lio_f2ord(mx[a])); }
        }
        if (fail >= 0) atomicMax(&m->recent_fail, fail);
    }
}

// sorted hits (d2 bits, i) -> the pose filter's input records (x, y, z, intensity = i) and its (voxel key, position) pairs,
// in place.  Past the hits: key 2^31 + position (above every voxel key, < 2^31: each miss is a voxel of its own after the
// hits' voxels, one cheap segment instead of one crowded one), a zero record.  The grid is laid over the box
// of the hits here, on the device, by the same code as the host's voxel filter; an overflowing index passes the input
// through (key = position), as pcl::VoxelGrid does.
__global__ __launch_bounds__(256) void k_nb_voxkeys(LioPoseTab tab, int n, float inv, const LioNbMeta* __restrict__ m,
                                                    uint2* __restrict__ pairs, float4* __restrict__ pts)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int n_sel = m->n_sel;
    if (j >= n_sel) { pairs[j] = make_uint2(0x80000000u | (unsigned)j, (unsigned)j); pts[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); return; }
    float mn[3], mx[3];
    lio_ord_box_decode(m->box, mn, mx);
    LioVsGrid g;
    long long n_keys = 0;
    const bool pass = lio_vs_grid_from_box(mn, mx, inv, &g, &n_keys) != 0;
    const int i = (int)pairs[j].y;
    const float x = tab.x[i], y = tab.y[i], z = tab.z[i];
    pts[j] = make_float4(x, y, z, (float)i);
    pairs[j] = make_uint2(pass ? (unsigned)j : lio_vs_key(g, x, y, z), (unsigned)j);
}

// voxels of the pose filter = segments of the sorted pairs minus the trailing one-point segments of the misses
__device__ __forceinline__ int nb_n_vox(const LioNbMeta* m, const int* d_no, int n) { return d_no[0] - (n - m->n_sel); }

// MO:1537-1541: the nearest key pose of every centroid over ALL N, argmin of (d2 bits, i) in one 64-bit compare (ties go
// to the lowest index).  One thread per centroid, the poses streamed through LDS 64 at a time; blockIdx.y takes the poses
// [y * NB_SPLIT, (y + 1) * NB_SPLIT) and the splits meet in a 64-bit atomic min (order-independent: the result is exact).
#define NB_SPLIT 1024
__global__ __launch_bounds__(64) void k_nb_relabel(LioPoseTab tab, int n, const float4* __restrict__ cent, const LioNbMeta* __restrict__ m,
                                                   const int* __restrict__ d_no, unsigned long long* __restrict__ cid)
{
    __shared__ float s_x[64], s_y[64], s_z[64];
    const int n_vox = nb_n_vox(m, d_no, n);
    if ((int)(blockIdx.x * 64) >= n_vox) return;                 // workgroup-uniform
    const int o = blockIdx.x * 64 + threadIdx.x;
    const float4 c = o < n_vox ? cent[o] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    unsigned long long best = ~0ull;
    const int b_end = min(n, (int)(blockIdx.y + 1) * NB_SPLIT);
    for (int b = blockIdx.y * NB_SPLIT; b < b_end; b += 64) {
        const int k = b + threadIdx.x;
        __syncthreads();
        if (k < n) { s_x[threadIdx.x] = tab.x[k]; s_y[threadIdx.x] = tab.y[k]; s_z[threadIdx.x] = tab.z[k]; }
        __syncthreads();
        const int m_ = min(64, b_end - b);
        for (int j = 0; j < m_; ++j) {
            const float dx = c.x - s_x[j], dy = c.y - s_y[j], dz = c.z - s_z[j];
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)(b + j);
            best = key < best ? key : best;
        }
    }
    if (o < n_vox) atomicMin(&cid[o], best);
}

// The list of MO:1535-1551 in order -- centroids (own coordinates, relabelled id), then i = last .. recent_fail + 1 --
// minus the entries farther than R from the last key pose (MO:1562: sqrtf, strict >), compacted in order by ONE workgroup
// with running prefix sums of the kept entries, their points and their 256-point chunks.
__global__ __launch_bounds__(256) void k_nb_compact(LioPoseTab tab, int n, float R, const float4* __restrict__ cent,
                                                    const unsigned long long* __restrict__ cid, LioNbMeta* __restrict__ m, const int* __restrict__ d_no,
                                                    int* __restrict__ ids, LioKfDesc* __restrict__ kf, float* __restrict__ poses)
{
    __shared__ int s_wi[4];
    __shared__ unsigned long long s_wl[4];
    const int n_vox = nb_n_vox(m, d_no, n), n_rec = (n - 1) - m->recent_fail, total_e = n_vox + n_rec;
    const float lx = tab.x[n - 1], ly = tab.y[n - 1], lz = tab.z[n - 1];
    int run_ids = 0, run_ch = 0;
    unsigned long long run_pts = 0;
    for (int b = 0; b < total_e; b += 256) {
        const int e = b + threadIdx.x;
        bool keep = false;
        int id = 0;
        if (e < total_e) {
            float x, y, z;
            if (e < n_vox) { const float4 c = cent[e]; x = c.x; y = c.y; z = c.z; id = (int)(unsigned)(cid[e] & 0xffffffffull); }
            else { id = (n - 1) - (e - n_vox); x = tab.x[id]; y = tab.y[id]; z = tab.z[id]; }
            const float ex = x - lx, ey = y - ly, ez = z - lz;
            keep = !(sqrtf((ex * ex + ey * ey) + ez * ez) > R);
        }
        const int cnt = keep ? tab.cnt[id] : 0;
        int t_ids, t_ch;
        unsigned long long t_pts;
        const int pos = run_ids + lio_wg_exclusive_scan<4>(keep ? 1 : 0, &t_ids, s_wi);
        const int cb = run_ch + lio_wg_exclusive_scan<4>(keep ? (cnt + 255) / 256 : 0, &t_ch, s_wi);
        const unsigned long long first = run_pts + lio_wg_exclusive_scan<4>((unsigned long long)cnt, &t_pts, s_wl);
        if (keep) {
            ids[pos] = id;
            LioKfDesc d;
            d.src = tab.off[id]; d.first = (int)first; d.n = cnt; d.pad = cb;     // (pad: the keyframe's first chunk)
            for (int j = 0; j < 12; ++j) d.T[j] = 0.0f;
            kf[pos] = d;
            const float p6[6] = { tab.roll[id], tab.pitch[id], tab.yaw[id], tab.x[id], tab.y[id], tab.z[id] };
            for (int j = 0; j < 6; ++j) poses[(size_t)pos * 6 + j] = p6[j];
        }
        run_ids += t_ids; run_ch += t_ch; run_pts += t_pts;
    }
    if (threadIdx.x == 0) { m->n_ids = run_ids; m->n_chunks = run_ch; m->total = run_pts; }
}

// the 256-point chunks of K6 for the kept list: keyframe k owns chunks [kf[k].pad, kf[k].pad + ceil(n / 256))
__global__ __launch_bounds__(64) void k_nb_chunks(const LioKfDesc* __restrict__ kf, int2* __restrict__ chunks)
{
    const int k = blockIdx.x;
    const int n = kf[k].n, base = kf[k].pad;
    for (int c = threadIdx.x; c * 256 < n; c += 64) chunks[base + c] = make_int2(k, c * 256);
}

void lio_nb_chunks(const LioKfDesc* kf, int n_sel, int2* chunks, hipStream_t s)
{
    if (n_sel) hipLaunchKernelGGL(k_nb_chunks, dim3((unsigned)n_sel), dim3(64), 0, s, kf, chunks);
}

extern "C" void lio_nearby_default_config(lio_nearby_config* cfg)
{
    if (!cfg) return;
    cfg->search_radius = 50.0f;      // surroundingKeyframeSearchRadius, UT:316
    cfg->pose_density = 1.0f;        // surroundingKeyframeDensity, UT:314
    cfg->recent_window_s = 10.0;     // MO:1547
}

// the selection of lio_assemble_map_nearby and of lio_kf_store_global_map (lio_kfstore.h)
int lio_nb_select(lio_kf_store* st, LioNbBufs& b, float R, float density, bool recent, double time_cur, double window, LioNbMeta* hm,
                  hipStream_t s)
{
    int rc;
    const int N = (int)st->off.size();
    if ((rc = lio_vsort_reserve<LioDevBytes>(N, b.cent, b.ws)) != LIO_OK) return rc;
    HIPCHK(b.pts.alloc(sizeof(float4) * (size_t)N));
    HIPCHK(b.cid.alloc(sizeof(unsigned long long) * (size_t)N));
    HIPCHK(b.ids.alloc(sizeof(int) * 2 * (size_t)N));
    HIPCHK(b.meta.alloc(sizeof(LioNbMeta)));
    HIPCHK(b.d_kf.alloc(sizeof(LioKfDesc) * 2 * (size_t)N));    // the list holds at most n_vox + n_recent <= 2N entries
    HIPCHK(b.d_poses.alloc(sizeof(float) * 6 * 2 * (size_t)N));
    const LioPoseTab tab = lio_kf_pose_tab(st);
    LioNbMeta* m = b.meta.as<LioNbMeta>();
    const unsigned nblk = (unsigned)((N + 255) / 256);
    hipLaunchKernelGGL(k_nb_init, dim3(1), dim3(1), 0, s, m);
    const float r2 = (float)((double)R * (double)R);                // what PCL hands FLANN
    if (recent) hipLaunchKernelGGL(k_nb_select<true>, dim3(nblk), dim3(256), 0, s, tab, N, r2, time_cur, window, b.ws.pairs_a.as<uint2>(), m);
    else hipLaunchKernelGGL(k_nb_select<false>, dim3(nblk), dim3(256), 0, s, tab, N, r2, time_cur, window, b.ws.pairs_a.as<uint2>(), m);
    uint2* hits = lio_vsort_pairs<LioDevBytes>(N, 32, s, b.ws);      // (d2, i) ascending, the misses last
    // (an even number of passes ends in pairs_a, where the second sort starts: k_nb_voxkeys rewrites the pairs in place)
    if (hits != b.ws.pairs_a.as<uint2>()) return lio_fail(LIO_ERR_HIP, "radix sort ended in the wrong buffer");
    hipLaunchKernelGGL(k_nb_voxkeys, dim3(nblk), dim3(256), 0, s, tab, N, 1.0f / density, m, hits, b.pts.as<float4>());
    const uint2* vox = lio_vsort_pairs<LioDevBytes>(N, 32, s, b.ws);
    if ((rc = lio_vsort_centroids<LioDevBytes>(b.pts.as<float4>(), vox, N, b.cent, s, b.ws)) != LIO_OK) return rc;
    const int* d_no = b.ws.d_no.as<int>();
    HIPCHK(hipMemsetAsync(b.cid.p, 0xff, sizeof(unsigned long long) * (size_t)N, s));
    hipLaunchKernelGGL(k_nb_relabel, dim3((unsigned)((N + 63) / 64), (unsigned)((N + NB_SPLIT - 1) / NB_SPLIT)), dim3(64), 0, s, tab, N,
                       b.cent.as<float4>(), m, d_no, b.cid.as<unsigned long long>());
    hipLaunchKernelGGL(k_nb_compact, dim3(1), dim3(256), 0, s, tab, N, R, b.cent.as<float4>(), b.cid.as<unsigned long long>(), m, d_no,
                       b.ids.as<int>(), b.d_kf.as<LioKfDesc>(), b.d_poses.as<float>());
    HIPCHK(hipMemcpyAsync(hm, m, sizeof(LioNbMeta), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));                                // THE wait of the selection: (n_ids, total points, chunks)
    HIPCHK(hipGetLastError());
    return LIO_OK;
}

extern "C" int lio_assemble_map_nearby(lio_s2m_handle* h, lio_kf_store* st, const lio_nearby_config* cfg, double time_cur,
                                       float leaf, int32_t* ids_out, int32_t ids_cap, int32_t* n_ids, void* out,
                                       size_t out_stride, size_t out_cap, size_t* n_out)
try {
    if (!st || !cfg || ids_cap < 0) return lio_fail(LIO_ERR_ARG, "null argument");
    if ((out && (out_stride < 20 || (out_stride & 3))) || !(leaf > 0.0f))
        return lio_fail(LIO_ERR_ARG, "output stride must be >= 20 and a multiple of 4, leaf > 0");
    const float R = cfg->search_radius;
    if (!(R > 0.0f) || !std::isfinite(R) || !(cfg->pose_density > 0.0f) || !std::isfinite(cfg->pose_density) ||
        !std::isfinite(cfg->recent_window_s) || !std::isfinite(time_cur))
        return lio_fail(LIO_ERR_ARG, "search_radius, pose_density > 0 and finite; recent_window_s, time_cur finite");
    if (n_ids) *n_ids = 0;
    if (n_out) *n_out = 0;
    int rc = lio_check_device(st->device_id);
    if (rc != LIO_OK) return rc;
    if (h && h->cfg.device_id != st->device_id)
        return lio_fail(LIO_ERR_ARG, "the handle and the keyframe store live on different devices");
    const int N = (int)st->off.size();
    if (N == 0) return LIO_OK;                       // MO:1592-1593: nothing to extract, the map stays as it is
    if (st->n_posed != (size_t)N) return lio_fail(LIO_ERR_ARG, "a keyframe has no pose (lio_kf_store_set_poses)");
    const bool node = lio_s2m_takes_device_map(h);
    hipStream_t s = node ? lio_s2m_stream_of(h) : nullptr;
    if ((rc = lio_kf_upload_pose_tab(st, s)) != LIO_OK) return rc;
    if (!st->ev_ids) HIPCHK(hipEventCreateWithFlags(&st->ev_ids, hipEventDisableTiming));
    LioNbBufs nb = { st->nws, st->nb_pts, st->nb_cent, st->nb_cid, st->nb_ids, st->nb_meta, st->d_kf, st->d_poses };
    LioNbMeta* hm = (LioNbMeta*)st->h_stage.p;                        // (the stage exists: the first call uploaded through it)
    if ((rc = lio_nb_select(st, nb, R, cfg->pose_density, true, time_cur, cfg->recent_window_s, hm, s)) != LIO_OK) return rc;
    const int n_sel = hm->n_ids, n_chunks = hm->n_chunks;
    const unsigned long long total = hm->total;
    if (n_ids) *n_ids = n_sel;
    if (ids_out && ids_cap < n_sel) return lio_fail(LIO_ERR_ARG, "ids_cap is smaller than the selected list (*n_ids)");
    if (total > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "too many points");
    int* h_ids = (int*)st->h_stage.p;
    if (ids_out && n_sel) {
        HIPCHK(st->h_stage.grow((size_t)n_sel * sizeof(int), (size_t)n_sel * sizeof(int) * 2, hipHostMallocPortable));
        h_ids = (int*)st->h_stage.p;
        HIPCHK(hipMemcpyAsync(h_ids, st->nb_ids.p, (size_t)n_sel * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipEventRecord(st->ev_ids, s));                      // (complete by the voxel filter's waits further down)
    }
    HIPCHK(st->d_chunks.alloc(sizeof(int2) * (n_chunks ? n_chunks : 1)));
    lio_nb_chunks(st->d_kf.as<LioKfDesc>(), n_sel, st->d_chunks.as<int2>(), s);
    rc = assemble_tail(h, st, n_sel, (size_t)total, n_chunks, st->d_kf.as<LioKfDesc>(), st->d_poses.as<float>(),
                       st->d_chunks.as<int2>(), s, leaf, out, out_stride, out_cap, n_out);
    if (ids_out && n_sel) {
        HIPCHK(hipEventSynchronize(st->ev_ids));
        memcpy(ids_out, h_ids, (size_t)n_sel * sizeof(int));
    }
    return rc;
} LIO_CATCH

// ------------------------------------------------ one callback on the device: downsample + register (SURVEY 8f / verdict r2)
// (struct LioRawWs, the staged cloud and voxel-filter workspace kept on the handle, is in lio_kfstore.h)

void lio_raw_ws_free(LioRawWs* w) { delete w; }

// downsampleCurrentScan MO:1605-1611 + scan2MapOptimization MO:1839-1865 without a host round trip in between:
// the deskewed cloud goes up once (or is read in place when it already lives on the device), is voxel-filtered on the
// handle's stream with the workspace kept on the handle, and the Gauss-Newton loop runs on the filter's output where it
// lies (float4 x,y,z,intensity records).  The result is bit-identical to lio_voxel_grid followed by lio_s2m_register
// on its output: same filter code, same registration code.  The filtered cloud stays staged on the handle, so
// lio_kf_store_add_from_handle turns it into a keyframe (saveKeyFramesAndFactor MO:2136-2142) with its intensities.
extern "C" int lio_s2m_register_raw(lio_s2m_handle* h, const void* data, size_t n_points, const lio_pc2_layout* layout, float leaf,
                                    float pose[6], lio_s2m_result* res, void* ds_out, size_t ds_out_stride, size_t* n_ds)
try {
    if (!h || !layout || !pose) return lio_fail(LIO_ERR_ARG, "null argument");
    if (h->multi || h->corner_active) return lio_fail(LIO_ERR_ARG, "lio_s2m_register_raw needs a plain single-device handle");
    if (lio_pc2_check_xyz(layout) != LIO_OK) return LIO_ERR_ARG;
    if (!(leaf > 0.0f)) return lio_fail(LIO_ERR_ARG, "leaf must be positive");
    if (ds_out && (ds_out_stride < 20 || (ds_out_stride & 3))) return lio_fail(LIO_ERR_ARG, "output stride must be >= 20 and a multiple of 4");
    if (n_points && !data) return lio_fail(LIO_ERR_ARG, "null cloud");
    if (n_points > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    if (n_ds) *n_ds = 0;
    int rc = lio_check_device(h->cfg.device_id);
    if (rc != LIO_OK) return rc;
    if (!h->raw_ws) h->raw_ws = new LioRawWs();
    LioRawWs* w = h->raw_ws;
    if (!w->aux) {
        HIPCHK(hipStreamCreateWithFlags(&w->aux, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&w->ev_in, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&w->ev_done, hipEventDisableTiming));
    }
    hipStream_t s = w->aux;                              // upload + filter here; the registration on h->stream, behind the map
    w->has_raw = false;
    const size_t step = layout->point_step, n = n_points;
    // the blob: read in place when it is device memory of this device, else one H2D copy (a true DMA when pinned)
    const unsigned char* d_rec = nullptr;
    struct PinGuard {                                    // hipHostRegister for the duration of the call, released on every path
        void* p = nullptr;
        ~PinGuard() { if (p) (void)hipHostUnregister(p); }
    } pin;
    if (n) {
        hipPointerAttribute_t at;
        bool in_place = false;
        if (hipPointerGetAttributes(&at, data) == hipSuccess) in_place = at.type == hipMemoryTypeDevice && at.device == h->cfg.device_id;
        (void)hipGetLastError();                         // (pageable host memory is reported as an error)
        if (in_place) {
            d_rec = (const unsigned char*)data;
            // (device memory may have been produced by work queued on the handle's stream: keep that order)
            HIPCHK(hipEventRecord(w->ev_in, h->stream));
            HIPCHK(hipStreamWaitEvent(s, w->ev_in, 0));
        } else {
            if (layout->pin_host) {
                if (hipHostRegister(const_cast<void*>(data), n * step, hipHostRegisterDefault) == hipSuccess) pin.p = const_cast<void*>(data);
                (void)hipGetLastError();
            }
            HIPCHK(w->raw.alloc(n * step));
            HIPCHK(hipMemcpyAsync(w->raw.p, data, n * step, hipMemcpyHostToDevice, s));
            d_rec = w->raw.as<unsigned char>();
        }
        HIPCHK(w->xyzi.alloc(n * sizeof(float4)));
        lio_rec_to_xyzi4(d_rec, step, (size_t)layout->off_x, layout->off_intensity >= 0 ? layout->off_intensity : -1, (int)n, w->xyzi.as<float4>(), s);
    }
    w->n_raw = n; w->has_raw = true;                     // (lio_kf_store_sc_add_from_handle reads it on `aux`)
    int no = 0;
    // (the filter's first host wait -- the bounding box -- also covers the H2D copy: the caller's blob is free again)
    rc = lio_voxel_grid_device<LioDevBytes>(w->xyzi.as<float4>(), (int)n, leaf, w->ds, &no, s, w->vws, nullptr);
    if (rc < 0) return rc;                               // (rc == 1: PCL would pass the cloud through -- and so did we)
    if (n == 0) HIPCHK(w->ds.alloc(sizeof(float4)));
    // the filter's last kernels (centroids) may still be in flight: the registration on the handle's stream waits for them
    HIPCHK(hipEventRecord(w->ev_done, s));
    HIPCHK(hipStreamWaitEvent(h->stream, w->ev_done, 0));
    LioUploadOpts o;
    o.int_off = 12;                                      // the staged records are float4 (x, y, z, intensity)
    const int rr = lio_s2m_register_opts(h, w->ds.p, (size_t)no, sizeof(float4), pose, res, o);
    if (rr < 0) return rr;
    if (ds_out) { const int rc2 = lio_copy_out(w->ds.as<float4>(), no, ds_out, ds_out_stride, h->stream); if (rc2 < 0) return rc2; }
    if (n_ds) *n_ds = (size_t)no;
    return rr;
} LIO_CATCH
