// lio_mapbuild.hip -- the feeders of the registration path:
//   K6 transformPointCloud           MO:849-868
//   K7 pcl::VoxelGrid centroid filter MO:1605-1611 (scan), MO:1581-1583 (local map)
//   extractCloud = sum of K6 over the nearby keyframes, then K7   MO:1556-1588
// MO = /root/reference/src/liorf/src/mapOptmization.cpp.  -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <cmath>
#include <string.h>
#include <algorithm>
#include <vector>

#include "lio_handle.h"
#include "lio_icp.h"
#include "lio_kfstore.h"
#include "lio_heightmap.h"
#include "lio_localmap.h"
#include "lio_pool.h"
#include "lio_sc.h"
#include "lio_terrain.h"
#include "lio_device_math.h"
#include "lio_scan2.h"
#include "lio_voxsort.h"

int lio_s2m_set_map_device_xyzi(lio_s2m_handle* h, const float4* d_xyzi, size_t n);   // liogpu_api.hip
int lio_s2m_set_map_device_bbox(lio_s2m_handle* h, const float4* d_xyzi, size_t n, const float box[6]);
hipStream_t lio_s2m_stream_of(lio_s2m_handle* h);
bool lio_s2m_takes_device_map(const lio_s2m_handle* h);

// pose [roll,pitch,yaw,x,y,z] -> 3x4 transform, same trig definition as the GN loop
__global__ void k_kf_transforms(LioKfDesc* __restrict__ kf, const float* __restrict__ poses, int n_kf)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_kf) return;
    float pose[6], T[12], trig[6];
    for (int j = 0; j < 6; ++j) pose[j] = poses[k * 6 + j];
    lio_pose_to_transform(pose, T, trig);
    for (int j = 0; j < 12; ++j) kf[k].T[j] = T[j];
}

// K6: resident keyframe clouds (float4 x,y,z,intensity, lidar frame) -> world-frame float4
__global__ __launch_bounds__(256) void k_transform_clouds(const float4* __restrict__ store,
                                                          const LioKfDesc* __restrict__ kf,
                                                          const int2* __restrict__ chunks /* (kf, first) */,
                                                          float4* __restrict__ dst)
{
    const int2 c = chunks[blockIdx.x];
    const LioKfDesc d = kf[c.x];
    const int li = c.y + (int)threadIdx.x;
    if (li >= d.n) return;
    const float4 p = store[d.src + li];
    dst[d.first + li] = make_float4(d.T[0] * p.x + d.T[1] * p.y + d.T[2]  * p.z + d.T[3],
                                    d.T[4] * p.x + d.T[5] * p.y + d.T[6]  * p.z + d.T[7],
                                    d.T[8] * p.x + d.T[9] * p.y + d.T[10] * p.z + d.T[11], p.w);   // MO:861-864
}

__global__ void k_aos_to_xyzi4(const unsigned char* __restrict__ src, size_t stride, int n, float4* __restrict__ dst)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = reinterpret_cast<const float*>(src + (size_t)i * stride);
    dst[i] = make_float4(p[0], p[1], p[2], p[4]);
}

// getMinMax3D (PCL): bbox[0..2] = min, bbox[3..5] = max as order-preserving uints
__global__ void k_vox_bbox(const float4* __restrict__ p, int n, unsigned* __restrict__ bbox)
{
    float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 v = p[i];
        mn[0] = fminf(mn[0], v.x); mx[0] = fmaxf(mx[0], v.x);
        mn[1] = fminf(mn[1], v.y); mx[1] = fmaxf(mx[1], v.y);
        mn[2] = fminf(mn[2], v.z); mx[2] = fmaxf(mx[2], v.z);
    }
    __shared__ LioWgBoxLds<4> s_box;                  // one set of atomics per workgroup
    float lo, hi;
    lio_wg_box(mn, mx, s_box, lo, hi);
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        atomicMin(&bbox[a], lio_f2ord(lo));
        atomicMax(&bbox[3 + a], lio_f2ord(hi));
    }
}

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

__global__ void k_xyzi4_to_aos(const float4* __restrict__ src, int n, unsigned char* __restrict__ dst, size_t stride)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 v = src[i];
    float* o = reinterpret_cast<float*>(dst + (size_t)i * stride);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = 1.0f; o[4] = v.w;
}

namespace {

// Room for sorting n pairs and summing their segments (ws) and for n centroids (out).
template <class B>
static int vsort_reserve(int n, B& out, LioVoxWs<B>& ws)
{
    const int n_blocks = (n + LIO_VS_THREADS * 4 - 1) / (LIO_VS_THREADS * 4), n_hblk = (n + 1023) / 1024;
    HIPCHK(ws.pairs_a.alloc(sizeof(uint2) * (size_t)n));
    HIPCHK(ws.pairs_b.alloc(sizeof(uint2) * (size_t)n));
    HIPCHK(ws.hist.alloc(sizeof(int) * (size_t)LIO_VS_BINS * n_blocks));
    HIPCHK(ws.blk_heads.alloc(sizeof(int) * (size_t)(n_hblk + 1)));
    HIPCHK(ws.seg_start.alloc(sizeof(int) * ((size_t)n + 1)));
    HIPCHK(ws.d_no.alloc(sizeof(int) * 2));
    HIPCHK(ws.row_total.alloc(sizeof(int) * LIO_VS_BINS));
    HIPCHK(ws.large.alloc(sizeof(int) * ((size_t)n + 1)));
    HIPCHK(out.alloc(sizeof(float4) * (size_t)n));
    return LIO_OK;
}

// Stable LSD radix sort of the n pairs in ws.pairs_a by their low `bits` key bits; returns the buffer that holds the result.
template <class B>
static uint2* vsort_pairs(int n, int bits, hipStream_t s, LioVoxWs<B>& ws)
{
    const int passes = (bits + 7) / 8, dbits = (bits + passes - 1) / passes;      // e.g. 25 bits -> 4 passes of 7
    const unsigned mask = dbits >= 32 ? 0xffffffffu : (1u << dbits) - 1u;
    const int items = n > (1 << 18) ? 8 : 4;
    const int tile = LIO_VS_THREADS * items, n_blocks = (n + tile - 1) / tile;
    uint2 *a = ws.pairs_a.template as<uint2>(), *b = ws.pairs_b.template as<uint2>();
    for (int p = 0; p < passes; ++p) {
        const int shift = p * dbits;
        int* hist = ws.hist.template as<int>();
        if (items == 8) hipLaunchKernelGGL(k_vsort_hist<8>, dim3(n_blocks), dim3(LIO_VS_THREADS), 0, s, a, n, shift, mask, hist, n_blocks);
        else hipLaunchKernelGGL(k_vsort_hist<4>, dim3(n_blocks), dim3(LIO_VS_THREADS), 0, s, a, n, shift, mask, hist, n_blocks);
        int* row_total = ws.row_total.template as<int>();
        hipLaunchKernelGGL(k_vsort_scan_rows, dim3(LIO_VS_BINS), dim3(256), 0, s, hist, n_blocks, row_total);
        if (items == 8) hipLaunchKernelGGL(k_vsort_scatter<8>, dim3(n_blocks), dim3(LIO_VS_THREADS), 0, s, a, n, shift, mask, hist, row_total, n_blocks, b);
        else hipLaunchKernelGGL(k_vsort_scatter<4>, dim3(n_blocks), dim3(LIO_VS_THREADS), 0, s, a, n, shift, mask, hist, row_total, n_blocks, b);
        uint2* t = a; a = b; b = t;
    }
    return a;
}

// Segments (voxels) of the sorted pairs `a` and the in-order centroid of each -> out[0 .. ws.d_no[0]); nothing waits.
template <class B>
static int vsort_centroids(const float4* d_in, const uint2* a, int n, B& out, hipStream_t s, LioVoxWs<B>& ws)
{
    const int n_hblk = (n + 1023) / 1024;
    int* d_no = ws.d_no.template as<int>();
    HIPCHK(hipMemsetAsync(d_no, 0, 2 * sizeof(int), s));                          // [0] voxels, [1] crowded voxels queued
    hipLaunchKernelGGL(k_vsort_head_count, dim3(n_hblk), dim3(256), 0, s, a, n, ws.blk_heads.template as<int>());
    hipLaunchKernelGGL(k_wg_scan_in_place<4>, dim3(1), dim3(256), 0, s, ws.blk_heads.template as<int>(), n_hblk, d_no);
    hipLaunchKernelGGL(k_vsort_head_emit, dim3(n_hblk), dim3(256), 0, s, a, n, ws.blk_heads.template as<int>(), d_no, ws.seg_start.template as<int>());
    hipLaunchKernelGGL(k_vsort_centroid, dim3((n_hblk + 3) / 4), dim3(256), 0, s, d_in, a, n, ws.seg_start.template as<int>(),
                       ws.blk_heads.template as<int>(), n_hblk, d_no, out.template as<float4>(), ws.large.template as<int>(), d_no + 1);
    hipLaunchKernelGGL(k_vsort_centroid_large, dim3(n < 1024 * 64 ? (n + 63) / 64 : 1024), dim3(256), 0, s, d_in, a, ws.seg_start.template as<int>(),
                       out.template as<float4>(), ws.large.template as<int>(), d_no + 1);
    return LIO_OK;
}

// K7 proper (lio_voxsort.h): keys -> stable LSD radix sort of (key, index) pairs -> segment heads -> in-order sums.  g describes
// the voxel grid, n_keys its size (< 2^31).  (Rounds 1-2 used a counting sort with count / start / rank arrays over the whole
// key space, atomics for the slots and a per-voxel sort for the order; round 3 first replaced the per-voxel sorts, then measured
// the sorting form faster on every input -- map assembly 0.37 against 0.43 ms, the raw-sweep chain 0.50 against 0.57 ms at leaf
// 0.4 m and 0.88 against 1.09 ms at 0.15 m, profiles/r03_k7_forms.txt -- and removed the counting form.)  `out` is allocated for the worst case (n voxels) so that the centroid kernels are
// enqueued without waiting for the count; the one host wait (*n_out) comes last and overlaps them.
template <class B>
static int voxel_grid_sorted(const float4* d_in, int n, const LioVsGrid& vg, long long n_keys, B& out, int* n_out, hipStream_t s, LioVoxWs<B>& ws)
{
    int bits = 1;
    while (bits < 31 && (1LL << bits) < n_keys) ++bits;
    int rc = vsort_reserve<B>(n, out, ws);
    if (rc != LIO_OK) return rc;
    hipLaunchKernelGGL(k_vsort_keys, dim3((n + 255) / 256), dim3(256), 0, s, vg, d_in, n, ws.pairs_a.template as<uint2>());
    const uint2* a = vsort_pairs<B>(n, bits, s, ws);
    if ((rc = vsort_centroids<B>(d_in, a, n, out, s, ws)) != LIO_OK) return rc;
    int no = 0;
    HIPCHK(hipMemcpyAsync(&no, ws.d_no.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));                                              // (`no`; the centroid kernels ran under this wait)
    HIPCHK(hipGetLastError());
    *n_out = no;
    return LIO_OK;
}

// getMinMax3D of a device-resident cloud (n > 0) in two halves, so that a caller whose box is already in `bbox`
// (k_transform_clouds_bbox) takes the second alone: clear + k_vox_bbox, then the copy, the wait and the decoding.
template <class B>
int cloud_box_launch(const float4* d_in, int n, B& bbox, hipStream_t s)
{
    HIPCHK(bbox.alloc(6 * sizeof(unsigned)));
    unsigned init[6];
    lio_ord_box_clear(init);
    HIPCHK(hipMemcpyAsync(bbox.p, init, sizeof(init), hipMemcpyHostToDevice, s));
    int nbb = (n + 1023) / 1024; if (nbb > 512) nbb = 512; if (nbb < 1) nbb = 1;
    hipLaunchKernelGGL(k_vox_bbox, dim3(nbb), dim3(256), 0, s, d_in, n, bbox.template as<unsigned>());
    return LIO_OK;
}

template <class B>
int cloud_box_wait(B& bbox, float mn[3], float mx[3], hipStream_t s)
{
    unsigned hb[6];
    HIPCHK(hipMemcpyAsync(hb, bbox.p, sizeof(hb), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    lio_ord_box_decode(hb, mn, mx);
    return LIO_OK;
}

// K7 on a device-resident float4 cloud.  *d_out receives a freshly allocated device array.
// Returns LIO_OK, or 1 when PCL would pass the cloud through (voxel index overflow).
// `ws`: the temporaries; `wait`: block until the result is complete (required when ws is made of pool temporaries, which
// are recycled when the caller returns); `box` (optional) receives min[3], max[3] of the INPUT cloud, a box around the output.
// have_box: ws.bbox already holds the bounding box of d_in (k_transform_clouds_bbox), no pass for it.
template <class B>
int voxel_grid_device(const float4* d_in, int n, float leaf, B& out, int* n_out, hipStream_t s, LioVoxWs<B>& ws, bool wait, float* box,
                      bool have_box = false)
{
    *n_out = 0;
    if (box) for (int a = 0; a < 6; ++a) box[a] = 0.0f;
    if (n == 0) return LIO_OK;
    B& bbox = ws.bbox;
    if (!have_box) {
        int brc = cloud_box_launch<B>(d_in, n, bbox, s);
        if (brc != LIO_OK) return brc;
    }
    float mn[3], mx[3];
    int wrc = cloud_box_wait<B>(bbox, mn, mx, s);
    if (wrc != LIO_OK) return wrc;
    if (box) for (int a = 0; a < 3; ++a) { box[a] = mn[a]; box[3 + a] = mx[a]; }
    // (a box that is not finite -- inf coordinates, or no finite point at all -- is outside what PCL defines; such a cloud
    // takes the same way out as an overflowing index, deterministically)
    LioVsGrid g;
    long long n_keys_ll = 0;
    const int grc = lio_vs_grid_from_box(mn, mx, 1.0f / leaf, &g, &n_keys_ll);
    if (grc == 1) {                                  // "Leaf size is too small": PCL copies the input
        HIPCHK(out.alloc(sizeof(float4) * (size_t)n));
        HIPCHK(hipMemcpyAsync(out.p, d_in, sizeof(float4) * (size_t)n, hipMemcpyDeviceToDevice, s));
        *n_out = n;
        return 1;
    }
    if (grc == 2) return lio_fail(LIO_ERR_CAPACITY, "voxel grid has more than 2^31 - 1 voxels");
    (void)wait;                                  // (the sorting form always ends with the wait for the voxel count)
    return voxel_grid_sorted<B>(d_in, n, g, n_keys_ll, out, n_out, s, ws);
}

int voxel_grid_device(const float4* d_in, int n, float leaf, LioTemp& out, int* n_out, hipStream_t s)
{
    LioVoxWs<LioTemp> ws;
    return voxel_grid_device<LioTemp>(d_in, n, leaf, out, n_out, s, ws, true, nullptr);
}

int copy_out(const float4* d_pts, int n, void* out, size_t out_stride, hipStream_t s)
{
    if (!out || n == 0) return LIO_OK;
    LioTemp aos;
    HIPCHK(aos.alloc((size_t)n * out_stride));
    HIPCHK(hipMemsetAsync(aos.p, 0, (size_t)n * out_stride, s));
    hipLaunchKernelGGL(k_xyzi4_to_aos, dim3((n + 255) / 256), dim3(256), 0, s, d_pts, n, aos.as<unsigned char>(), out_stride);
    HIPCHK(hipMemcpyAsync(out, aos.p, (size_t)n * out_stride, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return LIO_OK;
}

int check_device(int device_id)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return lio_fail(LIO_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    HIPCHK(hipSetDevice(device_id));
    (void)hipGetLastError();
    return LIO_OK;
}
}  // namespace

extern "C" int lio_voxel_grid(int32_t device_id, const void* pts, size_t n, size_t stride, float leaf,
                              void* out, size_t out_stride, size_t* n_out)
try {
    if (!n_out || (n && (!pts || !out))) return lio_fail(LIO_ERR_ARG, "null argument");
    if (stride < 20 || (stride & 3) || out_stride < 20 || (out_stride & 3) || !(leaf > 0.0f))
        return lio_fail(LIO_ERR_ARG, "strides must be >= 20 and multiples of 4, leaf > 0");
    if (n > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    *n_out = 0;
    if (n == 0) return LIO_OK;
    int rc = check_device(device_id);
    if (rc != LIO_OK) return rc;
    hipStream_t s = nullptr;
    LioTemp raw, xyzi, ds;
    HIPCHK(raw.alloc(n * stride));
    HIPCHK(xyzi.alloc(n * sizeof(float4)));
    HIPCHK(hipMemcpyAsync(raw.p, pts, n * stride, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_aos_to_xyzi4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, raw.as<unsigned char>(), stride, (int)n, xyzi.as<float4>());
    int no = 0;
    rc = voxel_grid_device(xyzi.as<float4>(), (int)n, leaf, ds, &no, s);
    if (rc < 0) return rc;
    const int rc2 = copy_out(ds.as<float4>(), no, out, out_stride, s);
    if (rc2 < 0) return rc2;
    *n_out = (size_t)no;
    return rc;
} LIO_CATCH

// ------------------------------------------------------- resident keyframe store
// struct lio_kf_store -- surfCloudKeyFrames (MO:128) in HBM -- is in lio_kfstore.h.

extern "C" int lio_kf_store_create(int32_t device_id, lio_kf_store** out)
try {
    if (!out) return lio_fail(LIO_ERR_ARG, "null argument");
    int rc = check_device(device_id);
    if (rc != LIO_OK) return rc;
    lio_kf_store* s = new lio_kf_store();
    s->device_id = device_id;
    *out = s;
    return LIO_OK;
} LIO_CATCH

extern "C" void lio_kf_store_destroy(lio_kf_store* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device_id);
    (void)hipDeviceSynchronize();
    delete s;
}

extern "C" int lio_kf_store_count(const lio_kf_store* s) { return s ? (int)s->off.size() : 0; }
extern "C" size_t lio_kf_store_points(const lio_kf_store* s, int32_t id) { return (s && id >= 0 && (size_t)id < s->cnt.size()) ? s->cnt[(size_t)id] : 0; }

static int kf_store_reserve(lio_kf_store* s, size_t n)
{
    if (s->used + n > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "keyframe store is full");
    if (s->used + n > s->d_pts.cap) {                   // grow geometrically, keep the resident clouds
        size_t ncap = (s->d_pts.cap ? s->d_pts.cap * 2 : (size_t)1 << 20);
        while (ncap < s->used + n) ncap *= 2;
        LioDevBuf<float4> np_;
        HIPCHK(np_.grow(ncap, 1.0, 0));
        if (s->used) HIPCHK(hipMemcpy(np_, s->d_pts, s->used * sizeof(float4), hipMemcpyDeviceToDevice));
        s->d_pts = std::move(np_);                       // (frees the old block)
    }
    return LIO_OK;
}

static void kf_store_commit(lio_kf_store* s, size_t n, int32_t* id_out)
{
    if (id_out) *id_out = (int32_t)s->off.size();
    s->dirty_lo = std::min(s->dirty_lo, s->off.size());
    s->dirty_hi = s->off.size() + 1;
    s->off.push_back(s->used);
    s->cnt.push_back(n);
    s->used += n;
    for (std::vector<float>* v : { &s->px, &s->py, &s->pz, &s->proll, &s->ppitch, &s->pyaw }) v->push_back(0.0f);
    s->ptime.push_back(0.0);
    s->has_pose.push_back(0);
    s->has_time.push_back(0);
}

// records (x,y,z at xyz_off, FLOAT32 intensity at int_off, < 0 = the record carries none) -> float4 (x,y,z,intensity)
__global__ void k_rec_to_xyzi4(const unsigned char* __restrict__ src, size_t stride, size_t xyz_off, int int_off, int n,
                               float4* __restrict__ dst)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned char* rec = src + (size_t)i * stride;
    const float* p = reinterpret_cast<const float*>(rec + xyz_off);
    dst[i] = make_float4(p[0], p[1], p[2], int_off >= 0 ? *reinterpret_cast<const float*>(rec + int_off) : 0.0f);
}

extern "C" int lio_kf_store_add(lio_kf_store* s, const void* cloud, size_t n, size_t stride, int32_t* id_out)
try {
    if (!s || (n && !cloud)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (stride < 20 || (stride & 3)) return lio_fail(LIO_ERR_ARG, "stride must be >= 20 and a multiple of 4");
    int rc = check_device(s->device_id);
    if (rc != LIO_OK) return rc;
    if ((rc = kf_store_reserve(s, n)) != LIO_OK) return rc;
    if (n) {
        LioTemp raw;
        HIPCHK(raw.alloc(n * stride));
        HIPCHK(hipMemcpyAsync(raw.p, cloud, n * stride, hipMemcpyDefault, nullptr));
        hipLaunchKernelGGL(k_aos_to_xyzi4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr,
                           raw.as<unsigned char>(), stride, (int)n, s->d_pts + s->used);
        HIPCHK(hipStreamSynchronize(nullptr));
        HIPCHK(hipGetLastError());
    }
    kf_store_commit(s, n, id_out);
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_kf_store_add_device(lio_kf_store* s, const void* d_cloud, size_t n, size_t stride, int32_t* id_out)
try {
    if (!s || (n && !d_cloud)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (stride < 12 || (stride & 3)) return lio_fail(LIO_ERR_ARG, "stride must be >= 12 and a multiple of 4");
    int rc = check_device(s->device_id);
    if (rc != LIO_OK) return rc;
    if ((rc = kf_store_reserve(s, n)) != LIO_OK) return rc;
    if (n) {
        HIPCHK(hipDeviceSynchronize());                  // the producer of d_cloud may have used any stream
        hipLaunchKernelGGL(k_rec_to_xyzi4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr,
                           (const unsigned char*)d_cloud, stride, (size_t)0, stride >= 20 ? 16 : -1, (int)n, s->d_pts + s->used);
        HIPCHK(hipStreamSynchronize(nullptr));
        HIPCHK(hipGetLastError());
    }
    kf_store_commit(s, n, id_out);
    return LIO_OK;
} LIO_CATCH

int lio_s2m_staged_scan(lio_s2m_handle* h, int scan, const unsigned char** d_rec, size_t* n, size_t* stride, size_t* xyz_off, int* int_off,
                        int* device_id, hipStream_t* stream);   // liogpu_api.hip

extern "C" int lio_kf_store_add_from_handle(lio_kf_store* s, lio_s2m_handle* h, int32_t scan, int32_t* id_out)
try {
    if (!s || !h) return lio_fail(LIO_ERR_ARG, "null argument");
    const unsigned char* rec = nullptr;
    size_t n = 0, stride = 0, xyz_off = 0;
    int dev = 0, int_off = -1;
    hipStream_t st = nullptr;
    int rc = lio_s2m_staged_scan(h, scan, &rec, &n, &stride, &xyz_off, &int_off, &dev, &st);
    if (rc != LIO_OK) return rc;
    if (dev != s->device_id) return lio_fail(LIO_ERR_ARG, "the handle and the keyframe store live on different devices");
    if ((rc = check_device(s->device_id)) != LIO_OK) return rc;
    if ((rc = kf_store_reserve(s, n)) != LIO_OK) return rc;
    if (n) {
        // the intensity sits where the upload said it does (lio_pc2_layout.off_intensity; byte 16 for PCL records; byte 12 for
        // the float4 records lio_s2m_register_raw stages), not at a guessed offset
        hipLaunchKernelGGL(k_rec_to_xyzi4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rec, stride, xyz_off, int_off, (int)n,
                           s->d_pts + s->used);
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
    }
    kf_store_commit(s, n, id_out);
    return LIO_OK;
} LIO_CATCH

// K6 + K7 from selection descriptors already on the device -- src / first / n of every selected keyframe (d_kf, T filled
// here), its pose (d_poses, [roll,pitch,yaw,x,y,z]) and the 256-point chunks of K6 (d_chunks) -- then the map into `h`:
// the common tail of lio_assemble_map_resident and lio_assemble_map_nearby.  `s` is h's stream on the node path, else the
// null stream.
static int assemble_tail(lio_s2m_handle* h, lio_kf_store* st, int n_sel, size_t total, int n_chunks, LioKfDesc* d_kf,
                         const float* d_poses, const int2* d_chunks, hipStream_t s, float leaf, void* out, size_t out_stride, size_t out_cap,
                         size_t* n_out);

extern "C" int lio_assemble_map_resident(lio_s2m_handle* h, lio_kf_store* st, int32_t n_sel, const int32_t* ids,
                                         const float* poses, float leaf, void* out, size_t out_stride, size_t* n_out)
try {
    if (!st || n_sel < 0 || (n_sel && (!ids || !poses))) return lio_fail(LIO_ERR_ARG, "null argument");
    if ((out && (out_stride < 20 || (out_stride & 3))) || !(leaf > 0.0f))
        return lio_fail(LIO_ERR_ARG, "output stride must be >= 20 and a multiple of 4, leaf > 0");
    int rc = check_device(st->device_id);
    if (rc != LIO_OK) return rc;
    size_t total = 0;
    std::vector<LioKfDesc> kf((size_t)n_sel);
    std::vector<int2> chunks;
    for (int k = 0; k < n_sel; ++k) {
        if (ids[k] < 0 || (size_t)ids[k] >= st->off.size()) return lio_fail(LIO_ERR_ARG, "unknown keyframe id");
        kf[k].src = (int)st->off[ids[k]]; kf[k].first = (int)total; kf[k].n = (int)st->cnt[ids[k]]; kf[k].pad = 0;
        for (size_t b = 0; b < st->cnt[ids[k]]; b += 256) chunks.push_back(make_int2(k, (int)b));
        total += st->cnt[ids[k]];
    }
    if (total > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "too many points");
    if (n_out) *n_out = 0;
    const int n_chunks = (int)chunks.size();
    if (lio_s2m_takes_device_map(h)) {
        // The node path (MO:1556-1588 straight into the resident map of `h`): everything on the handle's stream, the
        // temporaries kept in the store, the map's grid laid over the bounding box the voxel filter measured anyway, and no
        // wait at the end -- the registration that follows is ordered behind the build.  The two waits left are the voxel
        // filter's (bounding box, then the number of occupied voxels: both size what comes next).
        hipStream_t s = lio_s2m_stream_of(h);
        st->v_kf.swap(kf);                 // (host arrays of the asynchronous copies live in the store)
        st->v_chunks.swap(chunks);
        HIPCHK(st->d_kf.alloc(sizeof(LioKfDesc) * (size_t)(n_sel ? n_sel : 1)));
        HIPCHK(st->d_poses.alloc(sizeof(float) * 6 * (size_t)(n_sel ? n_sel : 1)));
        HIPCHK(st->d_chunks.alloc(sizeof(int2) * (n_chunks ? n_chunks : 1)));
        if (n_sel) {
            HIPCHK(hipMemcpyAsync(st->d_kf.p, st->v_kf.data(), sizeof(LioKfDesc) * (size_t)n_sel, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(st->d_poses.p, poses, sizeof(float) * 6 * (size_t)n_sel, hipMemcpyHostToDevice, s));
        }
        if (n_chunks) HIPCHK(hipMemcpyAsync(st->d_chunks.p, st->v_chunks.data(), sizeof(int2) * n_chunks, hipMemcpyHostToDevice, s));
        // (`poses` is consumed by the voxel filter's first wait, which follows its copy on the same stream)
        return assemble_tail(h, st, n_sel, total, n_chunks, st->d_kf.as<LioKfDesc>(), st->d_poses.as<float>(), st->d_chunks.as<int2>(),
                             s, leaf, out, out_stride, SIZE_MAX, n_out);
    }
    hipStream_t s = nullptr;
    LioTemp d_kf, d_poses, d_chunks;
    HIPCHK(d_kf.alloc(sizeof(LioKfDesc) * (size_t)(n_sel ? n_sel : 1)));
    HIPCHK(d_poses.alloc(sizeof(float) * 6 * (size_t)(n_sel ? n_sel : 1)));
    HIPCHK(d_chunks.alloc(sizeof(int2) * (n_chunks ? n_chunks : 1)));
    if (n_sel) {
        HIPCHK(hipMemcpyAsync(d_kf.p, kf.data(), sizeof(LioKfDesc) * (size_t)n_sel, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_poses.p, poses, sizeof(float) * 6 * (size_t)n_sel, hipMemcpyHostToDevice, s));
    }
    if (n_chunks) HIPCHK(hipMemcpyAsync(d_chunks.p, chunks.data(), sizeof(int2) * n_chunks, hipMemcpyHostToDevice, s));
    return assemble_tail(h, st, n_sel, total, n_chunks, d_kf.as<LioKfDesc>(), d_poses.as<float>(), d_chunks.as<int2>(), s, leaf, out,
                         out_stride, SIZE_MAX, n_out);
} LIO_CATCH

static int assemble_tail(lio_s2m_handle* h, lio_kf_store* st, int n_sel, size_t total, int n_chunks, LioKfDesc* d_kf,
                         const float* d_poses, const int2* d_chunks, hipStream_t s, float leaf, void* out, size_t out_stride, size_t out_cap,
                         size_t* n_out)
{
    if (n_sel) hipLaunchKernelGGL(k_kf_transforms, dim3((n_sel + 63) / 64), dim3(64), 0, s, d_kf, d_poses, n_sel);
    int rc;
    if (lio_s2m_takes_device_map(h)) {
        HIPCHK(st->world.alloc(total * sizeof(float4)));
        HIPCHK(st->vws.bbox.alloc(6 * sizeof(unsigned)));
        HIPCHK(st->blk_box.alloc(sizeof(float) * 6 * (n_chunks ? n_chunks : 1)));
        if (n_chunks)
            hipLaunchKernelGGL(k_transform_clouds_bbox, dim3((unsigned)n_chunks), dim3(256), 0, s, st->d_pts, d_kf, d_chunks,
                               st->world.as<float4>(), st->blk_box.as<float>());
        hipLaunchKernelGGL(k_bbox_reduce, dim3(1), dim3(256), 0, s, st->blk_box.as<float>(), n_chunks, st->vws.bbox.as<unsigned>());
        int no = 0;
        float box[6];
        rc = voxel_grid_device<LioDevBytes>(st->world.as<float4>(), (int)total, leaf, st->ds, &no, s, st->vws, false, box, true);
        if (rc < 0) return rc;
        const int rc3 = lio_s2m_set_map_device_bbox(h, st->ds.as<float4>(), (size_t)no, box);
        if (rc3 != LIO_OK) return rc3;
        if (out && (size_t)no > out_cap) { if (n_out) *n_out = (size_t)no; return lio_fail(LIO_ERR_ARG, "out holds fewer records than the map (*n_out)"); }
        const int rc2 = copy_out(st->ds.as<float4>(), no, out, out_stride, s);
        if (rc2 < 0) return rc2;
        if (n_out) *n_out = (size_t)no;
        return rc;
    }
    LioTemp world, ds;
    HIPCHK(world.alloc(total * sizeof(float4)));
    if (n_chunks)
        hipLaunchKernelGGL(k_transform_clouds, dim3((unsigned)n_chunks), dim3(256), 0, s, st->d_pts, d_kf, d_chunks, world.as<float4>());
    HIPCHK(hipStreamSynchronize(s));       // (the descriptors may be pool temporaries or host arrays of the caller)
    int no = 0;
    rc = voxel_grid_device(world.as<float4>(), (int)total, leaf, ds, &no, s);
    if (rc < 0) return rc;
    if (h) {                               // (a multi-device or map-sharing handle: through the generic path)
        const int rc3 = lio_s2m_set_map_device_xyzi(h, ds.as<float4>(), (size_t)no);
        if (rc3 != LIO_OK) return rc3;
    }
    if (out && (size_t)no > out_cap) { if (n_out) *n_out = (size_t)no; return lio_fail(LIO_ERR_ARG, "out holds fewer records than the map (*n_out)"); }
    const int rc2 = copy_out(ds.as<float4>(), no, out, out_stride, s);
    if (rc2 < 0) return rc2;
    if (n_out) *n_out = (size_t)no;
    return rc;
}

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

static LioPoseTab pose_tab(lio_kf_store* st)
{
    const size_t c = st->tab_cap;
    const float* f = st->d_tab.as<float>();
    LioPoseTab t = { f, f + c, f + 2 * c, f + 3 * c, f + 4 * c, f + 5 * c, (const double*)(f + 6 * c), (const int*)(f + 8 * c),
                     (const int*)(f + 9 * c) };
    return t;
}

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

extern "C" void lio_nearby_default_config(lio_nearby_config* cfg)
{
    if (!cfg) return;
    cfg->search_radius = 50.0f;      // surroundingKeyframeSearchRadius, UT:316
    cfg->pose_density = 1.0f;        // surroundingKeyframeDensity, UT:314
    cfg->recent_window_s = 10.0;     // MO:1547
}

extern "C" int lio_kf_store_set_poses(lio_kf_store* s, int32_t first, int32_t n, const float* poses, const double* times)
try {
    if (!s || first < 0 || n < 0 || (n && !poses)) return lio_fail(LIO_ERR_ARG, "null argument");
    if ((size_t)first + (size_t)n > s->off.size())
        return lio_fail(LIO_ERR_ARG, "poses for keyframes the store does not hold (add the cloud first)");
    for (int k = 0; k < n; ++k) {
        for (int j = 0; j < 6; ++j)
            if (!std::isfinite(poses[(size_t)k * 6 + j])) return lio_fail(LIO_ERR_ARG, "non-finite key pose");
        if (times ? !std::isfinite(times[k]) : !s->has_time[(size_t)first + k])
            return lio_fail(LIO_ERR_ARG, times ? "non-finite key pose time" : "times == NULL for a keyframe that has no time yet");
    }
    for (int k = 0; k < n; ++k) {                    // host only: whatever is in flight keeps the table it was given
        const size_t i = (size_t)first + k;
        const float* p = poses + (size_t)k * 6;
        s->proll[i] = p[0]; s->ppitch[i] = p[1]; s->pyaw[i] = p[2]; s->px[i] = p[3]; s->py[i] = p[4]; s->pz[i] = p[5];
        if (times) { s->ptime[i] = times[k]; s->has_time[i] = 1; }
        if (!s->has_pose[i]) { s->has_pose[i] = 1; ++s->n_posed; }
    }
    if (n) { s->dirty_lo = std::min(s->dirty_lo, (size_t)first); s->dirty_hi = std::max(s->dirty_hi, (size_t)first + n); }
    return LIO_OK;
} LIO_CATCH

// the dirty range of the key-pose table (and off / cnt) to the device, on stream `s`, through the pinned stage
static int upload_pose_tab(lio_kf_store* st, hipStream_t s)
{
    const size_t N = st->off.size();
    if (N > st->tab_cap) {                           // (growing waits for the device: the old table may still be read)
        st->tab_cap = std::max<size_t>(1024, ((2 * N) + 63) / 64 * 64);
        HIPCHK(st->d_tab.alloc(st->tab_cap * 40));
        st->dirty_lo = 0; st->dirty_hi = N;
    }
    HIPCHK(st->h_stage.grow(0, 4096, hipHostMallocPortable));   // (the stage also receives the selection's counts)
    if (st->dirty_lo >= st->dirty_hi) return LIO_OK;
    const size_t lo = st->dirty_lo, L = std::min(st->dirty_hi, N) - lo;
    // (the stage is idle: every call ends with a wait behind its copies)
    HIPCHK(st->h_stage.grow(L * 40, std::max<size_t>(L * 40 + L * 10, 4096), hipHostMallocPortable));
    float* f = (float*)st->h_stage.p;
    const std::vector<float>* cols[6] = { &st->px, &st->py, &st->pz, &st->proll, &st->ppitch, &st->pyaw };
    for (int c = 0; c < 6; ++c) memcpy(f + c * L, cols[c]->data() + lo, L * sizeof(float));
    memcpy(f + 6 * L, st->ptime.data() + lo, L * sizeof(double));
    int* o = (int*)(f + 8 * L);
    for (size_t k = 0; k < L; ++k) { o[k] = (int)st->off[lo + k]; o[L + k] = (int)st->cnt[lo + k]; }
    float* d = st->d_tab.as<float>();
    const size_t C = st->tab_cap;
    for (int c = 0; c < 6; ++c) HIPCHK(hipMemcpyAsync(d + c * C + lo, f + c * L, L * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync((double*)(d + 6 * C) + lo, f + 6 * L, L * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync((int*)(d + 8 * C) + lo, o, L * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync((int*)(d + 9 * C) + lo, o + L, L * sizeof(int), hipMemcpyHostToDevice, s));
    st->dirty_lo = SIZE_MAX; st->dirty_hi = 0;
    return LIO_OK;
}

// the selection of lio_assemble_map_nearby and of lio_kf_store_global_map (lio_kfstore.h)
int lio_mb_select(lio_kf_store* st, LioNbBufs& b, float R, float density, bool recent, double time_cur, double window, LioNbMeta* hm,
                  hipStream_t s)
{
    int rc;
    const int N = (int)st->off.size();
    if ((rc = vsort_reserve<LioDevBytes>(N, b.cent, b.ws)) != LIO_OK) return rc;
    HIPCHK(b.pts.alloc(sizeof(float4) * (size_t)N));
    HIPCHK(b.cid.alloc(sizeof(unsigned long long) * (size_t)N));
    HIPCHK(b.ids.alloc(sizeof(int) * 2 * (size_t)N));
    HIPCHK(b.meta.alloc(sizeof(LioNbMeta)));
    HIPCHK(b.d_kf.alloc(sizeof(LioKfDesc) * 2 * (size_t)N));    // the list holds at most n_vox + n_recent <= 2N entries
    HIPCHK(b.d_poses.alloc(sizeof(float) * 6 * 2 * (size_t)N));
    const LioPoseTab tab = pose_tab(st);
    LioNbMeta* m = b.meta.as<LioNbMeta>();
    const unsigned nblk = (unsigned)((N + 255) / 256);
    hipLaunchKernelGGL(k_nb_init, dim3(1), dim3(1), 0, s, m);
    const float r2 = (float)((double)R * (double)R);                // what PCL hands FLANN
    if (recent) hipLaunchKernelGGL(k_nb_select<true>, dim3(nblk), dim3(256), 0, s, tab, N, r2, time_cur, window, b.ws.pairs_a.as<uint2>(), m);
    else hipLaunchKernelGGL(k_nb_select<false>, dim3(nblk), dim3(256), 0, s, tab, N, r2, time_cur, window, b.ws.pairs_a.as<uint2>(), m);
    uint2* hits = vsort_pairs<LioDevBytes>(N, 32, s, b.ws);      // (d2, i) ascending, the misses last
    // (an even number of passes ends in pairs_a, where the second sort starts: k_nb_voxkeys rewrites the pairs in place)
    if (hits != b.ws.pairs_a.as<uint2>()) return lio_fail(LIO_ERR_HIP, "radix sort ended in the wrong buffer");
    hipLaunchKernelGGL(k_nb_voxkeys, dim3(nblk), dim3(256), 0, s, tab, N, 1.0f / density, m, hits, b.pts.as<float4>());
    const uint2* vox = vsort_pairs<LioDevBytes>(N, 32, s, b.ws);
    if ((rc = vsort_centroids<LioDevBytes>(b.pts.as<float4>(), vox, N, b.cent, s, b.ws)) != LIO_OK) return rc;
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
    int rc = check_device(st->device_id);
    if (rc != LIO_OK) return rc;
    if (h && h->cfg.device_id != st->device_id)
        return lio_fail(LIO_ERR_ARG, "the handle and the keyframe store live on different devices");
    const int N = (int)st->off.size();
    if (N == 0) return LIO_OK;                       // MO:1592-1593: nothing to extract, the map stays as it is
    if (st->n_posed != (size_t)N) return lio_fail(LIO_ERR_ARG, "a keyframe has no pose (lio_kf_store_set_poses)");
    const bool node = lio_s2m_takes_device_map(h);
    hipStream_t s = node ? lio_s2m_stream_of(h) : nullptr;
    if ((rc = upload_pose_tab(st, s)) != LIO_OK) return rc;
    if (!st->ev_ids) HIPCHK(hipEventCreateWithFlags(&st->ev_ids, hipEventDisableTiming));
    LioNbBufs nb = { st->nws, st->nb_pts, st->nb_cent, st->nb_cid, st->nb_ids, st->nb_meta, st->d_kf, st->d_poses };
    LioNbMeta* hm = (LioNbMeta*)st->h_stage.p;                        // (the stage exists: the first call uploaded through it)
    if ((rc = lio_mb_select(st, nb, R, cfg->pose_density, true, time_cur, cfg->recent_window_s, hm, s)) != LIO_OK) return rc;
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
    if (n_sel) hipLaunchKernelGGL(k_nb_chunks, dim3((unsigned)n_sel), dim3(64), 0, s, st->d_kf.as<LioKfDesc>(), st->d_chunks.as<int2>());
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
    int rc = check_device(h->cfg.device_id);
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
        hipLaunchKernelGGL(k_rec_to_xyzi4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_rec, step, (size_t)layout->off_x,
                           layout->off_intensity >= 0 ? layout->off_intensity : -1, (int)n, w->xyzi.as<float4>());
    }
    w->n_raw = n; w->has_raw = true;                     // (lio_kf_store_sc_add_from_handle reads it on `aux`)
    int no = 0;
    // (the filter's first host wait -- the bounding box -- also covers the H2D copy: the caller's blob is free again)
    rc = voxel_grid_device<LioDevBytes>(w->xyzi.as<float4>(), (int)n, leaf, w->ds, &no, s, w->vws, false, nullptr);
    if (rc < 0) return rc;                               // (rc == 1: PCL would pass the cloud through -- and so did we)
    if (n == 0) HIPCHK(w->ds.alloc(sizeof(float4)));
    // the filter's last kernels (centroids) may still be in flight: the registration on the handle's stream waits for them
    HIPCHK(hipEventRecord(w->ev_done, s));
    HIPCHK(hipStreamWaitEvent(h->stream, w->ev_done, 0));
    h->int_off = 12;                                     // the staged records are float4 (x, y, z, intensity)
    const int rr = lio_s2m_register(h, w->ds.p, (size_t)no, sizeof(float4), pose, res);
    h->int_off = -2;
    if (rr < 0) return rr;
    if (ds_out) { const int rc2 = copy_out(w->ds.as<float4>(), no, ds_out, ds_out_stride, h->stream); if (rc2 < 0) return rc2; }
    if (n_ds) *n_ds = (size_t)no;
    return rr;
} LIO_CATCH

// ------------------------------------------------ loop-closure registration (performRSLoopClosure MO:1098-1143)
// The kernels and the loop are in lio_icp.hip; here are the entry points: they need the store, K6 + K7 and the record
// conversions of this file.

// host records (x,y,z @0,4,8) -> device float4 (x, y, z, 0)
static int icp_upload(const void* pts, size_t n, size_t stride, LioTemp& raw, LioTemp& xyz4, hipStream_t s)
{
    HIPCHK(xyz4.alloc(sizeof(float4) * (n ? n : 1)));
    if (!n) return LIO_OK;
    HIPCHK(raw.alloc(n * stride));
    HIPCHK(hipMemcpyAsync(raw.p, pts, n * stride, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_rec_to_xyzi4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, raw.as<unsigned char>(), stride, (size_t)0, -1, (int)n,
                       xyz4.as<float4>());
    return LIO_OK;
}

static int icp_align_host(int32_t device_id, const void* src, size_t n_src, size_t src_stride, const void* tgt, size_t n_tgt, size_t tgt_stride,
                          const lio_icp_config* cfg, const float* guess, lio_icp_result* res, LioIcpTrace* trace)
{
    if (!res || (n_src && !src) || (n_tgt && !tgt)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (src_stride < 12 || (src_stride & 3) || tgt_stride < 12 || (tgt_stride & 3)) return lio_fail(LIO_ERR_ARG, "strides must be >= 12 and multiples of 4");
    if (n_src > 0x7fffffffull - 1024 || n_tgt > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    int rc = lio_icp_check_config(cfg);
    if (rc != LIO_OK) return rc;
    if ((rc = check_device(device_id)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    LioTemp raw_s, raw_t, d_src, d_tgt;
    if ((rc = icp_upload(src, n_src, src_stride, raw_s, d_src, s)) != LIO_OK) return rc;
    if ((rc = icp_upload(tgt, n_tgt, tgt_stride, raw_t, d_tgt, s)) != LIO_OK) return rc;
    rc = lio_icp_device(d_src.as<float4>(), (int)n_src, d_tgt.as<float4>(), (int)n_tgt, *cfg, guess, res, s, trace, nullptr);
    res->status = rc;
    return rc;
}

extern "C" int lio_icp_align(int32_t device_id, const void* source, size_t n_source, size_t source_stride, const void* target, size_t n_target,
                             size_t target_stride, const lio_icp_config* cfg, const float* guess, lio_icp_result* result)
try {
    return icp_align_host(device_id, source, n_source, source_stride, target, n_target, target_stride, cfg, guess, result, nullptr);
} LIO_CATCH

extern "C" int lio_icp_debug_trace(int32_t device_id, const void* source, size_t n_source, size_t source_stride, const void* target,
                                   size_t n_target, size_t target_stride, const lio_icp_config* cfg, const float* guess, int32_t rec_iter,
                                   lio_icp_result* result, float* steps, int32_t* n_corr, double* mse, int32_t* corr, int32_t* n_trace)
try {
    LioIcpTrace tr;
    tr.step = steps; tr.n_corr = n_corr; tr.mse = mse; tr.corr = corr; tr.rec_iter = rec_iter;
    if (n_trace) *n_trace = 0;
    const int rc = icp_align_host(device_id, source, n_source, source_stride, target, n_target, target_stride, cfg, guess, result, &tr);
    if (n_trace) *n_trace = tr.n_trace;
    return rc;
} LIO_CATCH

// loopFindNearKeyframes MO:1360-1383: the keyframes key - search_num .. key + search_num the store holds, each under its own
// stored pose or all under pose_index's, summed and voxel-filtered -- the h == NULL path of lio_assemble_map_resident with
// those ids and poses, kernel for kernel.  An empty sum stays empty (MO:1375-1376).
static int loop_submap(lio_kf_store* st, int key, int search_num, int pose_index, float leaf, LioTemp& ds, int* n_out, hipStream_t s)
{
    *n_out = 0;
    const int N = (int)st->off.size();
    std::vector<LioKfDesc> kf;
    std::vector<int2> chunks;
    std::vector<float> poses;
    size_t total = 0;
    for (long long i = -(long long)search_num; i <= (long long)search_num; ++i) {
        const long long near = (long long)key + i;
        if (near < 0 || near >= N) continue;
        const size_t id = (size_t)near, pid = pose_index >= 0 ? (size_t)pose_index : id;
        if (!st->has_pose[pid]) return lio_fail(LIO_ERR_ARG, "a keyframe has no pose (lio_kf_store_set_poses)");
        LioKfDesc d;
        d.src = (int)st->off[id]; d.first = (int)total; d.n = (int)st->cnt[id]; d.pad = 0;
        for (int j = 0; j < 12; ++j) d.T[j] = 0.0f;
        for (size_t b = 0; b < st->cnt[id]; b += 256) chunks.push_back(make_int2((int)kf.size(), (int)b));
        kf.push_back(d);
        const float p6[6] = { st->proll[pid], st->ppitch[pid], st->pyaw[pid], st->px[pid], st->py[pid], st->pz[pid] };
        poses.insert(poses.end(), p6, p6 + 6);
        total += st->cnt[id];
    }
    if (total > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "too many points");
    if (total == 0) return LIO_OK;
    const int n_sel = (int)kf.size(), n_chunks = (int)chunks.size();
    LioTemp d_kf, d_poses, d_chunks, world;
    HIPCHK(d_kf.alloc(sizeof(LioKfDesc) * (size_t)n_sel));
    HIPCHK(d_poses.alloc(sizeof(float) * 6 * (size_t)n_sel));
    HIPCHK(d_chunks.alloc(sizeof(int2) * (size_t)n_chunks));
    HIPCHK(world.alloc(total * sizeof(float4)));
    HIPCHK(hipMemcpyAsync(d_kf.p, kf.data(), sizeof(LioKfDesc) * (size_t)n_sel, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_poses.p, poses.data(), sizeof(float) * 6 * (size_t)n_sel, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_chunks.p, chunks.data(), sizeof(int2) * (size_t)n_chunks, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_kf_transforms, dim3((n_sel + 63) / 64), dim3(64), 0, s, d_kf.as<LioKfDesc>(), d_poses.as<float>(), n_sel);
    hipLaunchKernelGGL(k_transform_clouds, dim3((unsigned)n_chunks), dim3(256), 0, s, st->d_pts, d_kf.as<LioKfDesc>(), d_chunks.as<int2>(),
                       world.as<float4>());
    HIPCHK(hipStreamSynchronize(s));                       // (the descriptors are host arrays of this function)
    const int rc = voxel_grid_device(world.as<float4>(), (int)total, leaf, ds, n_out, s);
    return rc < 0 ? rc : LIO_OK;                           // (1 = the leaf overflows PCL's voxel index: the sum passes through, as in PCL)
}

extern "C" int lio_kf_store_loop_icp(lio_kf_store* st, int32_t key_cur, int32_t key_pre, int32_t search_num, int32_t pose_index, float leaf,
                                     const lio_icp_config* cfg, lio_icp_result* res, lio_icp_clouds* clouds)
try {
    if (!st || !res) return lio_fail(LIO_ERR_ARG, "null argument");
    int rc = lio_icp_check_config(cfg);
    if (rc != LIO_OK) return rc;
    const int N = (int)st->off.size();
    if (key_cur < 0 || key_cur >= N || key_pre < 0 || key_pre >= N || search_num < 0 || pose_index < -1 || pose_index >= N || !(leaf > 0.0f))
        return lio_fail(LIO_ERR_ARG, "key_cur, key_pre and pose_index must name keyframes of the store; search_num >= 0; leaf > 0");
    if (!st->has_pose[(size_t)key_cur]) return lio_fail(LIO_ERR_ARG, "a keyframe has no pose (lio_kf_store_set_poses)");
    if (clouds && (clouds->stride < 20 || (clouds->stride & 3))) return lio_fail(LIO_ERR_ARG, "output stride must be >= 20 and a multiple of 4");
    if ((rc = check_device(st->device_id)) != LIO_OK) return rc;
    memset(res, 0, sizeof(*res));
    hipStream_t s = nullptr;
    LioTemp src, tgt, closed;
    int n_src = 0, n_tgt = 0;
    if ((rc = loop_submap(st, key_cur, 0, pose_index, leaf, src, &n_src, s)) != LIO_OK) return rc;
    if ((rc = loop_submap(st, key_pre, search_num, pose_index, leaf, tgt, &n_tgt, s)) != LIO_OK) return rc;
    res->n_source = n_src; res->n_target = n_tgt;
    if (clouds) {
        clouds->n_source = (size_t)n_src; clouds->n_target = (size_t)n_tgt; clouds->n_closed = 0;
        if ((clouds->source && clouds->cap_source < (size_t)n_src) || (clouds->target && clouds->cap_target < (size_t)n_tgt))
            return lio_fail(LIO_ERR_ARG, "a submap holds more records than its output (n_source, n_target)");
        if (clouds->source && (rc = copy_out(src.as<float4>(), n_src, clouds->source, clouds->stride, s)) < 0) return rc;
        if (clouds->target && (rc = copy_out(tgt.as<float4>(), n_tgt, clouds->target, clouds->stride, s)) < 0) return rc;
    }
    if (n_src < cfg->min_source_points || n_tgt < cfg->min_target_points) {                  // MO:1104
        res->status = LIO_TOO_FEW_POINTS;
        res->state = LIO_ICP_NOT_CONVERGED;
        res->fitness = DBL_MAX;
        for (int i = 0; i < 16; i += 5) res->T[i] = 1.0f;
        return LIO_TOO_FEW_POINTS;
    }
    const bool want_closed = clouds && clouds->closed;
    if (want_closed) {
        clouds->n_closed = (size_t)n_src;
        if (clouds->cap_closed < (size_t)n_src) return lio_fail(LIO_ERR_ARG, "closed holds fewer records than the source submap (n_closed)");
        HIPCHK(closed.alloc(sizeof(float4) * (size_t)(n_src ? n_src : 1)));
    }
    rc = lio_icp_device(src.as<float4>(), n_src, tgt.as<float4>(), n_tgt, *cfg, nullptr, res, s, nullptr, want_closed ? closed.as<float4>() : nullptr);
    res->status = rc;
    if (rc != LIO_OK) return rc;
    if (want_closed && (rc = copy_out(closed.as<float4>(), n_src, clouds->closed, clouds->stride, s)) < 0) return rc;
    // tCorrect = correctionLidarFrame * tWrong, then pcl::getTranslationAndEulerAngles (MO:1136-1143); host, fp64 from the
    // fp32 inputs, rounded once
    {
        const size_t k = (size_t)key_cur;
        const double A = cos((double)st->pyaw[k]), B = sin((double)st->pyaw[k]), Cc = cos((double)st->ppitch[k]), D = sin((double)st->ppitch[k]),
                     E = cos((double)st->proll[k]), F = sin((double)st->proll[k]), DE = D * E, DF = D * F;
        const double W[16] = { A * Cc, A * DF - B * E, B * F + A * DE, (double)st->px[k],
                               B * Cc, A * E + B * DF, B * DE - A * F, (double)st->py[k],
                               -D, Cc * F, Cc * E, (double)st->pz[k], 0.0, 0.0, 0.0, 1.0 };
        double Tc[16];
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) {
                double v = 0.0;
                for (int j = 0; j < 4; ++j) v += (double)res->T[4 * a + j] * W[4 * j + b];
                Tc[4 * a + b] = v;
            }
        res->pose_corrected[0] = (float)atan2(Tc[9], Tc[10]);
        res->pose_corrected[1] = (float)asin(-Tc[8]);
        res->pose_corrected[2] = (float)atan2(Tc[4], Tc[0]);
        res->pose_corrected[3] = (float)Tc[3]; res->pose_corrected[4] = (float)Tc[7]; res->pose_corrected[5] = (float)Tc[11];
    }
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_kf_store_detect_loop(lio_kf_store* st, float radius, double time_diff, double time_cur, int32_t* key_cur, int32_t* key_pre)
try {
    if (!st || !key_cur || !key_pre) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!(radius > 0.0f) || !std::isfinite(radius) || !std::isfinite(time_diff) || !std::isfinite(time_cur))
        return lio_fail(LIO_ERR_ARG, "radius > 0 and finite; time_diff, time_cur finite");
    *key_cur = -1; *key_pre = -1;
    const int N = (int)st->off.size();
    if (N == 0) return 0;                                  // MO:1083-1084
    for (int i = 0; i < N; ++i)
        if (!st->has_pose[(size_t)i] || !st->has_time[(size_t)i]) return lio_fail(LIO_ERR_ARG, "a keyframe has no pose or no time (lio_kf_store_set_poses)");
    const int last = N - 1;
    const float r2 = (float)((double)radius * (double)radius);          // what PCL hands FLANN
    const float lx = st->px[(size_t)last], ly = st->py[(size_t)last], lz = st->pz[(size_t)last];
    // the radius set is visited in (d2, index) order; only its first entry that is old enough matters
    int best = -1;
    float best_d2 = 0.0f;
    for (int i = 0; i < N; ++i) {
        const float dx = st->px[(size_t)i] - lx, dy = st->py[(size_t)i] - ly, dz = st->pz[(size_t)i] - lz;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (!(d2 < r2)) continue;
        if (!(std::fabs(st->ptime[(size_t)i] - time_cur) > time_diff)) continue;            // MO:1290
        if (best < 0 || d2 < best_d2) { best = i; best_d2 = d2; }
    }
    if (best < 0 || best == last) return 0;               // MO:1297-1298
    *key_cur = last; *key_pre = best;
    return 1;
} LIO_CATCH

// ------------------------------------------------ Scan Context loop detection (performSCLoopClosure MO:1163-1269)
// The kernels and the detection are in lio_sc.hip; here are the entry points that need the store and the staged raw cloud.
extern "C" int lio_kf_store_sc_add(lio_kf_store* s, const void* cloud, size_t n, size_t stride, const lio_sc_config* cfg, int32_t* id_out)
try {
    if (!s || (n && !cloud)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (stride < 12 || (stride & 3)) return lio_fail(LIO_ERR_ARG, "stride must be >= 12 and a multiple of 4");
    if (n > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    int rc = check_device(s->device_id);
    if (rc != LIO_OK) return rc;
    LioTemp raw;
    if (n) {
        HIPCHK(raw.alloc(n * stride));
        HIPCHK(hipMemcpyAsync(raw.p, cloud, n * stride, hipMemcpyDefault, nullptr));
    }
    return lio_sc_store_append(s->sc, raw.as<unsigned char>(), stride, 0, n, cfg, nullptr, id_out);
} LIO_CATCH

extern "C" int lio_kf_store_sc_add_device(lio_kf_store* s, const void* d_cloud, size_t n, size_t stride, const lio_sc_config* cfg, int32_t* id_out)
try {
    if (!s || (n && !d_cloud)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (stride < 12 || (stride & 3)) return lio_fail(LIO_ERR_ARG, "stride must be >= 12 and a multiple of 4");
    if ((uintptr_t)d_cloud & 3) return lio_fail(LIO_ERR_ARG, "d_cloud must be aligned to 4 bytes");      // k_sc_fold reads it as floats
    int rc = check_device(s->device_id);
    if (rc != LIO_OK) return rc;
    if (n) HIPCHK(hipDeviceSynchronize());               // the producer of d_cloud may have used any stream
    return lio_sc_store_append(s->sc, (const unsigned char*)d_cloud, stride, 0, n, cfg, nullptr, id_out);
} LIO_CATCH

// thisRawCloudKeyFrame of MO:2149-2156 is cloud_info.cloud_deskewed: the cloud lio_s2m_register_raw has just turned into
// float4 records on the handle (before the voxel filter).  Read where it lies, on the stream that wrote it.
extern "C" int lio_kf_store_sc_add_from_handle(lio_kf_store* s, lio_s2m_handle* h, const lio_sc_config* cfg, int32_t* id_out)
try {
    if (!s || !h) return lio_fail(LIO_ERR_ARG, "null argument");
    if (h->cfg.device_id != s->device_id) return lio_fail(LIO_ERR_ARG, "the handle and the keyframe store live on different devices");
    if (h->multi || !h->raw_ws || !h->raw_ws->has_raw) return lio_fail(LIO_ERR_ARG, "the handle holds no cloud staged by lio_s2m_register_raw");
    int rc = check_device(s->device_id);
    if (rc != LIO_OK) return rc;
    LioRawWs* w = h->raw_ws;
    return lio_sc_store_append(s->sc, w->xyzi.as<unsigned char>(), sizeof(float4), 0, w->n_raw, cfg, w->aux, id_out);
} LIO_CATCH

extern "C" int lio_kf_store_sc_count(const lio_kf_store* s)
try {
    return s ? (int)s->sc.count : 0;
} LIO_CATCH

extern "C" int lio_kf_store_sc_geometry(const lio_kf_store* s, int32_t* num_rings, int32_t* num_sectors)
try {
    if (!s || !num_rings || !num_sectors) return lio_fail(LIO_ERR_ARG, "null argument");
    *num_rings = s->sc.count ? s->sc.rings : 0;
    *num_sectors = s->sc.count ? s->sc.sectors : 0;
    return LIO_OK;
} LIO_CATCH

extern "C" int lio_kf_store_sc_get(lio_kf_store* s, int32_t id, float* desc, float* ring_key, double* sector_key)
try {
    if (!s) return lio_fail(LIO_ERR_ARG, "null argument");
    int rc = check_device(s->device_id);
    if (rc != LIO_OK) return rc;
    return lio_sc_store_get(s->sc, id, desc, ring_key, sector_key);
} LIO_CATCH

extern "C" int lio_kf_store_sc_detect(lio_kf_store* s, const lio_sc_config* cfg, lio_sc_result* res)
try {
    if (!s || !res) return lio_fail(LIO_ERR_ARG, "null argument");
    int rc = check_device(s->device_id);
    if (rc != LIO_OK) return rc;
    rc = lio_sc_store_detect(s->sc, cfg, res, nullptr);
    res->status = rc;
    return rc;
} LIO_CATCH

// ------------------------------------------------ planning local map (publishLocalMap MO:2442-2541)
// The crop and the outlier filter are in lio_localmap.hip; here are the entry points: they need the store, K6 + K7 and the
// record conversions of this file.
extern "C" int lio_sor_filter(int32_t device_id, const void* pts, size_t n, size_t stride, int32_t mean_k, float stddev_mul, void* out,
                              size_t out_stride, size_t* n_out, float* mean_dist, double stats[3])
try {
    if (!n_out || (n && !pts)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (stride < 12 || (stride & 3) || (out && (out_stride < 20 || (out_stride & 3))))
        return lio_fail(LIO_ERR_ARG, "stride must be >= 12, the output stride >= 20, both multiples of 4");
    if (n > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    int rc = lio_sor_check(mean_k, stddev_mul);
    if (rc != LIO_OK) return rc;
    *n_out = 0;
    if (stats) { stats[0] = 0.0; stats[1] = 0.0; stats[2] = INFINITY; }
    if (n == 0) return 1;                                  // nothing to filter: the pass-through of at most mean_k points
    if ((rc = check_device(device_id)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    LioTemp raw, xyzi, inl, dist;
    HIPCHK(raw.alloc(n * stride));
    HIPCHK(xyzi.alloc(n * sizeof(float4)));
    if (mean_dist) HIPCHK(dist.alloc(n * sizeof(float)));
    HIPCHK(hipMemcpyAsync(raw.p, pts, n * stride, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_rec_to_xyzi4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, raw.as<unsigned char>(), stride, (size_t)0,
                       stride >= 20 ? 16 : -1, (int)n, xyzi.as<float4>());
    int no = 0;
    LioSorReport rep;
    rc = lio_sor_device(xyzi.as<float4>(), (int)n, mean_k, stddev_mul, inl, &no, mean_dist ? dist.as<float>() : nullptr, &rep, s);
    if (rc < 0) return rc;
    if (mean_dist) HIPCHK(hipMemcpyAsync(mean_dist, dist.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
    const int rc2 = copy_out(inl.as<float4>(), no, out, out_stride, s);
    if (rc2 < 0) return rc2;
    HIPCHK(hipStreamSynchronize(s));
    if (stats) { stats[0] = rep.mean; stats[1] = rep.stddev; stats[2] = rep.threshold; }
    *n_out = (size_t)no;
    return rc;
} LIO_CATCH

extern "C" void lio_local_map_default_config(lio_local_map_config* cfg)
{
    if (!cfg) return;
    cfg->n_keyframes = 30;                                 // localMapKeyFramesNumber, UT:219
    cfg->front = 70.0f; cfg->left = 40.0f; cfg->back = 20.0f; cfg->right = 40.0f;        // UT:220-223
    cfg->remove_outliers = 1;                              // useRemovingOutliers, UT:227
    cfg->mean_k = 10;                                      // meanK, UT:228
    cfg->stddev_mul = 1.0f;                                // stddevThreshold, UT:229
    cfg->downsample = 1;                                   // useDownSamplingLocalMap, UT:224
    cfg->leaf = 0.01f;                                     // localMappingSurfLeafSize, UT:226
}

namespace {
struct LocalMapBufs { LioTemp d_kf, d_poses, d_chunks, world, cropped, inl, ds; };

// MO:2447-2540 up to the cloud on the device: *cur / *n_cur = the local map in B (null / 0 for an empty store or an empty
// sum), complete when this returns.  What lio_kf_store_local_map copies out and lio_kf_store_height_map goes on with.
int local_map_device(lio_kf_store* st, const lio_local_map_config* cfg, const float* pose, LocalMapBufs& B, const float4** cur_out,
                     int* n_cur_out, size_t* n_out, lio_local_map_info* info, hipStream_t s)
{
    LioTemp &d_kf = B.d_kf, &d_poses = B.d_poses, &d_chunks = B.d_chunks, &world = B.world, &cropped = B.cropped, &inl = B.inl, &ds = B.ds;
    *cur_out = nullptr; *n_cur_out = 0;
    if (cfg->n_keyframes < 1) return lio_fail(LIO_ERR_ARG, "n_keyframes must be >= 1");
    if (!std::isfinite(cfg->front) || !std::isfinite(cfg->left) || !std::isfinite(cfg->back) || !std::isfinite(cfg->right) ||
        !(-cfg->left <= cfg->right) || !(-cfg->back <= cfg->front))
        return lio_fail(LIO_ERR_ARG, "front, left, back, right must be finite with -left <= right and -back <= front");
    if ((cfg->remove_outliers != 0 && cfg->remove_outliers != 1) || (cfg->downsample != 0 && cfg->downsample != 1))
        return lio_fail(LIO_ERR_ARG, "remove_outliers and downsample are 0 or 1");
    int rc = lio_sor_check(cfg->mean_k, cfg->stddev_mul);
    if (rc != LIO_OK) return rc;
    if (!(cfg->leaf > 0.0f) || !std::isfinite(cfg->leaf)) return lio_fail(LIO_ERR_ARG, "leaf must be positive and finite");
    for (int j = 0; j < 6; ++j) if (!std::isfinite(pose[j])) return lio_fail(LIO_ERR_ARG, "non-finite pose");
    if (n_out) *n_out = 0;
    if (info) memset(info, 0, sizeof(*info));
    if ((rc = check_device(st->device_id)) != LIO_OK) return rc;
    const int N = (int)st->off.size();
    if (N == 0) return LIO_OK;                             // MO:2444-2445
    const int first = N < cfg->n_keyframes ? 0 : N - cfg->n_keyframes;                     // startPoseNum, MO:2462
    // ---- K6 over first .. N - 1 under the stored poses: the h == NULL path of lio_assemble_map_resident, kernel for kernel
    std::vector<LioKfDesc> kf;
    std::vector<int2> chunks;
    std::vector<float> poses;
    size_t total = 0;
    for (int id = first; id < N; ++id) {
        if (!st->has_pose[(size_t)id]) return lio_fail(LIO_ERR_ARG, "a keyframe has no pose (lio_kf_store_set_poses)");
        LioKfDesc d;
        d.src = (int)st->off[(size_t)id]; d.first = (int)total; d.n = (int)st->cnt[(size_t)id]; d.pad = 0;
        for (int j = 0; j < 12; ++j) d.T[j] = 0.0f;
        for (size_t b = 0; b < st->cnt[(size_t)id]; b += 256) chunks.push_back(make_int2((int)kf.size(), (int)b));
        kf.push_back(d);
        const float p6[6] = { st->proll[(size_t)id], st->ppitch[(size_t)id], st->pyaw[(size_t)id], st->px[(size_t)id], st->py[(size_t)id], st->pz[(size_t)id] };
        poses.insert(poses.end(), p6, p6 + 6);
        total += st->cnt[(size_t)id];
    }
    if (total > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "too many points");
    if (info) { info->first_keyframe = first; info->n_keyframes = N - first; info->n_summed = (int)total; }
    if (total == 0) return LIO_OK;
    const int n_sel = (int)kf.size(), n_chunks = (int)chunks.size();
    HIPCHK(d_kf.alloc(sizeof(LioKfDesc) * (size_t)n_sel));
    HIPCHK(d_poses.alloc(sizeof(float) * 6 * (size_t)n_sel));
    HIPCHK(d_chunks.alloc(sizeof(int2) * (size_t)n_chunks));
    HIPCHK(world.alloc(total * sizeof(float4)));
    HIPCHK(hipMemcpyAsync(d_kf.p, kf.data(), sizeof(LioKfDesc) * (size_t)n_sel, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_poses.p, poses.data(), sizeof(float) * 6 * (size_t)n_sel, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_chunks.p, chunks.data(), sizeof(int2) * (size_t)n_chunks, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_kf_transforms, dim3((n_sel + 63) / 64), dim3(64), 0, s, d_kf.as<LioKfDesc>(), d_poses.as<float>(), n_sel);
    hipLaunchKernelGGL(k_transform_clouds, dim3((unsigned)n_chunks), dim3(256), 0, s, st->d_pts, d_kf.as<LioKfDesc>(), d_chunks.as<int2>(),
                       world.as<float4>());
    // ---- vehicle frame + the two pass-throughs (the wait for the count also covers the descriptors' copies)
    float M[12];
    lio_local_map_vehicle_frame(pose, M);
    int n_cur = 0;
    if ((rc = lio_crop_device(world.as<float4>(), (int)total, M, cfg->front, cfg->left, cfg->back, cfg->right, cropped, &n_cur, s)) != LIO_OK)
        return rc;
    const float4* cur = cropped.as<float4>();
    if (info) info->n_cropped = n_cur;
    if (cfg->remove_outliers) {                            // MO:2510-2516
        LioSorReport rep;
        int n_inl = 0;
        if ((rc = lio_sor_device(cur, n_cur, cfg->mean_k, cfg->stddev_mul, inl, &n_inl, nullptr, &rep, s)) < 0) return rc;
        cur = inl.as<float4>(); n_cur = n_inl;
        if (info) { info->sor_mean = rep.mean; info->sor_stddev = rep.stddev; info->sor_threshold = rep.threshold; }
    }
    if (info) info->n_inliers = n_cur;
    if (cfg->downsample) {                                 // MO:2517-2540
        int n_ds = 0;
        if ((rc = voxel_grid_device(cur, n_cur, cfg->leaf, ds, &n_ds, s)) < 0) return rc;
        if (info) info->voxel_passthrough = rc == 1 ? 1 : 0;
        if (n_cur > 0) { cur = ds.as<float4>(); n_cur = n_ds; }
    }
    if (info) info->n_out = n_cur;
    if (n_out) *n_out = (size_t)n_cur;
    *cur_out = cur; *n_cur_out = n_cur;
    return LIO_OK;
}
}  // namespace

extern "C" int lio_kf_store_local_map(lio_kf_store* st, const lio_local_map_config* cfg, const float* pose, void* out, size_t out_stride,
                                      size_t out_cap, size_t* n_out, lio_local_map_info* info)
try {
    if (!st || !cfg || !pose) return lio_fail(LIO_ERR_ARG, "null argument");
    if (out && (out_stride < 20 || (out_stride & 3))) return lio_fail(LIO_ERR_ARG, "output stride must be >= 20 and a multiple of 4");
    hipStream_t s = nullptr;
    LocalMapBufs B;
    const float4* cur = nullptr;
    int n_cur = 0;
    int rc = local_map_device(st, cfg, pose, B, &cur, &n_cur, n_out, info, s);
    if (rc != LIO_OK) return rc;
    if (out && (size_t)n_cur > out_cap) return lio_fail(LIO_ERR_ARG, "out holds fewer records than the local map (*n_out)");
    if ((rc = copy_out(cur, n_cur, out, out_stride, s)) < 0) return rc;
    return LIO_OK;
} LIO_CATCH

// ------------------------------------------------ planning height map (grid_map_pcl's loader, helpers.cpp:97-105)
// The kernels are in lio_heightmap.hip; here is the chain (it needs the outlier filter, K7 and K7's sort) and the entry points.
extern "C" void lio_height_map_default_config(lio_height_map_config* cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->roll = 0.0f; cfg->pitch = 0.0f;
    cfg->level_and_ego_filter = 1;                         // GridMapPclLoader.cpp:80-85
    cfg->remove_outliers = 1; cfg->mean_k = 10; cfg->stddev_mul = 1.0f;                  // parameters.yaml outlier_removal
    cfg->downsample = 0; cfg->voxel[0] = cfg->voxel[1] = cfg->voxel[2] = 0.1f;           // downsampling
    cfg->resolution = 0.2;                                 // grid_map
    cfg->min_points_per_cell = 1; cfg->max_points_per_cell = 1000000000;
    cfg->use_cluster = 0; cfg->cluster_tolerance = 1.0f;   // cluster_extraction
    cfg->cluster_min_points = 1; cfg->cluster_max_points = 1000000000; cfg->use_max_height = 0;
    cfg->fill_holes = 0;                                   // the reference as written
}

namespace {
int height_map_check(const lio_height_map_config* c)
{
    const int32_t flags[] = { c->level_and_ego_filter, c->remove_outliers, c->downsample, c->use_cluster, c->use_max_height, c->fill_holes };
    for (int32_t f : flags)
        if (f != 0 && f != 1) return lio_fail(LIO_ERR_ARG, "the flags of lio_height_map_config are 0 or 1");
    if (!std::isfinite(c->roll) || !std::isfinite(c->pitch)) return lio_fail(LIO_ERR_ARG, "roll and pitch must be finite");
    if (!(c->resolution >= 1e-4) || !std::isfinite(c->resolution)) return lio_fail(LIO_ERR_ARG, "resolution must be at least 1e-4");
    int rc = lio_sor_check(c->mean_k, c->stddev_mul);
    if (rc != LIO_OK) return rc;
    if (c->downsample) {                                   // K7 takes one leaf
        if (!(c->voxel[0] > 0.0f) || !std::isfinite(c->voxel[0]) || c->voxel[1] != c->voxel[0] || c->voxel[2] != c->voxel[0])
            return lio_fail(LIO_ERR_ARG, "downsample needs one positive, finite voxel size on all three axes");
    }
    if (c->min_points_per_cell < 0 || c->max_points_per_cell < 0 || c->cluster_min_points < 0 || c->cluster_max_points < 0)
        return lio_fail(LIO_ERR_ARG, "point counts must not be negative");
    if (c->use_cluster && (!(c->cluster_tolerance >= 0.0f) || !std::isfinite(c->cluster_tolerance)))
        return lio_fail(LIO_ERR_ARG, "cluster_tolerance must be finite and not negative");
    return LIO_OK;
}

// helpers.cpp:97-105 on a device-resident float4 cloud (w is not read): the reference's order, everything on the device, the
// grid copy last.  Host waits, each for a number that sizes the next launch: outlier filter 3 (box, grid choice, compaction
// count), voxel filter 2, ego filter 1, the box, and the grid copy with the counters.  `keep` (optional) receives the device
// grid, which is then built whether or not `grid` is given.
int height_map_device(const float4* d_in, int n, const lio_height_map_config* cfg, float* grid, size_t grid_cap, lio_height_map_info* info,
                      hipStream_t s, LioTemp* keep = nullptr)
{
    int rc;
    const float4* cur = d_in;
    int n_cur = n;
    LioTemp inl, ds, lev;
    info->n_in = n;
    if (cfg->remove_outliers) {                            // PointcloudProcessor.cpp:62-70
        LioSorReport rep;
        int n_inl = 0;
        if ((rc = lio_sor_device(cur, n_cur, cfg->mean_k, cfg->stddev_mul, inl, &n_inl, nullptr, &rep, s)) < 0) return rc;
        cur = inl.as<float4>(); n_cur = n_inl;
    }
    info->n_inliers = n_cur;
    if (cfg->downsample && n_cur > 0) {                    // PointcloudProcessor.cpp:114-122
        int n_ds = 0;
        if ((rc = voxel_grid_device(cur, n_cur, cfg->voxel[0], ds, &n_ds, s)) < 0) return rc;
        info->voxel_passthrough = rc == 1 ? 1 : 0;
        cur = ds.as<float4>(); n_cur = n_ds;
    }
    float R1[9], R2[9];
    lio_hm_rotations(cfg->roll, cfg->pitch, R1, R2);
    int n_lev = 0;
    if ((rc = lio_hm_level_ego(cur, n_cur, R1, R2, cfg->level_and_ego_filter, lev, &n_lev, s)) != LIO_OK) return rc;
    cur = lev.as<float4>(); n_cur = n_lev;
    info->n_filtered = n_cur;
    if (n_cur == 0) return LIO_OK;                         // no point: no grid
    float mn[3], mx[3];
    LioTemp bbox;                                          // K7's box pass (k_vox_bbox)
    if ((rc = cloud_box_launch(cur, n_cur, bbox, s)) != LIO_OK) return rc;
    if ((rc = cloud_box_wait(bbox, mn, mx, s)) != LIO_OK) return rc;
    HIPCHK(hipGetLastError());
    LioHmGeom g;
    lio_hm_geometry(mn, mx, cfg->resolution, &g);
    info->rows = g.rows; info->cols = g.cols;
    for (int a = 0; a < 2; ++a) { info->length[a] = g.length[a]; info->position[a] = g.position[a]; }
    if (g.rows == 0 || g.cols == 0) return LIO_OK;         // (the reference asserts in GridMap::setGeometry)
    if ((long long)g.rows * g.cols > 0x7fffffffLL - 1024) return lio_fail(LIO_ERR_CAPACITY, "the grid has more than 2^31 cells");
    const size_t n_cells = (size_t)g.rows * (size_t)g.cols;
    if (!grid && !keep) return LIO_OK;                     // the geometry only
    if (grid && n_cells > grid_cap) return lio_fail(LIO_ERR_ARG, "grid holds fewer cells than rows x cols (info)");
    // ---- cells: keys, K7's stable sort (the key space: the cells and one key behind them), then lio_hm_grid
    LioVoxWs<LioTemp> ws;
    LioTemp counters;
    const int n_blocks = (n_cur + LIO_VS_THREADS * 4 - 1) / (LIO_VS_THREADS * 4);
    HIPCHK(ws.pairs_a.alloc(sizeof(uint2) * (size_t)n_cur));
    HIPCHK(ws.pairs_b.alloc(sizeof(uint2) * (size_t)n_cur));
    HIPCHK(ws.hist.alloc(sizeof(int) * (size_t)LIO_VS_BINS * n_blocks));
    HIPCHK(ws.row_total.alloc(sizeof(int) * LIO_VS_BINS));
    HIPCHK(counters.alloc(4 * sizeof(int)));
    HIPCHK(hipMemsetAsync(counters.p, 0, 4 * sizeof(int), s));
    lio_hm_launch_keys(cur, n_cur, g, ws.pairs_a.as<uint2>(), counters.as<int>(), s);
    int bits = 1;
    while (bits < 31 && (1LL << bits) < (long long)n_cells + 1) ++bits;
    const uint2* sorted = vsort_pairs<LioTemp>(n_cur, bits, s, ws);
    int hc[3] = { 0, 0, 0 };
    if ((rc = lio_hm_grid(cur, sorted, n_cur, g, cfg, grid, counters.as<int>(), hc, s, keep)) != LIO_OK) return rc;
    info->n_binned = hc[0]; info->n_valid_cells = hc[1]; info->n_filled_cells = hc[2];
    return LIO_OK;
}
}  // namespace

extern "C" int lio_height_map(int32_t device_id, const void* pts, size_t n, size_t stride, const lio_height_map_config* cfg, float* grid,
                              size_t grid_cap, lio_height_map_info* info)
try {
    if (!cfg || !info || (n && !pts)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (stride < 12 || (stride & 3)) return lio_fail(LIO_ERR_ARG, "stride must be >= 12 and a multiple of 4");
    if (n > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    int rc = height_map_check(cfg);
    if (rc != LIO_OK) return rc;
    memset(info, 0, sizeof(*info));
    if (n == 0) return LIO_OK;                             // an empty cloud: rows = cols = 0
    if ((rc = check_device(device_id)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    LioTemp raw, xyzi;
    HIPCHK(raw.alloc(n * stride));
    HIPCHK(xyzi.alloc(n * sizeof(float4)));
    HIPCHK(hipMemcpyAsync(raw.p, pts, n * stride, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_rec_to_xyzi4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, raw.as<unsigned char>(), stride, (size_t)0, -1, (int)n,
                       xyzi.as<float4>());
    rc = height_map_device(xyzi.as<float4>(), (int)n, cfg, grid, grid_cap, info, s);
    const hipError_t e = hipStreamSynchronize(s);          // (an early return: `raw` goes back to the pool when this returns)
    if (rc < 0) return rc;                                 // the chain's own error comes first
    HIPCHK(e);
    return rc;
} LIO_CATCH

extern "C" int lio_kf_store_height_map(lio_kf_store* st, const lio_local_map_config* lm, const float* pose, const lio_height_map_config* cfg,
                                       float* grid, size_t grid_cap, lio_local_map_info* lm_info, lio_height_map_info* info)
try {
    if (!st || !lm || !pose || !cfg || !info) return lio_fail(LIO_ERR_ARG, "null argument");
    int rc = height_map_check(cfg);
    if (rc != LIO_OK) return rc;
    memset(info, 0, sizeof(*info));
    hipStream_t s = nullptr;
    LocalMapBufs B;
    const float4* cur = nullptr;
    int n_cur = 0;
    if ((rc = local_map_device(st, lm, pose, B, &cur, &n_cur, nullptr, lm_info, s)) != LIO_OK) return rc;
    if (n_cur == 0) return LIO_OK;                         // an empty store or an empty crop: rows = cols = 0
    return height_map_device(cur, n_cur, cfg, grid, grid_cap, info, s);
} LIO_CATCH

// The height map's chain, then the terrain layers (lio_terrain.hip) on the device grid it leaves: the same null stream, complete
// on return.
extern "C" int lio_kf_store_terrain_map(lio_kf_store* st, const lio_local_map_config* lm, const float* pose, const lio_height_map_config* hm,
                                        const lio_terrain_config* cfg, float* grid, size_t grid_cap, float* layers, size_t layers_cap,
                                        lio_local_map_info* lm_info, lio_height_map_info* hm_info, lio_terrain_info* info)
try {
    if (!st || !lm || !pose || !hm || !cfg || !hm_info || !info) return lio_fail(LIO_ERR_ARG, "null argument");
    int rc = height_map_check(hm);
    if (rc != LIO_OK) return rc;
    LioTerrPlan plan;
    if ((rc = lio_terrain_check(cfg, hm->resolution, &plan)) != LIO_OK) return rc;
    memset(hm_info, 0, sizeof(*hm_info));
    memset(info, 0, sizeof(*info));
    info->normal_method_used = plan.method_used; info->edge_window_size = plan.window;
    hipStream_t s = nullptr;
    LocalMapBufs B;
    const float4* cur = nullptr;
    int n_cur = 0;
    if ((rc = local_map_device(st, lm, pose, B, &cur, &n_cur, nullptr, lm_info, s)) != LIO_OK) return rc;
    if (n_cur == 0) return LIO_OK;                         // an empty store or an empty crop: rows = cols = 0
    LioTemp d_grid;
    rc = height_map_device(cur, n_cur, hm, grid, grid_cap, hm_info, s, &d_grid);
    info->rows = hm_info->rows; info->cols = hm_info->cols;
    if (rc != LIO_OK) return rc;
    if (!d_grid.p) return LIO_OK;                          // no point left or no extent along an axis: no grid, no layers
    const size_t n_cells = (size_t)info->rows * (size_t)info->cols;
    if (layers && (size_t)plan.n_out * n_cells > layers_cap) return lio_fail(LIO_ERR_ARG, "layers holds fewer floats than the requested layers (info)");
    if ((rc = lio_terrain_set_geometry(&plan, info->rows, info->cols, hm->resolution, hm_info->length, hm_info->position)) != LIO_OK) return rc;
    return lio_terrain_device(d_grid.as<float>(), plan, layers, info, s);
} LIO_CATCH

// ------------------------------------------------ for lio_globalmap.hip (lio_kfstore.h): the global map, the map export,
// the keyframe read-back and the registered clouds run this file's kernels through these launches
int lio_mb_check_device(int device_id) { return check_device(device_id); }
int lio_mb_upload_pose_tab(lio_kf_store* st, hipStream_t s) { return upload_pose_tab(st, s); }

void lio_mb_launch_nb_chunks(const LioKfDesc* kf, int n_sel, int2* chunks, hipStream_t s)
{
    if (n_sel) hipLaunchKernelGGL(k_nb_chunks, dim3((unsigned)n_sel), dim3(64), 0, s, kf, chunks);
}

void lio_mb_launch_kf_transforms(LioKfDesc* kf, const float* poses, int n_kf, hipStream_t s)
{
    if (n_kf) hipLaunchKernelGGL(k_kf_transforms, dim3((unsigned)((n_kf + 63) / 64)), dim3(64), 0, s, kf, poses, n_kf);
}

void lio_mb_launch_transform_clouds(const float4* store, const LioKfDesc* kf, const int2* chunks, int n_chunks, float4* dst, hipStream_t s)
{
    if (n_chunks) hipLaunchKernelGGL(k_transform_clouds, dim3((unsigned)n_chunks), dim3(256), 0, s, store, kf, chunks, dst);
}

void lio_mb_launch_rec_to_xyzi4(const unsigned char* src, size_t stride, size_t xyz_off, int int_off, int n, float4* dst, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(k_rec_to_xyzi4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, stride, xyz_off, int_off, n, dst);
}

int lio_mb_voxel_grid(const float4* d_in, int n, float leaf, LioDevBytes& out, int* n_out, hipStream_t s, LioVoxWs<LioDevBytes>& ws)
{
    return voxel_grid_device<LioDevBytes>(d_in, n, leaf, out, n_out, s, ws, true, nullptr);
}

int lio_mb_copy_out(const float4* d_pts, int n, void* out, size_t out_stride, hipStream_t s) { return copy_out(d_pts, n, out, out_stride, s); }
