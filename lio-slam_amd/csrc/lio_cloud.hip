// lio_cloud.hip -- what every chain over a device-resident float4 cloud uses (lio_cloud.h): the record conversions and the
// upload of a host cloud, the box pass (pcl::getMinMax3D), the cloud as its own search target (box step, cell sort) and K7, the pcl::VoxelGrid centroid filter of MO:1605-1611 (scan) and
// MO:1581-1583 (local map) with its kernels in lio_voxsort.h; lio_voxel_grid is nothing more than these.
// MO = the reference's src/liorf/src/mapOptmization.cpp.  -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "lio_cloud.h"
#include "lio_kernels.h"
#include "lio_voxsort.h"

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

__global__ void k_xyzi4_to_aos(const float4* __restrict__ src, int n, unsigned char* __restrict__ dst, size_t stride)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 v = src[i];
    float* o = reinterpret_cast<float*>(dst + (size_t)i * stride);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = 1.0f; o[4] = v.w;
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

void lio_rec_to_xyzi4(const unsigned char* src, size_t stride, size_t xyz_off, int int_off, int n, float4* dst, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(k_rec_to_xyzi4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, stride, xyz_off, int_off, n, dst);
}

int lio_upload_xyzi(const void* pts, size_t n, size_t stride, int int_off, LioTemp& raw, float4* dst, hipStream_t s, hipMemcpyKind kind)
{
    HIPCHK(raw.alloc(n * stride));
    HIPCHK(hipMemcpyAsync(raw.p, pts, n * stride, kind, s));
    lio_rec_to_xyzi4(raw.as<unsigned char>(), stride, 0, int_off, (int)n, dst, s);
    return LIO_OK;
}

template <class B>
int lio_vsort_reserve(int n, B& out, LioVoxWs<B>& ws)
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

template <class B>
uint2* lio_vsort_pairs(int n, int bits, hipStream_t s, LioVoxWs<B>& ws)
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

template <class B>
int lio_vsort_centroids(const float4* d_in, const uint2* a, int n, B& out, hipStream_t s, LioVoxWs<B>& ws)
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

// K7 proper (lio_voxsort.h, which tells why it sorts): keys -> stable LSD radix sort of (key, index) pairs -> segment heads ->
// in-order sums.  g describes the voxel grid, n_keys its size (< 2^31).  `out` is allocated for the worst case (n voxels) so that
// the centroid kernels are enqueued without waiting for the count; the one host wait (*n_out) comes last and overlaps them.
template <class B>
static int voxel_grid_sorted(const float4* d_in, int n, const LioVsGrid& vg, long long n_keys, B& out, int* n_out, hipStream_t s, LioVoxWs<B>& ws)
{
    int bits = 1;
    while (bits < 31 && (1LL << bits) < n_keys) ++bits;
    int rc = lio_vsort_reserve<B>(n, out, ws);
    if (rc != LIO_OK) return rc;
    hipLaunchKernelGGL(k_vsort_keys, dim3((n + 255) / 256), dim3(256), 0, s, vg, d_in, n, ws.pairs_a.template as<uint2>());
    const uint2* a = lio_vsort_pairs<B>(n, bits, s, ws);
    if ((rc = lio_vsort_centroids<B>(d_in, a, n, out, s, ws)) != LIO_OK) return rc;
    int no = 0;
    HIPCHK(hipMemcpyAsync(&no, ws.d_no.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));                                              // (`no`; the centroid kernels ran under this wait)
    HIPCHK(hipGetLastError());
    *n_out = no;
    return LIO_OK;
}

template <class B>
int lio_cloud_box_launch(const float4* d_in, int n, B& bbox, hipStream_t s)
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
int lio_cloud_box_wait(B& bbox, float mn[3], float mx[3], hipStream_t s)
{
    unsigned hb[6];
    HIPCHK(hipMemcpyAsync(hb, bbox.p, sizeof(hb), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    lio_ord_box_decode(hb, mn, mx);
    return LIO_OK;
}

int lio_search_target_box(const float4* d_pts, int n, hipStream_t s, LioSearchTarget& T, float mn[3], float mx[3])
{
    LioTemp bbox;
    HIPCHK(T.tx.alloc(sizeof(float) * (size_t)n)); HIPCHK(T.ty.alloc(sizeof(float) * (size_t)n)); HIPCHK(T.tz.alloc(sizeof(float) * (size_t)n));
    HIPCHK(T.t4.alloc(sizeof(float4) * (size_t)n));
    HIPCHK(bbox.alloc(6 * sizeof(unsigned)));
    lio_launch_xyzi4_to_soa(d_pts, n, T.tx.as<float>(), T.ty.as<float>(), T.tz.as<float>(), T.t4.as<float4>(), s);
    unsigned hb[6];
    lio_ord_box_clear(hb);
    HIPCHK(hipMemcpyAsync(bbox.p, hb, sizeof(hb), hipMemcpyHostToDevice, s));
    lio_launch_map_bbox(T.tx.as<float>(), T.ty.as<float>(), T.tz.as<float>(), n, bbox.as<unsigned>(), s);
    HIPCHK(hipMemcpyAsync(hb, bbox.p, sizeof(hb), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    lio_ord_box_decode(hb, mn, mx);
    T.any = true;
    for (int a = 0; a < 3; ++a) T.any = T.any && hb[a] != LIO_ORD_NO_MIN && mn[a] <= mx[a];
    return LIO_OK;
}

int lio_search_target_sort(int n, hipStream_t s, LioSearchTarget& T)
{
    const LioGrid& g = T.g;
    HIPCHK(T.cell_of.alloc(sizeof(int) * (size_t)n));
    HIPCHK(T.cell_count.alloc(sizeof(int) * (size_t)g.n_cells));
    HIPCHK(T.cell_start.alloc(sizeof(int) * ((size_t)g.n_cells + 1)));
    HIPCHK(T.tiles.alloc(sizeof(int) * ((size_t)lio_scan_tiles(g.n_cells) + 2)));
    HIPCHK(T.sorted.alloc(sizeof(float4) * (size_t)n));
    lio_launch_map_cell_sort(g, T.tx.as<float>(), T.ty.as<float>(), T.tz.as<float>(), n, T.cell_of.as<int>(), T.cell_count.as<int>(),
                             T.cell_start.as<int>(), T.tiles.as<int>(), T.sorted.as<float4>(), s);
    return LIO_OK;
}

template <class B>
int lio_voxel_grid_device(const float4* d_in, int n, float leaf, B& out, int* n_out, hipStream_t s, LioVoxWs<B>& ws, float* box,
                          bool have_box)
{
    *n_out = 0;
    if (box) for (int a = 0; a < 6; ++a) box[a] = 0.0f;
    if (n == 0) return LIO_OK;
    B& bbox = ws.bbox;
    if (!have_box) {
        int brc = lio_cloud_box_launch<B>(d_in, n, bbox, s);
        if (brc != LIO_OK) return brc;
    }
    float mn[3], mx[3];
    int wrc = lio_cloud_box_wait<B>(bbox, mn, mx, s);
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
    return voxel_grid_sorted<B>(d_in, n, g, n_keys_ll, out, n_out, s, ws);
}

#define LIO_CLOUD_INSTANTIATE(B) /* both workspaces: pool temporaries and buffers kept between calls */                          \
    template int lio_cloud_box_launch<B>(const float4*, int, B&, hipStream_t);                                                          \
    template int lio_cloud_box_wait<B>(B&, float*, float*, hipStream_t);                                                                \
    template int lio_vsort_reserve<B>(int, B&, LioVoxWs<B>&);                                                                           \
    template uint2* lio_vsort_pairs<B>(int, int, hipStream_t, LioVoxWs<B>&);                                                            \
    template int lio_vsort_centroids<B>(const float4*, const uint2*, int, B&, hipStream_t, LioVoxWs<B>&);                               \
    template int lio_voxel_grid_device<B>(const float4*, int, float, B&, int*, hipStream_t, LioVoxWs<B>&, float*, bool);
LIO_CLOUD_INSTANTIATE(LioTemp)
LIO_CLOUD_INSTANTIATE(LioDevBytes)

int lio_voxel_grid_device(const float4* d_in, int n, float leaf, LioTemp& out, int* n_out, hipStream_t s)
{
    LioVoxWs<LioTemp> ws;
    return lio_voxel_grid_device<LioTemp>(d_in, n, leaf, out, n_out, s, ws, nullptr);
}

int lio_copy_out(const float4* d_pts, int n, void* out, size_t out_stride, hipStream_t s)
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

int lio_check_device(int device_id)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return lio_fail(LIO_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    HIPCHK(hipSetDevice(device_id));
    (void)hipGetLastError();
    return LIO_OK;
}

extern "C" int lio_voxel_grid(int32_t device_id, const void* pts, size_t n, size_t stride, float leaf,
                              void* out, size_t out_stride, size_t* n_out)
try {
    if (!n_out || (n && (!pts || !out))) return lio_fail(LIO_ERR_ARG, "null argument");
    if (stride < 20 || (stride & 3) || out_stride < 20 || (out_stride & 3) || !(leaf > 0.0f))
        return lio_fail(LIO_ERR_ARG, "strides must be >= 20 and multiples of 4, leaf > 0");
    if (n > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    *n_out = 0;
    if (n == 0) return LIO_OK;
    int rc = lio_check_device(device_id);
    if (rc != LIO_OK) return rc;
    hipStream_t s = nullptr;
    LioTemp raw, xyzi, ds;
    HIPCHK(xyzi.alloc(n * sizeof(float4)));
    if ((rc = lio_upload_xyzi(pts, n, stride, 16, raw, xyzi.as<float4>(), s)) != LIO_OK) return rc;
    int no = 0;
    rc = lio_voxel_grid_device(xyzi.as<float4>(), (int)n, leaf, ds, &no, s);
    if (rc < 0) return rc;
    const int rc2 = lio_copy_out(ds.as<float4>(), no, out, out_stride, s);
    if (rc2 < 0) return rc2;
    *n_out = (size_t)no;
    return rc;
} LIO_CATCH
