// lio_kfstore.hip -- the resident keyframe store, surfCloudKeyFrames (MO:128) and cloudKeyPoses6D in HBM (MO:2136-2142), K6
// transformPointCloud (MO:849-868), and the keyframe sum -- "keyframes ids[k] under poses p[k], concatenated in the world
// frame" -- that the map assembly, the loop-closure submaps, the planning local map and the map export share.
// MO = the reference's src/liorf/src/mapOptmization.cpp.  -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <cmath>
#include <string.h>
#include <algorithm>

#include "lio_handle.h"
#include "lio_kfstore.h"
#include "lio_device_math.h"

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

void lio_kf_transforms(LioKfDesc* d_kf, const float* d_poses, int n_kf, hipStream_t s)
{
    if (n_kf) hipLaunchKernelGGL(k_kf_transforms, dim3((unsigned)((n_kf + 63) / 64)), dim3(64), 0, s, d_kf, d_poses, n_kf);
}

void lio_kf_sum_launch(const lio_kf_store* st, LioKfDesc* d_kf, const float* d_poses, const int2* d_chunks, int n_sel, int n_chunks, float4* dst, hipStream_t s)
{
    lio_kf_transforms(d_kf, d_poses, n_sel, s);
    if (n_chunks) hipLaunchKernelGGL(k_transform_clouds, dim3((unsigned)n_chunks), dim3(256), 0, s, st->d_pts, d_kf, d_chunks, dst);
}

LioKfDesc lio_kf_desc(const lio_kf_store* st, size_t id, size_t first)
{
    LioKfDesc d;
    d.src = (int)st->off[id]; d.first = (int)first; d.n = (int)st->cnt[id]; d.pad = 0;
    for (int j = 0; j < 12; ++j) d.T[j] = 0.0f;
    return d;
}

void lio_kf_stored_pose(const lio_kf_store* st, size_t id, float pose[6])
{
    pose[0] = st->proll[id]; pose[1] = st->ppitch[id]; pose[2] = st->pyaw[id]; pose[3] = st->px[id]; pose[4] = st->py[id]; pose[5] = st->pz[id];
}

void lio_kf_sum_tables(const lio_kf_store* st, const int32_t* ids, const int32_t* pose_ids, int n, LioKfSum& t)
{
    t = LioKfSum();
    if (pose_ids) t.poses.resize(6 * (size_t)n);
    for (int k = 0; k < n; ++k) {
        const size_t id = (size_t)ids[k];
        t.kf.push_back(lio_kf_desc(st, id, t.total));
        for (size_t b = 0; b < st->cnt[id]; b += 256) t.chunks.push_back(make_int2(k, (int)b));
        if (pose_ids) lio_kf_stored_pose(st, (size_t)pose_ids[k], &t.poses[6 * (size_t)k]);
        t.total += st->cnt[id];
    }
}

template <class B>
int lio_kf_sum_upload(const LioKfSum& t, const float* poses, B& d_kf, B& d_poses, B& d_chunks, hipStream_t s)
{
    const int n_sel = (int)t.kf.size(), n_chunks = (int)t.chunks.size();
    HIPCHK(d_kf.alloc(sizeof(LioKfDesc) * (size_t)(n_sel ? n_sel : 1)));
    HIPCHK(d_poses.alloc(sizeof(float) * 6 * (size_t)(n_sel ? n_sel : 1)));
    HIPCHK(d_chunks.alloc(sizeof(int2) * (n_chunks ? n_chunks : 1)));
    if (n_sel) {
        HIPCHK(hipMemcpyAsync(d_kf.p, t.kf.data(), sizeof(LioKfDesc) * (size_t)n_sel, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_poses.p, poses, sizeof(float) * 6 * (size_t)n_sel, hipMemcpyHostToDevice, s));
    }
    if (n_chunks) HIPCHK(hipMemcpyAsync(d_chunks.p, t.chunks.data(), sizeof(int2) * n_chunks, hipMemcpyHostToDevice, s));
    return LIO_OK;
}
template int lio_kf_sum_upload<LioTemp>(const LioKfSum&, const float*, LioTemp&, LioTemp&, LioTemp&, hipStream_t);
template int lio_kf_sum_upload<LioDevBytes>(const LioKfSum&, const float*, LioDevBytes&, LioDevBytes&, LioDevBytes&, hipStream_t);

// ------------------------------------------------------- the store (struct lio_kf_store is in lio_kfstore.h)

extern "C" int lio_kf_store_create(int32_t device_id, lio_kf_store** out)
try {
    if (!out) return lio_fail(LIO_ERR_ARG, "null argument");
    int rc = lio_check_device(device_id);
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

// the end of every lio_kf_store_add*: the wait for the conversion queued on `q`, then the bookkeeping
static int kf_store_commit(lio_kf_store* s, size_t n, hipStream_t q, int32_t* id_out)
{
    if (n) HIPCHK(hipStreamSynchronize(q));
    if (n) HIPCHK(hipGetLastError());
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
    return LIO_OK;
}

extern "C" int lio_kf_store_add(lio_kf_store* s, const void* cloud, size_t n, size_t stride, int32_t* id_out)
try {
    if (!s || (n && !cloud)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (stride < 20 || (stride & 3)) return lio_fail(LIO_ERR_ARG, "stride must be >= 20 and a multiple of 4");
    int rc = lio_check_device(s->device_id);
    if (rc != LIO_OK) return rc;
    if ((rc = kf_store_reserve(s, n)) != LIO_OK) return rc;
    LioTemp raw;
    if (n && (rc = lio_upload_xyzi(cloud, n, stride, 16, raw, s->d_pts + s->used, nullptr, hipMemcpyDefault)) != LIO_OK) return rc;
    return kf_store_commit(s, n, nullptr, id_out);
} LIO_CATCH

extern "C" int lio_kf_store_add_device(lio_kf_store* s, const void* d_cloud, size_t n, size_t stride, int32_t* id_out)
try {
    if (!s || (n && !d_cloud)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (stride < 12 || (stride & 3)) return lio_fail(LIO_ERR_ARG, "stride must be >= 12 and a multiple of 4");
    int rc = lio_check_device(s->device_id);
    if (rc != LIO_OK) return rc;
    if ((rc = kf_store_reserve(s, n)) != LIO_OK) return rc;
    if (n) {
        HIPCHK(hipDeviceSynchronize());                  // the producer of d_cloud may have used any stream
        lio_rec_to_xyzi4((const unsigned char*)d_cloud, stride, 0, stride >= 20 ? 16 : -1, (int)n, s->d_pts + s->used, nullptr);
    }
    return kf_store_commit(s, n, nullptr, id_out);
} LIO_CATCH

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
    if ((rc = lio_check_device(s->device_id)) != LIO_OK) return rc;
    if ((rc = kf_store_reserve(s, n)) != LIO_OK) return rc;
    // the intensity sits where the upload said it does (lio_pc2_layout.off_intensity; byte 16 for PCL records; byte 12 for
    // the float4 records lio_s2m_register_raw stages), not at a guessed offset
    lio_rec_to_xyzi4(rec, stride, xyz_off, int_off, (int)n, s->d_pts + s->used, st);
    return kf_store_commit(s, n, st, id_out);
} LIO_CATCH

LioPoseTab lio_kf_pose_tab(lio_kf_store* st)
{
    const size_t c = st->tab_cap;
    const float* f = st->d_tab.as<float>();
    LioPoseTab t = { f, f + c, f + 2 * c, f + 3 * c, f + 4 * c, f + 5 * c, (const double*)(f + 6 * c), (const int*)(f + 8 * c),
                     (const int*)(f + 9 * c) };
    return t;
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

int lio_kf_upload_pose_tab(lio_kf_store* st, hipStream_t s)
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
