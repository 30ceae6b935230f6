// lio_debug_math.hip -- the test hooks of include/liogpu.h: the host entries of all of them (second half of the file) and the
// kernels of the two designed-input hooks of the Gauss-Newton arithmetic, lio_debug_gn_step and lio_debug_corner_fit.
// These call lio_gn_step and lio_corner_assoc themselves, the functions of
// lio_s2m_device.h / lio_device_math.h that k_s2m_iterate and k_s2m_persist call.  A translation unit of its own, NOT part of
// lio_kernels.hip: both functions are static, and one more caller in that file -- with speculation arguments that are not
// constants -- changes how the compiler specialises and inlines them into k_s2m_iterate (measured: every instantiation's code
// differed).  Here the library's kernels stay byte for byte what they were.  Every operation is IEEE fp32 / fp64 with
// contraction off, so the bits are determined by the source; what the hooks cannot see is a miscompilation of one particular
// inlined copy -- the whole-registration tests remain that net.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <cmath>
#include <vector>
#include "lio_types.h"
#include "lio_kernels.h"
#include "lio_s2m_device.h"
#include "lio_gridplan.h"
#include "lio_handle.h"

// Test hook (lio_debug_gn_step): lio_gn_step itself on n independent cases, one wave per case (four to a workgroup), each with its
// own LioSolveWs and sums in LDS and its own LioScanState, which the host prepared (pose, iter, is_degenerate, matP; the rest zero)
// and reads back.  sums[i] = the LIO_SUMS doubles of case i as the reduction leaves them; ret[i] = what lio_gn_step returned.
__global__ __launch_bounds__(256) void k_debug_gn_step(LioScanState* __restrict__ st, long long n, const double* __restrict__ sums, LioConsts c,
                                                       int deg_override, int skip_eigen, int hold_if_done, int* __restrict__ ret)
{
    __shared__ LioSolveWs s_ws[4];
    __shared__ double s_sum[4][LIO_SUMS];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 4 + wave;
    if (i >= n) return;                                    // wave-uniform; lio_gn_step synchronises within the wave only
    if (lane < LIO_SUMS) s_sum[wave][lane] = sums[i * LIO_SUMS + lane];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // one wave: the sums are in LDS before any lane reads them
    const int r = lio_gn_step(&st[i], s_sum[wave], c, &s_ws[wave], nullptr, lane, deg_override, skip_eigen != 0, hold_if_done != 0);
    if (lane == 0) ret[i] = r;
}

void lio_launch_debug_gn_step(LioScanState* st, long long n, const double* sums, const LioConsts& c, int deg_override, int skip_eigen,
                              int hold_if_done, int* ret, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_debug_gn_step, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, st, n, sums, c, deg_override, skip_eigen, hold_if_done, ret);
}

// Test hook (lio_debug_corner_fit): lio_corner_assoc, the function lio_assoc_point calls for an edge point, on caller-supplied
// neighbour sets (the caller's order) and transformed points, one case per thread.  out[5 i ..] = the bits of the four coefficients, then the accept flag.
__global__ __launch_bounds__(256) void k_debug_corner_fit(const float* __restrict__ sets, const float* __restrict__ pts, long long n,
                                                          double weight, double min_s, unsigned* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float m[5][3];
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) m[j][c] = sets[i * 15 + j * 3 + c];
    float cx, cy, cz, cw;
    const bool accept = lio_corner_assoc(m, pts[i * 3 + 0], pts[i * 3 + 1], pts[i * 3 + 2], weight, min_s, cx, cy, cz, cw);
    unsigned* o = out + i * 5;
    o[0] = __float_as_uint(cx); o[1] = __float_as_uint(cy); o[2] = __float_as_uint(cz); o[3] = __float_as_uint(cw);
    o[4] = accept ? 1u : 0u;
}

void lio_launch_debug_corner_fit(const float* sets, const float* pts, long long n, double weight, double min_s, unsigned* out, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_debug_corner_fit, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, sets, pts, n, weight, min_s, out);
}

// ---------------------------------------------------------------- host entries of the test hooks (include/liogpu.h)

// Test hook: the plane fit of the association kernels (lio_plane_fit5: the 5x3 column-pivoting QR solve, the unit normal and the
// plane test) on n caller-supplied neighbour sets, sets[n][5][3] in host memory.  out[n][8] receives the raw bits of
// X0[0..2], pa, pb, pc, pd and planeValid (0 / 1).
extern "C" int lio_debug_plane_fit(int32_t device_id, const float* sets, size_t n, double plane_tol, uint32_t* out)
try {
    if ((!sets || !out) && n) return lio_fail(LIO_ERR_ARG, "null pointer");
    if (n > ((size_t)1 << 27)) return lio_fail(LIO_ERR_CAPACITY, "at most 2^27 sets per call");
    if (!n) return LIO_OK;
    HIPCHK(hipSetDevice(device_id));
    LioDevBuf<float> d_sets;
    LioDevBuf<unsigned> d_out;
    HIPCHK(d_sets.grow(n * 15, 1.0, 0));
    HIPCHK(d_out.grow(n * 8, 1.0, 0));
    HIPCHK(hipMemcpy(d_sets, sets, n * 15 * sizeof(float), hipMemcpyHostToDevice));
    lio_launch_debug_plane_fit(d_sets, (long long)n, plane_tol, d_out, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, d_out, n * 8 * sizeof(unsigned), hipMemcpyDeviceToHost));
    return LIO_OK;
} LIO_CATCH

// Test hook: the serial Gauss-Newton step that ends every launch (lio_gn_step: the 6x6 QR solve, on iteration 0 the Jacobi
// eigen-decomposition over a wave, the degeneracy rule, the LU inverse and the product, then the projection, the pose update, the
// convergence test and the loop control) on n independent cases, one wave each.  The source function as compiled into the hook's
// kernel, not as inlined into k_s2m_iterate / k_s2m_persist.  Non-finite sums or poses are refused before any launch: the lane
// code's pivot search is defined for finite matrices only (a NaN would make it index lanes the serial code never reads), and
// the library keeps non-finite values out of the sums (tests/test_gpu_nonfinite.py).
extern "C" int lio_debug_gn_step(int32_t device_id, const lio_s2m_config* cfg, size_t n, const double* sums, const float* pose,
                                 const int32_t* iter, const int32_t* is_degenerate, const float* matP, int32_t deg_override,
                                 int32_t skip_eigen, int32_t hold_if_done, lio_debug_gn_record* out)
try {
    if ((!sums || !pose || !iter || !is_degenerate || !matP || !out) && n) return lio_fail(LIO_ERR_ARG, "null pointer");
    if (n > ((size_t)1 << 18)) return lio_fail(LIO_ERR_CAPACITY, "at most 2^18 cases per call");
    lio_s2m_config g;
    if (cfg) g = *cfg; else lio_s2m_default_config(&g);
    if (g.max_iters < 1 || g.max_iters > LIO_MAX_ITERS) return lio_fail(LIO_ERR_ARG, "max_iters out of range");
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 27; ++k)                       // finite as the fp32 value the step takes, too
            if (!std::isfinite(sums[i * 28 + k]) || !std::isfinite((float)sums[i * 28 + k])) return lio_fail(LIO_ERR_ARG, "non-finite sum");
        const double nc = sums[i * 28 + LIO_SUM_NC];
        if (!(nc >= 0.0 && nc <= 2147483647.0)) return lio_fail(LIO_ERR_ARG, "the correspondence count must be in [0, 2^31)");
        for (int k = 0; k < 6; ++k) if (!std::isfinite(pose[i * 6 + k])) return lio_fail(LIO_ERR_ARG, "non-finite pose");
        if (iter[i] < 0 || iter[i] >= LIO_MAX_ITERS) return lio_fail(LIO_ERR_ARG, "iter out of range");
    }
    if (!n) return LIO_OK;
    LioConsts c;
    lio_consts_from_config(g, c);
    std::vector<LioScanState> st(n);
    std::vector<double> h_sums(n * LIO_SUMS, 0.0);
    std::vector<int> ret(n, 0);
    memset(st.data(), 0, n * sizeof(LioScanState));
    for (size_t i = 0; i < n; ++i) {
        memcpy(st[i].pose, pose + i * 6, sizeof(float) * 6);
        memcpy(st[i].matP, matP + i * 36, sizeof(float) * 36);
        st[i].iter = iter[i];
        st[i].is_degenerate = is_degenerate[i];
        memcpy(&h_sums[i * LIO_SUMS], sums + i * 28, sizeof(double) * 28);
    }
    HIPCHK(hipSetDevice(device_id));
    LioDevBuf<LioScanState> d_st;
    LioDevBuf<double> d_sums;
    LioDevBuf<int> d_ret;
    HIPCHK(d_st.grow(n, 1.0, 0));
    HIPCHK(d_sums.grow(n * LIO_SUMS, 1.0, 0));
    HIPCHK(d_ret.grow(n, 1.0, 0));
    HIPCHK(hipMemcpy(d_st, st.data(), n * sizeof(LioScanState), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_sums, h_sums.data(), n * LIO_SUMS * sizeof(double), hipMemcpyHostToDevice));
    lio_launch_debug_gn_step(d_st, (long long)n, d_sums, c, deg_override, skip_eigen, hold_if_done, d_ret, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(st.data(), d_st, n * sizeof(LioScanState), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ret.data(), d_ret, n * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
        lio_debug_gn_record& o = out[i];
        const LioScanState& s = st[i];
        memcpy(o.pose, s.pose, sizeof(o.pose)); memcpy(o.matP, s.matP, sizeof(o.matP));
        memcpy(o.AtA, s.AtA, sizeof(o.AtA)); memcpy(o.AtB, s.AtB, sizeof(o.AtB));
        memcpy(o.T, s.T, sizeof(o.T)); memcpy(o.trig, s.trig, sizeof(o.trig));
        o.iter = s.iter; o.done = s.done; o.status = s.status; o.converged = s.converged;
        o.is_degenerate = s.is_degenerate; o.n_corr_last = s.n_corr_last; o.ret = ret[i];
    }
    return LIO_OK;
} LIO_CATCH

// Test hook: the line fit of the corner association (lio_corner_assoc: centroid, covariance, the 3x3 Jacobi, the e0 > 3 e1 test,
// the point-to-line distance and its gradient, the weight) on n cases: sets[n][5][3] = the five neighbours in the caller's order,
// pts[n][3] = the transformed points.  out[n][5]: the raw bits of the four coefficients, then the accept flag (0 / 1).  Non-finite
// inputs are allowed: the code is serial.
extern "C" int lio_debug_corner_fit(int32_t device_id, const float* sets, const float* pts, size_t n, double weight, double min_s, uint32_t* out)
try {
    if ((!sets || !pts || !out) && n) return lio_fail(LIO_ERR_ARG, "null pointer");
    if (n > ((size_t)1 << 27)) return lio_fail(LIO_ERR_CAPACITY, "at most 2^27 cases per call");
    if (!n) return LIO_OK;
    HIPCHK(hipSetDevice(device_id));
    LioDevBuf<float> d_sets, d_pts;
    LioDevBuf<unsigned> d_out;
    HIPCHK(d_sets.grow(n * 15, 1.0, 0));
    HIPCHK(d_pts.grow(n * 3, 1.0, 0));
    HIPCHK(d_out.grow(n * 5, 1.0, 0));
    HIPCHK(hipMemcpy(d_sets, sets, n * 15 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_pts, pts, n * 3 * sizeof(float), hipMemcpyHostToDevice));
    lio_launch_debug_corner_fit(d_sets, d_pts, (long long)n, weight, min_s, d_out, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, d_out, n * 5 * sizeof(unsigned), hipMemcpyDeviceToHost));
    return LIO_OK;
} LIO_CATCH

// Test hook: the fast fp32 operations of the association (lio_device_math.h) against the device's plain operators.  op 0: square
// root, op 1: x / 5, op 2: the fourth root of the squared range of the scan point (x, 0, 0) through the plane fit's flag; raw != 0
// (ops 0, 1): the fast sequence without its guard.  The operands are the bit patterns patterns[0..count) or, with
// patterns null, first, first + 1, ...  *n_diff receives the number of results whose bits differ from the plain operator's (two
// NaNs are equal), first_diff[0..8) up to eight such patterns (*n_first of them), values (may be null) the library's result bits.
extern "C" int lio_debug_fast_f32_ops(int32_t device_id, int32_t op, int32_t raw, const uint32_t* patterns, uint64_t first, uint64_t count,
                                      uint32_t* values, uint64_t* n_diff, uint32_t* first_diff, int32_t* n_first)
try {
    if (!n_diff || !first_diff || !n_first) return lio_fail(LIO_ERR_ARG, "null pointer");
    if (op < 0 || op > 2) return lio_fail(LIO_ERR_ARG, "op must be 0 (sqrt), 1 (x / 5) or 2 (fourth root of the range)");
    if (count > ((uint64_t)1 << 32)) return lio_fail(LIO_ERR_CAPACITY, "at most 2^32 patterns per call");
    if ((patterns || values) && count > ((uint64_t)1 << 27)) return lio_fail(LIO_ERR_CAPACITY, "at most 2^27 listed patterns or returned values per call");
    *n_diff = 0; *n_first = 0;
    if (!count) return LIO_OK;
    HIPCHK(hipSetDevice(device_id));
    LioDevBuf<unsigned> d_pat, d_val, d_diff;
    LioDevBuf<unsigned long long> d_n;
    if (patterns) {
        HIPCHK(d_pat.grow(count, 1.0, 0));
        HIPCHK(hipMemcpy(d_pat, patterns, count * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (values) HIPCHK(d_val.grow(count, 1.0, 0));
    HIPCHK(d_diff.grow(9, 1.0, 0));
    HIPCHK(d_n.grow(1, 1.0, 0));
    HIPCHK(hipMemset(d_diff, 0, 9 * sizeof(unsigned)));
    HIPCHK(hipMemset(d_n, 0, sizeof(unsigned long long)));
    lio_launch_debug_fast_f32_ops(op, raw ? 1 : 0, patterns ? (const unsigned*)d_pat : nullptr, first, count,
                                  values ? (unsigned*)d_val : nullptr, d_n, d_diff, nullptr);
    HIPCHK(hipGetLastError());
    unsigned h_diff[9];
    unsigned long long h_n = 0;
    HIPCHK(hipMemcpy(h_diff, d_diff, sizeof(h_diff), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&h_n, d_n, sizeof(h_n), hipMemcpyDeviceToHost));
    if (values) HIPCHK(hipMemcpy(values, d_val, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *n_diff = h_n;
    *n_first = (int32_t)(h_diff[0] < 8 ? h_diff[0] : 8);
    for (int i = 0; i < 8; ++i) first_diff[i] = h_diff[1 + i];
    return LIO_OK;
} LIO_CATCH

// Test hook: the fp32 threshold the surface association compares against in place of the double t (lio_threshold_f32: the
// largest float not above t).  Host only.
extern "C" float lio_debug_threshold_f32(double t) { return lio_threshold_f32(t); }

// Test hook (host only): the plan of lio_map_finish for a box and a cell count given by the caller.
extern "C" int lio_debug_grid_plan(const lio_s2m_config* cfg, const float mn[3], const float mx[3], size_t n, int32_t occupied,
                                   int32_t caller_box, lio_grid_plan_info* out)
try {
    if (!cfg || !mn || !mx || !out) return lio_fail(LIO_ERR_ARG, "null argument");
    const LioGridOverrides ov = lio_grid_overrides_from_env();
    LioGridPlan plan = lio_plan_grid(*cfg, lio_gate_reach(cfg->max_sq_dist), mn, mx, n, caller_box != 0, ov);
    lio_plan_tables(plan, *cfg, mn, mx, n, occupied, ov);
    const LioGrid& g = plan.grid;
    out->origin[0] = g.ox; out->origin[1] = g.oy; out->origin[2] = g.oz; out->inv_cell = g.inv_cell;
    out->nx = g.nx; out->ny = g.ny; out->nz = g.nz; out->n_cells = g.n_cells; out->k = g.k; out->xs = g.xs; out->nxf = g.nxf;
    out->inv_cell_x = g.inv_cell_x;
    for (int l = 0; l < LIO_TB_MAX; ++l) {
        out->tb_row0[l] = g.tb_row0[l]; out->tb_ny[l] = g.tb_ny[l]; out->tb_nz[l] = g.tb_nz[l];
        out->tb_oy[l] = g.tb_oy[l]; out->tb_oz[l] = g.tb_oz[l]; out->tb_inv_cell[l] = g.tb_inv_cell[l]; out->tb_reach[l] = g.tb_reach[l];
        out->tb_try_b2[l] = g.tb_try_b2[l];
    }
    out->tb_try = g.tb_try;
    out->cell = plan.cell; out->n_tb = plan.n_tb; out->grow_steps = plan.grow_steps; out->want_occupancy = plan.want_occupancy ? 1 : 0;
    out->pts_per_cell = plan.pts_per_cell;
    out->buckets = (int64_t)(plan.len_a + plan.len_b);
    return LIO_OK;
} LIO_CATCH

// Test hook (host only): lio_plan_scan_tiles on a box given by the caller.
extern "C" int lio_debug_scan_tile_plan(const float mn[3], const float mx[3], float tile, int32_t shard_axis, int32_t out_i[6],
                                        float out_f[4])
try {
    if (!mn || !mx || !out_i || !out_f) return lio_fail(LIO_ERR_ARG, "null argument");
    if (!(tile > 0.0f) || shard_axis < -1 || shard_axis > 2) return lio_fail(LIO_ERR_ARG, "need tile > 0 and shard_axis in -1..2");
    const LioScanTiles t = lio_plan_scan_tiles(mn, mx, tile, shard_axis);
    out_i[0] = t.ntx; out_i[1] = t.nty; out_i[2] = t.ntz; out_i[3] = t.mx; out_i[4] = t.my; out_i[5] = t.mz;
    out_f[0] = t.ox; out_f[1] = t.oy; out_f[2] = t.oz; out_f[3] = t.inv_tile;
    return LIO_OK;
} LIO_CATCH

// Test hook: bound of the one-launch loop's barrier polls for this handle (0 = default) and the index of an association
// workgroup that never arrives (-1 = none), which forces the time-out and with it the fall-back to the launch loop.
extern "C" int lio_s2m_debug_persist_spin(lio_s2m_handle* h, int32_t spin_max, int32_t withhold_wg)
try {
    if (!h) return lio_fail(LIO_ERR_ARG, "null handle");
    h->persist_spin_max = spin_max > 0 ? (unsigned)spin_max : 0u;
    h->persist_withhold = withhold_wg;
    return LIO_OK;
} LIO_CATCH

// Diagnostic: phase clock of the LAST iterate launch (cfg.profile == 2):
// n_blocks x 4 waves x 8 cycle counters.  Returns the number of blocks.
extern "C" int lio_s2m_debug_stamps(lio_s2m_handle* h, long long* out, size_t cap_entries)
{
    if (!h || !h->d_stamps) return 0;
    const size_t n = (size_t)h->n_blocks * (LIO_BLOCK / 64) * 8;
    if (out && cap_entries >= n) {
        if (hipMemcpy(out, h->d_stamps, n * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    }
    return h->n_blocks;
}

// Test hook: the permutation and the SoA the upload-time tile sort left for the resident batch (include/liogpu.h).
extern "C" int lio_s2m_debug_scan_order(lio_s2m_handle* h, int32_t* perm, float* xyz, size_t cap_points, int32_t* sorted)
try {
    if (!h) return lio_fail(LIO_ERR_ARG, "null handle");
    if (h->multi) return lio_fail(LIO_ERR_ARG, "not available on a multi-device handle");
    if (const int rc = lio_enter(h); rc != LIO_OK) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t total = h->total_pts;
    if (sorted) *sorted = h->sorted ? 1 : 0;
    if (perm || xyz) {
        if (cap_points < total) return lio_fail(LIO_ERR_ARG, "cap_points is below the batch's point count");
        if (perm && total && h->sorted)
            HIPCHK(hipMemcpy(perm, h->d_perm, total * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (xyz && total && h->soa_valid) {
            HIPCHK(hipMemcpy(xyz, h->d_sx, total * sizeof(float), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(xyz + total, h->d_sy, total * sizeof(float), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(xyz + 2 * total, h->d_sz, total * sizeof(float), hipMemcpyDeviceToHost));
        }
    }
    return (int)total;
} LIO_CATCH
