// lio_icp.hip -- loop-closure registration: pcl::IterativeClosestPoint<PointXYZI, PointXYZI>::computeTransformation and
// getFitnessScore as performRSLoopClosure uses them (MO:1110-1124; no rejectors, TransformationEstimationSVD,
// DefaultConvergenceCriteria), restated for the device.  DESIGN.md section 2 lists what is defined here because PCL is
// not a function of its inputs there (parity unpinned, restated from memory).
//   target   cell-sorted into a uniform grid over its own box: the counting / scan / scatter pieces of the map build
//   k_icp_pass<false>  one launch per iteration, one lane per source point: the incremental transform of the previous
//                      step, the exact 1-NN (Chebyshev shells of cells, outwards), fp64 sums in a fixed order; the
//                      workgroup that arrives last solves the rigid step, composes `final`, tests convergence
//   k_icp_pass<true>   getFitnessScore: the original source under `final`, 1-NN without a gate, fixed-order fp64 mean
// -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <cmath>
#include <stddef.h>
#include <string.h>

#include "lio_icp.h"
#include "lio_cloud.h"
#include "lio_kernels.h"
#include "lio_kfstore.h"
#include "lio_pool.h"
#include "lio_wg.h"

#define ICP_NV 17            // sums of one iteration: d2, count, s[3], t[3], t s^T [9]
#define ICP_NV_PAD 24        // doubles per workgroup in the partials table
#define ICP_SWEEPS 12        // Jacobi sweeps of the 3x3 SVD (it converges in 5 - 6; the count is fixed, not tested)

struct LioIcpState {
    float step[16];          // the step the next pass applies to the points first (the guess before the first one)
    float final_[16];
    double mse_prev, fitness;
    int32_t iters, done, converged, state, n_corr_last, similar, n_trace, n_fit;
    unsigned arrive, pad;
};

struct LioIcpParams {
    LioGrid g;
    float cell;              // cell edge
    float reach;             // no correspondence beyond this distance (a little over the gate)
    double gate2;            // max_corr_dist^2, the double PCL compares the float distance with
    const int* cell_start;
    const float4* sorted;    // target, cell-sorted: x, y, z, bits(index in the caller's order)
    const float4* src;       // the source as given
    float4* cur;             // input_transformed
    float4* closed;          // optional: the source under `final`
    int n_src;
    LioIcpState* st;
    double* partials;        // [workgroup][ICP_NV_PAD]
    float* tr_step;
    int* tr_ncorr;
    double* tr_mse;
    int* corr_rec;
    int rec_iter;
    double transform_eps, fitness_eps, rel_mse_eps, rotation_threshold;
    int max_iters, min_corr, max_similar;
};

// ---- exact nearest neighbour ------------------------------------------------------------------------------------------
// The query's cell c = floor((q - origin) / e) by the formula that binned the target.  Shell r = the cells at Chebyshev
// distance r from c.  A point of shell r is more than (r - 1) e away from q along one axis at least, so once the best
// squared distance found is at most ((r - 1) e - slack)^2 no later shell can hold a closer or an equally close point, and
// once (r - 1) e - slack exceeds `reach` no later shell can hold a point inside the gate.  slack (1e-3 e + 1e-5 |q -
// origin|) is three orders above the rounding of the cell formula and of the fp32 distance.  The winner is the minimum of
// (d2 bits << 32 | caller's index): ties go to the lower index whatever the visiting order.  Returns ~0 for no point.
__device__ __forceinline__ void icp_scan_run(const float4* __restrict__ sorted, int beg, int end, float qx, float qy, float qz,
                                             unsigned long long& best, int& best_slot)
{
    for (int s = beg; s < end; ++s) {
        const float4 m = sorted[s];
        const float dx = qx - m.x, dy = qy - m.y, dz = qz - m.z;
        const float d2 = ((dx * dx) + dy * dy) + dz * dz;          // FLANN L2_Simple
        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)__float_as_int(m.w);
        if (key < best) { best = key; best_slot = s; }
    }
}

__device__ static unsigned long long icp_nearest(const LioIcpParams& P, float qx, float qy, float qz, int& best_slot)
{
    const LioGrid& g = P.g;
    const float e = P.cell;
    const float fx = fminf(fmaxf(floorf((qx - g.ox) * g.inv_cell), -1.0e6f), 1.0e6f);
    const float fy = fminf(fmaxf(floorf((qy - g.oy) * g.inv_cell), -1.0e6f), 1.0e6f);
    const float fz = fminf(fmaxf(floorf((qz - g.oz) * g.inv_cell), -1.0e6f), 1.0e6f);
    const int cx = (int)fx, cy = (int)fy, cz = (int)fz;
    // first shell that touches the grid, last shell that does
    const int r0 = max(max(max(-cx, cx - (g.nx - 1)), max(-cy, cy - (g.ny - 1))), max(max(-cz, cz - (g.nz - 1)), 0));
    const int r_far = max(max(max(cx, g.nx - 1 - cx), max(cy, g.ny - 1 - cy)), max(cz, g.nz - 1 - cz));
    const float span = fmaxf(fmaxf(fabsf(qx - g.ox), fabsf(qy - g.oy)), fabsf(qz - g.oz));
    const float slack = 1.0e-3f * e + 1.0e-5f * span;
    unsigned long long best = ~0ull;
    best_slot = -1;
    for (int r = r0; r <= r_far; ++r) {
        if (r > 1) {
            const float lb = (float)(r - 1) * e - slack;
            if (lb > 0.0f) {
                if (lb > P.reach) break;
                if (best != ~0ull && lb * lb * 0.99999f >= __uint_as_float((unsigned)(best >> 32))) break;
            }
        }
        const int z0 = max(cz - r, 0), z1 = min(cz + r, g.nz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, g.ny - 1);
        for (int z = z0; z <= z1; ++z) {
            for (int y = y0; y <= y1; ++y) {
                const int row = (z * g.ny + y) * g.nx;
                if (abs(z - cz) == r || abs(y - cy) == r) {          // a face of the shell: one contiguous run of the row
                    const int xa = max(cx - r, 0), xb = min(cx + r, g.nx - 1);
                    if (xa <= xb) icp_scan_run(P.sorted, P.cell_start[row + xa], P.cell_start[row + xb + 1], qx, qy, qz, best, best_slot);
                } else {                                               // the two end cells of the row
                    const int xl = cx - r, xh = cx + r;
                    if (xl >= 0 && xl < g.nx) icp_scan_run(P.sorted, P.cell_start[row + xl], P.cell_start[row + xl + 1], qx, qy, qz, best, best_slot);
                    if (xh >= 0 && xh < g.nx) icp_scan_run(P.sorted, P.cell_start[row + xh], P.cell_start[row + xh + 1], qx, qy, qz, best, best_slot);
                }
            }
        }
    }
    return best;
}

// ---- rigid step -------------------------------------------------------------------------------------------------------
// One-sided Jacobi SVD of a 3x3 matrix (row-major) in fp64, ICP_SWEEPS sweeps over the column pairs (0,1), (0,2), (1,2):
// A V = W, singular values = column norms of W, sorted descending with their columns.
__device__ static void icp_svd3(const double A[9], double W[9], double V[9], double sv[3])
{
    for (int k = 0; k < 9; ++k) { W[k] = A[k]; V[k] = (k % 4 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < ICP_SWEEPS; ++sweep) {
        for (int pr = 0; pr < 3; ++pr) {
            const int i = pr == 2 ? 1 : 0, j = pr == 0 ? 1 : 2;
            double alpha = 0.0, beta = 0.0, gamma = 0.0;
            for (int k = 0; k < 3; ++k) { alpha += W[3 * k + i] * W[3 * k + i]; beta += W[3 * k + j] * W[3 * k + j]; gamma += W[3 * k + i] * W[3 * k + j]; }
            if (gamma == 0.0) continue;
            const double zeta = (beta - alpha) / (2.0 * gamma);
            const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
            for (int k = 0; k < 3; ++k) {
                const double wi = W[3 * k + i], wj = W[3 * k + j];
                W[3 * k + i] = c * wi - s * wj; W[3 * k + j] = s * wi + c * wj;
                const double vi = V[3 * k + i], vj = V[3 * k + j];
                V[3 * k + i] = c * vi - s * vj; V[3 * k + j] = s * vi + c * vj;
            }
        }
    }
    for (int j = 0; j < 3; ++j) sv[j] = sqrt(W[j] * W[j] + W[3 + j] * W[3 + j] + W[6 + j] * W[6 + j]);
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2 - a; ++b)
            if (sv[b] < sv[b + 1]) {
                const double t = sv[b]; sv[b] = sv[b + 1]; sv[b + 1] = t;
                for (int k = 0; k < 3; ++k) {
                    const double w = W[3 * k + b]; W[3 * k + b] = W[3 * k + b + 1]; W[3 * k + b + 1] = w;
                    const double v = V[3 * k + b]; V[3 * k + b] = V[3 * k + b + 1]; V[3 * k + b + 1] = v;
                }
            }
}

__device__ __forceinline__ double icp_det3(const double M[9])
{
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// Umeyama without scaling (TransformationEstimationSVD): R = U S V^T of the cross-covariance cov = sum (t - mt)(s - ms)^T / n,
// S = diag(1, 1, sign(det U det V)); a proper rotation always.  Columns of U whose singular value vanishes (collinear or
// coincident points) are completed to a right-handed frame; no pair at all with a direction: the identity.
__device__ static void icp_rotation(const double cov[9], double R[9])
{
    double W[9], V[9], sv[3], U[9];
    icp_svd3(cov, W, V, sv);
    const double tiny = sv[0] * 1.0e-12;
    for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    if (!(sv[0] > 0.0) || !(sv[0] <= DBL_MAX)) return;
    for (int k = 0; k < 3; ++k) U[3 * k] = W[3 * k] / sv[0];
    if (sv[1] > tiny) {
        for (int k = 0; k < 3; ++k) U[3 * k + 1] = W[3 * k + 1] / sv[1];
    } else {                                                           // rank 1: any unit vector orthogonal to U0
        int a = 0;
        if (fabs(U[3]) < fabs(U[3 * a])) a = 1;
        if (fabs(U[6]) < fabs(U[3 * a])) a = 2;
        double ex[3] = { 0.0, 0.0, 0.0 };
        ex[a] = 1.0;
        double c[3] = { ex[1] * U[6] - ex[2] * U[3], ex[2] * U[0] - ex[0] * U[6], ex[0] * U[3] - ex[1] * U[0] };
        const double nc = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        for (int k = 0; k < 3; ++k) U[3 * k + 1] = c[k] / nc;
    }
    if (sv[1] > tiny && sv[2] > tiny) {
        for (int k = 0; k < 3; ++k) U[3 * k + 2] = W[3 * k + 2] / sv[2];
    } else {                                                           // U2 = U0 x U1
        U[2] = U[3] * U[7] - U[6] * U[4];
        U[5] = U[6] * U[1] - U[0] * U[7];
        U[8] = U[0] * U[4] - U[3] * U[1];
    }
    const double sgn = icp_det3(U) * icp_det3(V) < 0.0 ? -1.0 : 1.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            R[3 * a + b] = (U[3 * a] * V[3 * b] + U[3 * a + 1] * V[3 * b + 1]) + sgn * (U[3 * a + 2] * V[3 * b + 2]);
}

// what the workgroup that arrived last does with the sums of one iteration (one thread)
__device__ static void icp_finish_iteration(const LioIcpParams& P, LioIcpState* st, const double* sum)
{
    const int k = st->iters;
    const int n = (int)sum[1];
    const double mse = n > 0 ? sum[0] / (double)n : 0.0;               // DefaultConvergenceCriteria::calculateMSE
    if (P.tr_ncorr) P.tr_ncorr[k] = n;
    if (P.tr_mse) P.tr_mse[k] = mse;
    st->n_corr_last = n;
    st->n_trace = k + 1;
    float step[16];
    for (int i = 0; i < 16; ++i) step[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    if (n < P.min_corr) {                                              // "Not enough correspondences found": converged_ = false, break
        if (P.tr_step) for (int i = 0; i < 16; ++i) P.tr_step[(size_t)k * 16 + i] = step[i];
        st->converged = 0; st->state = 5; st->done = 1;
        return;
    }
    double ms[3], mt[3], cov[9], R[9];
    for (int a = 0; a < 3; ++a) { ms[a] = sum[2 + a] / (double)n; mt[a] = sum[5 + a] / (double)n; }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) cov[3 * a + b] = sum[8 + 3 * a + b] / (double)n - mt[a] * ms[b];
    icp_rotation(cov, R);
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) step[4 * a + b] = (float)R[3 * a + b];
        step[4 * a + 3] = (float)(mt[a] - ((R[3 * a] * ms[0] + R[3 * a + 1] * ms[1]) + R[3 * a + 2] * ms[2]));
    }
    // final = step * final (4x4, fp32, each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3)
    float fin[16];
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b)
            fin[4 * a + b] = ((step[4 * a] * st->final_[b] + step[4 * a + 1] * st->final_[4 + b]) + step[4 * a + 2] * st->final_[8 + b]) +
                             step[4 * a + 3] * st->final_[12 + b];
    for (int i = 0; i < 16; ++i) { st->final_[i] = fin[i]; st->step[i] = step[i]; }
    if (P.tr_step) for (int i = 0; i < 16; ++i) P.tr_step[(size_t)k * 16 + i] = step[i];
    st->iters = k + 1;
    // DefaultConvergenceCriteria::hasConverged, in its order
    bool conv = false, similar = false;
    int state = 0;
    if (k + 1 >= P.max_iters) { conv = true; state = 1; }
    if (!conv) {
        const double cosang = 0.5 * ((((double)step[0] + (double)step[5]) + (double)step[10]) - 1.0);
        const double tsq = ((double)step[3] * (double)step[3] + (double)step[7] * (double)step[7]) + (double)step[11] * (double)step[11];
        if (cosang >= P.rotation_threshold && tsq <= P.transform_eps) {
            if (st->similar >= P.max_similar) { conv = true; state = 2; }
            similar = true;
        }
    }
    if (!conv && fabs(mse - st->mse_prev) < P.fitness_eps) {
        if (st->similar >= P.max_similar) { conv = true; state = 3; }
        similar = true;
    }
    if (!conv && fabs(mse - st->mse_prev) / st->mse_prev < P.rel_mse_eps) {
        if (st->similar >= P.max_similar) { conv = true; state = 4; }
        similar = true;
    }
    if (conv) { st->converged = 1; st->state = state; st->done = 1; return; }
    st->similar = similar ? st->similar + 1 : 0;
    st->mse_prev = mse;
}

// FIT = false: one ICP iteration.  FIT = true: getFitnessScore.  One lane per source point; 256 threads.
// Hand-off between workgroups: wave 0 stores the workgroup's sums with agent-scope (write-through) stores, releases at agent
// scope and adds one to the arrival counter; the workgroup that reads n_wg - 1 back acquires and reads every workgroup's
// sums with agent-scope loads, in workgroup order.
template <bool FIT>
__global__ __launch_bounds__(256) void k_icp_pass(LioIcpParams P)
{
    constexpr int NV = FIT ? 2 : ICP_NV;
    __shared__ double s_part[4][ICP_NV];
    __shared__ double s_sum[ICP_NV];
    __shared__ int s_last;
    LioIcpState* st = P.st;
    if (!FIT && st->done) return;                                      // (uniform over the launch: `done` is written by the last arrival only)
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    const int it = st->iters;
    float M[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = FIT ? st->final_[k] : st->step[k];
    double v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0.0;
    int corr = -1;
    if (i < P.n_src) {
        const float4 p = FIT ? P.src[i] : P.cur[i];
        float4 q = p;
        const bool fin = fabsf(p.x) <= FLT_MAX && fabsf(p.y) <= FLT_MAX && fabsf(p.z) <= FLT_MAX;
        if (fin) {                                                     // pcl::transformPointCloud, per point
            q.x = ((M[0] * p.x + M[1] * p.y) + M[2] * p.z) + M[3];
            q.y = ((M[4] * p.x + M[5] * p.y) + M[6] * p.z) + M[7];
            q.z = ((M[8] * p.x + M[9] * p.y) + M[10] * p.z) + M[11];
        }
        if (!FIT) P.cur[i] = q;
        else if (P.closed) P.closed[i] = q;
        if (fin && fabsf(q.x) <= FLT_MAX && fabsf(q.y) <= FLT_MAX && fabsf(q.z) <= FLT_MAX) {
            int slot;
            const unsigned long long key = icp_nearest(P, q.x, q.y, q.z, slot);
            if (key != ~0ull) {
                const float d2 = __uint_as_float((unsigned)(key >> 32));
                if constexpr (FIT) {
                    if ((double)d2 <= DBL_MAX) { v[0] = (double)d2; v[1] = 1.0; }
                } else if ((double)d2 <= P.gate2) {                    // the fp32 distance against the double square, as PCL
                    const float4 t = P.sorted[slot];
                    corr = __float_as_int(t.w);
                    v[0] = (double)d2; v[1] = 1.0;
                    const double s3[3] = { (double)q.x, (double)q.y, (double)q.z }, t3[3] = { (double)t.x, (double)t.y, (double)t.z };
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        v[2 + a] = s3[a]; v[5 + a] = t3[a];
#pragma unroll
                        for (int b = 0; b < 3; ++b) v[8 + 3 * a + b] = t3[a] * s3[b];      // (fp32 x fp32: exact in fp64)
                    }
                }
            }
        }
        if (!FIT && P.corr_rec && it == P.rec_iter) P.corr_rec[i] = corr;
    }
    // fixed order: xor butterfly 32 .. 1 in the wave, the waves ascending, the workgroups ascending
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) s_part[wave][k] = v[k];
    }
    if (threadIdx.x == 0) s_last = 0;
    __syncthreads();
    if (wave == 0) {
        if (lane < NV) {
            const double w = ((s_part[0][lane] + s_part[1][lane]) + s_part[2][lane]) + s_part[3][lane];
            __hip_atomic_store(reinterpret_cast<unsigned long long*>(P.partials + (size_t)blockIdx.x * ICP_NV_PAD + lane),
                               (unsigned long long)__double_as_longlong(w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        if (lane == 0) {
            const unsigned old = __hip_atomic_fetch_add(&st->arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old == gridDim.x - 1u) s_last = 1;
        }
    }
    __syncthreads();
    if (!s_last || wave != 0) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (lane < NV) {
        double w = 0.0;
        for (unsigned b = 0; b < gridDim.x; ++b)
            w += __longlong_as_double((long long)__hip_atomic_load(
                reinterpret_cast<unsigned long long*>(P.partials + (size_t)b * ICP_NV_PAD + lane), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        s_sum[lane] = w;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");             // (s_sum: written and read inside this wave)
    if (lane == 0) {
        __hip_atomic_store(&st->arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // re-arm for the next launch
        if (FIT) {
            const int n = (int)s_sum[1];
            st->n_fit = n;
            st->fitness = n > 0 ? s_sum[0] / (double)n : DBL_MAX;      // getFitnessScore: no point at all -> max()
        } else {
            icp_finish_iteration(P, st, s_sum);
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
extern "C" void lio_icp_default_config(lio_icp_config* cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->max_corr_dist = 30.0;        // historyKeyframeSearchRadius * 2, MO:1112 (UT:322: 15.0 in the yaml)
    cfg->transform_eps = 1e-6;        // MO:1114
    cfg->fitness_eps = 1e-6;          // MO:1115
    cfg->rel_mse_eps = 1e-5;          // DefaultConvergenceCriteria (PCL 1.10), from memory
    cfg->rotation_threshold = 0.99999;
    cfg->fitness_max = 0.3;           // historyKeyframeFitnessScore, UT:324
    cfg->max_iters = 100;             // MO:1113
    cfg->min_corr = 3;
    cfg->max_similar = 0;
    cfg->min_source_points = 300;     // MO:1104
    cfg->min_target_points = 1000;
    cfg->lookahead = 0;
}

int lio_icp_check_config(const lio_icp_config* c)
{
    if (!c) return lio_fail(LIO_ERR_ARG, "null icp config");
    if (!(c->max_corr_dist > 0.0) || !std::isfinite(c->max_corr_dist)) return lio_fail(LIO_ERR_ARG, "max_corr_dist must be positive and finite");
    if (c->max_iters < 1 || c->max_iters > LIO_ICP_MAX_ITERS) return lio_fail(LIO_ERR_ARG, "max_iters must be in [1, LIO_ICP_MAX_ITERS]");
    if (!(c->transform_eps >= 0.0) || !std::isfinite(c->transform_eps) || !(c->fitness_eps >= 0.0) || !std::isfinite(c->fitness_eps) ||
        !(c->rel_mse_eps >= 0.0) || !std::isfinite(c->rel_mse_eps))
        return lio_fail(LIO_ERR_ARG, "transform_eps, fitness_eps, rel_mse_eps must be >= 0 and finite");
    if (!(c->rotation_threshold >= -1.0 && c->rotation_threshold <= 1.0)) return lio_fail(LIO_ERR_ARG, "rotation_threshold must be in [-1, 1]");
    if (!(c->fitness_max >= 0.0)) return lio_fail(LIO_ERR_ARG, "fitness_max must be >= 0");
    if (c->min_corr < 1 || c->max_similar < 0 || c->min_source_points < 0 || c->min_target_points < 0)
        return lio_fail(LIO_ERR_ARG, "min_corr >= 1; max_similar, min_source_points, min_target_points >= 0");
    if (c->lookahead < 0 || c->lookahead > 64) return lio_fail(LIO_ERR_ARG, "lookahead must be in [0, 64]");
    return LIO_OK;
}

namespace {
struct IcpEvents {
    hipEvent_t ev[2] = { nullptr, nullptr };
    ~IcpEvents() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

void icp_empty_result(lio_icp_result* res, const float* guess, int n_src, int n_tgt)
{
    memset(res, 0, sizeof(*res));
    res->state = LIO_ICP_NO_CORRESPONDENCES;
    res->fitness = DBL_MAX;
    res->n_source = n_src; res->n_target = n_tgt;
    for (int i = 0; i < 16; ++i) res->T[i] = guess ? guess[i] : ((i % 5 == 0) ? 1.0f : 0.0f);
}

}  // namespace

// The grid over the target's box.  Cell edge from the target's density: points per occupied cell of a trial grid (64 cells
// along the longest side), scaled as for points on surfaces (count ~ edge^2) to about `per_cell` per occupied cell (the
// alignment asks for four).
int lio_icp_choose_grid(const float* x, const float* y, const float* z, int n, const float mn[3], const float mx[3], float per_cell,
                        hipStream_t s, LioGrid* g, float* edge, int* occupied)
{
    const float ext = fmaxf(fmaxf(mx[0] - mn[0], mx[1] - mn[1]), mx[2] - mn[2]);
    auto lay = [&](float e) {
        memset(g, 0, sizeof(*g));
        g->ox = mn[0]; g->oy = mn[1]; g->oz = mn[2];
        g->inv_cell = 1.0f / e;
        g->nx = (int)floorf((mx[0] - mn[0]) * g->inv_cell) + 1;
        g->ny = (int)floorf((mx[1] - mn[1]) * g->inv_cell) + 1;
        g->nz = (int)floorf((mx[2] - mn[2]) * g->inv_cell) + 1;
        g->k = 1; g->xs = 1; g->nxf = g->nx; g->inv_cell_x = g->inv_cell; g->tb_try = -1;
        for (int l = 0; l < LIO_TB_MAX; ++l) g->tb_reach[l] = -1.0f;
        const long long nc = (long long)g->nx * g->ny * g->nz;
        g->n_cells = nc > 0x7fffffffLL ? 0x7fffffff : (int)nc;
        return nc;
    };
    float e = 1.0f;
    if (ext > 1.0e-6f && ext <= FLT_MAX) {
        const float e0 = ext / 64.0f;
        lay(e0);
        LioTemp flags;
        HIPCHK(flags.alloc(sizeof(int) * ((size_t)g->n_cells + 1)));
        lio_launch_map_occupancy(*g, x, y, z, n, flags.as<int>(), s);
        int occ = 0;
        HIPCHK(hipMemcpyAsync(&occ, flags.as<int>() + g->n_cells, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (occupied) *occupied = occ;
        const float ppc = occ > 0 ? (float)n / (float)occ : 1.0f;
        e = e0 * sqrtf(per_cell / ppc);
        e = fminf(fmaxf(e, ext / 500.0f), ext);
        while (lay(e) > (1LL << 22)) e *= 1.26f;
    }
    lay(e);
    *edge = e;
    return LIO_OK;
}

// The target side of an alignment up to its grid: the box step of lio_cloud.h, then the grid at four points per occupied
// cell; no grid without a point on some axis.  lio_icp_device and the test hook lio_icp_debug_grid both go through here.
static int icp_lay_grid(const float4* d_tgt, int n_tgt, hipStream_t s, LioSearchTarget& T)
{
    float mn[3], mx[3];
    const int rc = lio_search_target_box(d_tgt, n_tgt, s, T, mn, mx);
    if (rc != LIO_OK || !T.any) return rc;
    return lio_icp_choose_grid(T.tx.as<float>(), T.ty.as<float>(), T.tz.as<float>(), n_tgt, mn, mx, 4.0f, s, &T.g, &T.edge, &T.occupied);
}

int lio_icp_device(const float4* d_src, int n_src, const float4* d_tgt, int n_tgt, const lio_icp_config& cfg, const float* guess,
                   lio_icp_result* res, hipStream_t s, LioIcpTrace* trace, float4* d_closed)
{
    if (trace) trace->n_trace = 0;
    if (guess) for (int i = 0; i < 16; ++i) if (!std::isfinite(guess[i])) return lio_fail(LIO_ERR_ARG, "non-finite guess");
    icp_empty_result(res, guess, n_src, n_tgt);
    if (n_src <= 0 || n_tgt <= 0) {
        if (d_closed && n_src > 0) HIPCHK(hipMemcpyAsync(d_closed, d_src, sizeof(float4) * (size_t)n_src, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        return LIO_OK;
    }
    // ---- the target: SoA, box, grid (icp_lay_grid), cell sort
    LioSearchTarget tg;
    int rc = icp_lay_grid(d_tgt, n_tgt, s, tg);
    if (rc != LIO_OK) return rc;
    if (!tg.any) {                                                     // no target point within the bound: nothing to correspond with
        if (d_closed) HIPCHK(hipMemcpyAsync(d_closed, d_src, sizeof(float4) * (size_t)n_src, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        return LIO_OK;
    }
    if ((rc = lio_search_target_sort(n_tgt, s, tg)) != LIO_OK) return rc;
    // ---- state, trace, loop
    const int n_wg = (n_src + 255) / 256, mi = cfg.max_iters;
    LioTemp cur, d_st, partials, tr_step, tr_ncorr, tr_mse, corr_rec;
    HIPCHK(cur.alloc(sizeof(float4) * (size_t)n_src));
    HIPCHK(d_st.alloc(sizeof(LioIcpState)));
    HIPCHK(partials.alloc(sizeof(double) * ICP_NV_PAD * (size_t)n_wg));
    HIPCHK(tr_step.alloc(sizeof(float) * 16 * (size_t)mi));
    HIPCHK(tr_ncorr.alloc(sizeof(int) * (size_t)mi));
    HIPCHK(tr_mse.alloc(sizeof(double) * (size_t)mi));
    const bool rec = trace && trace->corr && trace->rec_iter >= 0;
    if (rec) {
        HIPCHK(corr_rec.alloc(sizeof(int) * (size_t)n_src));
        HIPCHK(hipMemsetAsync(corr_rec.p, 0xff, sizeof(int) * (size_t)n_src, s));
    }
    LioIcpState h_st;
    memset(&h_st, 0, sizeof(h_st));
    for (int i = 0; i < 16; ++i) h_st.step[i] = h_st.final_[i] = res->T[i];
    h_st.mse_prev = DBL_MAX; h_st.fitness = DBL_MAX;
    HIPCHK(hipMemcpyAsync(d_st.p, &h_st, sizeof(h_st), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(cur.p, d_src, sizeof(float4) * (size_t)n_src, hipMemcpyDeviceToDevice, s));
    LioIcpParams P;
    memset(&P, 0, sizeof(P));
    P.g = tg.g; P.cell = tg.edge;
    P.gate2 = cfg.max_corr_dist * cfg.max_corr_dist;
    P.reach = (float)cfg.max_corr_dist * 1.0001f + 1.0e-6f;
    P.cell_start = tg.cell_start.as<int>(); P.sorted = tg.sorted.as<float4>();
    P.src = d_src; P.cur = cur.as<float4>(); P.closed = d_closed; P.n_src = n_src;
    P.st = d_st.as<LioIcpState>(); P.partials = partials.as<double>();
    P.tr_step = tr_step.as<float>(); P.tr_ncorr = tr_ncorr.as<int>(); P.tr_mse = tr_mse.as<double>();
    P.corr_rec = rec ? corr_rec.as<int>() : nullptr; P.rec_iter = rec ? trace->rec_iter : -1;
    P.transform_eps = cfg.transform_eps; P.fitness_eps = cfg.fitness_eps; P.rel_mse_eps = cfg.rel_mse_eps;
    P.rotation_threshold = cfg.rotation_threshold;
    P.max_iters = mi; P.min_corr = cfg.min_corr; P.max_similar = cfg.max_similar;
    // The host does not wait per iteration: `look` launches are enqueued, then a copy of the done flag and an event; the
    // flag of a chunk is looked at while the next chunk is already enqueued (launches after `done` exit at once).
    // (the flags' pinned words: one small block per calling thread, kept for the life of the process)
    static thread_local int* t_flags = nullptr;
    if (!t_flags) HIPCHK(hipHostMalloc((void**)&t_flags, 16 * sizeof(int), hipHostMallocPortable));
    IcpEvents evs;
    for (hipEvent_t& e : evs.ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const int look = cfg.lookahead > 0 ? cfg.lookahead : 4;
    int enq = 0, chunk = 0;
    for (bool done = false; !done; ++chunk) {
        const int m = mi - enq < look ? mi - enq : look;
        for (int j = 0; j < m; ++j) hipLaunchKernelGGL(k_icp_pass<false>, dim3(n_wg), dim3(256), 0, s, P);
        enq += m;
        t_flags[chunk & 1] = 0;
        HIPCHK(hipMemcpyAsync(&t_flags[chunk & 1], (const char*)d_st.p + offsetof(LioIcpState, done), sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipEventRecord(evs.ev[chunk & 1], s));
        if (chunk > 0) {
            HIPCHK(hipEventSynchronize(evs.ev[(chunk - 1) & 1]));
            if (t_flags[(chunk - 1) & 1]) done = true;
        }
        if (enq >= mi) done = true;                                    // (the max_iters-th iteration ends the loop by itself)
    }
    // getFitnessScore: P.reach off, no gate
    LioIcpParams F = P;
    F.reach = INFINITY;
    hipLaunchKernelGGL(k_icp_pass<true>, dim3(n_wg), dim3(256), 0, s, F);
    HIPCHK(hipMemcpyAsync(&h_st, d_st.p, sizeof(h_st), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    const int nt = h_st.n_trace;
    if (trace && nt > 0) {
        if (trace->step) HIPCHK(hipMemcpy(trace->step, tr_step.p, sizeof(float) * 16 * (size_t)nt, hipMemcpyDeviceToHost));
        if (trace->n_corr) HIPCHK(hipMemcpy(trace->n_corr, tr_ncorr.p, sizeof(int) * (size_t)nt, hipMemcpyDeviceToHost));
        if (trace->mse) HIPCHK(hipMemcpy(trace->mse, tr_mse.p, sizeof(double) * (size_t)nt, hipMemcpyDeviceToHost));
    }
    if (rec) HIPCHK(hipMemcpy(trace->corr, corr_rec.p, sizeof(int) * (size_t)n_src, hipMemcpyDeviceToHost));
    if (trace) trace->n_trace = nt;
    res->converged = h_st.converged;
    res->state = h_st.state;
    res->iters = h_st.iters;
    res->n_corr_last = h_st.n_corr_last;
    res->fitness = h_st.fitness;
    res->accepted = (h_st.converged && h_st.fitness <= cfg.fitness_max) ? 1 : 0;
    res->n_launches = enq + 1;
    for (int i = 0; i < 16; ++i) res->T[i] = h_st.final_[i];
    return LIO_OK;
}

// ------------------------------------------------ loop-closure registration (performRSLoopClosure MO:1098-1143)
// The entry points: host clouds, and submaps summed from the resident keyframe store (lio_kfstore.h).

// host records (x,y,z @0,4,8) -> device float4 (x, y, z, 0)
static int icp_upload(const void* pts, size_t n, size_t stride, LioTemp& raw, LioTemp& xyz4, hipStream_t s)
{
    HIPCHK(xyz4.alloc(sizeof(float4) * (n ? n : 1)));
    if (!n) return LIO_OK;
    return lio_upload_xyzi(pts, n, stride, -1, raw, xyz4.as<float4>(), s);
}

static int icp_align_host(int32_t device_id, const void* src, size_t n_src, size_t src_stride, const void* tgt, size_t n_tgt, size_t tgt_stride,
                          const lio_icp_config* cfg, const float* guess, lio_icp_result* res, LioIcpTrace* trace)
{
    if (!res || (n_src && !src) || (n_tgt && !tgt)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (src_stride < 12 || (src_stride & 3) || tgt_stride < 12 || (tgt_stride & 3)) return lio_fail(LIO_ERR_ARG, "strides must be >= 12 and multiples of 4");
    if (n_src > 0x7fffffffull - 1024 || n_tgt > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    int rc = lio_icp_check_config(cfg);
    if (rc != LIO_OK) return rc;
    if ((rc = lio_check_device(device_id)) != LIO_OK) return rc;
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

extern "C" int lio_icp_debug_grid(int32_t device_id, const void* target, size_t n_target, size_t target_stride, lio_icp_grid_info* out)
try {
    if (!out || (n_target && !target)) return lio_fail(LIO_ERR_ARG, "null argument");
    if (target_stride < 12 || (target_stride & 3)) return lio_fail(LIO_ERR_ARG, "strides must be >= 12 and multiples of 4");
    if (n_target > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "cloud too large");
    memset(out, 0, sizeof(*out));
    out->occupied = -1;
    int rc = lio_check_device(device_id);
    if (rc != LIO_OK) return rc;
    if (!n_target) return LIO_OK;
    hipStream_t s = nullptr;
    LioTemp raw_t, d_tgt;
    if ((rc = icp_upload(target, n_target, target_stride, raw_t, d_tgt, s)) != LIO_OK) return rc;
    LioSearchTarget tg;
    if ((rc = icp_lay_grid(d_tgt.as<float4>(), (int)n_target, s, tg)) != LIO_OK) return rc;
    if (!tg.any) return LIO_OK;
    out->any = 1;
    out->origin[0] = tg.g.ox; out->origin[1] = tg.g.oy; out->origin[2] = tg.g.oz;
    out->edge = tg.edge; out->inv_cell = tg.g.inv_cell;
    out->nx = tg.g.nx; out->ny = tg.g.ny; out->nz = tg.g.nz; out->n_cells = tg.g.n_cells;
    out->occupied = tg.occupied;
    return LIO_OK;
} LIO_CATCH

// loopFindNearKeyframes MO:1360-1383: the keyframes key - search_num .. key + search_num the store holds, each under its own
// stored pose or all under pose_index's, summed (the keyframe sum of lio_kfstore.h) and voxel-filtered.  An empty sum stays
// empty (MO:1375-1376).
static int loop_submap(lio_kf_store* st, int key, int search_num, int pose_index, float leaf, LioTemp& ds, int* n_out, hipStream_t s)
{
    *n_out = 0;
    const int N = (int)st->off.size();
    std::vector<int32_t> ids, pose_ids;
    for (long long i = -(long long)search_num; i <= (long long)search_num; ++i) {
        const long long near = (long long)key + i;
        if (near < 0 || near >= N) continue;
        const int32_t id = (int32_t)near, pid = pose_index >= 0 ? pose_index : id;
        if (!st->has_pose[(size_t)pid]) return lio_fail(LIO_ERR_ARG, "a keyframe has no pose (lio_kf_store_set_poses)");
        ids.push_back(id); pose_ids.push_back(pid);
    }
    LioKfSum t;
    lio_kf_sum_tables(st, ids.data(), pose_ids.data(), (int)ids.size(), t);
    if (t.total > 0x7fffffffull - 1024) return lio_fail(LIO_ERR_CAPACITY, "too many points");
    if (t.total == 0) return LIO_OK;
    LioTemp d_kf, d_poses, d_chunks, world;
    int rc = lio_kf_sum_upload(t, t.poses.data(), d_kf, d_poses, d_chunks, s);
    if (rc != LIO_OK) return rc;
    HIPCHK(world.alloc(t.total * sizeof(float4)));
    lio_kf_sum_launch(st, d_kf.as<LioKfDesc>(), d_poses.as<float>(), d_chunks.as<int2>(), (int)t.kf.size(), (int)t.chunks.size(), world.as<float4>(), s);
    HIPCHK(hipStreamSynchronize(s));                       // (the descriptors are host arrays of this function)
    rc = lio_voxel_grid_device(world.as<float4>(), (int)t.total, leaf, ds, n_out, s);
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
    if ((rc = lio_check_device(st->device_id)) != LIO_OK) return rc;
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
        if (clouds->source && (rc = lio_copy_out(src.as<float4>(), n_src, clouds->source, clouds->stride, s)) < 0) return rc;
        if (clouds->target && (rc = lio_copy_out(tgt.as<float4>(), n_tgt, clouds->target, clouds->stride, s)) < 0) return rc;
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
    if (want_closed && (rc = lio_copy_out(closed.as<float4>(), n_src, clouds->closed, clouds->stride, s)) < 0) return rc;
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
