// lio_s2m_block.h -- the work of one association workgroup on one entry of the block list: the body that k_s2m_iterate
// (lio_kernels.hip, one entry per workgroup) and k_s2m_iterate_tail (lio_tail.hip, a fixed grid looping over the live
// entries of its share) have in common, with the LDS form of the candidate scan and the occupancy targets.
#pragma once
#include <hip/hip_runtime.h>
#include "lio_types.h"
#include "lio_device_math.h"
#include "lio_kernels.h"
#include "lio_s2m_device.h"
#include "lio_wg.h"

// Record entry oi (caller's point order) of a point this rank does not process in the recorded iteration.
__device__ __forceinline__ void lio_record_unprocessed(const LioIterParams& P, int oi)
{
    P.rec_flag[oi] = 0;
    reinterpret_cast<float4*>(P.rec_coeff)[oi] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int j = 0; j < 5; ++j) P.rec_nn[(size_t)oi * 5 + j] = -1;
}

// ---- candidate scan, LDS form ---------------------------------------------
// s_pts holds the map points of the workgroup's cell region (rows of the
// region are contiguous runs), s_cell the run offsets of every cell of the
// region: rx+1 entries per (y,z) row.
LIO_DEV void lio_knn_lds(const float4* s_pts, const int* s_cell, int rx1, int ry,
                         int rx0, int ry0, int rz0, int ry1, int rz1, int nx, int k,
                         float qx, float qy, float qz, int cx, int cy, int cz, LioTop5& top)
{
    const int xa = max(cx - k, 0), xb = min(cx + k, nx - 1);
    if (xa > xb) return;
#pragma unroll 1
    for (int dz = -k; dz <= k; ++dz) {
        const int z = cz + dz;
        if (z < rz0 || z > rz1) continue;
#pragma unroll 1
        for (int dy = -k; dy <= k; ++dy) {
            const int y = cy + dy;
            if (y < ry0 || y > ry1) continue;
            const int r = (z - rz0) * ry + (y - ry0);
            const int b = s_cell[r * rx1 + (xa - rx0)];
            const int e = s_cell[r * rx1 + (xb + 1 - rx0)];
            for (int j = b; j < e; ++j) {
                const float4 m = s_pts[j];
                const float d2 = lio_sqdist(m.x, m.y, m.z, qx, qy, qz);
                lio_top5_insert(top, lio_make_key(d2, __float_as_int(m.w)));
            }
        }
    }
}

#ifndef LIO_MIN_WAVES
#define LIO_MIN_WAVES 5      // waves per SIMD asked of the register allocator for the general one-point instantiation (<= 96 VGPRs; it
                             // spills 18 SGPRs to lanes and 12 VGPRs to 52 B of scratch; measured: 4 -> 5 is -6 % time, 6 spills
                             // inside the candidate loop and is 20 % slower); the other instantiations keep 4
#endif
#ifndef LIO_MIN_WAVES_PLAIN
#define LIO_MIN_WAVES_PLAIN 6   // the same for the plain instantiation (see k_s2m_iterate; make EXTRA=-DLIO_MIN_WAVES_PLAIN=5 for the A/B).
                                // Measured: 5 is +2.2 % registrations/s over the general kernel, 6 another +1.9 %.
                                // 6 (<= 80 VGPRs, 30 spilled, all of them in lio_gn_step) is admissible only while tools/count_valu.py
                                // shows no scratch access and no lane move between the kernel's entry and the arrival atomic
#endif
#define LIO_LDS_PTS   2048     // staged map points per workgroup (32 KiB)
#define LIO_LDS_CELLS 4096     // staged run offsets (16 KiB)
#define LIO_LDS_ROWS  256      // (y,z) rows of a region (one thread each)

// One thread = one scan point (x PPT points, strided by the workgroup size).
// STAGE: the workgroup's points are spatially sorted at upload, so their
// 27-cell neighbourhoods overlap heavily: the union region of the map is staged
// through LDS once (coalesced 16-byte loads) and every lane scans its
// candidates from LDS.  Regions that do not fit fall back to the global form;
// both forms visit the same candidate set, so results are identical.
// CORNER (extension): the same workgroup structure over the scan's EDGE points against
// the corner map with the point-to-line association of upstream LIO-SAM; its rows join the same
// per-scan sums (combineOptimizationCoeffs) through the partials of chunks n_surf_chunks.. .
// PLAIN (only with PPT == 1, !STAGE, !CORNER; chosen by lio_launch_iterate): the batch path of one device -- no map sharding
// (P.shard.axis < 0, P.blk_skip and P.sums_out null), no association record (P.rec_*, P.perm unused) and no phase clock
// (P.stamps null) are compile-time facts instead of wave-uniform values held in SGPRs across the whole kernel.  Same code,
// same arithmetic; the conditions below fold.
// A wave-uniform value that was loaded after the first store of a kernel sits in a VGPR of every lane (the compiler may only use
// scalar loads on memory nothing can have written yet): LOOPED, move it to an SGPR so that the register budget stays the same.
template <bool LOOPED> LIO_DEV int lio_uni(int v) { return LOOPED ? __builtin_amdgcn_readfirstlane(v) : v; }
template <bool LOOPED> LIO_DEV float lio_uni(float v) { return LOOPED ? __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))) : v; }

// The work of one association workgroup on ONE entry `wg` of P.blocks: the body of k_s2m_iterate (one entry per workgroup,
// LOOPED false) and of k_s2m_iterate_tail (the live entries of a fixed share of the list one after the other, LOOPED true:
// the caller has seen the entry's scan live in this launch, and `wg` is wave-uniform).
template <int PPT, bool STAGE, bool CORNER, bool PLAIN, bool LOOPED>
__device__ __forceinline__ void lio_s2m_block(const LioIterParams& P, const int wg)
{
    static_assert(!PLAIN || (PPT == 1 && !STAGE && !CORNER), "the plain instantiation is the one-point, unstaged surface kernel");
    static_assert(!LOOPED || PLAIN, "only the plain instantiation has a looped form");
    const bool sharded = !PLAIN && P.shard.axis >= 0;
    // LOOPED: opaque once per entry, so that nothing derived from the thread's index is hoisted out of the caller's loop and kept
    // in registers across all of it (LDS addresses, the reduction's column pair ..: the register budget is that of ONE entry)
    unsigned tid = threadIdx.x;
    if (LOOPED) asm volatile("" : "+v"(tid));
    __shared__ __attribute__((aligned(16))) double s_rows[LIO_BLOCK][8];  // [arz ary arx cx cy cz | -cw | accepted], widened once
    __shared__ double s_part[8][28];
    __shared__ double s_sum[28];
    __shared__ LioSolveWs s_ws;
    __shared__ __attribute__((aligned(16))) float4 s_pts[STAGE ? LIO_LDS_PTS : 1];
    __shared__ int s_cell[STAGE ? LIO_LDS_CELLS : 1];
    __shared__ int s_row_beg[STAGE ? LIO_LDS_ROWS : 1];
    __shared__ int s_row_off[STAGE ? LIO_LDS_ROWS + 1 : 1];
    __shared__ int s_box[8];
    __shared__ int s_scan4[4];

    // map sharding, decided per workgroup by k_shard_cull: 1 = it has already reported for this workgroup (not ours),
    // 2 = the WHOLE workgroup is ours (no per-point ownership test), 0 = per-point ownership
    const int wg_mode = (!PLAIN && P.blk_skip != nullptr) ? (int)P.blk_skip[wg] : 0;
    if (wg_mode == 1) return;
    const LioBlockDesc bd_ld = P.blocks[wg];
    const LioBlockDesc bd = { lio_uni<LOOPED>(bd_ld.scan), lio_uni<LOOPED>(bd_ld.first), lio_uni<LOOPED>(bd_ld.blk), lio_uni<LOOPED>(bd_ld.n_blk) };
    LioScanState* st = &P.state[bd.scan];
    if (!LOOPED && st->done) return;                       // workgroup-uniform
    // wave-uniform per-scan values, read BEFORE the first store of the kernel (the phase clock's stamp below): with no store
    // between the kernel's entry and these loads they are scalar loads into SGPRs, not 30 vector loads whose results every
    // lane holds in VGPRs.  (The scan's last workgroup rewrites T / Tp / trig in lio_gn_step after every workgroup of the
    // scan has arrived, i.e. after all of them have read these.)
    // (LOOPED: stores of earlier entries precede these loads; see lio_uni)
    float T[12], tr[6];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = st->T[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) tr[k] = st->trig[k];
    float Tp[12];                                          // the transform of the previous iteration (read only under use_cache)
#pragma unroll
    for (int k = 0; k < 12; ++k) Tp[k] = st->Tp[k];
    int n_pts = CORNER ? st->c_n_pts : st->n_pts;
    int base = CORNER ? st->c_offset : st->offset;
    int st_iter = st->iter;
    if (LOOPED) {
#pragma unroll
        for (int k = 0; k < 12; ++k) { T[k] = lio_uni<true>(T[k]); Tp[k] = lio_uni<true>(Tp[k]); }
#pragma unroll
        for (int k = 0; k < 6; ++k) tr[k] = lio_uni<true>(tr[k]);
        n_pts = lio_uni<true>(n_pts); base = lio_uni<true>(base); st_iter = lio_uni<true>(st_iter);
    }
    // diagnostic phase clock (P.stamps is null outside profiling experiments)
    long long* stamp = (!PLAIN && P.stamps) ? P.stamps + ((size_t)wg * (LIO_BLOCK / 64) + (tid >> 6)) * 8 : nullptr;
#define LIO_STAMP(k) do { if (stamp && (tid & 63) == 0) stamp[k] = (long long)__builtin_readcyclecounter(); } while (0)
    LIO_STAMP(0);

    const bool record = !PLAIN && (P.rec_flag != nullptr) && (st_iter == P.c.record_iter);
    const bool use_cache = (P.d5_cache != nullptr) && !STAGE && st_iter > 0;   // iteration 0 has nothing to re-use
    const LioGrid g_own = P.grid;
    const LioGrid& g = LOOPED ? P.grid : g_own;            // (LOOPED: P is memory the compiler does not see through; a copy would live in scratch)
    const int lane = tid & 63, wave = tid >> 6;

    // ---- phase A: transform (pointAssociateToMap, MO:841-847), cells, ownership
    float px[PPT], py[PPT], pz[PPT], qx[PPT], qy[PPT], qz[PPT];
    int cx[PPT], cy[PPT], cz[PPT];
    bool act[PPT], inr[PPT];
    int bmn[3] = { 0x7fffffff, 0x7fffffff, 0x7fffffff }, bmx[3] = { -0x7fffffff, -0x7fffffff, -0x7fffffff };
#pragma unroll
    for (int pp = 0; pp < PPT; ++pp) {
        const int li = bd.first + pp * LIO_BLOCK + (int)tid;
        inr[pp] = li < n_pts;
        const int gi = base + (inr[pp] ? li : 0);
        px[pp] = P.sx[gi]; py[pp] = P.sy[gi]; pz[pp] = P.sz[gi];     // coalesced SoA
        qx[pp] = T[0] * px[pp] + T[1] * py[pp] + T[2]  * pz[pp] + T[3];
        qy[pp] = T[4] * px[pp] + T[5] * py[pp] + T[6]  * pz[pp] + T[7];
        qz[pp] = T[8] * px[pp] + T[9] * py[pp] + T[10] * pz[pp] + T[11];
        bool a = inr[pp];
        if (sharded && wg_mode != 2) {                               // owner-computes (multi-GPU)
            const float qa = P.shard.axis == 0 ? qx[pp] : (P.shard.axis == 1 ? qy[pp] : qz[pp]);
            int gc = lio_cell_coord(qa, P.shard.gorigin, P.shard.inv_cell, P.shard.gdim);
            gc = min(max(gc, 0), P.shard.gdim - 1);
            a = a && gc >= P.shard.lo && gc < P.shard.hi;
        }
        cx[pp] = lio_cell_coord(qx[pp], g.ox, g.inv_cell, g.nx);
        cy[pp] = lio_cell_coord(qy[pp], g.oy, g.inv_cell, g.ny);
        cz[pp] = lio_cell_coord(qz[pp], g.oz, g.inv_cell, g.nz);
        // a point whose 27 cells all lie outside the grid has no candidates at all; a non-finite point has no
        // neighbours either (and would put NaN into the distance keys)
        a = a && (fabsf(qx[pp]) <= 3.0e38f) && (fabsf(qy[pp]) <= 3.0e38f) && (fabsf(qz[pp]) <= 3.0e38f);
        a = a && cx[pp] >= -g.k && cx[pp] < g.nx + g.k && cy[pp] >= -g.k && cy[pp] < g.ny + g.k &&
            cz[pp] >= -g.k && cz[pp] < g.nz + g.k;
        act[pp] = a;
        if (STAGE && a) {
            bmn[0] = min(bmn[0], cx[pp]); bmx[0] = max(bmx[0], cx[pp]);
            bmn[1] = min(bmn[1], cy[pp]); bmx[1] = max(bmx[1], cy[pp]);
            bmn[2] = min(bmn[2], cz[pp]); bmx[2] = max(bmx[2], cz[pp]);
        }
    }

    // A workgroup none of whose points is active (typically: owned by other ranks) only reports
    // an all-zero partial sum and leaves.
    if (sharded) {
        bool any = false;
#pragma unroll
        for (int pp = 0; pp < PPT; ++pp) any = any || act[pp];
        if (!__syncthreads_or(any ? 1 : 0)) {
            // the search bound of a point is only valid from one pass to the very next: drop it for points that sit this pass out
            if (P.d5_cache) {
#pragma unroll
                for (int pp = 0; pp < PPT; ++pp)
                    if (inr[pp]) P.d5_cache[base + bd.first + pp * LIO_BLOCK + (int)tid] = -1.0f;
            }
            // and their record is "not processed here", whatever an earlier run on the same upload left in it
            if (record) {
#pragma unroll
                for (int pp = 0; pp < PPT; ++pp) {
                    const int li = bd.first + pp * LIO_BLOCK + (int)tid;
                    if (inr[pp]) lio_record_unprocessed(P, P.perm ? P.perm[base + li] : base + li);
                }
            }
            if (wave != 0) return;
            double* part0 = P.partials + ((size_t)bd.scan * P.max_blk + bd.blk) * LIO_SUMS;
            if (lane < 28) __hip_atomic_store(part0 + lane, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            lio_arrive_and_finish<PLAIN>(P, bd, st, lane, s_sum, &s_ws, stamp);   // (recorded flags stay "rejected")
            return;
        }
    }

    // ---- phase B: stage the union cell region of the workgroup through LDS
    bool staged = false;
    int rx0 = 0, ry0 = 0, rz0 = 0, rx1c = 0, ry1 = -1, rz1 = -1, rxn1 = 1, ryn = 1;
    if (STAGE) {
        if (tid < 3) { s_box[tid] = 0x7fffffff; s_box[3 + tid] = -0x7fffffff; }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                bmn[a] = min(bmn[a], __shfl_xor(bmn[a], off));
                bmx[a] = max(bmx[a], __shfl_xor(bmx[a], off));
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { atomicMin(&s_box[a], bmn[a]); atomicMax(&s_box[3 + a], bmx[a]); }
        }
        __syncthreads();
        rx0 = max(s_box[0] - g.k, 0); rx1c = min(s_box[3] + g.k, g.nx - 1);
        ry0 = max(s_box[1] - g.k, 0); ry1 = min(s_box[4] + g.k, g.ny - 1);
        rz0 = max(s_box[2] - g.k, 0); rz1 = min(s_box[5] + g.k, g.nz - 1);
        const bool any = s_box[0] != 0x7fffffff && rx0 <= rx1c && ry0 <= ry1 && rz0 <= rz1;
        rxn1 = rx1c - rx0 + 2;                      // run offsets per row (cells + 1)
        ryn = ry1 - ry0 + 1;
        const int rzn = rz1 - rz0 + 1;
        const int n_rows = ryn * rzn;
        bool fits = any && n_rows <= LIO_LDS_ROWS && n_rows * rxn1 <= LIO_LDS_CELLS;
        if (fits) {                                  // workgroup-uniform
            // run of every (y,z) row of the region, exclusive scan of the run lengths
            int cnt = 0;
            if ((int)tid < n_rows) {
                const int z = rz0 + (int)tid / ryn, y = ry0 + (int)tid % ryn;
                const int row = (z * g.ny + y) * g.nx;
                const int b = P.cell_start[row + rx0];
                cnt = P.cell_start[row + rx1c + 1] - b;
                s_row_beg[tid] = b;
            }
            int total;
            const int off = lio_wg_exclusive_scan<LIO_BLOCK / 64>(cnt, &total, s_scan4);
            if ((int)tid < n_rows) s_row_off[tid] = off;
            if ((int)tid == n_rows) s_row_off[n_rows] = total;
            fits = total <= LIO_LDS_PTS;
            __syncthreads();
            if (fits) {
                for (int i = tid; i < n_rows * rxn1; i += LIO_BLOCK) {
                    const int r = i / rxn1, xi = i - r * rxn1;
                    const int z = rz0 + r / ryn, y = ry0 + r % ryn;
                    const int row = (z * g.ny + y) * g.nx;
                    s_cell[i] = s_row_off[r] + (P.cell_start[row + rx0 + xi] - s_row_beg[r]);
                }
                for (int i = tid; i < total; i += LIO_BLOCK) {
                    // row of staged slot i: last r with s_row_off[r] <= i
                    int lo = 0, hi = n_rows - 1;
                    while (lo < hi) {
                        const int mid = (lo + hi + 1) >> 1;
                        if (s_row_off[mid] <= i) lo = mid; else hi = mid - 1;
                    }
                    s_pts[i] = P.map_sorted[s_row_beg[lo] + (i - s_row_off[lo])];
                }
                staged = true;
            }
            __syncthreads();
        }
    }

    // Normal equations (matAtA = matAt*matA, matAtB = matAt*matB, MO:1781-1783) as
    // a transposed reduction: every lane parks its Jacobian row in LDS, then lane
    // (g, s) = (tid / 32, tid % 32) accumulates sum s over the points p = g (mod 8)
    // in fp64.  One accumulator per lane instead of 28, no cross-lane shuffles,
    // fixed summation order.
    const int red_g = tid >> 5, red_s = tid & 31;
    const int red_a = c_pair_a[red_s], red_b = c_pair_b[red_s];
    double red_acc = 0.0;
    LIO_STAMP(1);

#pragma unroll 1
    for (int pp = 0; pp < PPT; ++pp) {
        // ---- exact 5-NN over the 27-cell neighbourhood (MO:1631) ----
        // Search bound from the previous iteration (speed only).  The 5 neighbours found last time lie within
        // sqrt(d5_prev) of the point's previous position q_prev, hence within R = sqrt(d5_prev) + |q - q_prev| of
        // its new position q: the new 5th distance cannot exceed R, every member of the new 5-NN set lies
        // inside the x-cells [cell(qx - R), cell(qx + R)], and candidates beyond R^2 can be turned away by
        // the sentinel.  R is rounded up by 1e-4 (fp32 rounding of the distances is 1e-7).  Typically
        // R ~ 0.5 m against the 1 m gate: half the candidate run.  One float per point is kept.
        float bound2 = P.c.max_sq_dist;
        float Rx = P.c.gate_reach;                                    // reach along x: the gate, unless the bound below is tighter
        bool bounded = false;
        const int ci = base + bd.first + pp * LIO_BLOCK + (int)tid;   // slot in the batch SoA
        if (use_cache && act[pp]) {
            const float d5 = P.d5_cache[ci];
            if (d5 >= 0.0f) {
                const float ox = Tp[0] * px[pp] + Tp[1] * py[pp] + Tp[2]  * pz[pp] + Tp[3];
                const float oy = Tp[4] * px[pp] + Tp[5] * py[pp] + Tp[6]  * pz[pp] + Tp[7];
                const float oz = Tp[8] * px[pp] + Tp[9] * py[pp] + Tp[10] * pz[pp] + Tp[11];
                float rd5, mv;
                lio_bound_roots<!LOOPED>(d5, lio_sqdist(qx[pp], qy[pp], qz[pp], ox, oy, oz), rd5, mv);
                const float R = (rd5 + mv) * 1.0001f + 1e-6f;
                const float r2 = R * R * 1.0001f;
                if (r2 < bound2) { bound2 = r2; Rx = R; bounded = true; }
            }
        }
        // (d2 == bound2 with any real index sorts below the sentinel, so ties at the bound are kept)
        const double sentinel = lio_make_key(bound2, -1);                 // index 0xffffffff: above every real index
        LioTop5 top = { sentinel, sentinel, sentinel, sentinel, sentinel };
        if (act[pp]) {
            if (STAGE && staged)
                lio_knn_lds(s_pts, s_cell, rxn1, ryn, rx0, ry0, rz0, ry1, rz1, g.nx, g.k,
                            qx[pp], qy[pp], qz[pp], cx[pp], cy[pp], cz[pp], top);
            else
                lio_knn_global(P, g, qx[pp], qy[pp], qz[pp], cy[pp], cz[pp], Rx, bound2, bounded, top);
        }
        int nn[5] = { lio_key_idx(top.k0), lio_key_idx(top.k1), lio_key_idx(top.k2), lio_key_idx(top.k3), lio_key_idx(top.k4) };
        const float d2_5 = lio_key_d2(top.k4);
        // gate MO:1641: pointSearchSqDis[4] < 1.0
        const bool ok = act[pp] && (d2_5 < P.c.max_sq_dist);
        if (pp == 0) LIO_STAMP(2);

        if (P.d5_cache && inr[pp])                                    // for the next iteration (-1: nothing to re-use)
            P.d5_cache[ci] = ok ? d2_5 : -1.0f;
        float cxx = 0.0f, cyy = 0.0f, czz = 0.0f, cww = 0.0f;
        bool accept = false;
        // plane through the five neighbours, plane test, weight, coefficients MO:1642-1683 (the CORNER extension: point-to-line);
        // the same function the one-launch loop calls (lio_s2m_device.h): one copy of the arithmetic
        if (ok) accept = lio_assoc_point<CORNER, !LOOPED>(P, nn, qx[pp], qy[pp], qz[pp], px[pp], py[pp], pz[pp], cxx, cyy, czz, cww);
        if (record && inr[pp]) {
            // the record is kept in the CALLER's point order
            const int li = bd.first + pp * LIO_BLOCK + (int)tid;
            const int oi = P.perm ? P.perm[base + li] : base + li;
            P.rec_flag[oi] = accept ? 1 : 0;
            reinterpret_cast<float4*>(P.rec_coeff)[oi] = make_float4(cxx, cyy, czz, cww);
#pragma unroll
            for (int j = 0; j < 5; ++j) P.rec_nn[(size_t)oi * 5 + j] = ok ? nn[j] : -1;
        }
        // MO:1735-1778: row of matA / matB (zero row when the point is rejected)
        float row[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }, rhs = 0.0f;
        if (accept) lio_jacobian_row(tr, px[pp], py[pp], pz[pp], cxx, cyy, czz, cww, P.c.jac_exact, row, rhs);
        if (PPT > 1) __syncthreads();                                  // previous pass finished reading
        {   // each value is converted to fp64 once here instead of once per product below
            double2* dst = reinterpret_cast<double2*>(s_rows[tid]);
            dst[0] = make_double2((double)row[0], (double)row[1]);
            dst[1] = make_double2((double)row[2], (double)row[3]);
            dst[2] = make_double2((double)row[4], (double)row[5]);
            dst[3] = make_double2((double)rhs, accept ? 1.0 : 0.0);
        }
        if (pp == 0) LIO_STAMP(3);
        __syncthreads();
        if (red_s < 28) {
#pragma unroll 8
            for (int p = red_g; p < LIO_BLOCK; p += 8)
                red_acc = __builtin_fma(s_rows[p][red_a], s_rows[p][red_b], red_acc);   // the product of two widened fp32 is exact: fma == mul, add
        }
    }
    LIO_STAMP(4);
    if (red_s < 28) s_part[red_g][red_s] = red_acc;
    __syncthreads();
    LIO_STAMP(5);
    if (wave != 0) return;

    double* part = P.partials + ((size_t)bd.scan * P.max_blk + bd.blk) * LIO_SUMS;
    if (lane < 28) {
        double v = s_part[0][lane];
#pragma unroll
        for (int w = 1; w < 8; ++w) v += s_part[w][lane];
        // write-through (sc1) store: visible to the other XCDs without a release fence
        __hip_atomic_store(part + lane, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    lio_arrive_and_finish<PLAIN>(P, bd, st, lane, s_sum, &s_ws, stamp);
    LIO_STAMP(7);
#undef LIO_STAMP
}

