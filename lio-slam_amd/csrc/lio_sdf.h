// lio_sdf.h -- the signed distance field behind the planning height map (lio_sdf.hip): grid_map_sdf's arithmetic (GS =
// grid_map_sdf: PixelBorderDistance.hpp = PBD, SignedDistance2d.cpp = SD2, SignedDistanceField.cpp = SDF, DistanceDerivatives.hpp
// = DD, Gridmap3dLookup.hpp = G3L) as __host__ __device__ functions over accessors, so that the kernels (device arrays) and a
// host program (checked arrays) run the same text.  DESIGN.md section 4i lists the conventions.  Everything here relies on
// -ffp-contract=off; every float expression is fp32 in the order the reference writes it.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "../../include/liogpu.h"
#include "lio_gridmath.h"

#define LIO_SDF_INF (__builtin_huge_valf())          // Utils.hpp:18; it flows through the expressions below, never special-cased
#define LIO_SDF_MAX_LINE (1 << 24)                   // a pixel index must be exact as a float (the float loop counters)
#define LIO_SDF_MAX_NODES ((long long)LIO_SDF_NODE_LIMIT)   // 16 bytes each: 512 MiB of nodes, 128 MiB of distances
#define LIO_SDF_MAX_SLAB 32                          // layers per slab: 64 (layer, class) pairs, a wave
#define LIO_SDF_WS_BUDGET (128LL << 20)              // the slab shrinks until 24 bytes x cells x slab fits (never below 1 layer)

enum { LIO_SDF_MIXED = 0, LIO_SDF_ALL_OBSTACLE = 1, LIO_SDF_ALL_FREE = 2 };     // the three branches of SD2:242-261
enum { LIO_SDF_TO_OBSTACLE = 0, LIO_SDF_TO_FREE = 1 };                          // the two transforms of a layer

// ---- PBD:26-101 -----------------------------------------------------------------------------------------------------------
LIO_HD float lio_sdf_pbd(float i, float j)
{
    const float a = fabsf(i - j) - 0.5f;
    return a < 0.0f ? 0.0f : a;                      // std::max(a, 0.0F)
}

LIO_HD float lio_sdf_sq_pbd(float i, float j, float f)
{
    const float d = lio_sdf_pbd(i, j);
    return d * d + f;
}

// the point right of the origin that is as far from it as from pixel p > 0 carrying the offset fp: five solutions
LIO_HD float lio_sdf_right_of_origin(float p, float fp)
{
    const float pp = p * p;
    if (fp > pp) return (pp + p + fp) / (2.0f * p);
    if (fp < -pp) return (pp - p + fp) / (2.0f * p);
    const float bound = pp - 2.0f * p + 1.0f;
    if (fp > bound) return 0.5f + sqrtf(fp);
    if (fp < -bound) return p - 0.5f - sqrtf(-fp);
    return (pp - p + fp) / (2.0f * p - 2.0f);
}

LIO_HD float lio_sdf_equidistance(float q, float fq, float p, float fp)
{
    if (fp == fq) return 0.5f * (p + q);
    const float df = fp - fq, dr = p - q;
    const float off = dr > 0.0f ? lio_sdf_right_of_origin(dr, df) : -lio_sdf_right_of_origin(-dr, df);
    return off + q;
}

// ---- the 1-D transform of a line, SD2:30-167 ------------------------------------------------------------------------------
// In::at(q), q in [0, n): the untouched input of the line (the transform here writes elsewhere: the reference overwrites
// entry q after its last read of it, and keeps the offsets it still needs by value).
// The lower-bound stack keeps, per bound, the pixel index and z_rhs: z_lhs is the z_rhs of the bound below (-INF for the
// first live bound) and f is In::at(index).  Stk: v(k), z(k), set(k, v, z), set_z(k, z), k in [0, n).
template <class In>
LIO_HD int lio_sdf_last_zero(const In& in, int n)
{
    for (int q = 0; q < n; ++q)
        if (in.at(q) > 0.0f) return q > 0 ? q - 1 : 0;
    return n;
}

// -> the first live bound; *top_out = the last one
template <class In, class Stk>
LIO_HD int lio_sdf_fill_bounds(const In& in, int n, int start, Stk& st, int* top_out)
{
    const float nf = (float)n, sf = (float)start;
    int first = 0, top = 0;
    float tv = sf, tf = in.at(start), tzl = -LIO_SDF_INF;          // the top bound: origin, offset, z_lhs
    st.set(0, start, LIO_SDF_INF);
    float qf = tv + 1.0f;
    for (int q = start + 1; q < n; ++q) {
        const float fq = in.at(q);
        float s = lio_sdf_equidistance(qf, fq, tv, tf);
        if (s < nf) {                                              // else: active right of the line only
            while (s < tzl) {                                      // (tzl is -INF at `first`: the search stays among live bounds)
                --top;
                const int v = st.v(top);
                tv = (float)v; tf = in.at(v);
                tzl = top == first ? -LIO_SDF_INF : st.z(top - 1);
                s = lio_sdf_equidistance(qf, fq, tv, tf);
            }
            if (s > sf) {
                st.set_z(top, s);
                ++top;
                st.set(top, q, LIO_SDF_INF);
                tzl = s;
            } else {                                               // dominates everything before it: the first bound moves here
                st.set(top, q, LIO_SDF_INF);
                tzl = -LIO_SDF_INF;
                first = top;
            }
            tv = qf; tf = fq;
        }
        qf += 1.0f;
    }
    *top_out = top;
    return first;
}

// extractSquareDistances / extractDistances as a cursor: at(q) for q = 0, 1, .. n - 1 in this order gives the line's output.
// (float)q equals the reference's counter, which starts at (float)start and grows by 1.0F: both are exact below 2^24.
template <bool SQRT>
struct LioSdfCursor {
    int start, it, top;
    float lastz;
    template <class In, class Stk>
    LIO_HD void begin(const In& in, int n, Stk& st)
    {
        start = lio_sdf_last_zero(in, n);
        it = top = 0;
        lastz = LIO_SDF_INF;
        if (start < n) {
            it = lio_sdf_fill_bounds(in, n, start, st, &top);
            lastz = st.z(it);
        }
    }
    template <class In, class Stk>
    LIO_HD float at(const In& in, const Stk& st, int q)
    {
        const float x = in.at(q);
        if (q < start || !(x > 0.0f)) return x;                    // the leading zeros and every zero stay
        const float qf = (float)q;
        if (qf > lastz) {
            do { ++it; } while (it < top && st.z(it) < qf);        // (the top bound's z_rhs is INF: `it < top` never decides)
            lastz = st.z(it);
        }
        const int v = st.v(it);
        const float d2 = lio_sdf_sq_pbd(qf, (float)v, in.at(v));
        return SQRT ? sqrtf(d2) : d2;
    }
};

// ---- layers ---------------------------------------------------------------------------------------------------------------
// SD2:190-213: the squared height distance in pixels, ((1 / res) * max(h - e, 0))^2 towards obstacles, min towards free space
LIO_HD float lio_sdf_init(float e, float h, float inv_res, int cls)
{
    const float d = h - e;
    const float m = cls == LIO_SDF_TO_OBSTACLE ? (d < 0.0f ? 0.0f : d) : (0.0f < d ? 0.0f : d);
    const float t = inv_res * m;
    return t * t;
}

// SD2:229 / :234: an occupancy grid's offsets
LIO_HD float lio_sdf_init_occupancy(bool occupied, int cls)
{
    return (cls == LIO_SDF_TO_OBSTACLE) == occupied ? 0.0f : LIO_SDF_INF;
}

// SDF:112-134: gridOriginZ, gridOriginZ + resolution, then gridOriginZ + (layerZ + 1) * resolution with layerZ + 1 = z
LIO_HD float lio_sdf_layer_height(float origin_z, float res, int z)
{
    if (z == 0) return origin_z;
    if (z == 1) return origin_z + res;
    return origin_z + (float)z * res;
}

// SD2:244-245 with SDF:83-84: decided by the elevation layer's own extremes
LIO_HD int lio_sdf_layer_mode(float h, float e_min, float e_max)
{
    if (h < e_min) return LIO_SDF_ALL_OBSTACLE;
    if (h > e_max) return LIO_SDF_ALL_FREE;
    return LIO_SDF_MIXED;
}

LIO_HD bool lio_sdf_mode_uses(int mode, int cls)
{
    return mode == LIO_SDF_MIXED || (mode == LIO_SDF_ALL_OBSTACLE) == (cls == LIO_SDF_TO_FREE);
}

// SD2:250 / :254 / :259 (and :237)
LIO_HD float lio_sdf_combine(int mode, float to_obstacle, float to_free, float res)
{
    if (mode == LIO_SDF_ALL_OBSTACLE) return to_free * -res;
    if (mode == LIO_SDF_ALL_FREE) return to_obstacle * res;
    return res * (to_obstacle - to_free);
}

// SDF:35 in double
inline long long lio_sdf_num_layers(double min_h, double max_h, double res)
{
    const double n = ceil((max_h - min_h) / res);
    return n > 2.0 ? (n < 9.0e18 ? (long long)n : (long long)9.0e18) : 2;
}

// ---- DD:24-59 as SDF:120-161 applies them ---------------------------------------------------------------------------------
// Differences of one axis: the one-sided factor 1 / step at the ends, 1 / (2 * step) between.  lo, mid, hi: the values at
// i - 1, i, i + 1 (only the ones the position needs are read by the callers).
LIO_HD float lio_sdf_diff(int i, int n, float lo, float mid, float hi, float step)
{
    if (i == 0) return (1.0f / step) * (hi - mid);
    if (i == n - 1) return (1.0f / step) * (mid - lo);
    return (1.0f / (2.0f * step)) * (hi - lo);
}

// S::at(r, c, z): the distance layers.  {distance, dx, dy, dz}: dx along the rows and dy along the columns with -res (x and
// y fall as the indices grow), dz along the layers with +res.  rows, cols, layers >= 2.
template <class S>
LIO_HD float4 lio_sdf_node(const S& sd, int r, int c, int z, int rows, int cols, int layers, float res)
{
    const float d = sd.at(r, c, z);
    const float dx = lio_sdf_diff(r, rows, r > 0 ? sd.at(r - 1, c, z) : d, d, r + 1 < rows ? sd.at(r + 1, c, z) : d, -res);
    const float dy = lio_sdf_diff(c, cols, c > 0 ? sd.at(r, c - 1, z) : d, d, c + 1 < cols ? sd.at(r, c + 1, z) : d, -res);
    const float dz = lio_sdf_diff(z, layers, z > 0 ? sd.at(r, c, z - 1) : d, d, z + 1 < layers ? sd.at(r, c, z + 1) : d, res);
    return make_float4(d, dx, dy, dz);
}

// ---- G3L:69-101, SDF:58-78 ------------------------------------------------------------------------------------------------
struct LioSdfLookup {
    int rows, cols, layers;
    double origin[3], res;         // the centre of cell (0, 0) and the band's lower end
};

// getNearestPositiveInteger: std::round, then std::min and std::max as written (a NaN ends at 0)
LIO_HD int lio_sdf_nearest_index(double val, double mx)
{
    const double r = round(val);
    const double m = mx < r ? mx : r;
    return (int)(0.0 < m ? m : 0.0);
}

LIO_HD void lio_sdf_nearest_node(const LioSdfLookup& L, const double p[3], int idx[3])
{
    const double inv = 1.0 / L.res;
    idx[0] = lio_sdf_nearest_index((L.origin[0] - p[0]) * inv, (double)(L.rows - 1));
    idx[1] = lio_sdf_nearest_index((L.origin[1] - p[1]) * inv, (double)(L.cols - 1));
    idx[2] = lio_sdf_nearest_index((p[2] - L.origin[2]) * inv, (double)(L.layers - 1));
}

LIO_HD size_t lio_sdf_linear_index(const LioSdfLookup& L, const int idx[3])
{
    return ((size_t)idx[2] * (size_t)L.cols + (size_t)idx[1]) * (size_t)L.rows + (size_t)idx[0];
}

// valueAndDerivative: distance + derivative . (position - nodePosition) in double, the dot summed x, y, z left to right
// N::at(i): node i as float4
template <class N>
LIO_HD double lio_sdf_value(const LioSdfLookup& L, const N& nodes, const double p[3], double der[3])
{
    int idx[3];
    lio_sdf_nearest_node(L, p, idx);
    const double nx = L.origin[0] - (double)idx[0] * L.res, ny = L.origin[1] - (double)idx[1] * L.res, nz = L.origin[2] + (double)idx[2] * L.res;
    const float4 n = nodes.at(lio_sdf_linear_index(L, idx));
    der[0] = (double)n.y; der[1] = (double)n.z; der[2] = (double)n.w;
    const double dot = (der[0] * (p[0] - nx) + der[1] * (p[1] - ny)) + der[2] * (p[2] - nz);
    return (double)n.x + dot;
}

// ---- the host side (lio_sdf.hip) --------------------------------------------------------------------------------------------
// what can be refused before any device is touched: LIO_OK or LIO_ERR_ARG
int lio_sdf_check(const lio_sdf_config* cfg, int rows, int cols, double resolution, const double length[2], const double position[2]);
// the configuration alone: LIO_OK or LIO_ERR_ARG
int lio_sdf_config_check(const lio_sdf_config* cfg);
// What a chained entry point does before its first launch: LIO_ERR_ARG for an object on another device than `device_id`; the
// object then holds no field until a build succeeds.
int lio_sdf_begin(lio_sdf* sdf, int device_id);
// SignedDistanceField's constructor on the device grid d_elev (rows x cols, column-major) on stream s, for an entry point that
// has the grid on the device already; the geometry was checked (lio_sdf_check).  Synchronous.
int lio_sdf_build_device(lio_sdf* sdf, const float* d_elev, int rows, int cols, double resolution, const double* length, const double* position,
                         const lio_sdf_config& cfg, lio_sdf_info* info, hipStream_t s);
