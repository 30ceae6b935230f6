// lio_gridtransform.h -- grid_map::GridMap::getTransformedMap (GM = grid_map_core/src/GridMap.cpp:332-436) and
// GridMapRosConverter::toOccupancyGrid (GridMapRosConverter.cpp:329-365) behind the resident layer set
// (lio_gridtransform.hip): the new geometry, the sample positions, the transform, the key of the order-independent winner
// rule and the occupancy value as __host__ __device__ functions, so that the kernels and a host program
// (tools/grid_transform_host_check.cpp) run the same text.  Everything is fp64 in the order the reference writes it and
// relies on -ffp-contract=off.  The geometry and the destination index (lio_gm_index) are lio_gridmath.h's.  startIndex is
// always 0.  DESIGN.md section 4m lists the conventions, the argument for the rule and the labelled deviations (parity
// unpinned).
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "../../include/liogpu.h"
#include "lio_gridmath.h"
#include "lio_wg.h"

// visit number = 5 * (source linear index) + sample, kept in 31 bits of the key: 5 * cells <= 2^31
#define LIO_GT_MAX_SOURCE_CELLS LIO_GRID_TRANSFORM_MAX_SOURCE_CELLS

struct LioGtXf { double m[12]; };  // rows of [R | t]

// transform * p, one component: ((R_i0 x + R_i1 y) + R_i2 z) + t_i (Eigen's own order inside the product is not defined by
// the source: unpinned)
LIO_HD double lio_gt_apply(const LioGtXf& T, int i, double x, double y, double z)
{
    return ((T.m[4 * i] * x + T.m[4 * i + 1] * y) + T.m[4 * i + 2] * z) + T.m[4 * i + 3];
}

// GM:347-375: the four corners position +- 0.5 length at z = 0 in the order top left, top right, bottom left, bottom right,
// each transformed; their sum from zero in that order times 0.25; the largest |corner - centre| per axis, doubled.
LIO_HD void lio_gt_new_extent(const double length[2], const double position[2], const LioGtXf& T, double centre[2], double new_length[2])
{
    const double hx = length[0] * 0.5, hy = length[1] * 0.5;
    const double cx[4] = { position[0] + hx, position[0] + hx, position[0] - hx, position[0] - hx };
    const double cy[4] = { position[1] + hy, position[1] - hy, position[1] + hy, position[1] - hy };
    double e[4][2];
    for (int k = 0; k < 4; ++k)
        for (int a = 0; a < 2; ++a) e[k][a] = lio_gt_apply(T, a, cx[k], cy[k], 0.0);
    for (int a = 0; a < 2; ++a) {
        double c = 0.0;
        for (int k = 0; k < 4; ++k) c += e[k][a];
        c *= 0.25;
        double m = 0.0;
        for (int k = 0; k < 4; ++k) m = fmax(fabs(e[k][a] - c), m);
        centre[a] = c;
        new_length[a] = 2.0 * m;
    }
}

// GM:394-403: sample s of a cell centred on (cx, cy): the centre, then x - l, x + l, y - l, y + l
LIO_HD void lio_gt_sample(double cx, double cy, double sample_length, int s, double* x, double* y)
{
    *x = s == 1 ? cx - sample_length : (s == 2 ? cx + sample_length : cx);
    *y = s == 3 ? cy - sample_length : (s == 4 ? cy + sample_length : cy);
}

// ---- the rule of GM:416-431 without its order.  Serially a sample is skipped when the cell's stored float, widened, is
// greater than the sample's double z, and otherwise stores (float)z.  Per new cell, with F the largest (float)z among its
// samples (-0.0f and +0.0f are one class: they compare equal): a sample with (float)z == F and z >= (double)F always writes
// when it is met, and after any write of the class the stored float is F, which only such samples overwrite; so the last of
// them wins.  Where there is none, the first sample of the class writes (the stored float is still NaN or below F, and a z
// that rounds up to F is not below any float under F) and every later one is skipped.  As one integer whose maximum is the
// winner: the ordered bits of F, one bit "z >= F", then the visit number, or its complement where the first one wins.
// No key is 0 (the ordered word of -inf is 0x007fffff): 0 marks a cell nothing reached.  z must not be NaN: the entry point
// refuses transforms under which it could be.
LIO_HD unsigned long long lio_gt_key(double z, unsigned visit)
{
    float f = (float)z;
    if (__builtin_bit_cast(unsigned, f) == 0x80000000u) f = 0.0f;
    const bool high = z >= (double)f;
    const unsigned low = high ? (0x80000000u | visit) : (0x7fffffffu - visit);
    return ((unsigned long long)lio_f2ord(f) << 32) | (unsigned long long)low;
}

LIO_HD unsigned lio_gt_key_visit(unsigned long long key)
{
    const unsigned low = (unsigned)key;
    return (low & 0x80000000u) ? (low & 0x7fffffffu) : (0x7fffffffu - low);
}

// One source cell of the loop (GM:385-433) up to the rule: its samples in order, each transformed and looked up in the new
// map; sink.put(new linear index, key) for those inside.  lin is the column-major linear index (GridMapIterator's order
// and the layer's memory order), h the cell's finite height.  Returns the samples whose getIndex failed.
template <class Sink>
LIO_HD int lio_gt_cell(const LioGridGeom& S, const LioGridGeom& D, const LioGtXf& T, double sample_length, int n_samples, int lin, float h, Sink& sink)
{
    const int r = lin % S.rows, c = lin / S.rows;
    const double cx = lio_gm_centre(S, 0, r), cy = lio_gm_centre(S, 1, c), z = (double)h;
    int outside = 0;
    for (int s = 0; s < n_samples; ++s) {
        double x, y;
        lio_gt_sample(cx, cy, sample_length, s, &x, &y);
        const double tx = lio_gt_apply(T, 0, x, y, z), ty = lio_gt_apply(T, 1, x, y, z), tz = lio_gt_apply(T, 2, x, y, z);
        int i, j;
        if (!lio_gm_index(D, tx, ty, &i, &j)) { ++outside; continue; }
        sink.put((size_t)j * (size_t)D.rows + (size_t)i, lio_gt_key(tz, 5u * (unsigned)lin + (unsigned)s));
    }
    return outside;
}

// The height the winning visit stores: (float) of its transformed z, formed again from the source cell
LIO_HD float lio_gt_visit_height(const LioGridGeom& S, const LioGtXf& T, double sample_length, unsigned visit, float h)
{
    const int lin = (int)(visit / 5u), s = (int)(visit % 5u);
    const int r = lin % S.rows, c = lin / S.rows;
    double x, y;
    lio_gt_sample(lio_gm_centre(S, 0, r), lio_gm_centre(S, 1, c), sample_length, s, &x, &y);
    return (float)lio_gt_apply(T, 2, x, y, (double)h);
}

// toOccupancyGrid's cell (GridMapRosConverter.cpp:356-363), in float: NaN -> -1, otherwise 0 + min(max(0, value), 1) * 100
// with std::max / std::min as written (the first argument where neither is smaller), truncated to int8_t
LIO_HD int8_t lio_gt_occupancy(float v, float data_min, float data_max)
{
    float value = (v - data_min) / (data_max - data_min);
    if (value != value) value = -1.0f;
    else {
        const float lo = 0.0f < value ? value : 0.0f;       // max(0.0f, value)
        const float hi = 1.0f < lo ? 1.0f : lo;              // min(.., 1.0f)
        value = 0.0f + hi * 100.0f;
    }
    return (int8_t)value;
}
