// lio_gridmath.h -- the library's GridMapMath: grid_map's geometry (GM = grid_map_core/src/GridMap.cpp, GMM =
// GridMapMath.cpp) as every planning stage reads it.  The members setGeometry leaves, the one function that derives them,
// getPositionFromIndex, getIndexFromPosition with checkIfPositionWithinMap, boundPositionToRange, and the rule by which an
// entry point accepts a caller's geometry, with the two questions every stage asks of a cell (is it finite, which cells of a
// window lie in the grid): each exists here and nowhere else.  startIndex is always 0 (the library's grids are
// never circular buffers).  Everything is fp64 in the order the reference writes it and relies on -ffp-contract=off.  The two
// labelled deviations from the reference are lio_gm_bound_index's clamp and verdict 1 of lio_gm_lookup (DESIGN.md section 4,
// "The grid geometry").
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "../../include/liogpu.h"

#define LIO_HD __host__ __device__ __forceinline__
#define LIO_QNAN_BITS 0x7fc00000u                            // NAN as the reference's layers hold it; __builtin_nanf("") is this word
#define LIO_QNAN __builtin_bit_cast(float, LIO_QNAN_BITS)

// std::isfinite of a cell, as isValid and every filter ask it
LIO_HD bool lio_gm_finite(float v) { return fabsf(v) <= FLT_MAX; }

// [i - R, i + R] with both ends brought into [0, n - 1]: boundIndexToRange on the two corners of a window of cells
LIO_HD void lio_gm_clip(int i, int R, int n, int& lo, int& hi)
{
    lo = i - R < 0 ? 0 : i - R;
    hi = i + R > n - 1 ? n - 1 : i + R;
}

// grid_map's geometry as the iterators read it; base = position + (0.5 length - 0.5 resolution) (getVectorToFirstCell).
// rows = size(0) along x, cols = size(1) along y.  A kernel argument by value: the layout is part of the kernels' code.
struct LioGridGeom {
    double pos[2], len[2], half[2], base[2], res;
    int rows, cols;
};

// setGeometry's size along one axis (GM:50), as a double: round(length / resolution), halves away from zero.  The caller
// refuses what is not in [1, 2^24) before it becomes an int.
LIO_HD double lio_gm_size(double new_length, double resolution) { return round(new_length / resolution); }

// the members setGeometry leaves (GM:44-59) for a size already decided: length = size * resolution
LIO_HD LioGridGeom lio_gm_geom(int rows, int cols, double res, double px, double py)
{
    LioGridGeom G;
    G.rows = rows; G.cols = cols; G.res = res;
    G.pos[0] = px; G.pos[1] = py;
    G.len[0] = (double)rows * res; G.len[1] = (double)cols * res;
    for (int a = 0; a < 2; ++a) {
        G.half[a] = 0.5 * G.len[a];                          // getVectorToOrigin
        G.base[a] = G.pos[a] + (G.half[a] - 0.5 * res);      // mapPosition + getVectorToFirstCell
    }
    return G;
}

// getPositionFromIndex (GridMapMath.cpp:130-145), default start index, one component
LIO_HD double lio_gm_centre(const LioGridGeom& G, int a, int i) { return G.base[a] + G.res * (double)(-i); }

// boundPositionToRange (GridMapMath.cpp:255-280) then getIndexFromPosition (:147-160), one component.  The reference
// ignores getIndexFromPosition's verdict; an index outside the buffer (a length whose last ulp swallows the epsilon) would
// read past it there and is brought back to the last cell here.
LIO_HD int lio_gm_bound_index(const LioGridGeom& G, int a, double p)
{
    double eps = 10.0 * DBL_EPSILON;
    if (fabs(p) > 1.0) eps *= fabs(p);
    double sh = (p - G.pos[a]) + G.half[a];
    if (sh <= 0.0) sh = eps;
    else if (sh >= G.len[a]) sh = G.len[a] - eps;
    const double q = (sh + G.pos[a]) - G.half[a];
    const double v = ((q - G.half[a]) - G.pos[a]) / G.res;
    const int n = a == 0 ? G.rows : G.cols;
    const int idx = (int)(-v);
    return idx < 0 ? 0 : (idx >= n ? n - 1 : idx);
}

// checkIfPositionWithinMap (GMM:162-172): -((p - position) - 0.5 length) in [0, length) on both axes -- the high edge is
// inside, the low edge is not; a non-finite position fails every comparison.  Then getIndexFromPosition (:147-160):
// (int)(-v) per component, v = ((p - 0.5 length) - position) / resolution, and checkIfIndexInRange on it (a position within
// an ulp of the low edge can round to index n: outside as well, where the reference throws).
LIO_HD bool lio_gm_index(const LioGridGeom& G, double px, double py, int* i, int* j)
{
    const double p[2] = { px, py };
    int idx[2] = { 0, 0 };
    bool in = true;
    for (int a = 0; a < 2; ++a) {
        const double t = -((p[a] - G.pos[a]) - G.half[a]);
        if (!(t >= 0.0 && t < G.len[a])) { in = false; continue; }
        const double v = ((p[a] - G.half[a]) - G.pos[a]) / G.res;
        const int n = a == 0 ? G.rows : G.cols;
        idx[a] = (int)(-v);                                // (|v| <= n + 1 here: the conversion is defined)
        if (idx[a] < 0 || idx[a] >= n) in = false;
    }
    *i = idx[0]; *j = idx[1];
    return in;
}

// isInside then getIndex on G, as extendToInclude (GM:617-620) and addDataFrom (GM:539-542) call them: 0 the position is not
// inside the map, 2 the index (*i, *j) is the cell's.  1: inside, but getIndex fails (a position within an ulp of the low
// edge rounds to index n).  The reference ignores that verdict and reads past the buffer; the callers here skip the cell and
// count it (the labelled deviation).  With no index out of range, what remains of lio_gm_index is checkIfPositionWithinMap.
LIO_HD int lio_gm_lookup(const LioGridGeom& G, double px, double py, int* i, int* j)
{
    if (lio_gm_index(G, px, py, i, j)) return 2;
    LioGridGeom W = G;
    W.rows = W.cols = 0x7fffffff;
    int wi, wj;
    return lio_gm_index(W, px, py, &wi, &wj) ? 1 : 0;
}

// ---- what an entry point accepts of a caller's geometry, on the host: nullptr, or the message of the refusal (LIO_ERR_ARG).
// The limits on rows and cols are each caller's own, and so is the order in which it asks.
inline const char* lio_gm_resolution_refusal(double resolution)
{
    return (!std::isfinite(resolution) || resolution < 1e-4) ? "resolution must be finite and at least 1e-4" : nullptr;
}

// Axis by axis.  Past it length == size * resolution exactly, so lio_gm_geom(rows, cols, resolution, position) has the
// caller's length bit for bit.
inline const char* lio_gm_axes_refusal(int rows, int cols, double resolution, const double* length, const double* position)
{
    for (int a = 0; a < 2; ++a) {
        if (!std::isfinite(length[a]) || !std::isfinite(position[a])) return "length and position must be finite";
        if (length[a] != (double)(a == 0 ? rows : cols) * resolution) return "length must be size * resolution (GridMap::setGeometry)";
    }
    return nullptr;
}
