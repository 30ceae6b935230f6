// lio_gridfilter.h -- grid_map_filters on a resident layer (lio_gridfilter.hip): MinInRadiusFilter, MeanInRadiusFilter,
// SlidingWindowMathExpressionFilter over SlidingWindowIterator's four edge modes, CurvatureFilter and ThresholdFilter.  The
// per-cell arithmetic as __host__ __device__ functions over a grid accessor, so that the kernels (an LDS tile, or the layer
// itself) and a host program (a checked array) run the same text.  The base of the one-lane-per-cell stages: the circle's
// window, sumOfFinites and the halo of a reach live here, and the terrain layers (whose header includes this
// one) call the MEAN and the STDDEV / CROP cells for their smooth and edges layers.  DESIGN.md section 4p lists the
// conventions and the labelled deviations (parity unpinned).  Everything here relies on -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include "../../include/liogpu.h"
#include "lio_gridmath.h"
#include "lio_gridtile.h"

#define LIO_GF_N_RADIUS_OPS 2
#define LIO_GW_N_EDGES 4
#define LIO_GW_N_OPS 7
#define LIO_GW_MAX_SIZE (2 * LIO_TILE_MAX_REACH + 1)

// what one cell of a filter yields: `value` is stored where `written`, the quiet NaN 0x7fc00000 elsewhere
struct LioGfCell {
    float value;
    bool visited, written;
};

// ---- MinInRadiusFilter.cpp:50-93, MeanInRadiusFilter.cpp:51-82
struct LioGfRadius {
    LioGridGeom G;
    double radius;
    int halo;                      // lio_gf_halo(radius / resolution), or wider: what lio_gf_circle_window never leaves
};

// The cells a circle of `reach` cells can hold on either side of its centre: a circle's window ends at
// trunc(i + 0.5 +- reach) up to the rounding of its corner, hence one cell of slack (section 4g.1).
LIO_HD int lio_gf_halo(double reach) { return (int)floor(reach + 0.5) + 1; }

// CircleIterator::findSubmapParameters: [lo, hi] of the candidates along one axis, additionally kept within `halo` cells
// of the centre (never narrower than the reference's window when halo >= lio_gf_halo(radius / resolution))
LIO_HD void lio_gf_circle_window(const LioGridGeom& G, int a, int i, double centre, double radius, int halo, int& lo, int& hi)
{
    lo = lio_gm_bound_index(G, a, centre + radius);
    hi = lio_gm_bound_index(G, a, centre - radius);
    if (lo < i - halo) lo = i - halo;
    if (hi > i + halo) hi = i + halo;
}

// The circle of CircleIterator around the cell's own centre, in SubmapIterator's order (row index outer, column index
// inner); a member is read when it is finite (isValid).  Mean: every cell, the fp64 serial sum over the count, written where
// the count is not 0.  Min: where the centre is finite; the first finite member initialises, a later one replaces it only
// when it is smaller, so of +0 and -0 the first seen stays.  T::at(i, j) for every (i, j) of the grid within P.halo cells.
template <int OP, class T>
LIO_HD LioGfCell lio_gf_radius_cell(const LioGfRadius& P, const T& in, int r, int c)
{
    const LioGridGeom& G = P.G;
    LioGfCell o;
    o.value = LIO_QNAN;
    o.visited = o.written = false;
    if (OP == LIO_GF_MIN && !lio_gm_finite(in.at(r, c))) return o;
    o.visited = true;
    const double cx = lio_gm_centre(G, 0, r), cy = lio_gm_centre(G, 1, c);
    int i0, i1, j0, j1;
    lio_gf_circle_window(G, 0, r, cx, P.radius, P.halo, i0, i1);
    lio_gf_circle_window(G, 1, c, cy, P.radius, P.halo, j0, j1);
    const double r2 = P.radius * P.radius;
    double sum = 0.0;
    float lowest = 0.0f;
    int cnt = 0;
    for (int i = i0; i <= i1; ++i) {
        const double dx = lio_gm_centre(G, 0, i) - cx, dx2 = dx * dx;
        for (int j = j0; j <= j1; ++j) {
            const double dy = lio_gm_centre(G, 1, j) - cy;
            if (!(dx2 + dy * dy <= r2)) continue;
            const float v = in.at(i, j);
            if (!lio_gm_finite(v)) continue;
            if (OP == LIO_GF_MIN) { if (cnt == 0 || v < lowest) lowest = v; }
            else sum += (double)v;
            ++cnt;
        }
    }
    if (cnt == 0) return o;
    o.value = OP == LIO_GF_MIN ? lowest : (float)(sum / (double)cnt);
    o.written = true;
    return o;
}

// ---- SlidingWindowMathExpressionFilter.cpp:74-92 over SlidingWindowIterator.cpp:35-115
struct LioGfWindow {
    int rows, cols;
    int size, margin;              // the window and (size - 1) / 2
    int first_lin;                 // INSIDE: the column-major linear index below which no cell is visited (the iterator's
                                   // two setup() calls with a size derived from the length; 0 with an explicit size)
};

// scalar_sum_of_finites_op (FunctorsPlugin.hpp:3-12)
LIO_HD float lio_gf_sum_of_finites(float a, float b)
{
    const bool fa = lio_gm_finite(a), fb = lio_gm_finite(b);
    if (fa && fb) return a + b;
    if (fa) return a;
    if (fb) return b;
    return a + b;
}

// scalar_min_of_finites_op / scalar_max_of_finites_op (FunctorsPlugin.hpp:21-52) with std::min(a, b) = b < a ? b : a and
// std::max(a, b) = a < b ? b : a, also on two operands that are not finite
LIO_HD float lio_gf_min_of_finites(float a, float b)
{
    const bool fa = lio_gm_finite(a), fb = lio_gm_finite(b);
    if (fa && !fb) return a;
    if (fb && !fa) return b;
    return b < a ? b : a;
}

LIO_HD float lio_gf_max_of_finites(float a, float b)
{
    const bool fa = lio_gm_finite(a), fb = lio_gm_finite(b);
    if (fa && !fb) return a;
    if (fb && !fa) return b;
    return a < b ? b : a;
}

// the rows or columns getData() returns around centre index i of an axis of n cells: the clipped block (boundIndexToRange)
// for INSIDE and CROP, the full window for EMPTY and EDGE_MEAN
template <int EDGE>
LIO_HD void lio_gf_span(int i, int n, int margin, int& lo, int& hi)
{
    if (EDGE == LIO_GW_INSIDE || EDGE == LIO_GW_CROP) lio_gm_clip(i, margin, n, lo, hi);
    else { lo = i - margin; hi = i + margin; }
}

// coefficient (i, j) of the window matrix: the layer inside the grid, the fill of the mode outside it
template <int EDGE, class T>
LIO_HD float lio_gf_coeff(const LioGfWindow& P, const T& in, int i, int j, float fill)
{
    if (EDGE == LIO_GW_INSIDE || EDGE == LIO_GW_CROP) return in.at(i, j);
    return (i >= 0 && i < P.rows && j >= 0 && j < P.cols) ? in.at(i, j) : fill;
}

// One cell of the window filter.  Every reduction is Eigen's default-traversal redux with a functor that has no packet
// form: serial, column-major over the window matrix, the first coefficient initialises.  T::at(i, j) for every (i, j) of the
// grid within P.margin cells; K: size x size weights, column-major (LIO_GW_WEIGHTED_SUM only).
template <int OP, int EDGE, class T>
LIO_HD LioGfCell lio_gf_window_cell(const LioGfWindow& P, const T& in, const float* K, int r, int c)
{
    LioGfCell o;
    o.value = LIO_QNAN;
    o.visited = o.written = false;
    if (EDGE == LIO_GW_INSIDE) {                             // dataInsideMap(), from where the second setup() left the iterator
        if (r - P.margin < 0 || r + P.margin > P.rows - 1 || c - P.margin < 0 || c + P.margin > P.cols - 1) return o;
        if (r + c * P.rows < P.first_lin) return o;
    }
    o.visited = o.written = true;
    float fill = LIO_QNAN;                                   // returnData.setConstant(NAN)
    if (EDGE == LIO_GW_EDGE_MEAN) {                          // returnData.setConstant(data.meanOfFinites()) of the clipped block
        int i0, i1, j0, j1;
        lio_gf_span<LIO_GW_CROP>(r, P.rows, P.margin, i0, i1);
        lio_gf_span<LIO_GW_CROP>(c, P.cols, P.margin, j0, j1);
        float sum = 0.0f;
        int cnt = 0;
        bool first = true;
        for (int j = j0; j <= j1; ++j)
            for (int i = i0; i <= i1; ++i) {
                const float v = in.at(i, j);
                sum = first ? v : lio_gf_sum_of_finites(sum, v);
                first = false;
                cnt += v == v ? 1 : 0;
            }
        fill = sum / (float)cnt;
    }
    int i0, i1, j0, j1;
    lio_gf_span<EDGE>(r, P.rows, P.margin, i0, i1);
    lio_gf_span<EDGE>(c, P.cols, P.margin, j0, j1);
    float acc = 0.0f;
    int cnt = 0;
    bool first = true;
    for (int j = j0; j <= j1; ++j)
        for (int i = i0; i <= i1; ++i) {
            float v = lio_gf_coeff<EDGE>(P, in, i, j, fill);
            if (OP == LIO_GW_WEIGHTED_SUM) v = K[(i - (r - P.margin)) + (j - (c - P.margin)) * P.size] * v;
            if (OP == LIO_GW_MIN_OF_FINITES) acc = first ? v : lio_gf_min_of_finites(acc, v);
            else if (OP == LIO_GW_MAX_OF_FINITES) acc = first ? v : lio_gf_max_of_finites(acc, v);
            else if (OP != LIO_GW_NUMBER_OF_FINITES) acc = first ? v : lio_gf_sum_of_finites(acc, v);
            first = false;
            cnt += v == v ? 1 : 0;                           // numberOfFinites counts x == x: an infinity counts
        }
    const float nf = (float)cnt;
    if (OP == LIO_GW_NUMBER_OF_FINITES) o.value = nf;
    else if (OP == LIO_GW_MEAN_OF_FINITES) o.value = acc / nf;
    else if (OP == LIO_GW_STDDEV) {                          // sqrt(sumOfFinites(square(W - meanOfFinites(W))) ./ numberOfFinites(W))
        const float mean = acc / nf;
        float sq = 0.0f;
        first = true;
        for (int j = j0; j <= j1; ++j)
            for (int i = i0; i <= i1; ++i) {
                const float d = lio_gf_coeff<EDGE>(P, in, i, j, fill) - mean;
                const float d2 = d * d;
                sq = first ? d2 : lio_gf_sum_of_finites(sq, d2);
                first = false;
            }
        o.value = sqrtf(sq / nf);
    } else o.value = acc;
    return o;
}

// ---- CurvatureFilter.cpp:39-68.  T::at(i, j) on the cell and its four neighbours inside the grid; a neighbour the grid
// lacks is the cell itself.
template <class T>
LIO_HD LioGfCell lio_gf_curvature_cell(int rows, int cols, float L2, const T& in, int r, int c)
{
    LioGfCell o;
    o.value = LIO_QNAN;
    o.visited = true;
    o.written = false;
    const float z = in.at(r, c);
    if (!lio_gm_finite(z)) return o;
    const float left = in.at(r, c == 0 ? c : c - 1), right = in.at(r, c == cols - 1 ? c : c + 1);
    const float up = in.at(r == 0 ? r : r - 1, c), down = in.at(r == rows - 1 ? r : r + 1, c);
    float D = (float)(((double)(left + right) / 2.0 - (double)z) / (double)L2);
    float E = (float)(((double)(up + down) / 2.0 - (double)z) / (double)L2);
    if (!lio_gm_finite(D)) D = 0.0f;
    if (!lio_gm_finite(E)) E = 0.0f;
    o.value = (float)(-2.0 * (double)(D + E));
    o.written = true;
    return o;
}

// ---- ThresholdFilter.cpp:79-90: the cell is set where the condition fails the comparison (a NaN fails both)
LIO_HD bool lio_gf_threshold_sets(float condition, int upper, double threshold)
{
    return upper ? !((double)condition <= threshold) : !((double)condition >= threshold);
}

// ---- the plans the entry points and a host program derive before any layer is read.  nullptr, or the refusal's message.
// setWindowLength (SlidingWindowIterator.cpp:35-42) for window_size == 0; an explicit size is used as given.
inline const char* lio_gf_window_plan(int rows, int cols, double resolution, int edge, int window_size, double window_length, LioGfWindow* P)
{
    long long size = window_size;
    if (window_size == 0) {
        const double cells = round(window_length / resolution);
        if (!(cells <= (double)LIO_GW_MAX_SIZE)) return "the window reaches further than 32 cells";
        size = (long long)cells;
        if (size % 2 != 1) ++size;
    }
    if ((size - 1) / 2 > LIO_TILE_MAX_REACH) return "the window reaches further than 32 cells";
    P->rows = rows; P->cols = cols;
    P->size = (int)size; P->margin = (int)((size - 1) / 2);
    P->first_lin = 0;
    // the filter builds the iterator with its default size of 3, which walks to the first cell whose 3 x 3 window fits
    // -- (1, 1), or past the end -- before setWindowLength() calls setup() again from there
    if (edge == LIO_GW_INSIDE && window_size == 0)
        P->first_lin = (rows >= 3 && cols >= 3) ? rows + 1 : rows * cols;       // (a layer has fewer than 2^31 cells)
    return nullptr;
}

inline const char* lio_gf_radius_plan(const LioGridGeom& G, double radius, LioGfRadius* P)
{
    const double reach = radius / G.res;
    if (!(reach <= (double)LIO_TILE_MAX_REACH)) return "the radius reaches further than 32 cells";
    P->G = G;
    P->radius = radius;
    P->halo = lio_gf_halo(reach);
    return nullptr;
}
