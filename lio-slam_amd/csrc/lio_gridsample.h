// lio_gridsample.h -- grid_map::GridMap::atPosition with its four InterpolationMethods (GM = grid_map_core/src/GridMap.cpp,
// GMM = GridMapMath.cpp, CI = CubicInterpolation.cpp / .hpp) behind the resident layer set (lio_gridsample.hip): the query's
// arithmetic as __host__ __device__ functions over a grid accessor, so that the kernel (device layers) and a host program
// (a checked array) run the same text.  Everything is fp64 in the order the reference writes it, a tap is a float widened to
// double, and everything here relies on -ffp-contract=off.  The geometry and getIndexFromPosition (lio_gm_index) are
// lio_gridmath.h's.  startIndex is always 0: the library's grids are never circular buffers, so getIndexFromBufferIndex and
// its inverse are the identity and are left out.
// DESIGN.md section 4k lists the conventions and the labelled deviations (parity unpinned).
//
// A query has two halves.  The geometry (LioGsQuery: the cell, the quadrant, every tap index, the normalised coordinates)
// depends on the position alone and is formed once; the evaluation gathers the taps of one layer and runs the fall-back
// chain of GM:161-204 on it, since finiteness differs from layer to layer.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "../../include/liogpu.h"
#include "lio_gridmath.h"

#define LIO_GS_MAX_LINE (1 << 24)  // rows and cols stay below it

// ---- the two constant matrices, CI.hpp:70-74 and :159-163, as the entries a product reads
LIO_HD double lio_gs_conv_m(int r, int c)
{
    const int k = 4 * r + c;                               //  0  2  0  0 / -1  0  1  0 /  2 -5  4 -1 / -1  3 -3  1
    return k == 1 ? 2.0 : k == 4 ? -1.0 : k == 6 ? 1.0 : k == 8 ? 2.0 : k == 9 ? -5.0 : k == 10 ? 4.0 : k == 11 ? -1.0
         : k == 12 ? -1.0 : k == 13 ? 3.0 : k == 14 ? -3.0 : k == 15 ? 1.0 : 0.0;
}

LIO_HD double lio_gs_bicubic_m(int r, int c)
{
    const int k = 4 * r + c;                               //  1  0  0  0 /  0  0  1  0 / -3  3 -2 -1 /  2 -2  1  1
    return k == 0 ? 1.0 : k == 6 ? 1.0 : k == 8 ? -3.0 : k == 9 ? 3.0 : k == 10 ? -2.0 : k == 11 ? -1.0
         : k == 12 ? 2.0 : k == 13 ? -2.0 : k == 14 ? 1.0 : k == 15 ? 1.0 : 0.0;
}

// A dot product of the two cubic methods: four terms, summed k = 0 .. 3, the terms of a zero matrix entry included (one
// non-finite tap makes the result non-finite, and the sign of a zero is the dense product's).  Eigen's own order inside a
// fixed-size product is not defined by the source: unpinned.
LIO_HD double lio_gs_dot4(double a0, double a1, double a2, double a3, double b0, double b1, double b2, double b3)
{
    return ((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3;
}

// bindIndexToRange (CI:15-21) on an index formed in int and read as unsigned: a negative index goes to the last row or
// column, like one past the end.  border = 1 (the labelled extension): clamped into [0, n - 1].
LIO_HD int lio_gs_bind(int i, int n, int border)
{
    if (border) return i < 0 ? 0 : (i >= n ? n - 1 : i);
    return (unsigned)i >= (unsigned)n ? n - 1 : i;
}

// ---- the geometry of one query
struct LioGsLinear {               // GM:777-846
    int tap[4];                    // the column-major linear index of tap k in idxShift order (valid when ok)
    bool ok;                       // every tap passed the range test
    double tx, ty, ux, uy;         // positionRed and Position(1, 1) - positionRed
};
struct LioGsConv {                 // CI:44-135
    int ri[4], ci[4];              // rows i + 1, i, i - 1, i - 2 and columns j + 1, j, j - 1, j - 2, bound
    double tx, ty;
};
struct LioGsBicubic {              // CI:150-432
    int r[2], c[2];                // rows of the left / right corners, columns of the bottom / top corners, bound
    int rm[2], rp[2], cm[2], cp[2];        // their neighbours at - 1 and + 1, bound the same way
    double tx, ty;                 // from the bottom-left corner after binding
};
struct LioGsQuery {
    bool outside;
    int i, j;                      // the position's cell
    LioGsLinear lin;
    LioGsConv conv;
    LioGsBicubic bic;
};

// atPositionLinearInterpolated's index work.  The neighbour row is chosen by position.x >= centre.x and the column likewise;
// the taps are indices[idxShift[k]], and idxShift[k] = idxShift[0] ^ k in all four cases of GM:793-820.  border 0: each tap is
// tested through its linear index col * rows + row alone, so (rows, c) reads (0, c + 1) and (-1, c) reads (rows - 1, c - 1);
// a negative index fails as its size_t does, and so does rows * cols (the reference's `>` lets that one read past the
// buffer: the labelled deviation).  The second getPosition (GM:839) leaves `point` alone when tap 0's own index is outside
// the grid, so t is then measured from the cell's centre, as written.  border 1: every index clamped, nothing fails.
LIO_HD void lio_gs_linear_geom(const LioGridGeom& G, int border, double px, double py, int i, int j, LioGsLinear* L)
{
    const double cx = lio_gm_centre(G, 0, i), cy = lio_gm_centre(G, 1, j);
    const bool up = px >= cx, right = py >= cy;
    int r[4], c[4];
    r[0] = i; c[0] = j;
    r[1] = up ? i - 1 : i + 1; c[1] = j;
    r[2] = i; c[2] = right ? j - 1 : j + 1;
    r[3] = r[1]; c[3] = c[2];
    const int s0 = right ? (up ? 0 : 1) : (up ? 2 : 3);
    const long long cells = (long long)G.rows * (long long)G.cols;
    L->ok = true;
    for (int k = 0; k < 4; ++k) {
        int rr = r[s0 ^ k], cc = c[s0 ^ k];
        if (border) { rr = lio_gs_bind(rr, G.rows, 1); cc = lio_gs_bind(cc, G.cols, 1); }
        const long long lin = (long long)cc * (long long)G.rows + (long long)rr;
        if (lin < 0 || lin >= cells) { L->ok = false; L->tap[k] = 0; }
        else L->tap[k] = (int)lin;
    }
    int r0 = r[s0], c0 = c[s0];
    if (border) { r0 = lio_gs_bind(r0, G.rows, 1); c0 = lio_gs_bind(c0, G.cols, 1); }
    const bool in_range = r0 >= 0 && r0 < G.rows && c0 >= 0 && c0 < G.cols;
    const double ox = in_range ? lio_gm_centre(G, 0, r0) : cx, oy = in_range ? lio_gm_centre(G, 1, c0) : cy;
    L->tx = (px - ox) / G.res; L->ty = (py - oy) / G.res;
    L->ux = 1.0 - L->tx; L->uy = 1.0 - L->ty;
}

LIO_HD void lio_gs_conv_geom(const LioGridGeom& G, int border, double px, double py, int i, int j, LioGsConv* V)
{
    for (int k = 0; k < 4; ++k) {
        V->ri[k] = lio_gs_bind(i + 1 - k, G.rows, border);
        V->ci[k] = lio_gs_bind(j + 1 - k, G.cols, border);
    }
    V->tx = (px - lio_gm_centre(G, 0, i)) / G.res;
    V->ty = (py - lio_gm_centre(G, 1, j)) / G.res;
}

// getUnitSquareCornerIndices (CI:204-255) with its strict `>`, bindIndicesToRange, and the neighbours the derivatives read
LIO_HD void lio_gs_bicubic_geom(const LioGridGeom& G, int border, double px, double py, int i, int j, LioGsBicubic* B)
{
    const bool xq = px > lio_gm_centre(G, 0, i), yq = py > lio_gm_centre(G, 1, j);
    B->r[0] = lio_gs_bind(xq ? i : i + 1, G.rows, border);           // topLeft / bottomLeft
    B->r[1] = lio_gs_bind(xq ? i - 1 : i, G.rows, border);           // topRight / bottomRight
    B->c[0] = lio_gs_bind(yq ? j : j + 1, G.cols, border);           // bottom
    B->c[1] = lio_gs_bind(yq ? j - 1 : j, G.cols, border);           // top
    for (int k = 0; k < 2; ++k) {
        B->rm[k] = lio_gs_bind(B->r[k] - 1, G.rows, border); B->rp[k] = lio_gs_bind(B->r[k] + 1, G.rows, border);
        B->cm[k] = lio_gs_bind(B->c[k] - 1, G.cols, border); B->cp[k] = lio_gs_bind(B->c[k] + 1, G.cols, border);
    }
    B->tx = (px - lio_gm_centre(G, 0, B->r[0])) / G.res;
    B->ty = (py - lio_gm_centre(G, 1, B->c[0])) / G.res;
}

// The geometry a query of `method` needs: its own and that of the methods it can fall back to.
LIO_HD void lio_gs_query(const LioGridGeom& G, int method, int border, double px, double py, LioGsQuery* Q)
{
    Q->outside = !lio_gm_index(G, px, py, &Q->i, &Q->j);
    if (Q->outside) return;
    if (method != LIO_GRID_NEAREST) lio_gs_linear_geom(G, border, px, py, Q->i, Q->j, &Q->lin);
    if (method == LIO_GRID_CUBIC_CONVOLUTION) lio_gs_conv_geom(G, border, px, py, Q->i, Q->j, &Q->conv);
    if (method == LIO_GRID_CUBIC) lio_gs_bicubic_geom(G, border, px, py, Q->i, Q->j, &Q->bic);
}

// ---- the evaluation on one layer.  T::at(r, c): the layer at row r, column c, inside the grid only; T::at_lin(k): the
// layer at its column-major linear index k in [0, rows * cols), which is how the linear method reads (layerMat(indexLin)).
// GM:843-844, left to right; there is no finiteness test
template <class T>
LIO_HD float lio_gs_linear(const LioGsLinear& L, const T& in)
{
    double f[4];
    for (int k = 0; k < 4; ++k) f[k] = (double)in.at_lin(L.tap[k]);
    const double v = ((f[0] * L.ux * L.uy + f[1] * L.tx * L.uy) + f[2] * L.ux * L.ty) + f[3] * L.tx * L.ty;
    return (float)v;
}

// convolve1D (CI:72-79): 0.5 * (tVector . (M * f))
LIO_HD double lio_gs_convolve(double t, double f0, double f1, double f2, double f3)
{
    const double t2 = t * t, t3 = t2 * t;
    double tmp[4];
    for (int r = 0; r < 4; ++r)
        tmp[r] = lio_gs_dot4(lio_gs_conv_m(r, 0), lio_gs_conv_m(r, 1), lio_gs_conv_m(r, 2), lio_gs_conv_m(r, 3), f0, f1, f2, f3);
    return 0.5 * lio_gs_dot4(1.0, t, t2, t3, tmp[0], tmp[1], tmp[2], tmp[3]);
}

// evaluateBicubicConvolutionInterpolation: row a of the function value matrix holds column j + 1 - a of the layer, taken at
// rows i + 1, i, i - 1, i - 2 (CI:106-108)
template <class T>
LIO_HD double lio_gs_conv(const LioGsConv& V, const T& in)
{
    double b[4];
    for (int a = 0; a < 4; ++a)
        b[a] = lio_gs_convolve(V.tx, (double)in.at(V.ri[0], V.ci[a]), (double)in.at(V.ri[1], V.ci[a]), (double)in.at(V.ri[2], V.ci[a]),
                               (double)in.at(V.ri[3], V.ci[a]));
    return lio_gs_convolve(V.ty, b[0], b[1], b[2], b[3]);
}

// evaluateBicubicInterpolation.  Corner (kr, kc): kr 0 left, 1 right; kc 0 bottom, 1 top.  The function value matrix of
// CI:416-432 is F[2 a + kr][2 b + kc], (a, b) = (0, 0) f, (1, 0) dfx, (0, 1) dfy, (1, 1) ddfxy.
template <class T>
LIO_HD double lio_gs_bicubic(const LioGridGeom& G, const LioGsBicubic& B, const T& in)
{
    const double res = G.res;
    double F[4][4];
    for (int kr = 0; kr < 2; ++kr)
        for (int kc = 0; kc < 2; ++kc) {
            const int r = B.r[kr], c = B.c[kc], rm = B.rm[kr], rp = B.rp[kr], cm = B.cm[kc], cp = B.cp[kc];
            F[kr][kc] = (double)in.at(r, c);
            {                                              // firstOrderDerivativeAt, X: right at index - 1, left at index + 1
                const double left = (double)in.at(rp, c), right = (double)in.at(rm, c);
                F[2 + kr][kc] = (right - left) / (2.0 * res) * res;
            }
            {
                const double left = (double)in.at(r, cp), right = (double)in.at(r, cm);
                F[kr][2 + kc] = (right - left) / (2.0 * res) * res;
            }
            {                                              // mixedSecondOrderDerivativeAt
                const double f11 = (double)in.at(rm, cm), f1m1 = (double)in.at(rm, cp), fm11 = (double)in.at(rp, cm), fm1m1 = (double)in.at(rp, cp);
                F[2 + kr][2 + kc] = (f11 - f1m1 - fm11 + fm1m1) / (4.0 * res * res) * res * res;
            }
        }
    // evaluatePolynomial (CI:405-414): F * M^T, then M * that, then * yVector, then xVector . that
    double A[4][4], P[4][4], v[4];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            A[r][c] = lio_gs_dot4(F[r][0], F[r][1], F[r][2], F[r][3], lio_gs_bicubic_m(c, 0), lio_gs_bicubic_m(c, 1), lio_gs_bicubic_m(c, 2),
                                  lio_gs_bicubic_m(c, 3));
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            P[r][c] = lio_gs_dot4(lio_gs_bicubic_m(r, 0), lio_gs_bicubic_m(r, 1), lio_gs_bicubic_m(r, 2), lio_gs_bicubic_m(r, 3), A[0][c], A[1][c], A[2][c],
                                  A[3][c]);
    const double tx = B.tx, ty = B.ty, tx2 = tx * tx, ty2 = ty * ty;
    const double tx3 = tx2 * tx, ty3 = ty2 * ty;
    for (int r = 0; r < 4; ++r) v[r] = lio_gs_dot4(P[r][0], P[r][1], P[r][2], P[r][3], 1.0, ty, ty2, ty3);
    return lio_gs_dot4(1.0, tx, tx2, tx3, v[0], v[1], v[2], v[3]);
}

LIO_HD bool lio_gs_finite(double v) { return fabs(v) <= DBL_MAX; }          // std::isfinite

// atPosition (GM:161-204) on one layer: a cubic result that is not finite falls back to linear, linear whose taps fail to
// nearest.  A finite double beyond float's range is rounded to +-inf, as written.  Outside the map nothing is read: the
// quiet NaN 0x7fc00000 and LIO_GRID_OUTSIDE, where the reference throws (the labelled deviation).  Returns the method used.
template <class T>
LIO_HD int lio_gs_eval(const LioGridGeom& G, const LioGsQuery& Q, int method, const T& in, float* value)
{
    if (Q.outside) { *value = LIO_QNAN; return LIO_GRID_OUTSIDE; }
    if (method == LIO_GRID_CUBIC_CONVOLUTION) {
        const double v = lio_gs_conv(Q.conv, in);
        if (lio_gs_finite(v)) { *value = (float)v; return LIO_GRID_CUBIC_CONVOLUTION; }
    } else if (method == LIO_GRID_CUBIC) {
        const double v = lio_gs_bicubic(G, Q.bic, in);
        if (lio_gs_finite(v)) { *value = (float)v; return LIO_GRID_CUBIC; }
    }
    if (method != LIO_GRID_NEAREST && Q.lin.ok) { *value = lio_gs_linear(Q.lin, in); return LIO_GRID_LINEAR; }
    *value = in.at(Q.i, Q.j);                              // the cell's bits
    return LIO_GRID_NEAREST;
}

// ---- the host side (lio_gridsample.hip): what a chained entry point needs of the resident object
// Before the first launch: LIO_ERR_ARG for an object on another device than `device_id`; the object then holds no layer.
int lio_grid_begin(lio_grid* g, int device_id);
// The object holds no layer (its memory stays).
void lio_grid_clear(lio_grid* g);
// What lio_grid_set_geometry refuses, with the object untouched: LIO_OK, LIO_ERR_ARG or LIO_ERR_CAPACITY.
int lio_grid_geometry_check(int rows, int cols, double resolution, const double* length, const double* position);
// The geometry of the layers to come, checked as the upload's: LIO_ERR_ARG / LIO_ERR_CAPACITY as include/liogpu.h lists.
int lio_grid_set_geometry(lio_grid* g, int rows, int cols, double resolution, const double length[2], const double position[2]);
// Slot `layer` of the object, grown to the geometry's cells and marked present: where a chain copies or writes that layer on
// the device.  *d_out = nullptr on failure.
int lio_grid_layer_slot(lio_grid* g, int layer, float** d_out);
