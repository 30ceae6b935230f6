// lio_terrain.h -- the terrain layers behind the planning height map (lio_terrain.hip): what the entry points need, and the
// per-cell arithmetic of the chain as __host__ __device__ functions over a grid accessor, so that the kernels (an LDS tile)
// and a host program (the grid itself) run the same text.  A client of lio_gridfilter.h: smooth is its MEAN in a radius,
// edges its STDDEV over a cropped window, the area normals read its circle window; the eigen solver, the raster stencil and
// the float expressions are this header's own.  DESIGN.md section 4g lists the conventions (parity unpinned).  Everything here
// relies on -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include "../../include/liogpu.h"
#include "lio_gridmath.h"
#include "lio_gridfilter.h"

struct LioTerrParams {
    LioGridGeom G;
    double r_smooth, r_normal;
    int method, axis;              // method as used: 0 area, 1 raster
    int halo;                      // cells of input a tile needs around itself: the circles' windows and the raster stencil
    int margin;                    // (edge window size - 1) / 2
    float s_crit, r_crit, w_s, w_r;
};

// what one cell of the first kernel yields; the normal is NaN where none is written
struct LioTerrCell {
    float smooth, nx, ny, nz, slope, rough, trav;
    bool valid, normal, few, degenerate;
};

struct LioTerrV3 { double x, y, z; };

LIO_HD LioTerrV3 lio_terr_cross(const LioTerrV3& a, const LioTerrV3& b)
{
    LioTerrV3 c;
    c.x = a.y * b.z - a.z * b.y;
    c.y = a.z * b.x - a.x * b.z;
    c.z = a.x * b.y - a.y * b.x;
    return c;
}

LIO_HD double lio_terr_dot(const LioTerrV3& a, const LioTerrV3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// extract_kernel of Eigen's direct 3 x 3 solver on the symmetric matrix (a00 a10 a20; a10 a11 a21; a20 a21 a22): the column
// of the largest |diagonal| (the first of equals) crossed with the two others, the longer product normalised
LIO_HD void lio_terr_kernel_of(double a00, double a11, double a22, double a10, double a20, double a21, LioTerrV3& res, LioTerrV3& rep)
{
    int i0 = 0;
    double m = fabs(a00);
    if (fabs(a11) > m) { i0 = 1; m = fabs(a11); }
    if (fabs(a22) > m) i0 = 2;
    const LioTerrV3 c0 = { a00, a10, a20 }, c1 = { a10, a11, a21 }, c2 = { a20, a21, a22 };
    rep = i0 == 0 ? c0 : (i0 == 1 ? c1 : c2);
    const LioTerrV3 A = i0 == 0 ? c1 : (i0 == 1 ? c2 : c0), B = i0 == 0 ? c2 : (i0 == 1 ? c0 : c1);
    const LioTerrV3 pa = lio_terr_cross(rep, A), pb = lio_terr_cross(rep, B);
    const double n0 = lio_terr_dot(pa, pa), n1 = lio_terr_dot(pb, pb);
    if (n0 > n1) { const double s = sqrt(n0); res.x = pa.x / s; res.y = pa.y / s; res.z = pa.z / s; }
    else         { const double s = sqrt(n1); res.x = pb.x / s; res.y = pb.y / s; res.z = pb.z / s; }
}

// SelfAdjointEigenSolver<Matrix3d>::computeDirect on the covariance of n points from their sums s = (x, y, z) and
// q = (xx, yx, yy, zx, zy, zz): *v0 = eigenvectors().col(0); returns eigenvalues()(1).  Shift by trace / 3, scale by the
// largest |coefficient|, the roots by the trigonometric closed form, the eigenvector of the better separated of the extreme
// eigenvalues by extract_kernel, column 0 from it as the solver does.
LIO_HD double lio_terr_eigen(int n, const double s[3], const double q[6], LioTerrV3* v0)
{
    const double dn = (double)n;
    const double m0 = s[0] / dn, m1 = s[1] / dn, m2 = s[2] / dn;
    double a00 = q[0] / dn - m0 * m0, a10 = q[1] / dn - m1 * m0, a11 = q[2] / dn - m1 * m1;
    double a20 = q[3] / dn - m2 * m0, a21 = q[4] / dn - m2 * m1, a22 = q[5] / dn - m2 * m2;
    const double shift = ((a00 + a11) + a22) / 3.0;
    a00 -= shift; a11 -= shift; a22 -= shift;
    double scale = fabs(a00);
    scale = fmax(scale, fabs(a10)); scale = fmax(scale, fabs(a20)); scale = fmax(scale, fabs(a11));
    scale = fmax(scale, fabs(a21)); scale = fmax(scale, fabs(a22));
    if (scale > 0.0) { a00 /= scale; a10 /= scale; a20 /= scale; a11 /= scale; a21 /= scale; a22 /= scale; }
    // computeRoots: x^3 - c2 x^2 + c1 x - c0 = 0
    const double inv3 = 1.0 / 3.0, sqrt3 = sqrt(3.0);
    const double c0 = ((((a00 * a11) * a22 + ((2.0 * a10) * a20) * a21) - (a00 * a21) * a21) - (a11 * a20) * a20) - (a22 * a10) * a10;
    const double c1 = ((((a00 * a11 - a10 * a10) + a00 * a22) - a20 * a20) + a11 * a22) - a21 * a21;
    const double c2 = (a00 + a11) + a22;
    const double c2_3 = c2 * inv3;
    double a_3 = (c2 * c2_3 - c1) * inv3;
    a_3 = a_3 > 0.0 ? a_3 : 0.0;
    const double half_b = 0.5 * (c0 + c2_3 * ((2.0 * c2_3) * c2_3 - c1));
    double qq = (a_3 * a_3) * a_3 - half_b * half_b;
    qq = qq > 0.0 ? qq : 0.0;
    const double rho = sqrt(a_3);
    const double theta = atan2(sqrt(qq), half_b) * inv3;
    const double ct = cos(theta), st = sin(theta);
    const double r0 = c2_3 - rho * (ct + sqrt3 * st);
    const double r1 = c2_3 - rho * (ct - sqrt3 * st);
    const double r2 = c2_3 + (2.0 * rho) * ct;
    LioTerrV3 col0 = { 1.0, 0.0, 0.0 };                    // all three numerically the same: the identity
    if (!((r2 - r0) <= DBL_EPSILON)) {
        const double d0 = r2 - r1, d1 = r1 - r0;
        LioTerrV3 rep;
        if (d0 > d1) {                                     // the largest is the better separated: column 2 first
            LioTerrV3 col2;
            lio_terr_kernel_of(a00 - r2, a11 - r2, a22 - r2, a10, a20, a21, col2, rep);
            if (d1 <= 2.0 * DBL_EPSILON * d1) {            // (the solver's test after d0 = d1: true for d1 = 0 only)
                const double t = lio_terr_dot(col2, rep);
                col0.x = rep.x - t * rep.x; col0.y = rep.y - t * rep.y; col0.z = rep.z - t * rep.z;
                const double z = lio_terr_dot(col0, col0);
                if (z > 0.0) { const double w = sqrt(z); col0.x /= w; col0.y /= w; col0.z /= w; }
            } else {
                lio_terr_kernel_of(a00 - r0, a11 - r0, a22 - r0, a10, a20, a21, col0, rep);
            }
        } else {
            lio_terr_kernel_of(a00 - r0, a11 - r0, a22 - r0, a10, a20, a21, col0, rep);
        }
    }
    *v0 = col0;
    return r1 * scale + shift;
}

// One cell of the first kernel: smooth, the normal, slope, roughness, traversability.  T::at(i, j) = the input layer at
// row i, column j, for every (i, j) of the grid within P.halo cells of (r, c).
template <class T>
LIO_HD void lio_terr_cell(const LioTerrParams& P, const T& in, int r, int c, LioTerrCell* o)
{
    const LioGridGeom& G = P.G;
    const double cx = lio_gm_centre(G, 0, r), cy = lio_gm_centre(G, 1, c);
    const float z = in.at(r, c);
    o->valid = lio_gm_finite(z);
    o->normal = o->few = o->degenerate = false;
    // ---- smooth: MeanInRadiusFilter.cpp:59-79, every cell.  Under the tile's halo, which is never narrower than the radius's own
    const LioGfRadius S = { G, P.r_smooth, P.halo };
    o->smooth = lio_gf_radius_cell<LIO_GF_MEAN>(S, in, r, c).value;
    // ---- normal
    double n[3] = { 0.0, 0.0, 0.0 };
    if (P.method == 0) {                                   // NormalVectorsFilter.cpp:195-251, where the centre is finite
        if (o->valid) {
            int i0, i1, j0, j1;
            lio_gf_circle_window(G, 0, r, cx, P.r_normal, P.halo, i0, i1);
            lio_gf_circle_window(G, 1, c, cy, P.r_normal, P.halo, j0, j1);
            const double r2 = P.r_normal * P.r_normal;
            double s[3] = { 0.0, 0.0, 0.0 }, q[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
            int cnt = 0;
            for (int i = i0; i <= i1; ++i) {
                const double x = lio_gm_centre(G, 0, i), dx = x - cx, dx2 = dx * dx;
                for (int j = j0; j <= j1; ++j) {
                    const double y = lio_gm_centre(G, 1, j), dy = y - cy;
                    if (!(dx2 + dy * dy <= r2)) continue;
                    const float v = in.at(i, j);
                    if (!lio_gm_finite(v)) continue;
                    const double w = (double)v;
                    s[0] += x; s[1] += y; s[2] += w;
                    q[0] += x * x; q[1] += y * x; q[2] += y * y; q[3] += w * x; q[4] += w * y; q[5] += w * w;
                    ++cnt;
                }
            }
            n[2] = 1.0;                                    // UnitZ unless the solver gives a direction
            if (cnt < 3) {
                o->few = true;
            } else {
                LioTerrV3 v0;
                const double ev1 = lio_terr_eigen(cnt, s, q, &v0);
                if (ev1 > 1e-8) { n[0] = v0.x; n[1] = v0.y; n[2] = v0.z; }
                else o->degenerate = true;
            }
            o->normal = true;
        }
    } else if (r >= 1 && c >= 1 && r < G.rows - 1 && c < G.cols - 1) {          // :304-394, interior cells
        const float ft = in.at(r - 1, c), fb = in.at(r + 1, c), fl = in.at(r, c - 1), fr = in.at(r, c + 1);
        const double centre = (double)z;
        double top = (double)ft, bottom = (double)fb, left = (double)fl, right = (double)fr;
        const int fc = o->valid ? 2 : 0;
        const int kx = (lio_gm_finite(ft) ? 1 : 0) + fc + (lio_gm_finite(fb) ? 4 : 0);
        const int ky = (lio_gm_finite(fl) ? 1 : 0) + fc + (lio_gm_finite(fr) ? 4 : 0);
        bool ok = true;
        double dX = 0.0, dY = 0.0;
        if (kx == 7 || kx == 5) dX = 2.0 * G.res;
        else if (kx == 6) { top = centre; dX = G.res; }
        else if (kx == 3) { bottom = centre; dX = G.res; }
        else ok = false;
        if (ky == 7 || ky == 5) dY = 2.0 * G.res;
        else if (ky == 6) { left = centre; dY = G.res; }
        else if (ky == 3) { right = centre; dY = G.res; }
        else ok = false;
        if (ok) {
            n[0] = (bottom - top) / dX;
            n[1] = (right - left) / dY;
            n[2] = 1.0;
            const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
            n[0] /= len; n[1] /= len; n[2] /= len;
            o->normal = true;
        }
    }
    if (o->normal) {
        const double along = P.axis == 0 ? n[0] : (P.axis == 1 ? n[1] : n[2]);
        if (along < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
        o->nx = (float)n[0]; o->ny = (float)n[1]; o->nz = (float)n[2];
    } else {
        o->nx = o->ny = o->nz = LIO_QNAN;
    }
    // ---- the MathExpressionFilters (EigenLab on MatrixXf: float) and the two ThresholdFilters (ThresholdFilter.cpp:79-90)
    o->slope = acosf(o->nz);
    o->rough = fabsf(z - o->smooth);
    float t = (P.w_s * (1.0f - o->slope / P.s_crit)) + (P.w_r * (1.0f - o->rough / P.r_crit));
    if (!(t >= 0.0f)) t = 0.0f;
    if (!(t <= 1.0f)) t = 1.0f;
    o->trav = t;
}

// The second kernel's cell is lio_gf_window_cell<LIO_GW_STDDEV, LIO_GW_CROP> on the slope layer over this window:
// sqrt(sumOfFinites(square(slope - meanOfFinites(slope))) ./ numberOfFinites(slope)), SlidingWindowIterator.cpp:59-73.
LIO_HD LioGfWindow lio_terr_edge_window(const LioTerrParams& P)
{
    LioGfWindow W;
    W.rows = P.G.rows; W.cols = P.G.cols;
    W.size = 2 * P.margin + 1; W.margin = P.margin;
    W.first_lin = 0;
    return W;
}

// ---- the host side (lio_terrain.hip)
struct LioTerrPlan {
    LioTerrParams P;
    unsigned mask;                 // cfg->layers
    int n_out;                     // its set bits
    int window, method_used;
};

// The configuration against `resolution`, before any device is touched: LIO_ERR_ARG as include/liogpu.h lists.  Fills
// everything of *plan but the geometry.
int lio_terrain_check(const lio_terrain_config* cfg, double resolution, LioTerrPlan* plan);
// The geometry; LIO_ERR_ARG for non-finite values and for length != size * resolution.
int lio_terrain_set_geometry(LioTerrPlan* plan, int rows, int cols, double resolution, const double length[2], const double position[2]);
// The two kernels on the device grid d_grid (rows x cols, column-major) on stream s, the requested layers copied to `layers`
// (host; NULL: none) and the counts to *info.  d_dst (may be NULL): LIO_TERRAIN_N_LAYERS device pointers, each of which (where
// not NULL) receives that layer, rows x cols floats, by device-to-device copy, whatever the mask.  Synchronous.
int lio_terrain_device(const float* d_grid, const LioTerrPlan& plan, float* layers, lio_terrain_info* info, hipStream_t s,
                       float* const* d_dst = nullptr);
