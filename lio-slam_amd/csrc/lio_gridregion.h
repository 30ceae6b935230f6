// lio_gridregion.h -- grid_map's region iterators (IT = grid_map_core/src/iterators/: LineIterator, CircleIterator,
// EllipseIterator, PolygonIterator over SubmapIterator; GMM = GridMapMath.cpp; PG = Polygon.cpp) behind the region reductions
// of the resident layer set (lio_gridregion.hip): the cells of a region and the reduction over them as __host__ __device__
// functions, so that the kernels and a host program (tools/grid_region_host_check.cpp) run the same text.  Everything is fp64
// in the order the reference writes it, only + - * / sqrt, and everything here relies on -ffp-contract=off.  The geometry is
// lio_gridmath.h's; startIndex is always 0, so getIndexFromBufferIndex and its inverse are the identity and are left out.
// DESIGN.md section 4l lists the conventions and the labelled deviations (parity unpinned).
//
// A region has two halves.  The plan (LioRgPlan) depends on the region alone: the window of an area kind (one axis per
// call of lio_rg_plan_half), the two limited end cells of a line (one endpoint per call -- the walk of LineIterator.cpp:75-88
// is a serial fp64 accumulation and stays one).  The cells then follow from the plan by number: lio_rg_cell_by_order in the
// iterator's order, lio_rg_cell_by_rank in the order of the sum, lio_rg_member for the area kinds' membership.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "../../include/liogpu.h"
#include "lio_gridmath.h"
#include "lio_wg.h"

#define LIO_RG_LANES 64            // the partial sums of a region: fixed, whatever the launch shape

// A region as the device reads it: lio_grid_region with the ellipse's sin and cos of the rotation (libm, on the host, as
// EllipseIterator.cpp:21-22 calls them) in p[4] and p[5].
struct LioRgRegion {
    int kind, n_vertices;
    long long first_vertex;
    double p[6];
};

// What the plan kernel leaves of a region.  Area kinds: the window rows [r0, r0 + h), columns [c0, c0 + w).  Line: (r0, c0)
// the start cell, h cells, sr / sc the signs, major 0 when rows advance every cell, den / add Bresenham's fraction.
struct LioRgPlan {
    int status, kind;
    int r0, c0, h, w;
    int sr, sc, major, den, add, pad;
};

// The host's packing: libm's sin and cos, the only transcendental calls of a region; the device never makes them.
inline void lio_rg_pack(const lio_grid_region& r, LioRgRegion* o)
{
    o->kind = r.kind;
    o->n_vertices = r.kind == LIO_REGION_POLYGON ? r.n_vertices : 0;
    o->first_vertex = r.kind == LIO_REGION_POLYGON ? r.first_vertex : 0;
    for (int k = 0; k < 5; ++k) o->p[k] = r.p[k];
    o->p[5] = 0.0;
    if (r.kind == LIO_REGION_ELLIPSE) { o->p[4] = sin(r.p[4]); o->p[5] = cos(r.p[4]); }
}

LIO_HD bool lio_rg_finite(double v) { return fabs(v) <= DBL_MAX; }

// ---- INVALID: the causes the parameters alone show (a polygon's vertices are looked at by lio_rg_plan_half)
LIO_HD bool lio_rg_params_ok(const LioRgRegion& R)
{
    const int np = R.kind == LIO_REGION_CIRCLE ? 3 : R.kind == LIO_REGION_ELLIPSE ? 6 : R.kind == LIO_REGION_LINE ? 4 : 0;
    for (int k = 0; k < np; ++k)
        if (!lio_rg_finite(R.p[k])) return false;
    if (R.kind == LIO_REGION_CIRCLE && R.p[2] < 0.0) return false;
    if (R.kind == LIO_REGION_ELLIPSE && !(R.p[2] > 0.0 && R.p[3] > 0.0)) return false;
    return true;
}

// getIndexLimitedToMapRange (IT/LineIterator.cpp:75-88): from `s` towards `e` in steps of (resolution - epsilon) * direction
// until GridMap::getIndex succeeds; direction is Eigen's normalized(): v / sqrt(v.v) when v.v > 0, else v.  Gives up (EMPTY:
// the constructor throws) when what remains is shorter than a step.  The labelled deviation: LIO_REGION_MAX_WALK steps
// without an answer are INVALID, where the reference would keep walking.
LIO_HD int lio_rg_walk(const LioGridGeom& G, double sx, double sy, double ex, double ey, int* i, int* j)
{
    double vx = ex - sx, vy = ey - sy;
    const double z = vx * vx + vy * vy;
    if (z > 0.0) { const double n = sqrt(z); vx = vx / n; vy = vy / n; }
    const double step = G.res - DBL_EPSILON;
    double x = sx, y = sy;
    for (int k = 0; ; ++k) {
        if (lio_gm_index(G, x, y, i, j)) return LIO_REGION_OK;
        if (k == LIO_REGION_MAX_WALK) return LIO_REGION_INVALID;
        x += step * vx;
        y += step * vy;
        const double rx = ex - x, ry = ey - y;
        if (sqrt(rx * rx + ry * ry) < step) return LIO_REGION_EMPTY;
    }
}

// One half of a region's plan.  Area kinds: e is the axis, [*lo, *hi] the window along it -- findSubmapParameters of the
// three iterators (CircleIterator.cpp:74-85, EllipseIterator.cpp:82-97, PolygonIterator.cpp:71-85): the corner positions
// through boundPositionToRange and getIndexFromPosition (lio_gm_bound_index).  Line: e is the endpoint, (*lo, *hi) its limited
// cell.  verts: the flat (x, y) array the polygon's first_vertex counts in.  Returns the half's status.
LIO_HD int lio_rg_plan_half(const LioGridGeom& G, const LioRgRegion& R, const double* verts, int e, int* lo, int* hi)
{
    *lo = 0; *hi = 0;
    if (!lio_rg_params_ok(R)) return LIO_REGION_INVALID;
    double top, bottom;
    if (R.kind == LIO_REGION_LINE) {
        return e == 0 ? lio_rg_walk(G, R.p[0], R.p[1], R.p[2], R.p[3], lo, hi) : lio_rg_walk(G, R.p[2], R.p[3], R.p[0], R.p[1], lo, hi);
    } else if (R.kind == LIO_REGION_CIRCLE) {
        top = R.p[e] + R.p[2]; bottom = R.p[e] - R.p[2];
    } else if (R.kind == LIO_REGION_ELLIPSE) {
        // Rotation2Dd * (lx, 0) = (cos lx, sin lx), * (0, ly) = (-sin ly, cos ly); the products with the zeros add +-0
        const double s = R.p[4], c = R.p[5];
        const double u = (e == 0 ? c : s) * R.p[2], v = (e == 0 ? -s : c) * R.p[3];
        const double half = sqrt(u * u + v * v);
        top = R.p[e] + half; bottom = R.p[e] - half;
    } else {
        const double* v = verts + 2 * R.first_vertex + e;
        bool ok = true;
        top = bottom = v[0];
        for (int k = 0; k < R.n_vertices; ++k) {
            const double a = v[2 * k];
            if (!lio_rg_finite(a)) ok = false;
            top = top < a ? a : top;                       // Eigen's max and min
            bottom = a < bottom ? a : bottom;
        }
        if (!ok) return LIO_REGION_INVALID;
    }
    *lo = lio_gm_bound_index(G, e, top);
    *hi = lio_gm_bound_index(G, e, bottom);
    return LIO_REGION_OK;
}

// The two halves -> the plan.  The line's second walk does not run in the reference when the first fails: its verdict
// then does not count.  initializeIterationParameters (IT/LineIterator.cpp:90-136).
LIO_HD void lio_rg_plan_join(const LioRgRegion& R, int s0, int lo0, int hi0, int s1, int lo1, int hi1, LioRgPlan* P)
{
    P->kind = R.kind;
    P->r0 = P->c0 = P->h = P->w = P->den = P->add = P->major = P->pad = 0;
    P->sr = P->sc = 1;
    if (R.kind == LIO_REGION_LINE) {
        P->status = s0 != LIO_REGION_OK ? s0 : s1;
        if (P->status != LIO_REGION_OK) return;
        const int dr = lo1 >= lo0 ? lo1 - lo0 : lo0 - lo1, dc = hi1 >= hi0 ? hi1 - hi0 : hi0 - hi1;
        P->r0 = lo0; P->c0 = hi0;
        P->sr = lo1 >= lo0 ? 1 : -1;
        P->sc = hi1 >= hi0 ? 1 : -1;
        P->major = dr >= dc ? 0 : 1;
        P->den = dr >= dc ? dr : dc;
        P->add = dr >= dc ? dc : dr;
        P->h = P->den + 1; P->w = 1;
        return;
    }
    P->status = s0 != LIO_REGION_OK ? s0 : s1;             // (an area's halves fail for INVALID alone)
    if (P->status != LIO_REGION_OK) return;
    P->r0 = lo0; P->c0 = lo1;
    P->h = hi0 - lo0 + 1; P->w = hi1 - lo1 + 1;            // getSubmapSizeFromCornerIndices
    if (P->h < 1 || P->w < 1) { P->h = P->w = 0; }         // (top >= bottom and the index is monotone: never)
}

// how many cells the plan numbers: the window's, the line's
LIO_HD int lio_rg_n_slots(const LioRgPlan& P) { return P.status == LIO_REGION_OK ? P.h * P.w : 0; }

// Cell k of the line.  LineIterator's ++ (IT/LineIterator.cpp:43-55) adds numeratorAdd and carries at most once a step
// (numeratorAdd <= denominator), so after k steps the minor axis has moved (denominator / 2 + k numeratorAdd) / denominator
// cells: the closed form the kernels use; tests/test_grid_region_cpu.py proves it against the serial loop.
LIO_HD void lio_rg_line_cell(const LioRgPlan& P, int k, int* r, int* c)
{
    const int m = P.den > 0 ? (int)(((long long)(P.den / 2) + (long long)k * (long long)P.add) / (long long)P.den) : 0;
    *r = P.r0 + P.sr * (P.major == 0 ? k : m);
    *c = P.c0 + P.sc * (P.major == 0 ? m : k);
}

// Slot t in the iterator's order: SubmapIterator (incrementIndexForSubmap, GMM:485-516) runs the column index inside the
// row index; the line runs start to end.
LIO_HD void lio_rg_cell_by_order(const LioRgPlan& P, int t, int* r, int* c)
{
    if (P.kind == LIO_REGION_LINE) { lio_rg_line_cell(P, t, r, c); return; }
    *r = P.r0 + t / P.w; *c = P.c0 + t % P.w;
}

// Slot `rank` in the order of the sum: the window column-major (the row fastest, as the layers lie in memory), the line by k.
LIO_HD void lio_rg_cell_by_rank(const LioRgPlan& P, int rank, int* r, int* c)
{
    if (P.kind == LIO_REGION_LINE) { lio_rg_line_cell(P, rank, r, c); return; }
    *r = P.r0 + rank % P.h; *c = P.c0 + rank / P.h;
}

// isInside of the three area iterators on the centre of cell (r, c).  v: the polygon's own vertices, (x, y) pairs.
//  - circle (CircleIterator.cpp:66-72): the reference compares with pow(radius, 2); r * r here, as lio_terr_cell does for
//    the same iterator (the device is kept to + - * / sqrt; compilers fold pow(r, 2) to r * r themselves);
//  - ellipse (EllipseIterator.cpp:17-28, :74-80): the transform (cos sin; sin -cos), squares over (0.5 length)^2;
//  - polygon (PG:30-42): the even-odd crossing test, the division where the reference has it.
LIO_HD bool lio_rg_member(const LioGridGeom& G, const LioRgRegion& R, const double* v, int r, int c)
{
    if (R.kind == LIO_REGION_LINE) return true;
    const double px = lio_gm_centre(G, 0, r), py = lio_gm_centre(G, 1, c);
    if (R.kind == LIO_REGION_CIRCLE) {
        const double dx = px - R.p[0], dy = py - R.p[1];
        return dx * dx + dy * dy <= R.p[2] * R.p[2];
    }
    if (R.kind == LIO_REGION_ELLIPSE) {
        const double dx = px - R.p[0], dy = py - R.p[1], s = R.p[4], co = R.p[5];
        const double hx = 0.5 * R.p[2], hy = 0.5 * R.p[3];
        const double t0 = co * dx + s * dy, t1 = s * dx + (-co) * dy;
        return (t0 * t0) / (hx * hx) + (t1 * t1) / (hy * hy) <= 1.0;
    }
    int cross = 0;
    for (int i = 0, j = R.n_vertices - 1; i < R.n_vertices; j = i++) {
        const double xi = v[2 * i], yi = v[2 * i + 1], xj = v[2 * j], yj = v[2 * j + 1];
        if (((yi > py) != (yj > py)) && (px < (xj - xi) * (py - yi) / (yj - yi) + xi)) ++cross;
    }
    return (cross & 1) != 0;
}

// ---- the reduction.  One accumulator per partial sum (a lane of the wave on the device).
struct LioRgAcc {
    double sum;
    unsigned mn, mx;               // lio_f2ord words: -0.0 < +0.0, and the result does not depend on the order
    int n_finite, n_below;
};

LIO_HD void lio_rg_acc_clear(LioRgAcc* a)
{
    a->sum = 0.0; a->mn = LIO_ORD_NO_MIN; a->mx = LIO_ORD_NO_MAX; a->n_finite = 0; a->n_below = 0;
}

LIO_HD void lio_rg_acc_add(LioRgAcc* a, float v, float threshold)
{
    if (!lio_gm_finite(v)) return;
    a->sum = a->sum + (double)v;
    const unsigned o = lio_f2ord(v);
    a->mn = o < a->mn ? o : a->mn;
    a->mx = o > a->mx ? o : a->mx;
    a->n_finite += 1;
    a->n_below += v < threshold ? 1 : 0;
}

// part[k] += part[k + s]: one level of the tree s = 32, 16, .. 1 that follows the partial sums
LIO_HD void lio_rg_acc_fold(LioRgAcc* a, const LioRgAcc& b)
{
    a->sum = a->sum + b.sum;
    a->mn = b.mn < a->mn ? b.mn : a->mn;
    a->mx = b.mx > a->mx ? b.mx : a->mx;
    a->n_finite += b.n_finite;
    a->n_below += b.n_below;
}

LIO_HD void lio_rg_acc_store(const LioRgAcc& a, lio_grid_region_stat* o)
{
    o->sum = a.sum;
    o->min = a.n_finite ? lio_ord2f(a.mn) : LIO_QNAN;
    o->max = a.n_finite ? lio_ord2f(a.mx) : LIO_QNAN;
    o->n_finite = a.n_finite; o->n_below = a.n_below;
}

// The whole reduction of one region on one layer, serially: LIO_RG_LANES partial sums, partial p over the member cells of
// rank = p (mod 64) in ascending rank, then the tree.  T::at(r, c): the layer.  Returns the member cells.  (The host's form;
// k_rg_reduce holds one partial per lane.)
template <class T>
inline int lio_rg_reduce_serial(const LioGridGeom& G, const LioRgRegion& R, const double* v, const LioRgPlan& P, const T& in, float threshold,
                                lio_grid_region_stat* out)
{
    LioRgAcc part[LIO_RG_LANES];
    for (int p = 0; p < LIO_RG_LANES; ++p) lio_rg_acc_clear(&part[p]);
    const int slots = lio_rg_n_slots(P);
    int members = 0;
    for (int rank = 0; rank < slots; ++rank) {
        int r, c;
        lio_rg_cell_by_rank(P, rank, &r, &c);
        if (!lio_rg_member(G, R, v, r, c)) continue;
        ++members;
        lio_rg_acc_add(&part[rank % LIO_RG_LANES], in.at(r, c), threshold);
    }
    for (int s = LIO_RG_LANES / 2; s > 0; s >>= 1)
        for (int k = 0; k < s; ++k) lio_rg_acc_fold(&part[k], part[k + s]);
    lio_rg_acc_store(part[0], out);
    return members;
}
