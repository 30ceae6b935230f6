// lio_gridgeom.h -- grid_map::GridMap::getSubmap, move, extendToInclude and addDataFrom (GM = grid_map_core/src/GridMap.cpp:
// 282-330, 442-507, 554-627, 514-552; GMM = GridMapMath.cpp) behind the resident layer set (lio_gridgeom.hip): the geometry
// each call decides on the host, and the per-cell work of the two gather kernels as __host__ __device__ functions, so that
// the kernels and a host program (tools/grid_geom_host_check.cpp) run the same text.  Everything is fp64 in the order the
// reference writes it and relies on -ffp-contract=off.  The geometry, its constructor and GridMapMath's index functions
// (lio_gm_centre, lio_gm_index, lio_gm_bound_index, lio_gm_lookup, lio_gm_size) are lio_gridmath.h's.  startIndex is
// always 0: every result is the reference's after convertToDefaultStartIndex (GM:677-707).  What runs on the device is
// + - * /, compares and casts; fmod, round and copysign are in the host-only functions.  DESIGN.md section 4n lists the
// conventions and the labelled deviations (parity unpinned).
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "../../include/liogpu.h"
#include "lio_gridmath.h"

#define LIO_GG_MAX_SHIFT 1073741824.0                        // 2^30: |position shift / resolution| stays below it

LIO_HD bool lio_gg_word_finite(unsigned w) { return (w & 0x7f800000u) != 0x7f800000u; }       // isfinite on a float's bits

// ---- the geometry each call decides, on the host
// getSubmapInformation (GMM:287-341), default start index.  halfTransform is -0.5 I: requested - halfTransform * length is
// requested + 0.5 length bit for bit (the product's second term is -0.0 for a finite length >= 0), and likewise
// - halfTransform * Constant(resolution) adds 0.5 resolution.  Both corners go through boundPositionToRange and
// getIndexFromPosition (lio_gm_bound_index).  A bounded corner whose index still fails there (a length whose last ulp swallows
// the epsilon) is brought back to the last cell, where the reference returns false: lio_gm_bound_index's labelled deviation.
struct LioGgSubmap {
    int ok;                        // getSubmapInformation's return value
    int top_left[2], size[2], requested[2];
    double length[2], position[2];
};

inline void lio_gg_submap_information(const LioGridGeom& G, const double position[2], const double length[2], LioGgSubmap* S)
{
    double corner[2];
    for (int a = 0; a < 2; ++a) {
        S->top_left[a] = lio_gm_bound_index(G, a, position[a] + 0.5 * length[a]);
        const int bottom_right = lio_gm_bound_index(G, a, position[a] - 0.5 * length[a]);
        corner[a] = lio_gm_centre(G, a, S->top_left[a]) + 0.5 * G.res;
        S->size[a] = bottom_right - S->top_left[a] + 1;
        S->length[a] = (double)S->size[a] * G.res;
        S->position[a] = corner[a] - 0.5 * S->length[a];
    }
    S->requested[0] = S->requested[1] = 0;
    S->ok = 0;
    if (S->size[0] < 1 || S->size[1] < 1) return;
    const LioGridGeom M = lio_gm_geom(S->size[0], S->size[1], G.res, S->position[0], S->position[1]);
    S->ok = lio_gm_index(M, position[0], position[1], &S->requested[0], &S->requested[1]) ? 1 : 0;
}

// getIndexShiftFromPositionShift (GMM:183-196), one component: (int)(v + 0.5 * (v > 0 ? 1 : -1)) with v = shift / resolution,
// then the map-to-buffer negation.  false where the cast is not defined for every such v (|v| >= 2^30 or not finite): the
// labelled deviation, LIO_ERR_ARG.
inline bool lio_gg_index_shift(double position_shift, double res, int* index_shift)
{
    const double v = position_shift / res;
    if (!(fabs(v) < LIO_GG_MAX_SHIFT)) return false;
    const int iv = (int)(v + 0.5 * (double)(v > 0 ? 1 : -1));
    *index_shift = -iv;
    return true;
}

// getPositionShiftFromIndexShift (GMM:198-204), one component: transformBufferOrderToMapFrame(indexShift) * resolution
inline double lio_gg_position_shift(int index_shift, double res) { return (double)(-index_shift) * res; }

// extendToInclude's request along one axis (GM:556-584): the corners of both maps, the two comparisons, the half
// differences.  *position and *length come in as this map's and go out as setGeometry's arguments; returns resizeMap.
inline bool lio_gg_extend_axis(double other_position, double other_length, double* position, double* length)
{
    const double top_left = *position + *length / 2.0, bottom_right = *position - *length / 2.0;
    const double top_left_other = other_position + other_length / 2.0, bottom_right_other = other_position - other_length / 2.0;
    bool resize = false;
    if (top_left_other > top_left) {
        *position += (top_left_other - top_left) / 2.0;
        *length += top_left_other - top_left;
        resize = true;
    }
    if (bottom_right_other < bottom_right) {
        *position -= (bottom_right - bottom_right_other) / 2.0;
        *length += bottom_right - bottom_right_other;
        resize = true;
    }
    return resize;
}

// The alignment of the new map with the old one along one axis (GM:590-608): position is setGeometry's, old_position the
// copy's, the sizes the two maps' along the axis.
inline double lio_gg_align_axis(double position, double old_position, double res, int size, int old_size)
{
    const double shift = fmod(position - old_position, res);
    if (fabs(shift) < res / 2.0) position -= shift;
    else position += res - shift;
    if (size % 2 != old_size % 2) position += -copysign(res / 2.0, shift);
    return position;
}

// ---- the two gathers.  A table of layer pointers, as words: destination slot k is written from `self` (this map before the
// call; null: the layer is new, the quiet NaN) and, in addDataFrom, from `other` (null: the layer is not one to copy).
struct LioGgTable {
    const unsigned* self[LIO_GRID_MAX_LAYERS];
    unsigned* dst[LIO_GRID_MAX_LAYERS];
    const unsigned* other[LIO_GRID_MAX_LAYERS];
    int n;
    unsigned basic;                // bit k: slot k is one of basicLayers_
};

// The integer-offset form (getSubmap's block copy; move followed by convertToDefaultStartIndex): destination cell (r, c) of a
// grid of d_rows rows takes source cell (r + off0, c + off1) of the s_rows x s_cols grid where that exists, the quiet NaN
// elsewhere.  Returns whether the cell was cleared.
LIO_HD bool lio_gg_offset_cell(const LioGgTable& T, int d_rows, int s_rows, int s_cols, int off0, int off1, int r, int c)
{
    const long long sr = (long long)r + (long long)off0, sc = (long long)c + (long long)off1;
    const bool in = sr >= 0 && sr < (long long)s_rows && sc >= 0 && sc < (long long)s_cols;
    const size_t at = (size_t)c * (size_t)d_rows + (size_t)r;
    const size_t from = in ? (size_t)sc * (size_t)s_rows + (size_t)sr : 0;
    for (int k = 0; k < T.n; ++k) T.dst[k][at] = in ? T.self[k][from] : LIO_QNAN_BITS;
    return !in;
}

enum { LIO_GG_RESIZE = 1, LIO_GG_ADD = 2, LIO_GG_OVERWRITE = 4 };

struct LioGgCellCount {
    bool kept;                     // the cell took this map's old cell (the extension's copy)
    bool skipped_valid;            // isValid(*iterator) && !overwriteData
    bool outside_other;            // !other.isInside(position)
    bool index_outside_self;       // isInside held and getIndex failed on the old map,
    bool index_outside_other;      // on `other`
    int copied;                    // values taken from `other`
};

// The fp64 position form: cell (r, c) of the map of geometry N.
//   LIO_GG_RESIZE  the copy loop of extendToInclude (GM:610-624): the cell's centre on N, isInside and getIndex on the old
//                  geometry O; every slot takes the old cell's bits, or the quiet NaN (isValid(*iterator) is never true
//                  there: setGeometry has just cleared the map).  Without the flag the map is worked on in place: self[k] is
//                  dst[k] at the same cell, and a slot is written only where its value changes or its layer is new.
//   LIO_GG_ADD     the loop of addDataFrom (GM:532-549) on those values: valid = every basic slot finite (none: false);
//                  skipped if valid and not LIO_GG_OVERWRITE; isInside and getIndex on X; each slot with an `other` layer takes
//                  that cell's bits where they are finite.
LIO_HD void lio_gg_position_cell(const LioGgTable& T, const LioGridGeom& N, const LioGridGeom& O, const LioGridGeom& X, int flags, int r, int c,
                                    LioGgCellCount* n)
{
    const size_t at = (size_t)c * (size_t)N.rows + (size_t)r;
    const double cx = lio_gm_centre(N, 0, r), cy = lio_gm_centre(N, 1, c);
    n->kept = n->skipped_valid = n->outside_other = n->index_outside_self = n->index_outside_other = false;
    n->copied = 0;
    bool have_self = true;
    size_t self_at = at;
    if (flags & LIO_GG_RESIZE) {
        int i, j;
        const int st = lio_gm_lookup(O, cx, cy, &i, &j);
        have_self = n->kept = st == 2;
        n->index_outside_self = st == 1;
        self_at = have_self ? (size_t)j * (size_t)O.rows + (size_t)i : 0;
    }
    bool take = false;
    size_t from = 0;
    if (flags & LIO_GG_ADD) {
        bool valid = T.basic != 0u;
        for (int k = 0; k < T.n; ++k)
            if ((T.basic >> k) & 1u) valid = valid && have_self && T.self[k] && lio_gg_word_finite(T.self[k][self_at]);
        if (valid && !(flags & LIO_GG_OVERWRITE)) {
            n->skipped_valid = true;
        } else {
            int i, j;
            const int st = lio_gm_lookup(X, cx, cy, &i, &j);
            n->outside_other = st == 0;
            n->index_outside_other = st == 1;
            take = st == 2;
            from = take ? (size_t)j * (size_t)X.rows + (size_t)i : 0;
        }
    }
    for (int k = 0; k < T.n; ++k) {
        unsigned w = LIO_QNAN_BITS;
        bool copied = false;
        if (take && T.other[k]) {
            const unsigned o = T.other[k][from];
            if (lio_gg_word_finite(o)) { w = o; copied = true; }
        }
        const bool fresh = !T.self[k];
        if (!copied && (flags & LIO_GG_RESIZE) && have_self && !fresh) w = T.self[k][self_at];
        if (copied || fresh || (flags & LIO_GG_RESIZE)) T.dst[k][at] = w;
        n->copied += copied ? 1 : 0;
    }
}
