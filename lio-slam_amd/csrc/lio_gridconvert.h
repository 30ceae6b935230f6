// lio_gridconvert.h -- the per-cell arithmetic and the index maps of lio_gridconvert.hip: grid_map_cv's GridMapCvConverter
// (CV = GridMapCvConverter.hpp) and GridMapRosConverter's toPointCloud, toGridCells and fromOccupancyGrid (RC =
// GridMapRosConverter.cpp) as __host__ __device__ functions, so that the kernels and a host program
// (tools/grid_convert_host_check.cpp) run the same text.  Every float expression is fp32 in the order the reference writes it
// and relies on -ffp-contract=off.  DESIGN.md section 4o lists the conventions and the labelled deviations (parity unpinned).
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "lio_gridmath.h"
#include "lio_sdf.h"

#define LIO_GC_TILE 64                                      // cells of a tile along either axis
#define LIO_GC_PITCH (LIO_GC_TILE + 1)                      // words of a tile line in LDS: the odd pitch keeps a column walk on 32 banks
#define LIO_GC_EMPTY 0xffffffffu                            // the tile word of a cell that leaves its pixel zero (no pixel value has it)

LIO_HD int lio_gc_elem_bytes(int depth) { return depth == LIO_IMAGE_8U ? 1 : (depth == LIO_IMAGE_16U ? 2 : 4); }
// imageMax / maxImageValue as a float (CV:87-95, :206-214)
LIO_HD float lio_gc_image_max(int depth) { return depth == LIO_IMAGE_8U ? 255.0f : (depth == LIO_IMAGE_16U ? 65535.0f : 1.0f); }
// the same as the element's word
LIO_HD unsigned lio_gc_max_word(int depth) { return depth == LIO_IMAGE_8U ? 255u : (depth == LIO_IMAGE_16U ? 65535u : 0x3f800000u); }

// Clamp (eigen_plugins/Functors.hpp:14-26)
LIO_HD float lio_gc_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

enum { LIO_GC_IN_RANGE = 0, LIO_GC_CLAMPED_LOW, LIO_GC_CLAMPED_HIGH, LIO_GC_NONFINITE };

// toImage's cell (CV:218, :229-231): the element's word, LIO_GC_EMPTY where isfinite fails.  hi > lo and hi - lo finite
// (the entry refuses everything else), so the scaled value lies in [0, max] and the cast is defined.
LIO_HD unsigned lio_gc_pixel(float x, float lo, float hi, int depth, int* cls)
{
    const float v = lio_gc_clamp(x, lo, hi);
    if (!lio_gm_finite(v)) { *cls = LIO_GC_NONFINITE; return LIO_GC_EMPTY; }
    *cls = x < lo ? LIO_GC_CLAMPED_LOW : (x > hi ? LIO_GC_CLAMPED_HIGH : LIO_GC_IN_RANGE);
    const float s = ((v - lo) / (hi - lo)) * lio_gc_image_max(depth);
    if (depth == LIO_IMAGE_32F) return __builtin_bit_cast(unsigned, s);
    return (unsigned)(int)s;                                // (Type) of a value in [0, 65535]: truncation
}

// byte b (0 .. channels * element size - 1) of the pixel of a cell whose tile word is w (CV:233-242), little-endian elements
LIO_HD unsigned lio_gc_pixel_byte(unsigned w, int b, int channels, int depth)
{
    if (w == LIO_GC_EMPTY) return 0u;
    const int es = lio_gc_elem_bytes(depth), ch = b / es, k = b - ch * es;
    const unsigned e = (channels == 4 && ch == 3) ? lio_gc_max_word(depth) : w;
    return (e >> (8 * k)) & 0xffu;
}

// How a run of `bytes` bytes at byte offset `at` of a dword-aligned buffer is stored: bytes [at, head_end) one by one, the
// dwords [d0, d1) whole, bytes [tail_begin, at + bytes) one by one.  (A run inside one dword: head only.)
struct LioGcRun { size_t head_end, d0, d1, tail_begin, end; };

LIO_HD LioGcRun lio_gc_run(size_t at, size_t bytes)
{
    LioGcRun R;
    R.end = at + bytes;
    R.d0 = (at + 3) / 4;
    R.d1 = R.end / 4;
    if (R.d1 < R.d0) { R.d1 = R.d0; R.head_end = R.tail_begin = R.end; }
    else { R.head_end = 4 * R.d0; R.tail_begin = 4 * R.d1; }
    return R;
}

// byte `o` of a run that starts at the first pixel of `line` (Line::at(pixel): the tile words); px = channels * element size
template <class Line>
LIO_HD unsigned lio_gc_run_byte(const Line& line, size_t o, int px, int channels, int depth)
{
    const size_t pixel = o / (size_t)px;
    return lio_gc_pixel_byte(line.at((int)pixel), (int)(o - pixel * (size_t)px), channels, depth);
}

// dword `d` of the buffer inside such a run that starts at byte `at`
template <class Line>
LIO_HD unsigned lio_gc_run_dword(const Line& line, size_t d, size_t at, int px, int channels, int depth)
{
    unsigned w = 0u;
    for (int k = 0; k < 4; ++k) w |= lio_gc_run_byte(line, 4 * d + (size_t)k - at, px, channels, depth) << (8 * k);
    return w;
}

// element `ch` of the pixel at p, little-endian: the value for 8U and 16U, the float's bits for 32F
LIO_HD unsigned lio_gc_element(const unsigned char* p, int ch, int depth)
{
    if (depth == LIO_IMAGE_8U) return p[ch];
    if (depth == LIO_IMAGE_16U) return (unsigned)p[2 * ch] | ((unsigned)p[2 * ch + 1] << 8);
    return (unsigned)p[4 * ch] | ((unsigned)p[4 * ch + 1] << 8) | ((unsigned)p[4 * ch + 2] << 16) | ((unsigned)p[4 * ch + 3] << 24);
}

// the grey value of a colour pixel: cvtColor's BGR2GRAY / BGRA2GRAY for 8U and 16U as OpenCV publishes it (B2Y = 1868,
// G2Y = 9617, R2Y = 4899, 14 bits, rounded to nearest): unpinned.  The weights sum to 2^14: equal channels return the channel.
LIO_HD unsigned lio_gc_grey(unsigned c0, unsigned c1, unsigned c2) { return (c0 * 1868u + c1 * 9617u + c2 * 4899u + 8192u) >> 14; }

// addLayerFromImage's cell (CV:107-115): e = the image value's element (for 32F its bits); false: alpha below the threshold
LIO_HD bool lio_gc_cell_from_pixel(unsigned e, unsigned alpha, bool has_alpha, unsigned alpha_min, float lower, float upper, int depth, float* out)
{
    if (has_alpha && alpha < alpha_min) return false;
    const float iv = depth == LIO_IMAGE_32F ? __builtin_bit_cast(float, e) : (float)e;
    *out = lower + (upper - lower) * (iv / lio_gc_image_max(depth));
    return true;
}

// (Type)(alphaThreshold * maxImageValue), CV:97, for 8U and 16U; alpha_threshold in [0, 1]
inline unsigned lio_gc_alpha_min(double alpha_threshold, int depth) { return (unsigned)(alpha_threshold * lio_gc_image_max(depth)); }

// addColorLayerFromImage's cell (CV:141-155 with colorVectorToValue, GridMapMath.cpp:586-591): the word of the float
LIO_HD unsigned lio_gc_color_word(unsigned c0, unsigned c1, unsigned c2, bool has_alpha)
{
    if (has_alpha) { const unsigned t = c0; c0 = c2; c2 = t; }   // cvtColor(BGRA2RGB); without alpha imageRGB = image
    return (c0 << 16) + (c1 << 8) + c2;
}

// what both ingest kernels need of a call
struct LioGcIngest {
    int rows, cols, channels, depth;
    int color;                     // addColorLayerFromImage
    float lower, upper;
    unsigned alpha_min;
};

// the word of the cell whose pixel lies at p; *transparent: the alpha test failed (the word is NaN)
LIO_HD unsigned lio_gc_word_from_pixel(const LioGcIngest& I, const unsigned char* p, bool* transparent)
{
    *transparent = false;
    const unsigned e0 = lio_gc_element(p, 0, I.depth);
    if (I.channels == 1) {
        float v;
        (void)lio_gc_cell_from_pixel(e0, 0u, false, 0u, I.lower, I.upper, I.depth, &v);
        return __builtin_bit_cast(unsigned, v);
    }
    const unsigned e1 = lio_gc_element(p, 1, I.depth), e2 = lio_gc_element(p, 2, I.depth);
    const bool has_alpha = I.channels == 4;
    if (I.color) return lio_gc_color_word(e0, e1, e2, has_alpha);
    float v;
    if (!lio_gc_cell_from_pixel(lio_gc_grey(e0, e1, e2), has_alpha ? lio_gc_element(p, 3, I.depth) : 0u, has_alpha, I.alpha_min, I.lower, I.upper, I.depth, &v)) {
        *transparent = true;
        return LIO_QNAN_BITS;
    }
    return __builtin_bit_cast(unsigned, v);
}

// fromOccupancyGrid's cell (RC:322)
LIO_HD unsigned lio_gc_occupancy_word(int8_t v) { return v != -1 ? __builtin_bit_cast(unsigned, (float)v) : LIO_QNAN_BITS; }

// toGridCells' test (RC:377-379)
LIO_HD bool lio_gc_cell_kept(float v, float lower, float upper) { return lio_gm_finite(v) && v >= lower && v <= upper; }

// toPointCloud's test (RC:184-195): L::word(k, i) is cell i of table entry k
struct LioGcCloud {
    const unsigned* layer[LIO_GRID_MAX_LAYERS];             // the listed layers, in the caller's order
    const unsigned* basic[LIO_GRID_MAX_LAYERS];             // the basic layers
    const unsigned* point;                                  // the point layer
    int n_layers, n_basic, point_at;                        // point_at: its place in the list, -1 when it is not listed
    int n_fields;
};

LIO_HD bool lio_gc_word_finite(unsigned w) { return (w & 0x7f800000u) != 0x7f800000u; }

LIO_HD bool lio_gc_cloud_kept(const LioGcCloud& C, int i)
{
    for (int k = 0; k < C.n_basic; ++k)
        if (!lio_gc_word_finite(C.basic[k][i])) return false;
    return lio_gc_word_finite(C.point[i]);
}

// the record of cell i at out[0 .. n_fields)
LIO_HD void lio_gc_cloud_record(const LioGcCloud& C, const LioGridGeom& G, int i, unsigned* out)
{
    int f = 0;
    for (int k = 0; k < C.n_layers; ++k) {
        if (k == C.point_at) {
            out[f++] = __builtin_bit_cast(unsigned, (float)lio_gm_centre(G, 0, i % G.rows));
            out[f++] = __builtin_bit_cast(unsigned, (float)lio_gm_centre(G, 1, i / G.rows));
            out[f++] = C.point[i];
        } else out[f++] = C.layer[k][i];
    }
}

// filterPoints (SignedDistanceField.cpp:186-196) with a decimation: the visit's shape and visit i's node
struct LioGcSdfVisit { int nx, ny, nz, step; };

LIO_HD LioGcSdfVisit lio_gc_sdf_visit(const LioSdfLookup& L, int decimation)
{
    LioGcSdfVisit V;
    V.step = decimation;
    V.nx = (int)(((long long)L.rows + decimation - 1) / decimation);
    V.ny = (int)(((long long)L.cols + decimation - 1) / decimation);
    V.nz = (int)(((long long)L.layers + decimation - 1) / decimation);
    return V;
}

LIO_HD void lio_gc_sdf_node(const LioGcSdfVisit& V, int i, int idx[3])
{
    idx[0] = (i % V.nx) * V.step;
    idx[1] = ((i / V.nx) % V.ny) * V.step;
    idx[2] = (i / (V.nx * V.ny)) * V.step;
}

// the condition of lio_sdf_to_point_cloud: a closed interval, a NaN bound is none
LIO_HD bool lio_gc_sdf_kept(float d, float lower, float upper) { return !(d < lower) && !(d > upper) && (d == d || (lower != lower && upper != upper)); }

// nodePosition (Gridmap3dLookup.hpp:79-84) narrowed to float, and the distance
LIO_HD float4 lio_gc_sdf_point(const LioSdfLookup& L, const int idx[3], float d)
{
    return make_float4((float)(L.origin[0] - (double)idx[0] * L.res), (float)(L.origin[1] - (double)idx[1] * L.res),
                       (float)(L.origin[2] + (double)idx[2] * L.res), d);
}
