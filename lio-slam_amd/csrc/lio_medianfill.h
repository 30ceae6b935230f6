// lio_medianfill.h -- grid_map_filters' MedianFillFilter (MedianFillFilter.cpp) behind the planning height map
// (lio_medianfill.hip): what the entry points need, and the filter's arithmetic as __host__ __device__ functions over
// accessors, so that the kernels (LDS tiles) and a host program (the grid itself) run the same text.  Every operation is a
// selection or a comparison: there is no rounding, and the result is held to the restatement bit for bit.  DESIGN.md section
// 4j lists the conventions, the reference's two accidental behaviours included.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include "../../include/liogpu.h"
#include "lio_gridmath.h"
#include "lio_gridtile.h"                                   // LIO_TILE_MAX_REACH and the tile of the kernels
#include "lio_wg.h"

#define LIO_MF_MAX_ITERATIONS 15   // num_erode_dilation_iterations: the mask's halo 2 + max(N, 1) + N stays within LIO_TILE_MAX_REACH

struct LioMfParams {
    int rows, cols;
    int r_fill, r_existing;        // static_cast<size_t>(radius / resolution), :127-128
    int filter_existing;
    int n_iter, n_dilate;          // N erosions after max(N, 1) dilations (fillHoles, :226-239)
    int halo_mask;                 // 2 + n_dilate + n_iter: the opening's two cells, then the closing's
    int halo_fill;                 // the larger of the radii in use
};

// what one cell yields
struct LioMfCell {
    float out;
    bool nan_in, masked, filled, filtered, nan_out;
};

// One pass of a box erosion (and) or dilation (or) along a line.  L::at(k): mask cell k of the line, 0 or 1, for
// lo <= k <= hi; the caller has clipped [lo, hi] to the grid (lio_gm_clip: cells outside the image take no part,
// morphologyDefaultBorderValue), so an empty range yields the pass's identity.  k iterations of
// the 3 x 3 element under the default border are one (2k + 1)^2 box clipped to the grid, and a clipped box is the pass
// along the rows followed by the pass along the columns (tests/test_median_fill_cpu.py proves both on random masks).
template <class L>
LIO_HD unsigned lio_mf_line(const L& line, int lo, int hi, bool erode)
{
    unsigned v = erode ? 1u : 0u;
    for (int k = lo; k <= hi; ++k) {
        const unsigned m = line.at(k);
        v = erode ? (v & m) : (v | m);
    }
    return v;
}

// The four box operations of computeAndAddFillMask in order: cleanedMask's surviving erode + dilate (:220-221; the pair at
// :218-219 is overwritten), then fillHoles' max(N, 1) dilations and N erosions.
LIO_HD int lio_mf_op_radius(const LioMfParams& P, int op) { return op < 2 ? 1 : (op == 2 ? P.n_dilate : P.n_iter); }
LIO_HD bool lio_mf_op_erodes(int op) { return op == 0 || op == 3; }
#define LIO_MF_N_OPS 4
#define LIO_MF_OP_CLEANED 1        // the mask after this operation is the filter's debug layer

// getMedian (:153-186): the element at sorted position n / 2 of the n finite values in the window of R cells around (r, c),
// the canonical quiet NaN for none.  M::at(i, j): the input layer, read within R cells of (r, c) and inside the grid only.
// The selection runs on the ordered 32-bit key of lio_wg.h (-0 sorts below +0: a convention, std::nth_element leaves it
// open): one pass counts, then one pass per key bit, most significant first, fixes that bit of the answer by counting the
// values that agree with the bits fixed so far and have a 0 there.  No per-lane array: the window stays where M keeps it.
template <class M>
LIO_HD float lio_mf_median(const M& in, int r, int c, int R, int rows, int cols)
{
    int i0, i1, j0, j1;
    lio_gm_clip(r, R, rows, i0, i1);
    lio_gm_clip(c, R, cols, j0, j1);
    unsigned n = 0;
    for (int j = j0; j <= j1; ++j)
        for (int i = i0; i <= i1; ++i) n += lio_gm_finite(in.at(i, j)) ? 1u : 0u;
    if (n == 0) return __builtin_bit_cast(float, 0x7fc00000u);
    unsigned k = n / 2, key = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned fixed = ~((2u << bit) - 1u) | (1u << bit);                  // the bits above `bit`, and `bit`
        unsigned zeros = 0;
        for (int j = j0; j <= j1; ++j)
            for (int i = i0; i <= i1; ++i) {
                const float v = in.at(i, j);
                zeros += (lio_gm_finite(v) && (lio_f2ord(v) & fixed) == key) ? 1u : 0u;
            }
        if (k >= zeros) { k -= zeros; key |= 1u << bit; }
    }
    return lio_ord2f(key);
}

// One cell of update() (:132-145).  mask: shouldFill at (r, c), non-zero = fill (a NaN compares non-zero, as there).
template <class M>
LIO_HD void lio_mf_cell(const LioMfParams& P, const M& in, float mask, int r, int c, LioMfCell* o)
{
    const float v = in.at(r, c);
    const bool fin = lio_gm_finite(v);
    o->masked = mask != 0.0f;
    o->nan_in = !fin;
    o->filtered = false;
    o->out = v;                                            // the bits as they are: payloads and infinities pass through
    if (!fin && o->masked) {
        o->out = lio_mf_median(in, r, c, P.r_fill, P.rows, P.cols);
    } else if (P.filter_existing && o->masked) {
        o->out = lio_mf_median(in, r, c, P.r_existing, P.rows, P.cols);
        o->filtered = true;
    }
    o->nan_out = !lio_gm_finite(o->out);
    o->filled = !fin && !o->nan_out;
}

// ---- the host side (lio_medianfill.hip)
// The configuration against `resolution`, before any device is touched: LIO_ERR_ARG as include/liogpu.h lists.  Fills
// everything of *P but rows and cols.
int lio_median_fill_check(const lio_median_fill_config* cfg, double resolution, LioMfParams* P);
// *info zeroed, then the size and the two radii in cells: what the info holds before the filter has run.
void lio_median_fill_info_begin(lio_median_fill_info* info, const LioMfParams& P, int rows, int cols);
// The filter on the device grid d_in (P.rows x P.cols, column-major) on stream s: the filled grid to d_filled (device, the
// same size, not d_in), and to the host whatever of filled / fill_mask / cleaned_mask is not NULL.  mask_in (host, may be
// NULL): the mask of a previous run, used as it is; cleaned_mask is then left alone.  Synchronous.
int lio_median_fill_device(const float* d_in, const LioMfParams& P, const float* mask_in, float* d_filled, float* filled, float* fill_mask,
                           float* cleaned_mask, lio_median_fill_info* info, hipStream_t s);
