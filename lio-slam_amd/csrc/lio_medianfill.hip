// lio_medianfill.hip -- grid_map_filters' MedianFillFilter on the elevation grid the height map leaves on the device: the
// inpainting the reference asks for in front of the terrain chain and the signed distance field (SignedDistanceField.cpp:46-51).
//   k_mf_mask   the validity mask of a tile with the halo of all four box operations, opened (cleanedMask) and closed
//               (fillHoles) in LDS: eight separable passes over two byte planes, each window clipped to the grid, so a cell
//               outside the image never takes part (morphologyDefaultBorderValue) and nothing has to be reset between an
//               erosion and a dilation.  Every pass is computed for the whole staged region; what a pass cannot know (its
//               window leaves the region) lies in the rim the next passes no longer read.
//   k_mf_fill   update(): one lane per cell on the 32 x 8 tile of lio_gridtile.h staged with the halo of the larger radius.
//               A lane that fills selects the median by counting over the LDS window (lio_mf_median): 33 (2R + 1)^2 reads,
//               none for a lane that copies.  The five counts by ballot, one atomic per wave and counter.
// The per-cell arithmetic is lio_medianfill.h's.  DESIGN.md section 4j: conventions, resources, what was measured.
// The median fill only: the chain that runs it behind the height map of the resident keyframes is lio_planning.hip.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <cmath>
#include <string.h>

#include "lio_medianfill.h"
#include "lio_cloud.h"
#include "lio_pool.h"

struct MfLine {                    // a line of a byte plane in LDS: entry k at p[k * stride]
    const unsigned char* p;
    int stride;
    __device__ __forceinline__ unsigned at(int k) const { return p[k * stride]; }
};

// fill_mask, cleaned (may be NULL): rows x cols floats, 0.0f / 1.0f as cv2eigen leaves a Mat_<bool>
__global__ __launch_bounds__(LIO_TILE_LANES) void k_mf_mask(LioMfParams P, const float* __restrict__ in, float* __restrict__ fill_mask,
                                                                    float* __restrict__ cleaned)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_planes[];
    const int h = P.halo_mask, pitch = LIO_TILE_ROWS + 2 * h, width = LIO_TILE_COLS + 2 * h, n = pitch * width;
    int tr0, tc0;
    lio_tile_origin(P.rows, tr0, tc0);
    const int r0 = tr0 - h, c0 = tc0 - h;                  // the region's first cell
    unsigned char* a = s_planes;
    unsigned char* b = s_planes + n;
    for (int k = (int)threadIdx.x; k < n; k += LIO_TILE_LANES) {
        const int i = r0 + k % pitch, j = c0 + k / pitch;
        a[k] = (i >= 0 && i < P.rows && j >= 0 && j < P.cols && lio_gm_finite(in[(size_t)i + (size_t)j * (size_t)P.rows])) ? 1 : 0;
    }
    __syncthreads();
    // the part of the region that lies in the grid, in the region's own indices
    const int i_min = r0 < 0 ? -r0 : 0, i_max = (P.rows - 1 - r0 < pitch - 1) ? P.rows - 1 - r0 : pitch - 1;
    const int j_min = c0 < 0 ? -c0 : 0, j_max = (P.cols - 1 - c0 < width - 1) ? P.cols - 1 - c0 : width - 1;
    const int ti = h + ((int)threadIdx.x % LIO_TILE_ROWS), tj = h + ((int)threadIdx.x / LIO_TILE_ROWS);      // this lane's cell
    const bool in_grid = r0 + ti < P.rows && c0 + tj < P.cols;
    const size_t at = (size_t)(r0 + ti) + (size_t)(c0 + tj) * (size_t)P.rows;
    for (int op = 0; op < LIO_MF_N_OPS; ++op) {
        const int R = lio_mf_op_radius(P, op);
        const bool erode = lio_mf_op_erodes(op);
        if (R > 0) {                                       // (N = 0: no erosion at all)
            for (int k = (int)threadIdx.x; k < n; k += LIO_TILE_LANES) {        // along the rows: a -> b
                const int i = k % pitch, j = k / pitch;
                const MfLine line = { a + j * pitch, 1 };
                b[k] = (unsigned char)lio_mf_line(line, i - R < i_min ? i_min : i - R, i + R > i_max ? i_max : i + R, erode);
            }
            __syncthreads();
            for (int k = (int)threadIdx.x; k < n; k += LIO_TILE_LANES) {        // along the columns: b -> a
                const int i = k % pitch, j = k / pitch;
                const MfLine line = { b + i, pitch };
                a[k] = (unsigned char)lio_mf_line(line, j - R < j_min ? j_min : j - R, j + R > j_max ? j_max : j + R, erode);
            }
            __syncthreads();
        }
        if (op == LIO_MF_OP_CLEANED && cleaned && in_grid) cleaned[at] = a[ti + tj * pitch] ? 1.0f : 0.0f;
    }
    if (in_grid) fill_mask[at] = a[ti + tj * pitch] ? 1.0f : 0.0f;
}

// counters[0..4] += non-finite input cells, non-zero mask cells, cells filled, finite cells filtered, non-finite output cells
__global__ __launch_bounds__(LIO_TILE_LANES) void k_mf_fill(LioMfParams P, const float* __restrict__ in, const float* __restrict__ mask,
                                                                    float* __restrict__ out, int* __restrict__ counters)
{
    extern __shared__ __attribute__((aligned(16))) float s_tile[];
    int r, c;
    const LioTile T = lio_tile_stage(in, P.rows, P.cols, P.halo_fill, s_tile, r, c);
    LioMfCell o;
    o.nan_in = o.masked = o.filled = o.filtered = o.nan_out = false;
    if (r < P.rows && c < P.cols) {
        const size_t at = (size_t)r + (size_t)c * (size_t)P.rows;
        lio_mf_cell(P, T, mask[at], r, c, &o);
        out[at] = o.out;
    }
    const unsigned long long m0 = __ballot(o.nan_in), m1 = __ballot(o.masked), m2 = __ballot(o.filled), m3 = __ballot(o.filtered),
                             m4 = __ballot(o.nan_out);
    if ((threadIdx.x & 63) == 0) {
        if (m0) atomicAdd(&counters[0], __popcll(m0));
        if (m1) atomicAdd(&counters[1], __popcll(m1));
        if (m2) atomicAdd(&counters[2], __popcll(m2));
        if (m3) atomicAdd(&counters[3], __popcll(m3));
        if (m4) atomicAdd(&counters[4], __popcll(m4));
    }
}

// ---- the host side ------------------------------------------------------------------------------------------------------
extern "C" void lio_median_fill_default_config(lio_median_fill_config* cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->fill_hole_radius = 0.05;                          // the constructor's, MedianFillFilter.cpp:24-25
    cfg->existing_value_radius = 0.0;
    cfg->filter_existing_values = 0;
    cfg->num_erode_dilation_iterations = 4;
}

int lio_median_fill_check(const lio_median_fill_config* c, double resolution, LioMfParams* P)
{
    memset(P, 0, sizeof(*P));
    if (!(resolution >= 1e-4) || !std::isfinite(resolution)) return lio_fail(LIO_ERR_ARG, "resolution must be at least 1e-4");
    const double radii[] = { c->fill_hole_radius, c->existing_value_radius };
    int cells[2];
    for (int k = 0; k < 2; ++k) {
        if (!std::isfinite(radii[k]) || radii[k] < 0.0) return lio_fail(LIO_ERR_ARG, "radii must be finite and not negative");
        const double q = radii[k] / resolution;            // static_cast<size_t>(radius / resolution): truncated
        if (!(q < (double)(LIO_TILE_MAX_REACH + 1))) return lio_fail(LIO_ERR_ARG, "a radius reaches further than 32 cells");
        cells[k] = (int)q;
    }
    if (c->filter_existing_values != 0 && c->filter_existing_values != 1) return lio_fail(LIO_ERR_ARG, "filter_existing_values is 0 or 1");
    if (c->num_erode_dilation_iterations < 0 || c->num_erode_dilation_iterations > LIO_MF_MAX_ITERATIONS)
        return lio_fail(LIO_ERR_ARG, "num_erode_dilation_iterations must be in [0, 15]");
    P->r_fill = cells[0]; P->r_existing = cells[1];
    P->filter_existing = c->filter_existing_values;
    P->n_iter = c->num_erode_dilation_iterations;
    P->n_dilate = P->n_iter > 1 ? P->n_iter : 1;           // one dilation before the loop that starts at 1
    P->halo_mask = 2 + P->n_dilate + P->n_iter;
    P->halo_fill = (P->filter_existing && P->r_existing > P->r_fill) ? P->r_existing : P->r_fill;
    return LIO_OK;
}

void lio_median_fill_info_begin(lio_median_fill_info* info, const LioMfParams& P, int rows, int cols)
{
    memset(info, 0, sizeof(*info));
    info->rows = rows; info->cols = cols;
    info->fill_radius_cells = P.r_fill; info->existing_radius_cells = P.r_existing;
}

int lio_median_fill_device(const float* d_in, const LioMfParams& P, const float* mask_in, float* d_filled, float* filled, float* fill_mask,
                           float* cleaned_mask, lio_median_fill_info* info, hipStream_t s)
{
    const size_t n_cells = (size_t)P.rows * (size_t)P.cols;
    LioTemp mask, cleaned, counters;
    HIPCHK(mask.alloc(sizeof(float) * n_cells));
    HIPCHK(counters.alloc(5 * sizeof(int)));
    HIPCHK(hipMemsetAsync(counters.p, 0, 5 * sizeof(int), s));
    const unsigned tiles = lio_tile_count(P.rows, P.cols);
    if (mask_in) {                                         // :119-125: the mask of a previous run, as it is
        HIPCHK(hipMemcpyAsync(mask.p, mask_in, sizeof(float) * n_cells, hipMemcpyHostToDevice, s));
    } else {
        if (cleaned_mask) HIPCHK(cleaned.alloc(sizeof(float) * n_cells));
        hipLaunchKernelGGL(k_mf_mask, dim3(tiles), dim3(LIO_TILE_LANES), lio_tile_lds_bytes(P.halo_mask, 2), s, P, d_in, mask.as<float>(),    // (two byte planes)
                           cleaned_mask ? cleaned.as<float>() : nullptr);
    }
    hipLaunchKernelGGL(k_mf_fill, dim3(tiles), dim3(LIO_TILE_LANES), lio_tile_lds_bytes(P.halo_fill, sizeof(float)), s, P, d_in, (const float*)mask.p, d_filled, counters.as<int>());
    if (filled) HIPCHK(hipMemcpyAsync(filled, d_filled, sizeof(float) * n_cells, hipMemcpyDeviceToHost, s));
    if (fill_mask) HIPCHK(hipMemcpyAsync(fill_mask, mask.p, sizeof(float) * n_cells, hipMemcpyDeviceToHost, s));
    if (cleaned_mask && !mask_in) HIPCHK(hipMemcpyAsync(cleaned_mask, cleaned.p, sizeof(float) * n_cells, hipMemcpyDeviceToHost, s));
    int hc[5] = { 0, 0, 0, 0, 0 };
    HIPCHK(hipMemcpyAsync(hc, counters.p, sizeof(hc), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    info->n_nan_in = hc[0]; info->n_mask = hc[1]; info->n_filled = hc[2]; info->n_filtered = hc[3]; info->n_nan_out = hc[4];
    return LIO_OK;
}

extern "C" int lio_median_fill(int32_t device_id, const float* elevation, int32_t rows, int32_t cols, double resolution,
                               const lio_median_fill_config* cfg, const float* mask_in, float* filled, float* fill_mask, float* cleaned_mask,
                               lio_median_fill_info* info)
try {
    if (!cfg || !info) return lio_fail(LIO_ERR_ARG, "null argument");
    if (rows < 0 || cols < 0) return lio_fail(LIO_ERR_ARG, "rows and cols must not be negative");
    LioMfParams P;
    int rc = lio_median_fill_check(cfg, resolution, &P);
    if (rc != LIO_OK) return rc;
    lio_median_fill_info_begin(info, P, rows, cols);
    if (rows == 0 || cols == 0) return LIO_OK;             // no cell: nothing written
    if (!elevation || !filled) return lio_fail(LIO_ERR_ARG, "null argument");
    if ((long long)rows * cols > 0x7fffffffLL - 1024) return lio_fail(LIO_ERR_CAPACITY, "the grid has more than 2^31 cells");
    P.rows = rows; P.cols = cols;
    if ((rc = lio_check_device(device_id)) != LIO_OK) return rc;
    hipStream_t s = nullptr;
    const size_t n_cells = (size_t)rows * (size_t)cols;
    LioTemp grid, out;
    HIPCHK(grid.alloc(sizeof(float) * n_cells));
    HIPCHK(out.alloc(sizeof(float) * n_cells));
    HIPCHK(hipMemcpyAsync(grid.p, elevation, sizeof(float) * n_cells, hipMemcpyHostToDevice, s));
    rc = lio_median_fill_device(grid.as<float>(), P, mask_in, out.as<float>(), filled, fill_mask, cleaned_mask, info, s);
    const hipError_t e = hipStreamSynchronize(s);          // (an early return: the temporaries go back to the pool when this returns)
    if (rc < 0) return rc;
    HIPCHK(e);
    return rc;
} LIO_CATCH
