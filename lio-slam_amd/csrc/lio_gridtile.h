// lio_gridtile.h -- the tile of every kernel that runs one lane per cell of a column-major layer (the terrain layers,
// the median fill, the grid filters): its size, the largest halo it is staged with, how many workgroups cover a grid,
// how much LDS one of them asks for, where its tile begins, and the staging of a float layer into LDS.  Each exists here and
// nowhere else.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "lio_gridmath.h"

#define LIO_TILE_ROWS 32           // rows are the contiguous axis of the column-major grid, a wave covers 32 x 2
#define LIO_TILE_COLS 8
#define LIO_TILE_LANES (LIO_TILE_ROWS * LIO_TILE_COLS)
#define LIO_TILE_MAX_REACH 32      // the largest radius and half-window, in cells: bounds the halo of the LDS tile

// the workgroups of a launch over rows x cols cells: tile rows first, as lio_tile_origin reads blockIdx.x
inline unsigned lio_tile_count(int rows, int cols)
{
    return (unsigned)((rows + LIO_TILE_ROWS - 1) / LIO_TILE_ROWS) * (unsigned)((cols + LIO_TILE_COLS - 1) / LIO_TILE_COLS);
}

// the dynamic LDS of a tile staged with `halo` cells around it
inline size_t lio_tile_lds_bytes(int halo, size_t bytes_per_cell)
{
    return bytes_per_cell * (size_t)(LIO_TILE_ROWS + 2 * halo) * (size_t)(LIO_TILE_COLS + 2 * halo);
}

// the first cell of this workgroup's tile
__device__ __forceinline__ void lio_tile_origin(int rows, int& tr0, int& tc0)
{
    const int tiles_r = (rows + LIO_TILE_ROWS - 1) / LIO_TILE_ROWS;
    tr0 = ((int)blockIdx.x % tiles_r) * LIO_TILE_ROWS;
    tc0 = ((int)blockIdx.x / tiles_r) * LIO_TILE_COLS;
}

struct LioTile {                   // the LDS tile: rows [r0, r0 + pitch), columns from c0
    const float* t;
    int r0, c0, pitch;
    __device__ __forceinline__ float at(int i, int j) const { return t[(i - r0) + (j - c0) * pitch]; }
};

// The workgroup's tile of `src` and h cells around it -> LDS (NaN outside the grid); the cell of this lane -> (r, c).
// Ends with the barrier.
__device__ __forceinline__ LioTile lio_tile_stage(const float* __restrict__ src, int rows, int cols, int h, float* tile, int& r, int& c)
{
    int tr0, tc0;
    lio_tile_origin(rows, tr0, tc0);
    const int pitch = LIO_TILE_ROWS + 2 * h, n = pitch * (LIO_TILE_COLS + 2 * h);
    for (int k = (int)threadIdx.x; k < n; k += LIO_TILE_LANES) {
        const int i = tr0 - h + k % pitch, j = tc0 - h + k / pitch;
        tile[k] = (i >= 0 && i < rows && j >= 0 && j < cols) ? src[(size_t)i + (size_t)j * (size_t)rows] : LIO_QNAN;
    }
    __syncthreads();
    r = tr0 + ((int)threadIdx.x % LIO_TILE_ROWS);
    c = tc0 + ((int)threadIdx.x / LIO_TILE_ROWS);
    LioTile T;
    T.t = tile; T.r0 = tr0 - h; T.c0 = tc0 - h; T.pitch = pitch;
    return T;
}
