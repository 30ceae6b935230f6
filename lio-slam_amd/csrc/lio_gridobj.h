// lio_gridobj.h -- the resident layer set as the translation units that work on it see it (lio_gridsample.hip owns its
// life and its layers, lio_gridregion.hip the region workspace).  Every buffer is grown, never shrunk, and counted by
// lio_grid_memory.
#pragma once
#include "lio_pool.h"
#include "lio_terrain.h"

enum {                             // the region calls' workspace (lio_gridregion.hip)
    LIO_RG_BUF_REGIONS = 0,        // the packed regions
    LIO_RG_BUF_VERTICES,           // the polygons' vertices
    LIO_RG_BUF_PLANS,              // one LioRgPlan a region
    LIO_RG_BUF_STATS,              // lio_grid_region_reduce's records
    LIO_RG_BUF_SMALL,              // the counters, then n_cells and status per region
    LIO_RG_BUF_SCAN,               // lio_grid_region_cells: the offsets and the scan's scratch
    LIO_RG_BUF_CELLS,              // its cells
    LIO_RG_N_BUFS
};

struct lio_grid {
    int device_id = 0;
    unsigned mask = 0;             // bit k: layer k is present
    LioTerrGeom G{};               // rows = cols = 0: no geometry yet
    LioDevBuf<float> d_layer[LIO_GRID_MAX_LAYERS];
    LioDevBytes d_region[LIO_RG_N_BUFS];
};
