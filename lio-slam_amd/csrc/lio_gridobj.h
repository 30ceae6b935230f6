// lio_gridobj.h -- the resident layer set as the translation units that work on it see it (lio_gridsample.hip owns its
// life and its layers, lio_gridregion.hip the region workspace), and the guards their entry points share (defined in
// lio_gridsample.hip).  Every buffer is grown, never shrunk, and counted by lio_grid_memory.
#pragma once
#include "lio_pool.h"
#include "lio_stageclock.h"
#include "lio_gridmath.h"

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
    LioGridGeom G{};               // rows = cols = 0: no geometry yet
    LioDevBuf<float> d_layer[LIO_GRID_MAX_LAYERS];
    LioDevBytes d_region[LIO_RG_N_BUFS];
};

void lio_grid_clear(lio_grid* g);                          // (lio_gridsample.h)

// layer is one of 0 .. LIO_GRID_MAX_LAYERS - 1 and the object holds it
bool lio_grid_has_layer(const lio_grid* g, int layer);
// A caller's list of n <= LIO_GRID_MAX_LAYERS layer ids: each in range, none twice; *listed receives their bits.  LIO_OK or
// LIO_ERR_ARG.  Whether an object holds them is the caller's `listed & ~mask`.
int lio_grid_layer_list(const int32_t* ids, int n, unsigned* listed);

// What the object holds after a failure of the call that changes it: the layers it held when the guard was made, or
// nothing (clear_on_failure: the call replaced its geometry).  commit() once the call has succeeded.
struct LioGridRollback {
    lio_grid* g;
    unsigned mask;
    bool clear_on_failure;
    LioGridRollback(lio_grid* g_, bool clear) : g(g_), mask(g_->mask), clear_on_failure(clear) {}
    LioGridRollback(const LioGridRollback&) = delete;
    LioGridRollback& operator=(const LioGridRollback&) = delete;
    ~LioGridRollback() { if (g) { if (clear_on_failure) lio_grid_clear(g); else g->mask = mask; } }
    void commit() { g = nullptr; }
};

// The counters of one call in a pool temporary (extra: words a caller keeps behind them), cleared on the call's stream.
struct LioGridCounters {
    LioTemp t;
    int n = 0;
    hipError_t alloc(int n_, int extra = 0) { n = n_; return t.alloc((size_t)(n_ + extra) * sizeof(unsigned long long)); }
    hipError_t clear(hipStream_t s) { return hipMemsetAsync(t.p, 0, (size_t)n * sizeof(unsigned long long), s); }
    unsigned long long* d() { return t.as<unsigned long long>(); }
    // the counters down to host[n], a mark of clk (may be null), then the call's one host wait and the launches' error
    int finish(unsigned long long* host, hipStream_t s, LioStageClock* clk);
};
