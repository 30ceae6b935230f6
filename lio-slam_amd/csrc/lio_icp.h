// lio_icp.h -- what lio_icp.hip, the loop-closure registration, offers the other chains (the local map's grid choice).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/liogpu.h"
#include "lio_types.h"

// Optional per-iteration record of one alignment (lio_icp_debug_trace): host arrays, cfg.max_iters entries each
// (step: 16 floats per entry), corr: n_src entries for iteration rec_iter.  Any pointer may be null.
struct LioIcpTrace {
    float* step = nullptr;
    int32_t* n_corr = nullptr;
    double* mse = nullptr;
    int32_t* corr = nullptr;
    int rec_iter = -1;
    int n_trace = 0;          // out: entries written (the executed iterations, the one that found too few pairs included)
};

int lio_icp_check_config(const lio_icp_config* cfg);       // LIO_OK or LIO_ERR_ARG (lio_last_error says which field)

// pcl::IterativeClosestPoint::align + getFitnessScore on two device-resident clouds (float4 x, y, z, anything), on stream
// `s`; synchronous.  guess: 16 floats row-major or null.  d_closed (may be null, n_src entries): the source under the
// final transformation, w kept.  Fills every field of *res but pose_corrected.
int lio_icp_device(const float4* d_src, int n_src, const float4* d_tgt, int n_tgt, const lio_icp_config& cfg,
                   const float* guess, lio_icp_result* res, hipStream_t s, LioIcpTrace* trace, float4* d_closed);

// The uniform grid of a cell-walking search over the box mn .. mx of n device points (SoA): the edge (*edge) from their
// density, about `per_cell` points per occupied cell, at most 2^22 cells.  One host wait (the occupied cells of a trial grid,
// also written to *occupied when it is given and a trial grid is laid).
int lio_icp_choose_grid(const float* x, const float* y, const float* z, int n, const float mn[3], const float mx[3], float per_cell,
                        hipStream_t s, LioGrid* g, float* edge, int* occupied = nullptr);
