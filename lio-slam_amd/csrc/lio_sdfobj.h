// lio_sdfobj.h -- the resident distance field as the translation units that work on it see it (lio_sdf.hip owns its life and
// builds it, lio_gridconvert.hip reads the nodes).  Every buffer is grown, never shrunk, and counted by lio_sdf_memory.
#pragma once
#include "lio_pool.h"
#include "lio_sdf.h"

struct lio_sdf {
    int device_id = 0;
    bool built = false;
    LioSdfLookup L{};
    LioDevBuf<float> d_elev;       // the host grid of lio_sdf_build on its way in
    LioDevBuf<float> d_dist;       // [layer][col][row]
    LioDevBuf<float4> d_nodes;     // the same order
    LioDevBuf<float> d_mid;        // a slab's intermediate [col][2 slab][row]
    LioDevBuf<uint2> d_stack;      // the lines' lower bounds, [depth][line]
    LioDevBuf<unsigned> d_stats;   // min, max (ordered words), non-finite cells
};
