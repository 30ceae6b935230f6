// lio_planning.h -- the one planning chain that starts from the resident keyframes (lio_planning.hip), as its five entry points
// call it: lio_kf_store_height_map, lio_kf_store_terrain_map, lio_kf_store_sdf, lio_kf_store_planning_map and
// lio_kf_store_planning_grid.  DESIGN.md sections 4j and 4k.
#pragma once
#include "../../include/liogpu.h"

// What a call asks of the chain behind the height map.  Zero-initialised, it asks for the height map alone.
struct LioPlanningRequest {
    const lio_median_fill_config* fill;        // the stages: each one absent when its configuration is NULL
    const lio_terrain_config* terrain;
    const lio_sdf_config* sdf_cfg;             // (needed with sdf)
    lio_sdf* sdf;                              // the object that receives the field; NULL: no field
    lio_planning_map_buffers out;              // the host buffers, each skipped when NULL
    lio_local_map_info* lm_info;               // the infos: each may be NULL
    lio_height_map_info* hm_info;
    lio_median_fill_info* fill_info;
    lio_terrain_info* terrain_info;
    lio_sdf_info* sdf_info;
    lio_grid* sink;                            // a resident layer set that receives the grids on the device; NULL: none
};

// lio_local_map_device and lio_height_map_device once, then whichever of the fill, the terrain layers and the field is asked
// for, each on the grid the stage before it left on the device: the null stream, complete on return.  The height map's
// and the stages' infos are zeroed before anything is refused (lm_info is lio_local_map_device's to fill).  Refusals in this order, all before a device is touched: a NULL among st, lm, pose and
// hm or an sdf without its configuration; the height map's configuration; each stage's; a store and an sdf, then a store and
// a sink, on different devices.
int lio_planning_chain(lio_kf_store* st, const lio_local_map_config* lm, const float* pose, const lio_height_map_config* hm,
                       LioPlanningRequest rq);
