// lio_sc.h -- what the keyframe store (lio_kfstore.h) needs from lio_sc.hip: the Scan Context descriptors that live next
// to the resident keyframes, their build from a cloud on the device, and the loop detection over them.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/liogpu.h"
#include "lio_pool.h"

// polarcontexts_ / polarcontext_invkeys_mat_ / polarcontext_vkeys_ of one store, descriptor k = keyframe k.  The geometry
// (rings, sectors, max_radius, lidar_height) is that of the first descriptor.  counter / prefix: tree_making_period_conter
// and the length of polarcontext_invkeys_to_search_ (SC:270-282), kept between detections.
struct LioScStore {
    int rings = 0, sectors = 0;
    double max_radius = 0.0, lidar_height = 0.0;
    size_t count = 0, cap = 0;
    LioDevBuf<float> desc;                  // [cap][rings * sectors], ring-major
    LioDevBuf<float> rkey;                  // [cap][rings]
    LioDevBuf<double> skey;                 // [cap][sectors]
    LioDevBuf<unsigned> table;              // the cells of the descriptor being built, order-mapped
    LioDevBuf<unsigned long long> keys;     // [cap] (ring-key distance bits << 32 | index) of one detection
    LioDevBytes d_res;                      // the per-candidate results of one detection
    long long counter = 0;
    int prefix = 0;
};

int lio_sc_check_config(const lio_sc_config* cfg);        // LIO_OK or LIO_ERR_ARG (lio_last_error says which field)

// Appends the descriptor of the cloud d_rec[0..n) (records of `stride` bytes on the current device, x,y,z at xyz_off) on
// stream `s`; synchronous.  cfg == NULL: the store's geometry, or the defaults for the first descriptor.
int lio_sc_store_append(LioScStore& sc, const unsigned char* d_rec, size_t stride, size_t xyz_off, size_t n, const lio_sc_config* cfg,
                        hipStream_t s, int32_t* id_out);
int lio_sc_store_get(const LioScStore& sc, int id, float* desc, float* ring_key, double* sector_key);
int lio_sc_store_detect(LioScStore& sc, const lio_sc_config* cfg, lio_sc_result* res, hipStream_t s);      // res != NULL; checks cfg
