// lio_compact.h -- the order-preserving compaction the planning local map (lio_localmap.hip), the height map
// (lio_heightmap.hip), the occupancy grid (lio_ogm.hip) and the grid converters (lio_gridconvert.hip) share: a predicate decides
// per point whether it stays and as what; the survivors keep their order.
#pragma once
#include <hip/hip_runtime.h>
#include "lio_pool.h"
#include "lio_wg.h"

// ---- order-preserving compaction ------------------------------------------------------------------------------------------
// pred(i, &q): does point i stay, and as what.  k_lm_count: survivors per workgroup; k_wg_scan_in_place over those counts;
// k_lm_emit: the predicate again (cheaper than a flag array written and read back), a workgroup scan, the survivors only.
// Rec: what the predicate yields for a survivor (float4 unless named); Sink: sink(at, q) writes survivor number `at`.
template <class T>
struct LioCompactStore {           // the plain sink: record `at` of an array
    T* out;
    __device__ __forceinline__ void operator()(int at, const T& q) const { out[at] = q; }
};

template <class Pred, class Rec = float4>
__global__ __launch_bounds__(256) void k_lm_count(Pred pred, int n, int* __restrict__ wg_count)
{
    __shared__ int s_wave[4];
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    Rec q;
    const int keep = (i < n && pred(i, q)) ? 1 : 0;
    int tot;
    lio_wg_exclusive_scan<4>(keep, &tot, s_wave);
    if (threadIdx.x == 0) wg_count[blockIdx.x] = tot;
}

template <class Pred, class Rec = float4, class Sink = LioCompactStore<float4>>
__global__ __launch_bounds__(256) void k_lm_emit(Pred pred, int n, const int* __restrict__ wg_first, Sink sink)
{
    __shared__ int s_wave[4];
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    Rec q = Rec();
    const int keep = (i < n && pred(i, q)) ? 1 : 0;
    int tot;
    const int at = wg_first[blockIdx.x] + lio_wg_exclusive_scan<4>(keep, &tot, s_wave);
    if (keep) sink(at, q);
}

// The two halves, for a caller that sizes its output by the count (lio_gridconvert.hip): survivors per workgroup and their
// exclusive scan in counts[0 .. n_wg), the total behind them (n > 0; nothing waits) ...
template <class Rec, class Pred>
static int compact_count(const Pred& pred, int n, LioTemp& counts, hipStream_t s)
{
    const int n_wg = (n + 255) / 256;
    HIPCHK(counts.alloc(sizeof(int) * ((size_t)n_wg + 1)));
    int* c = counts.as<int>();
    hipLaunchKernelGGL((k_lm_count<Pred, Rec>), dim3(n_wg), dim3(256), 0, s, pred, n, c);
    hipLaunchKernelGGL(k_wg_scan_in_place<4>, dim3(1), dim3(256), 0, s, c, n_wg, c + n_wg);
    return LIO_OK;
}

// ... and the survivors through the sink, in order
template <class Rec, class Pred, class Sink>
static void compact_emit(const Pred& pred, int n, LioTemp& counts, const Sink& sink, hipStream_t s)
{
    hipLaunchKernelGGL((k_lm_emit<Pred, Rec, Sink>), dim3((n + 255) / 256), dim3(256), 0, s, pred, n, counts.as<int>(), sink);
}

// `out` = the points of [0, n) the predicate keeps, in order; one host wait (the count).
template <class Pred>
static int compact_device(const Pred& pred, int n, LioTemp& out, int* n_out, hipStream_t s)
{
    *n_out = 0;
    const int n_wg = (n + 255) / 256;
    LioTemp counts;
    HIPCHK(out.alloc(sizeof(float4) * (size_t)(n ? n : 1)));
    if (n == 0) return LIO_OK;
    const int rc = compact_count<float4>(pred, n, counts, s);
    if (rc != LIO_OK) return rc;
    compact_emit<float4>(pred, n, counts, LioCompactStore<float4>{ out.as<float4>() }, s);
    int total = 0;
    HIPCHK(hipMemcpyAsync(&total, counts.as<int>() + n_wg, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    *n_out = total;
    return LIO_OK;
}
