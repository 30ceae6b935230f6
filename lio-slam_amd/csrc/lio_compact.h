// lio_compact.h -- the order-preserving compaction the planning local map (lio_localmap.hip) and the height map
// (lio_heightmap.hip) share: a predicate decides per point whether it stays and as what; the survivors keep their order.
#pragma once
#include <hip/hip_runtime.h>
#include "lio_pool.h"
#include "lio_wg.h"

// ---- order-preserving compaction ------------------------------------------------------------------------------------------
// pred(i, &q): does point i stay, and as what.  k_lm_count: survivors per workgroup; k_wg_scan_in_place over those counts;
// k_lm_emit: the predicate again (cheaper than a flag array written and read back), a workgroup scan, the survivors only.
template <class Pred>
__global__ __launch_bounds__(256) void k_lm_count(Pred pred, int n, int* __restrict__ wg_count)
{
    __shared__ int s_wave[4];
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    float4 q;
    const int keep = (i < n && pred(i, q)) ? 1 : 0;
    int tot;
    lio_wg_exclusive_scan<4>(keep, &tot, s_wave);
    if (threadIdx.x == 0) wg_count[blockIdx.x] = tot;
}

template <class Pred>
__global__ __launch_bounds__(256) void k_lm_emit(Pred pred, int n, const int* __restrict__ wg_first, float4* __restrict__ out)
{
    __shared__ int s_wave[4];
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int keep = (i < n && pred(i, q)) ? 1 : 0;
    int tot;
    const int at = wg_first[blockIdx.x] + lio_wg_exclusive_scan<4>(keep, &tot, s_wave);
    if (keep) out[at] = q;
}

// `out` = the points of [0, n) the predicate keeps, in order; one host wait (the count).
template <class Pred>
static int compact_device(const Pred& pred, int n, LioTemp& out, int* n_out, hipStream_t s)
{
    *n_out = 0;
    const int n_wg = (n + 255) / 256;
    LioTemp counts;
    HIPCHK(counts.alloc(sizeof(int) * ((size_t)n_wg + 1)));
    HIPCHK(out.alloc(sizeof(float4) * (size_t)(n ? n : 1)));
    if (n == 0) return LIO_OK;
    int* c = counts.as<int>();
    hipLaunchKernelGGL(k_lm_count<Pred>, dim3(n_wg), dim3(256), 0, s, pred, n, c);
    hipLaunchKernelGGL(k_wg_scan_in_place<4>, dim3(1), dim3(256), 0, s, c, n_wg, c + n_wg);
    hipLaunchKernelGGL(k_lm_emit<Pred>, dim3(n_wg), dim3(256), 0, s, pred, n, c, out.as<float4>());
    int total = 0;
    HIPCHK(hipMemcpyAsync(&total, c + n_wg, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    *n_out = total;
    return LIO_OK;
}
