// lio_debug_math.hip -- the kernels of the two designed-input test hooks of the Gauss-Newton arithmetic, lio_debug_gn_step and
// lio_debug_corner_fit (include/liogpu.h).  They call lio_gn_step and lio_corner_assoc themselves, the functions of
// lio_s2m_device.h / lio_device_math.h that k_s2m_iterate and k_s2m_persist call.  A translation unit of its own, NOT part of
// lio_kernels.hip: both functions are static, and one more caller in that file -- with speculation arguments that are not
// constants -- changes how the compiler specialises and inlines them into k_s2m_iterate (measured: every instantiation's code
// differed).  Here the library's kernels stay byte for byte what they were.  Every operation is IEEE fp32 / fp64 with
// contraction off, so the bits are determined by the source; what the hooks cannot see is a miscompilation of one particular
// inlined copy -- the whole-registration tests remain that net.
#include <hip/hip_runtime.h>
#include "lio_types.h"
#include "lio_kernels.h"
#include "lio_s2m_device.h"

// Test hook (lio_debug_gn_step): lio_gn_step itself on n independent cases, one wave per case (four to a workgroup), each with its
// own LioSolveWs and sums in LDS and its own LioScanState, which the host prepared (pose, iter, is_degenerate, matP; the rest zero)
// and reads back.  sums[i] = the LIO_SUMS doubles of case i as the reduction leaves them; ret[i] = what lio_gn_step returned.
__global__ __launch_bounds__(256) void k_debug_gn_step(LioScanState* __restrict__ st, long long n, const double* __restrict__ sums, LioConsts c,
                                                       int deg_override, int skip_eigen, int hold_if_done, int* __restrict__ ret)
{
    __shared__ LioSolveWs s_ws[4];
    __shared__ double s_sum[4][LIO_SUMS];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 4 + wave;
    if (i >= n) return;                                    // wave-uniform; lio_gn_step synchronises within the wave only
    if (lane < LIO_SUMS) s_sum[wave][lane] = sums[i * LIO_SUMS + lane];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // one wave: the sums are in LDS before any lane reads them
    const int r = lio_gn_step(&st[i], s_sum[wave], c, &s_ws[wave], nullptr, lane, deg_override, skip_eigen != 0, hold_if_done != 0);
    if (lane == 0) ret[i] = r;
}

void lio_launch_debug_gn_step(LioScanState* st, long long n, const double* sums, const LioConsts& c, int deg_override, int skip_eigen,
                              int hold_if_done, int* ret, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_debug_gn_step, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, st, n, sums, c, deg_override, skip_eigen, hold_if_done, ret);
}

// Test hook (lio_debug_corner_fit): lio_corner_assoc, the function lio_assoc_point calls for an edge point, on caller-supplied
// neighbour sets (the caller's order) and transformed points, one case per thread.  out[5 i ..] = the bits of the four coefficients, then the accept flag.
__global__ __launch_bounds__(256) void k_debug_corner_fit(const float* __restrict__ sets, const float* __restrict__ pts, long long n,
                                                          double weight, double min_s, unsigned* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float m[5][3];
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) m[j][c] = sets[i * 15 + j * 3 + c];
    float cx, cy, cz, cw;
    const bool accept = lio_corner_assoc(m, pts[i * 3 + 0], pts[i * 3 + 1], pts[i * 3 + 2], weight, min_s, cx, cy, cz, cw);
    unsigned* o = out + i * 5;
    o[0] = __float_as_uint(cx); o[1] = __float_as_uint(cy); o[2] = __float_as_uint(cz); o[3] = __float_as_uint(cw);
    o[4] = accept ? 1u : 0u;
}

void lio_launch_debug_corner_fit(const float* sets, const float* pts, long long n, double weight, double min_s, unsigned* out, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_debug_corner_fit, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, sets, pts, n, weight, min_s, out);
}
