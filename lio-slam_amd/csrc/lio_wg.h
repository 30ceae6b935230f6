// lio_wg.h -- the workgroup building blocks the feeder kernels share: the order-preserving float <-> uint mapping of the
// bounding-box atomics, the per-wave counter, the exclusive scan over a workgroup (and the carry loop on top of it), and
// the min / max box of three coordinates over a workgroup.  Device code besides the float-order pair.  Every reduction here has a FIXED shape
// (stated at each function); the results of the kernels that call them are pinned bit for bit by the tests, so keep it.
#pragma once
#include <hip/hip_runtime.h>

// ---- order-preserving float <-> uint (atomicMin / atomicMax on floats through unsigned words) ---------------------------
__host__ __device__ inline unsigned lio_f2ord(float f)
{
    const unsigned u = __builtin_bit_cast(unsigned, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__host__ __device__ inline float lio_ord2f(unsigned u)
{
    return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// A box as six ordered words: [0..2] = min, [3..5] = max.  The identities of the atomics = the box of no point at all.
#define LIO_ORD_NO_MIN 0xffffffffu
#define LIO_ORD_NO_MAX 0u

__host__ __device__ inline void lio_ord_box_clear(unsigned b[6])
{
    for (int a = 0; a < 3; ++a) { b[a] = LIO_ORD_NO_MIN; b[3 + a] = LIO_ORD_NO_MAX; }
}

// (an untouched box decodes to NaN bit patterns, min > max in no ordered sense: every caller tests for its own notion of "empty")
__host__ __device__ inline void lio_ord_box_decode(const unsigned b[6], float mn[3], float mx[3])
{
    for (int a = 0; a < 3; ++a) { mn[a] = lio_ord2f(b[a]); mx[a] = lio_ord2f(b[3 + a]); }
}

// ---- counting --------------------------------------------------------------------------------------------------------
// counters[which] += the lanes of the wave whose flag is set: one ballot, one atomic per wave (none where no lane has it).
// Every lane of the wave must arrive.
__device__ __forceinline__ void lio_wave_count(unsigned long long* counters, int which, bool flag)
{
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&counters[which], (unsigned long long)__popcll(m));
}

// ---- exclusive scan -------------------------------------------------------------------------------------------------
// inclusive scan over the wave: shuffle-up by 1, 2, .. 32
template <typename T>
__device__ __forceinline__ T lio_wave_inclusive_scan(T v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    return v;
}

// Exclusive scan of one value per thread over a workgroup of WAVES waves; *total = the sum.  s_wave: WAVES values of LDS,
// free again on return (the closing barrier), so calls may follow each other on the same scratch.
template <int WAVES, typename T>
__device__ __forceinline__ T lio_wg_exclusive_scan(T v, T* total, T* s_wave)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = lio_wave_inclusive_scan(v);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    T wave_off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) { const T s = s_wave[w]; if (w < wave) wave_off += s; tot += s; }
    __syncthreads();
    *total = tot;
    return wave_off + incl - v;
}

// Exclusive scan of a[0..n) in place by ONE workgroup, chunks of its size with a carry; returns the sum (in every thread).
template <int WAVES, typename T>
__device__ __forceinline__ T lio_wg_scan_in_place(T* __restrict__ a, int n, T* s_wave)
{
    T carry = 0;
    for (int b = 0; b < n; b += WAVES * 64) {
        const int i = b + (int)threadIdx.x;
        const T v = i < n ? a[i] : T(0);
        T tot;
        const T ex = lio_wg_exclusive_scan<WAVES>(v, &tot, s_wave);
        if (i < n) a[i] = carry + ex;
        carry += tot;
    }
    return carry;
}

// exclusive scan of `n` ints in place by ONE workgroup of WAVES waves (per-workgroup counts: a few thousand entries at
// most); *total (optional) receives the sum.  A template, so that only the translation units that launch it hold a copy.
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_wg_scan_in_place(int* __restrict__ a, int n, int* __restrict__ total)
{
    __shared__ int s_wave[WAVES];
    const int sum = lio_wg_scan_in_place<WAVES>(a, n, s_wave);
    if (total && threadIdx.x == 0) *total = sum;
}

// ---- min / max box of three coordinates --------------------------------------------------------------------------------
// Shape (fminf / fmaxf are order-dependent on NaN and on -0 / +0, and not every caller filters its input): xor butterfly
// 32, 16, .. 1 inside a wave, then the waves folded in ascending order starting from wave 0.
__device__ __forceinline__ void lio_wave_box(float mn[3], float mx[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], off));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], off));
        }
    }
}

template <int WAVES> struct LioWgBoxLds { float mn[WAVES][3], mx[WAVES][3]; };

// wave boxes -> LDS; ends with the barrier after which lio_wg_box_axis may be called by any thread
template <int WAVES>
__device__ __forceinline__ void lio_wg_box_stage(float mn[3], float mx[3], LioWgBoxLds<WAVES>& s)
{
    lio_wave_box(mn, mx);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { s.mn[wave][a] = mn[a]; s.mx[wave][a] = mx[a]; }
    }
    __syncthreads();
}

template <int WAVES>
__device__ __forceinline__ void lio_wg_box_axis(const LioWgBoxLds<WAVES>& s, int a, float& lo, float& hi)
{
    lo = s.mn[0][a]; hi = s.mx[0][a];
    for (int w = 1; w < WAVES; ++w) { lo = fminf(lo, s.mn[w][a]); hi = fmaxf(hi, s.mx[w][a]); }
}

// The box of the workgroup: in, every thread's mn / mx (left holding its wave's box); out, lo / hi of axis a in thread a
// (threads 0..2; untouched in the others).  One barrier, none after the read: s is not to be reused without one.
template <int WAVES>
__device__ __forceinline__ void lio_wg_box(float mn[3], float mx[3], LioWgBoxLds<WAVES>& s, float& lo, float& hi)
{
    lio_wg_box_stage(mn, mx, s);
    if (threadIdx.x < 3) lio_wg_box_axis(s, (int)threadIdx.x, lo, hi);
}
