// lio_tail.hip -- the looped form of the plain k_s2m_iterate, for the late launches of a run.  A translation unit of its own
// because it is compiled with -mllvm -disable-machine-licm (Makefile): the machine-level hoisting pass moves the constants and
// addresses of the whole body in front of the entry loop, where they do not fit into the registers of a 6-wave kernel and go to
// scratch (counted on the assembly, profiles/tail_launches_static.txt: 26 scratch accesses and 9 lane moves before the arrival
// atomic with the pass, the one store of the thread index at the kernel's entry without it).
#include <hip/hip_runtime.h>
#include "lio_s2m_block.h"

// The looped form of the plain instantiation, for the late launches of a run, when most scans have finished: a FIXED grid of
// gridDim.x workgroups (a multiple of 8), each owning a fixed share of the same P.blocks list, instead of one workgroup per entry
// that mostly finds its scan done and leaves.  No list is built in global memory and nothing is added to the arrival protocol.
//   * A launch with no scan left (*P.n_active == 0) costs gridDim.x workgroups one load and one barrier each.
//   * Share of workgroup b, with x = b & 7 (its XCD under the round-robin dispatch), j = b >> 3, W = gridDim.x / 8, n8 = n_blocks / 8:
//     entries x n8 + j + t W, t = 0, 1, .. while j + t W < n8 -- XCD x keeps its contiguous eighth of the list as in the full-grid
//     form (with xcd_remap; without it the same share is as good as any), and a workgroup's entries lie W apart, in different
//     scans; entry 8 n8 + b besides, for b < n_blocks - 8 n8.  Every entry of the list belongs to exactly one workgroup.
//   * Liveness is looked up one entry per thread (descriptor -> state[scan].done), 256 entries a round, and the live ones are
//     compacted in LDS in entry order.  A scan's `done` only changes in lio_gn_step after ALL its workgroups of this launch have
//     arrived: an entry seen live is still due in this launch however late its turn comes, and one seen done stays done.
//   * No barrier beyond the body's own two separates consecutive entries: s_rows of entry i is last read before the body's second
//     barrier, which every wave has passed before any wave starts entry i + 1; s_part is written after the FIRST barrier of entry
//     i + 1, which wave 0 only reaches after it has read s_part of entry i, arrived and (for a scan's last arrival) taken the
//     Gauss-Newton step; s_sum / s_ws are wave 0's alone.  Waves 1-3 run the next entry's search meanwhile.
__global__ __launch_bounds__(LIO_BLOCK, LIO_MIN_WAVES_PLAIN)
void k_s2m_iterate_tail(LioIterParams P, int n_blocks)
{
    __shared__ int s_live[LIO_BLOCK];
    __shared__ int s_cnt[LIO_BLOCK / 64];
    __shared__ int s_go;
    // ONE read for the whole workgroup: the counter falls while the launch runs, and waves that each read it for themselves
    // can disagree -- one leaves, the others wait at barriers for counts it never writes.  (A 0 seen late is as good as one
    // seen at the start: every scan has finished, every entry is dead.)
    if (threadIdx.x == 0) s_go = *P.n_active;
    __syncthreads();
    if (s_go == 0) return;
    const int x = blockIdx.x & 7, j = blockIdx.x >> 3, W = gridDim.x >> 3, n8 = n_blocks >> 3;
    const int n_strided = j < n8 ? (n8 - j + W - 1) / W : 0;
    const int n_own = n_strided + (((int)blockIdx.x < n_blocks - 8 * n8) ? 1 : 0);
#pragma unroll 1
    for (int r0 = 0; r0 < n_own; r0 += LIO_BLOCK) {
        unsigned tid = threadIdx.x;
        asm volatile("" : "+v"(tid));                      // (opaque once per round: see lio_s2m_block)
        const int k = r0 + (int)tid, lane = tid & 63, wave = tid >> 6;
        int e = -1;
        bool live = false;
        if (k < n_own) {
            e = k < n_strided ? x * n8 + j + k * W : 8 * n8 + (int)blockIdx.x;
            live = P.state[P.blocks[e].scan].done == 0;
        }
        // compaction in entry order: the live lanes below this one in its wave, after the live lanes of the waves before it
        const unsigned long long m = __ballot(live);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        int slot = __popcll(m & ((1ull << lane) - 1ull)), n_live = 0;
#pragma unroll
        for (int w = 0; w < LIO_BLOCK / 64; ++w) { const int c = s_cnt[w]; if (w < wave) slot += c; n_live += c; }
        if (live) s_live[slot] = e;
        __syncthreads();
        n_live = __builtin_amdgcn_readfirstlane(n_live);
#pragma unroll 1
        for (int i = 0; i < n_live; ++i) {
            // Every entry reads the kernel's arguments afresh from the kernarg segment, by scalar loads where they are used, as
            // the full-grid form does: hoisted out of this loop, P and what is derived from it (~90 SGPRs) do not fit and spill to
            // lanes.  The offset is 0 (P is the first argument), opaque to the compiler so that the loads stay inside the loop.
            int z = 0;
            asm volatile("" : "+s"(z));
            typedef const __attribute__((address_space(4))) unsigned char lio_kernarg_byte;
            lio_kernarg_byte* ka = (lio_kernarg_byte*)__builtin_amdgcn_kernarg_segment_ptr() + __builtin_amdgcn_readfirstlane(z);
            const LioIterParams& Pe = *(const LioIterParams*)ka;
            lio_s2m_block<1, false, false, true, true>(Pe, __builtin_amdgcn_readfirstlane(s_live[i]));
        }
        __syncthreads();                                   // (the next round rewrites s_cnt and s_live)
    }
}

void lio_launch_iterate_tail(const LioIterParams& P, int n_blocks, int n_wgs, hipStream_t s)
{
    if (n_blocks <= 0 || n_wgs < 8) return;
    hipLaunchKernelGGL(k_s2m_iterate_tail, dim3(n_wgs & ~7), dim3(LIO_BLOCK), 0, s, P, n_blocks);
}
