// lio_stageclock.h -- the stage times behind every *_debug_stage_ms hook: the clock of one call and the calling thread's
// slot that the hook reads.  Host only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../include/liogpu.h"

// Stage boundaries as HIP events on the call's stream, only when the calling thread asked for the times: off, a mark does
// nothing and nothing is allocated.  An event that cannot be created turns this call's timing off; it never fails the call.
struct LioStageClock {
    std::vector<hipEvent_t> ev;
    bool on;
    explicit LioStageClock(bool want) : on(want) {}
    LioStageClock(const LioStageClock&) = delete;
    LioStageClock& operator=(const LioStageClock&) = delete;
    ~LioStageClock() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    void mark(hipStream_t s)
    {
        if (!on) return;
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) { on = false; return; }
        ev.push_back(e);
        (void)hipEventRecord(e, s);
    }
    size_t count() const { return on ? ev.size() : 0; }    // the marks made (none once the timing went off)
    float ms(size_t k) const                               // between marks k and k + 1, after a wait that covers both; 0 when either is missing
    {
        float t = 0.0f;
        return k + 1 < count() && hipEventElapsedTime(&t, ev[k], ev[k + 1]) == hipSuccess ? t : 0.0f;
    }
};

// The calling thread's request and the N stage times of its last call: one thread_local slot per hook.
template <int N>
struct LioStageTimes {
    float ms[N] = {};
    bool on = false;
    void clear() { memset(ms, 0, sizeof(ms)); }
    void read(const LioStageClock& clk)                    // a call that made all N + 1 marks; any other leaves the slot as it is
    {
        if (clk.count() != (size_t)N + 1) return;
        for (int k = 0; k < N; ++k) ms[k] = clk.ms((size_t)k);
    }
    int hook(int32_t enable, float* out)                   // the whole body of a *_debug_stage_ms entry
    {
        if (out) memcpy(out, ms, sizeof(ms));
        on = enable != 0;
        return LIO_OK;
    }
};
