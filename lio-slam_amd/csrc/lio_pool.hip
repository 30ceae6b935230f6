// lio_pool.hip -- the process-wide pool of device temporaries behind lio_pool.h (LioTemp).
#include <hip/hip_runtime.h>
#include <mutex>
#include <vector>

#include "lio_pool.h"

namespace {
struct PoolBlock { void* p; size_t cap; int device; bool busy; };
std::mutex g_pool_mu;
std::vector<PoolBlock> g_pool;
size_t g_pool_bytes = 0;
const size_t kPoolLimit = (size_t)8 << 30;      // idle + busy bytes kept before idle blocks are dropped

// Frees every idle block, each on its own device, and leaves `dev` current.  Called with g_pool_mu held.
void pool_drop_idle(int dev)
{
    for (size_t i = 0; i < g_pool.size();) {
        if (!g_pool[i].busy) {
            (void)hipSetDevice(g_pool[i].device);
            (void)hipFree(g_pool[i].p);
            g_pool_bytes -= g_pool[i].cap;
            g_pool[i] = g_pool.back();
            g_pool.pop_back();
        } else {
            ++i;
        }
    }
    (void)hipSetDevice(dev);
}
}  // namespace

hipError_t lio_pool_acquire(void** p, size_t bytes)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    int best = -1;
    for (size_t i = 0; i < g_pool.size(); ++i) {
        const PoolBlock& b = g_pool[i];
        if (!b.busy && b.device == dev && b.cap >= bytes && b.cap <= 2 * bytes + 4096 &&
            (best < 0 || b.cap < g_pool[best].cap))
            best = (int)i;
    }
    if (best >= 0) { g_pool[best].busy = true; *p = g_pool[best].p; return hipSuccess; }
    if (g_pool_bytes + bytes > kPoolLimit) pool_drop_idle(dev);   // before growing further
    const size_t cap = bytes + bytes / 4 + 256;
    e = hipMalloc(p, cap);
    if (e != hipSuccess) return e;
    g_pool.push_back({ *p, cap, dev, true });
    g_pool_bytes += cap;
    return hipSuccess;
}

void lio_pool_release(void* p)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (PoolBlock& b : g_pool)
        if (b.p == p) { b.busy = false; return; }
}

size_t lio_pool_disown(void* p)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_pool.size(); ++i)
        if (g_pool[i].p == p) {
            const size_t cap = g_pool[i].cap;
            g_pool_bytes -= cap;
            g_pool[i] = g_pool.back();
            g_pool.pop_back();
            return cap;
        }
    return 0;
}

void lio_pool_adopt(void* p, size_t cap, int device)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool.push_back({ p, cap, device, false });
    g_pool_bytes += cap;
}

void lio_pool_trim(void)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    int dev = 0;
    (void)hipGetDevice(&dev);
    pool_drop_idle(dev);
}
