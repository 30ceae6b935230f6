// lio_pool.h -- what every host translation unit of the library shares: the error plumbing of the C ABI (lio_fail, HIPCHK,
// LIO_CATCH), the owning device and pinned-host buffers, and the recycling device-memory pool of the stateless entry points
// (lio_deskew, lio_curvature, lio_voxel_grid, lio_assemble_map*).  hipMalloc/hipFree cost milliseconds each; the
// temporaries of those calls are taken from and returned to the pool instead.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <utility>

#include "../../include/liogpu.h"

int lio_fail(int code, const char* what, hipError_t e = hipSuccess);   // sets lio_last_error, returns `code`
int lio_fail_exception(void);                                            // inside a handler: the same for the exception

#define HIPCHK(expr)                                                              \
    do {                                                                          \
        hipError_t _e = (expr);                                                   \
        if (_e != hipSuccess) return lio_fail(LIO_ERR_HIP, #expr, _e);            \
    } while (0)

// Exception boundary of every extern "C" entry point that returns a status:
//   extern "C" int lio_x(...) try { ... } LIO_CATCH
#define LIO_CATCH catch (...) { return lio_fail_exception(); }

// Owning device buffer of `cap` elements of T.  The destructor frees it on the current device: the owner's *_destroy
// entry point sets that device first.
template <typename T>
struct LioDevBuf {
    T* p = nullptr;
    size_t cap = 0;

    LioDevBuf() = default;
    LioDevBuf(const LioDevBuf&) = delete;
    LioDevBuf& operator=(const LioDevBuf&) = delete;
    LioDevBuf(LioDevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    LioDevBuf& operator=(LioDevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }   // (o frees the old block)
    ~LioDevBuf() { if (p) (void)hipFree(p); }

    operator T*() const { return p; }
    template <typename U> U* as() const { return (U*)p; }

    // Room for `need` elements.  An empty or smaller buffer is replaced by one of need * slack + pad elements; the old block
    // is freed first, after a device-wide wait when `sync` (a reader of it may still be in flight).  *fresh tells whether the
    // buffer was replaced.
    hipError_t grow(size_t need, double slack = 1.25, size_t pad = 64, bool sync = false, bool* fresh = nullptr)
    {
        if (fresh) *fresh = false;
        if (p && need <= cap) return hipSuccess;
        if (p) {
            hipError_t e = sync ? hipDeviceSynchronize() : hipSuccess;
            if (e != hipSuccess) return e;
            e = hipFree(p);
            p = nullptr; cap = 0;
            if (e != hipSuccess) return e;
        }
        const size_t n = (size_t)((double)need * slack) + pad;
        const hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = n;
        if (fresh) *fresh = true;
        return hipSuccess;
    }

    // The call LioVoxWs makes (as on LioTemp), in bytes: the rule of the workspaces kept between calls -- bytes * 1.25 + 256,
    // waiting for the device before a block that is grown out of is freed.
    hipError_t alloc(size_t bytes)
    {
        static_assert(sizeof(T) == 1, "alloc() sizes byte buffers");
        return grow(bytes ? bytes : 16, 1.25, 256, true);
    }
};
typedef LioDevBuf<unsigned char> LioDevBytes;

// Owning pinned host buffer of `cap` elements of T.
template <typename T>
struct LioPinned {
    T* p = nullptr;
    size_t cap = 0;

    LioPinned() = default;
    LioPinned(const LioPinned&) = delete;
    LioPinned& operator=(const LioPinned&) = delete;
    ~LioPinned() { if (p) (void)hipHostFree(p); }

    operator T*() const { return p; }

    // An empty buffer, or one of fewer than `need` elements, is replaced by one of `n` elements.
    hipError_t grow(size_t need, size_t n, unsigned flags = hipHostMallocDefault)
    {
        if (p && need <= cap) return hipSuccess;
        if (p) {
            const hipError_t e = hipHostFree(p);
            p = nullptr; cap = 0;
            if (e != hipSuccess) return e;
        }
        const hipError_t e = hipHostMalloc((void**)&p, n * sizeof(T), flags);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = n;
        return hipSuccess;
    }
};

hipError_t lio_pool_acquire(void** p, size_t bytes);   // on the current device
void lio_pool_release(void* p);
void lio_pool_trim(void);                               // frees every idle block
// A busy block leaves the pool: the caller owns it from now on (hipFree).  Returns its capacity in bytes; 0 for a pointer the
// pool does not hold.
size_t lio_pool_disown(void* p);
// A hipMalloc'd block of `cap` bytes on `device` that nothing reads or writes any more joins the pool, idle.
void lio_pool_adopt(void* p, size_t cap, int device);

struct LioTemp {            // RAII temporary from the pool
    void* p = nullptr;
    ~LioTemp() { if (p) lio_pool_release(p); }
    hipError_t alloc(size_t bytes) { return lio_pool_acquire(&p, bytes ? bytes : 16); }
    template <typename T> T* as() { return (T*)p; }
};
