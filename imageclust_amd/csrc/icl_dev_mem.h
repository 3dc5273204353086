// icl_dev_mem.h -- who owns device memory on the host side ("Device memory on the host side").  Included by icl_common.h, behind
// icl_fail, ICL_HIP and ICL_TRY.
//   dev_guard + icl_dev_alloc   a buffer that lives for one call
//   icl_dev_grow                a buffer a context keeps between calls and grows on demand
//   icl_ws_layout               where the pieces of one such buffer lie (icl_ws_layout.h)
//   icl_ws_upload               host int32 arrays into the front of one such buffer, in one copy
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "icl_ws_layout.h"

// hip_guard releases a HIP resource on every way out of a scope (ICL_HIP / ICL_TRY / icl_fail return early).  One owner: no copies.
// Declare a call's guards behind its lock_guard and icl_device_guard, so that they are released first, on the context's device.
template <class T, hipError_t (*Release)(T)> struct hip_guard {
    T p = nullptr;
    hip_guard() = default;
    hip_guard(const hip_guard &) = delete;
    hip_guard &operator=(const hip_guard &) = delete;
    ~hip_guard() { if (p) (void)Release(p); }
    template <class U> U *as() const { return (U *)p; }
};
using ev_guard = hip_guard<hipEvent_t, hipEventDestroy>;
using dev_guard = hip_guard<void *, hipFree>;
using pin_guard = hip_guard<void *, hipHostFree>;

// hipMalloc into an empty guard.  Memory that does not fit is ICL_ERR_NOMEM, "<what>: <bytes> bytes of device memory do not fit" (what is a
// printf format: the entry point and the buffer); the sticky error is cleared, so that the next launch check does not report it again.
__attribute__((format(printf, 4, 5))) static inline int icl_dev_alloc(icl_ctx *ctx, dev_guard &g, size_t bytes, const char *what, ...)
{
    if (hipMalloc(&g.p, bytes) == hipSuccess) return ICL_OK;
    (void)hipGetLastError();
    g.p = nullptr;
    char name[192];
    va_list ap;
    va_start(ap, what);
    vsnprintf(name, sizeof name, what, ap);
    va_end(ap);
    return icl_fail(ctx, ICL_ERR_NOMEM, "%s: %zu bytes of device memory do not fit", name, bytes);
}

// icl_dev_alloc, then the upload of `bytes` bytes from host memory enqueued on the context's stream (what: a plain string here).
static inline int icl_dev_upload(icl_ctx *ctx, dev_guard &g, const void *host, size_t bytes, const char *what)
{
    ICL_TRY(icl_dev_alloc(ctx, g, bytes, "%s", what));
    ICL_HIP(ctx, hipMemcpyAsync(g.p, host, bytes, hipMemcpyHostToDevice, icl_main_stream(ctx)));
    return ICL_OK;
}

// A device buffer that outlives the call and only ever grows.  Its owner releases it by name (icl_destroy and the subsystems' teardown
// hooks, with the device selected and the streams alive): there is no destructor to do it at some other time.
struct icl_dev_grow {
    void *p = nullptr;
    size_t bytes = 0;
    template <class T> T *as() const { return (T *)p; }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // At least `need` bytes.  A buffer that is too small is replaced by one of max(need, floor) bytes, contents lost, once the context's
    // stream is idle (an earlier call's kernels may still read it); a failed growth leaves {nullptr, 0}.
    int ensure(icl_ctx *ctx, size_t need, const char *what, size_t floor = 0)
    {
        if (bytes >= need) return ICL_OK;
        if (p) ICL_HIP(ctx, hipStreamSynchronize(icl_main_stream(ctx)));
        release();
        const size_t b = need > floor ? need : floor;
        dev_guard g;
        ICL_TRY(icl_dev_alloc(ctx, g, b, "%s", what));
        p = g.p;
        g.p = nullptr;
        bytes = b;
        return ICL_OK;
    }
};

// Host int32 arrays into one workspace: add() places each (L goes on to place whatever else the workspace holds), go() sends them up
// in one transfer that has finished at return (the caller's arrays and the staging vector may go away then), ordered in front of the
// launches on the context's stream.
struct icl_ws_upload {
    icl_ws_layout L{16};
    struct part {
        size_t at, bytes;
        const int32_t *host;
    };
    std::vector<part> parts;
    size_t add(const int32_t *host, int64_t count) // -> the array's offset (a null array takes no room)
    {
        const size_t at = L.take(host ? (size_t)count * 4 : 0);
        if (host && count) parts.push_back({at, (size_t)count * 4, host});
        return at;
    }
    int go(icl_ctx *ctx, char *ws, size_t bytes) // bytes: L.total as it was behind the last add
    {
        if (!bytes) return ICL_OK;
        std::vector<char> meta(bytes, 0);
        for (const part &pt : parts) std::memcpy(meta.data() + pt.at, pt.host, pt.bytes);
        ICL_HIP(ctx, hipMemcpyAsync(ws, meta.data(), bytes, hipMemcpyHostToDevice, icl_main_stream(ctx)));
        ICL_HIP(ctx, hipStreamSynchronize(icl_main_stream(ctx)));
        return ICL_OK;
    }
};
