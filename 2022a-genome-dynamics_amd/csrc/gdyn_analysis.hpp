// gdyn_analysis.hpp -- the host-side plumbing that the device analyses (gdyn_flow, gdyn_rdf, gdyn_lamina, gdyn_cmap,
// gdyn_hic, gdyn_msd, gdyn_dcorr, gdyn_dmap, gdyn_sq, gdyn_cluster, gdyn_dcov, gdyn_gyr) and the recorder (gdyn_live) share: error reporting, owned device and pinned host
// buffers, the device and stream of a handle with its create prologue and destroy epilogue, the grid size of a
// one-lane-per-element launch, the opt-in to more than 64 KiB of dynamic LDS and the stage timer of gd_dcov and gd_gyr.  The stepper's host files (gdyn_system.hpp)
// take the error reporting and the buffers from here too.  The trajectory history that gd_msd, gd_dcorr, gd_dmap, gd_sq, gd_cluster, gd_dcov and gd_gyr hold is
// gdyn_history.hpp's.  Nothing here is extern "C" or device code.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <initializer_list>
#include <new>

#include "../../include/gdyn.h"
#include "gdyn_once.hpp"

int gd_report_error(int code, const char *msg);      // gdyn_capi.hip: sets gd_last_error()

namespace gd {

static int fail(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return gd_report_error(code, buf);
}
#define HIPCHK(call)                                                                                    \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) return gd::fail(GD_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define GDCHK(call)              \
    do {                         \
        int rc_ = (call);        \
        if (rc_ != GD_OK) return rc_; \
    } while (0)

// blocks of `block` lanes for n elements; no caller comes near the cap, which keeps the count inside a grid dimension
inline unsigned blocks_for(size_t n, unsigned block) { return (unsigned)std::min<size_t>((n + block - 1) / block, 1u << 30); }

// The dynamic LDS a block of `kernels` may ask for on a device: all 160 KiB of a gfx950 CU where the opt-in is granted to every one
// of them (once per device, gdyn_once.hpp), else 128 KiB, else the 64 KiB that need none.
static inline int lds_opt_in(DeviceOnce<> &once, int device, std::initializer_list<const void *> kernels)
{
    int const bytes = once.run(device, [&](int) {
        for (int want : {160 * 1024, 128 * 1024}) {
            bool ok = true;
            for (const void *k : kernels) ok = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, want) == hipSuccess && ok;
            if (ok) return want;
            (void)hipGetLastError();
        }
        return 64 * 1024;
    });
    return bytes > 0 ? bytes : 64 * 1024;
}

// device memory of the current device, freed with its owner (the owner's device must be current then: gd::close)
template <typename T>
struct dbuf {
    T *p = nullptr;
    size_t n = 0;

    dbuf() = default;
    dbuf(dbuf &&o) noexcept : p(o.p), n(o.n)
    {
        o.p = nullptr;
        o.n = 0;
    }
    dbuf &operator=(dbuf &&o) noexcept
    {
        std::swap(p, o.p);
        std::swap(n, o.n);
        return *this;
    }
    ~dbuf()
    {
        if (p) (void)hipFree(p);
    }
    // room for `count` elements; grows by reallocation (the content is lost), never shrinks; n is 0 after a failure
    hipError_t ensure(size_t count)
    {
        if (count <= n) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    // exactly `count` elements: as it is when it has them, else freed and allocated anew (the content is lost).  zero: the new block
    // is cleared, and the device idle, when this returns
    hipError_t resize(size_t count, bool zero = true)
    {
        if (count == n) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        if (count == 0) return hipSuccess;
        hipError_t e = hipMalloc(&p, count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        n = count;
        if (zero) {
            e = hipMemset(p, 0, count * sizeof(T));
            if (e == hipSuccess) e = hipDeviceSynchronize();
        }
        return e;
    }
    hipError_t upload(const T *src, size_t count)
    {
        hipError_t e = ensure(count);
        if (e == hipSuccess && count) e = hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
    hipError_t zero(hipStream_t st) { return n ? hipMemsetAsync(p, 0, n * sizeof(T), st) : hipSuccess; }
};

// pinned host memory, freed with its owner.  Grow-only like dbuf::ensure; a block that grows geometrically is asked for
// gd::grown_capacity(n, need) elements (gdyn_replica_pairs.hpp)
template <typename T>
struct pinned {
    T *p = nullptr;
    size_t n = 0;

    pinned() = default;
    pinned(pinned &&o) noexcept : p(o.p), n(o.n)
    {
        o.p = nullptr;
        o.n = 0;
    }
    pinned &operator=(pinned &&o) noexcept
    {
        std::swap(p, o.p);
        std::swap(n, o.n);
        return *this;
    }
    ~pinned()
    {
        if (p) (void)hipHostFree(p);
    }
    // room for `count` elements; grows by reallocation (the content is lost), never shrinks; unchanged after a failure
    hipError_t ensure(size_t count)
    {
        if (count <= n) return hipSuccess;
        T *q = nullptr;
        hipError_t e = hipHostMalloc((void **)&q, count * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) return e;
        if (p) (void)hipHostFree(p);
        p = q;
        n = count;
        return hipSuccess;
    }
};

// what every gd_<x> handle starts with.  The stream goes after the derived handle's members, so after its buffers.
struct handle {
    int device = 0;
    hipStream_t stream = nullptr;

    handle() = default;
    handle(const handle &) = delete;
    handle &operator=(const handle &) = delete;
    ~handle()
    {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// The device times of a handle's last calls (gd_<x>_last_times): three events for the marks on its stream, three stages to report.
struct StageTimer {
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    double ms[3] = {0.0, 0.0, 0.0};

    ~StageTimer()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    hipError_t create()
    {
        for (hipEvent_t &e : ev)
            if (hipError_t const rc = hipEventCreate(&e)) return rc;
        return hipSuccess;
    }
    hipError_t mark(int i, hipStream_t st) { return hipEventRecord(ev[i], st); }
    // the milliseconds from mark `from` to mark `to`, both reached
    hipError_t between(int from, int to, double *out) const
    {
        float f = 0.0f;
        hipError_t const rc = hipEventElapsedTime(&f, ev[from], ev[to]);
        *out = f;
        return rc;
    }
    void report(double *a, double *b, double *c) const
    {
        if (a) *a = ms[0];
        if (b) *b = ms[1];
        if (c) *c = ms[2];
    }
};

// the front of gd_<x>_create (`who`): *out is a new H on desc->device, which is made current, with its stream
template <typename H, typename Desc>
int open(const char *who, const Desc *desc, H **out)
{
    if (!desc || !out) return fail(GD_EINVAL, "%s: NULL argument", who);
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return fail(GD_ENODEVICE, "%s: no HIP device", who);
    if (desc->device < 0 || desc->device >= count) return fail(GD_EINVAL, "%s: device %d of %d", who, desc->device, count);
    HIPCHK(hipSetDevice(desc->device));
    H *h = new (std::nothrow) H;
    if (!h) return fail(GD_ENOMEM, "%s: out of host memory", who);
    h->device = desc->device;
    hipError_t const e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete h;
        return fail(GD_EHIP, "%s: hipStreamCreate failed: %s", who, hipGetErrorString(e));
    }
    *out = h;
    return GD_OK;
}

// gd_<x>_destroy: waits for the handle's work and frees it on its device
template <typename H>
int close(H *h)
{
    if (!h) return GD_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    delete h;
    return GD_OK;
}

}  // namespace gd
