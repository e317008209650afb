// hip_glue.hpp — the device-memory, stream and timing helpers every .hip file needs, and the host glue shared by the batched
// pipelines behind the C ABI.  Nothing here knows the bundle-adjustment core (engine.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include "exp_env.hpp"

#include <algorithm>
#include <cstdint>
#include <exception>
#include <stdexcept>
#include <string>

namespace cba {

struct HipError : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct NoDevice : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// Environment switches.  The shipped library reads a short, documented list of run-time switches with std::getenv (DESIGN.md
// section 9: every one of them selects between forms that give the same results).  Everything else that was ever tuned or ablated
// through the environment - part counts, layouts, timing-only ablations whose results are WRONG - is an experiment knob: read
// through cba_exp_env(), which answers only in a library built with -DCBA_EXPERIMENTS (make EXPERIMENTS=1; tools/exp.py uses such
// a build).  In the shipped library a stray variable in a user's environment cannot change what a calibration computes.

#define CBA_HIP(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            throw cba::HipError(std::string(#expr) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" +    \
                                std::to_string(__LINE__) + ")");                                           \
    } while (0)

// Process-wide cache of device / page-locked blocks and of streams (block_cache.cpp).  The reference's pipeline calls the
// one-shot entry points stage after stage; a handle is ~70 hipMalloc + ~10 hipHostMalloc, and giving them back cost 1.9 ms
// of a 5 ms C1-sized call (hipFree synchronises the device).  Released blocks up to 16 MiB are kept (at most 256 MiB per
// kind and device) in power-of-two size classes and handed to the next handle; cba_trim_cache() frees them.
void* cache_alloc(bool pinned, size_t bytes, size_t* granted);  // current device; throws HipError
void cache_release(bool pinned, int device, void* p, size_t granted) noexcept;
hipStream_t cache_stream();                                     // an idle non-blocking stream of the current device
void cache_stream_release(int device, hipStream_t s) noexcept;  // the caller has synchronised it
void cache_trim();

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    size_t granted = 0;  // bytes of the underlying block
    int device = 0;
    bool owned = true;   // false: a view into another buffer (view())
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    // A cached block may be handed to another handle at once: nothing may still be running on it.  Normal paths have
    // synchronised their stream before buffers go out of scope; unwinding from an exception and replacing a live buffer
    // have not, so those wait for the device.
    void release() {
        if (p && owned) {
            if (std::uncaught_exceptions() > 0) (void)hipDeviceSynchronize();
            cache_release(false, device, p, granted);
        }
        p = nullptr; n = 0; granted = 0; owned = true;
    }
    // non-owning window of `count` elements at `ptr` (inside a buffer that outlives this one)
    void view(T* ptr, size_t count) {
        release();
        p = ptr; n = count; owned = false;
    }
    void alloc(size_t count) {
        if (p && owned) (void)hipDeviceSynchronize();
        release();
        if (count == 0) count = 1;
        CBA_HIP(hipGetDevice(&device));
        p = static_cast<T*>(cache_alloc(false, count * sizeof(T), &granted));
        n = count;
    }
    // grow to at least `count` elements; the contents are not kept
    void ensure(size_t count) {
        if (n < count) alloc(count);
    }
    void upload(const T* src, size_t count, hipStream_t s, size_t first = 0) {
        if (count) CBA_HIP(hipMemcpyAsync(p + first, src, count * sizeof(T), hipMemcpyHostToDevice, s));
    }
    void download(T* dst, size_t count, hipStream_t s, size_t first = 0) const {
        if (count) CBA_HIP(hipMemcpyAsync(dst, p + first, count * sizeof(T), hipMemcpyDeviceToHost, s));
    }
    void zero(hipStream_t s) { CBA_HIP(hipMemsetAsync(p, 0, n * sizeof(T), s)); }
    // a host table on the device: alloc + upload
    void assign(const T* src, size_t count, hipStream_t s) {
        alloc(count);
        upload(src, count, s);
    }
};

// Page-locked host staging for the small device-to-host results of an LM step: a copy into pageable memory blocks the
// host once per call, a copy into pinned memory is queued on the stream and only the single hipStreamSynchronize waits.
template <typename T>
struct PinnedBuf {
    T* p = nullptr;
    size_t n = 0;
    size_t granted = 0;
    int device = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (p) cache_release(true, device, p, granted); }
    void reserve(size_t count) {
        if (count <= n) return;
        if (p) cache_release(true, device, p, granted);
        p = nullptr; n = 0; granted = 0;
        CBA_HIP(hipGetDevice(&device));
        p = static_cast<T*>(cache_alloc(true, count * sizeof(T), &granted));
        n = count;
    }
};

// An idle non-blocking stream of the current device, or of `dev`, which it makes current first, leased from the process-wide pool;
// synchronised and returned on scope exit.  Declare it BEFORE the buffers that are used on it (members are released in reverse order).
struct StreamLease {
    hipStream_t s = nullptr;
    int device = 0;
    StreamLease() {
        CBA_HIP(hipGetDevice(&device));
        s = cache_stream();
    }
    __attribute__((visibility("hidden"))) explicit StreamLease(int dev) : device(dev) {  // hidden: adds no dynamic symbol
        CBA_HIP(hipSetDevice(dev));
        s = cache_stream();
    }
    StreamLease(const StreamLease&) = delete;
    StreamLease& operator=(const StreamLease&) = delete;
    ~StreamLease() {
        if (s) {
            (void)hipStreamSynchronize(s);
            cache_stream_release(device, s);
        }
    }
    operator hipStream_t() const { return s; }
};

// ---- host glue shared by the batched pipelines behind the C ABI ------------------------------------------
// Workgroups of a grid-stride launch: one per `per_block` items, at least 1 and at most `cap`.
__attribute__((visibility("hidden"))) inline int launch_grid(int64_t items, int per_block, int cap) {
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(cap, (items + per_block - 1) / per_block)));
}

// The frame of a device handle (map, scanner, matcher, detector): its device and its stream, held from create to destroy.  The
// handles derive from it: a base is constructed before and destroyed after the derived members, which keeps the rule "the lease is
// declared before the buffers used on it".  Every call starts with begin().
struct __attribute__((visibility("hidden"))) DeviceHandle {
    int device;
    StreamLease lease;
    explicit DeviceHandle(int dev) : device(dev), lease(dev) {}
    hipStream_t begin() {
        CBA_HIP(hipSetDevice(device));
        return lease;
    }
};
template <class H>
__attribute__((visibility("hidden"))) void destroy_handle(H* h) noexcept {
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

// Stage timing of the experiment builds' _timed entry points: up to N device events on the call's stream.  The shipped library
// passes stage_ms == nullptr everywhere, so `on` is false there: no event exists, mark() does nothing and ms() is 0.  The events
// are created up front, outside the timed region.  (Hidden, like ObsSoA: internal helpers add nothing to the dynamic symbols.)
template <int N>
struct __attribute__((visibility("hidden"))) StageTimer {
    hipStream_t stream;
    hipEvent_t ev[N] = {};
    bool marked[N] = {};
    StageTimer(hipStream_t s, bool on) : stream(s) {
        if (on)
            for (hipEvent_t& e : ev) CBA_HIP(hipEventCreate(&e));
    }
    StageTimer(const StageTimer&) = delete;
    StageTimer& operator=(const StageTimer&) = delete;
    ~StageTimer() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void mark(int k) {
        if (!ev[k]) return;
        CBA_HIP(hipEventRecord(ev[k], stream));
        marked[k] = true;
    }
    // milliseconds from mark a to mark b (after the stream was synchronised); 0 when either was never recorded
    double ms(int a, int b) const {
        if (!marked[a] || !marked[b]) return 0.0;
        float t = 0.0f;
        CBA_HIP(hipEventElapsedTime(&t, ev[a], ev[b]));
        return t;
    }
    // stage_ms [N - 1], optional: the durations between consecutive marks
    void report(double* stage_ms) const {
        if (!stage_ms) return;
        for (int k = 0; k + 1 < N; ++k) stage_ms[k] = ms(k, k + 1);
    }
};

// The observations of a call on the device: the four arrays of the off_h[n_groups] observations and the offset table
// [n_groups + 1] of their groups (views, blocks, problems), queued on the call's stream.  Declare it after the stream lease.
struct __attribute__((visibility("hidden"))) ObsSoA {
    DevBuf<double> X, Y, u, v;
    DevBuf<int64_t> off;
    void upload(hipStream_t s, int n_groups, const int64_t* off_h, const double* X_h, const double* Y_h, const double* u_h,
                const double* v_h) {
        const size_t n = static_cast<size_t>(off_h[n_groups]);
        X.assign(X_h, n, s); Y.assign(Y_h, n, s); u.assign(u_h, n, s); v.assign(v_h, n, s);
        off.assign(off_h, static_cast<size_t>(n_groups) + 1, s);
    }
};

}  // namespace cba
