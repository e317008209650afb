// capi_common.hpp — what the two files of the extern "C" boundary (capi.cpp: the reprojection handle and the one-shot solvers;
// capi_pipelines.cpp: the batched pipelines) share: the translation of exceptions into status codes, the device checks and the
// check of an offset table.
#pragma once
#include <atomic>

#include "../../include/calibba.h"
#include "hip_glue.hpp"

// cba_last_error's message: one object per thread for the whole library, defined in capi.cpp
extern __attribute__((visibility("hidden"))) thread_local std::string g_err;

template <typename F>
static cba_status guarded(F&& f) {
    try {
        f();
        return CBA_OK;
    } catch (const std::invalid_argument& e) {
        g_err = e.what();
        return CBA_ERR_INVALID_ARGUMENT;
    } catch (const cba::NoDevice& e) {
        g_err = e.what();
        return CBA_ERR_NO_DEVICE;
    } catch (const cba::HipError& e) {
        g_err = e.what();
        return CBA_ERR_HIP;
    } catch (const std::runtime_error& e) {
        g_err = e.what();
        return CBA_ERR_RUNTIME;
    } catch (const std::exception& e) {
        g_err = e.what();
        return CBA_ERR_INTERNAL;
    }
}

// the device of the entry points that take no handle and no device argument (one process per GPU: cba_set_device(LOCAL_RANK))
extern __attribute__((visibility("hidden"))) std::atomic<int> g_default_device;  // capi.cpp (cba_set_device)
static int default_device() { return g_default_device.load(); }

// The offset table [n + 1] of a call's groups of observations.  The entry points differ in two policies, kept as they shipped:
// whether the table must start at 0, and whether a group is limited to INT32_MAX observations (the kernels that count a group in
// an int need it).  what: "view " / "block " / "" for the message.
enum : unsigned { OFF_ANY_START = 0, OFF_FROM_ZERO = 1, OFF_INT32_GROUPS = 2 };
static bool bad_offset_step(const int64_t* off, int i, unsigned policy) {
    return off[i + 1] < off[i] || ((policy & OFF_INT32_GROUPS) && off[i + 1] - off[i] > 0x7fffffff);
}
static void check_offsets(const int64_t* off, int n, const char* what, unsigned policy) {
    if ((policy & OFF_FROM_ZERO) && off[0] != 0) throw std::invalid_argument(std::string(what) + "offsets must start at 0");
    for (int i = 0; i < n; ++i)
        if (bad_offset_step(off, i, policy))
            throw std::invalid_argument(*what ? std::string("bad ") + what + "offsets" : "offsets must not decrease");
}

static int device_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// every entry point that needs a device, after its argument checks: the number of visible devices, or CBA_ERR_NO_DEVICE
static int require_device() {
    const int n = device_count();
    if (n <= 0) throw cba::NoDevice("no HIP device visible: libcalibba has no CPU fallback");
    return n;
}
// ... and those that take a device index
static void require_device(int device) {
    if (device < 0 || device >= require_device()) throw std::invalid_argument("device index out of range");
}
