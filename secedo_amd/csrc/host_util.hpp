// host_util.hpp -- the host plumbing every stand-alone library's host file needs: the last-error string, the
// early-return macros, a clock, RAII device buffers, a stream guard and events. Internal: nothing here is exported (the
// namespace is hidden), and each library that includes it gets its own error string, since the libraries do not
// link one another's copy.
#pragma once

#include "secedo_simmat.h"  // the error codes

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <string>

namespace secedo {
namespace host __attribute__((visibility("hidden"))) {

// One per library and thread: what the library's *_last_error() returns.
inline thread_local std::string g_error;

inline int fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}

#define SECEDO_TRY(expr)                                                                            \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return ::secedo::host::fail(SECEDO_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define SECEDO_CALL(expr)                 \
    do {                                  \
        int rc_ = (expr);                 \
        if (rc_ != SECEDO_OK) return rc_; \
    } while (0)

// The decimal value of environment variable `name` where it is set to a number above 0, else `fallback`. Read at every
// call; the caller clamps.
inline uint64_t env_u64(const char *name, uint64_t fallback) {
    const char *e = std::getenv(name);
    const unsigned long long v = e && *e ? std::strtoull(e, nullptr, 10) : 0;
    return v > 0 ? v : fallback;
}

// the calling thread's device, checked against the devices there are
inline int set_device(int device_id) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(SECEDO_E_NO_DEVICE, "no HIP device");
    if (device_id < 0 || device_id >= n_dev) return fail(SECEDO_E_INVALID_ARG, "device id out of range");
    SECEDO_TRY(hipSetDevice(device_id));
    return SECEDO_OK;
}

using Clock = std::chrono::steady_clock;

inline double ms_since(Clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

// ms_since that also restarts the clock: consecutive stages timed off one variable
inline double ms_lap(Clock::time_point &t0) {
    const Clock::time_point t1 = Clock::now();
    const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
    return ms;
}

// Device array of T. grow() multiplies the capacity by kGrowPercent / 100, to at least kMinGrow elements: the factor
// decides how many device-to-device copies a buffer that grows with a kept prefix costs.
template <class T, size_t kGrowPercent = 200, size_t kMinGrow = 0>
struct Dev {
    T *p = nullptr;
    size_t n = 0;
    Dev() = default;
    Dev(const Dev &) = delete;
    Dev &operator=(const Dev &) = delete;
    ~Dev() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t alloc(size_t count) {
        reset();
        const hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) n = count;
        else p = nullptr;
        return e;
    }
    // at least `count` elements, the first `keep` preserved (stream-ordered copy); on failure the buffer is as before
    hipError_t grow(size_t count, size_t keep, hipStream_t s) {
        if (count <= n && p) return hipSuccess;
        const size_t cap = std::max<size_t>(std::max<size_t>(count, n * kGrowPercent / 100), kMinGrow);
        T *q = nullptr;
        hipError_t e = hipMalloc(&q, std::max<size_t>(cap, 1) * sizeof(T));
        if (e != hipSuccess) return e;
        if (keep && p) {
            e = hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) {
                (void)hipFree(q);
                return e;
            }
        }
        reset();
        p = q;
        n = cap;
        return hipSuccess;
    }
    template <class U>
    U *as() const {
        return reinterpret_cast<U *>(p);
    }
};

// Device bytes whose element type the caller picks at each use: alloc(bytes), as<T>()
using Buf = Dev<unsigned char>;

struct StreamGuard {
    hipStream_t s = nullptr;
    ~StreamGuard() {
        if (s) (void)hipStreamDestroy(s);
    }
};

template <size_t N = 2>
struct Events {  // made by create(): a pair around a kernel whose time is reported, or more for hand-overs
    hipEvent_t e[N] = {};
    ~Events() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    int create() {
        for (hipEvent_t &x : e)
            if (!x) SECEDO_TRY(hipEventCreate(&x));
        return SECEDO_OK;
    }
};

}  // namespace host
}  // namespace secedo
