// Shared host-side helpers for the cookietts HIP library (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdint>

#include "../../include/cookietts_hip.h"

namespace ctts {

void set_error(const char* fmt, ...);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

#define CTTS_CHECK_ARG(cond, ...)            \
    do {                                     \
        if (!(cond)) {                       \
            ::ctts::set_error(__VA_ARGS__);  \
            return CTTS_E_ARG;               \
        }                                    \
    } while (0)

#define CTTS_CHECK_LAUNCH(what)                                                          \
    do {                                                                                 \
        hipError_t e__ = hipGetLastError();                                              \
        if (e__ != hipSuccess) {                                                         \
            ::ctts::set_error("%s: %s", what, hipGetErrorString(e__));                   \
            return CTTS_E_LAUNCH;                                                        \
        }                                                                                \
    } while (0)

#define CTTS_CHECK_HIP(expr)                                                             \
    do {                                                                                 \
        hipError_t e__ = (expr);                                                         \
        if (e__ != hipSuccess) {                                                         \
            ::ctts::set_error("%s: %s", #expr, hipGetErrorString(e__));                  \
            return CTTS_E_LAUNCH;                                                        \
        }                                                                                \
    } while (0)

// More than 64 KiB of dynamic LDS has to be allowed per kernel, and the attribute belongs to the CURRENT device's copy of the
// kernel: raised once per (kernel, device of the calling thread), `done` holding one bit per device.  No lock: two threads that
// meet a clear bit both set the same value; the bit is published only after a success, so a failure is returned to the caller
// that meets it and the next caller tries again.  Already set, a call costs hipGetDevice (a thread-local read) and one atomic
// load.
template <class K, K kernel>
int allow_dynamic_lds(int bytes) {
    static std::atomic<uint64_t> done{0};                                     // one per kernel instantiation
    if (bytes <= 64 * 1024) return CTTS_OK;
    int dev = 0;
    CTTS_CHECK_HIP(hipGetDevice(&dev));
    const uint64_t bit = dev < 64 ? uint64_t(1) << dev : 0;                  // (a device past 63 is never remembered)
    if (done.load(std::memory_order_acquire) & bit) return CTTS_OK;
    CTTS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.fetch_or(bit, std::memory_order_release);
    return CTTS_OK;
}
#define CTTS_ALLOW_LDS(kernel, bytes) ::ctts::allow_dynamic_lds<decltype(&kernel), &kernel>(bytes)

}  // namespace ctts
