// gsr_host.h -- what the C ABI's translation units (gsr_api.hip, gsr_api_aux.hip) share on the host:
// the thread-local error string and the profiling scopes.  Defined once, in gsr_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>

#include "../../include/gsr.h"

namespace gsr {

// stores the formatted text as the calling thread's gsr_last_error() and returns `code`
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess) return fail(GSR_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

// per-phase event profiling: an event pair around the scope's launches on `s` (on = false: never)
struct Phase {
    hipStream_t s; const char *name; hipEvent_t a = nullptr, b = nullptr;
    Phase(hipStream_t s_, const char *n, bool on = true);
    ~Phase();
};
// host-side timers (profiling mode only)
using hclock = std::chrono::steady_clock;
struct HostPhase {
    const char *name; hclock::time_point t0; bool on;
    explicit HostPhase(const char *n);
    ~HostPhase();
};

}  // namespace gsr
