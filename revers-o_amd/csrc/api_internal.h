// Plumbing every translation unit of the C ABI needs (not part of the C ABI): status guards, device guard, profiler scope.
// (What the two towers share is tower.h.)
#pragma once
#include <cstdlib>
#include <string>

#include "../../include/revo.h"
#include "common.h"

#define API_BEGIN try {
#define API_END                                            \
    }                                                      \
    catch (const std::exception& e) {                      \
        revo_set_error(std::string("exception: ") + e.what()); \
        return -3;                                         \
    }                                                      \
    catch (...) {                                          \
        revo_set_error("unknown exception");               \
        return -3;                                         \
    }
#define CHECK_RC(expr)            \
    do {                          \
        int _rc = (expr);         \
        if (_rc) return _rc;      \
    } while (0)

// A handle is bound to the device it was created on: every entry point that takes one makes that
// device current for the duration of the call (allocations, kernel attributes and launches all go
// to the current device) and puts the caller's device back afterwards.
struct DeviceGuard {
    int prev = -1; bool switched = false; hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) { err = hipSetDevice(device); switched = err == hipSuccess; }
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
#define REVO_ON_DEVICE(dev)                 \
    DeviceGuard dg_(dev);                   \
    REVO_HIP_CHECK(dg_.err)

// times what is enqueued on `s` during its lifetime as kernel class `cls` (revo_prof_enable; the state lives in api.hip)
struct ProfRec { std::string cls; hipEvent_t a, b; };
struct ProfScope {
    bool active; hipStream_t st; ProfRec rec;
    ProfScope(const char* cls, hipStream_t s);
    ~ProfScope();
};
