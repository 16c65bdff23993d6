// ophost.hpp -- host scaffolding the stream operators share (chanemu, userchan, rfchain, rfcal, cfr): the HIP-call check, the body of
// mcrx_hip_*_clipped and a device buffer that grows on demand.  Every operator keeps its own thread-local error string and its own
// mcrx_hip_*_last_error (the ABI); it passes the string in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/mcrx_hip.h"
#include "devscope.hpp"

// a HIP call inside an entry point: on failure its text goes to the operator's error string and the entry point returns MCRX_EHIP
#define MCRX_OP_CHK(err, x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { (err) = std::string(#x) + ": " + hipGetErrorString(e_); return MCRX_EHIP; } } while (0)

namespace mcrx {

// mcrx_hip_*_clipped of a handle with a device and a Sc16ClipCount clip
template <typename Handle> static int op_clipped(Handle *q, std::string &err, uint64_t *samples, int reset)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { err = "null handle"; return MCRX_EINVAL; }
    uint64_t n = 0;
    MCRX_OP_CHK(err, q->clip.read(&n, reset != 0));
    if (samples) *samples = n;
    return MCRX_OK;
}

// Device memory that is grown on demand and never shrunk.  ensure() below the size held does nothing; above it the buffer is freed
// (hipFree waits for the calls in flight) and allocated anew, its contents are not kept.  Steady state: never.
struct DevBuffer {
    void *ptr = nullptr; size_t bytes = 0;

    template <typename T> T *as() const { return static_cast<T *>(ptr); }
    hipError_t ensure(size_t want)
    {
        if (want <= bytes) return hipSuccess;
        hipError_t e = ptr ? hipFree(ptr) : hipSuccess;
        if (e != hipSuccess) return e;
        ptr = nullptr; bytes = 0;
        if ((e = hipMalloc(&ptr, want)) == hipSuccess) bytes = want; else ptr = nullptr;
        return e;
    }
    void release()
    {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr; bytes = 0;
    }
};

}  // namespace mcrx
