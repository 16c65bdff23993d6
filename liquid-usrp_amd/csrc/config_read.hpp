// config_read.hpp -- the caller's configuration structs read once, into the effective values the handle works with.  Both structs
// grow by appending 32-bit fields and say how much of them the caller knows in struct_size: a field that lies (even partly) behind
// the caller's struct_size reads as 0 = its default, whatever the memory there holds.  No HIP: host/acq_plan_test.cc checks it.
#pragma once
#include "../../include/mcrx_hip.h"
#include <cstring>

namespace mcrx {

// zeroed defaults, then the caller's first struct_size bytes, rounded down to whole fields (legacy_bytes stand in for struct_size == 0)
template <class C> static inline C read_config(const C *cfg, size_t legacy_bytes)
{
    static_assert(sizeof(C) % sizeof(uint32_t) == 0, "configuration structs are arrays of 32-bit fields");
    C e{};
    if (!cfg) return e;
    size_t n = cfg->struct_size ? cfg->struct_size : legacy_bytes;
    if (n > sizeof(C)) n = sizeof(C);
    memcpy(&e, cfg, n & ~(sizeof(uint32_t) - 1));
    return e;
}

// A caller that leaves struct_size at 0 predates the field's use: it gets the fields up to and including batch_samples, as ever.
// NULL: the defaults, with soft-decision decoding.
static inline mcrx_hip_config effective_config(const mcrx_hip_config *cfg)
{
    mcrx_hip_config e = read_config(cfg, offsetof(mcrx_hip_config, single_channel));
    if (!cfg) e.payload_soft = 1;
    return e;
}
static inline mcrx_hip_monitor_config effective_monitor_config(const mcrx_hip_monitor_config *cfg) { return read_config(cfg, 0); }

}  // namespace mcrx
