// rfcal_plan.hpp -- the host arithmetic of the receiver calibration (rfcal.hip: mcrx_hip_rfcal_*) that needs no
// device: the configuration check, how a call is split at the block boundaries of the absolute index, the launch grid, the forgetting
// rule mu_j (which the update lane on the device calls too) and the 2^31 guard of the integer moments.  selftest, create and execute
// all call it; host/rfcal_plan_test.cc compiles it with a main of its own.
#pragma once
#include <cmath>
#include <stdint.h>
#include "../../include/mcrx_hip.h"

#if defined(__HIPCC__)
#define RFCAL_HD __host__ __device__
#else
#define RFCAL_HD
#endif

namespace mcrx {

enum { RFCAL_WG = 256,              // lanes of a workgroup; a lane owns index-aligned sample pairs
       RFCAL_MAX_ROWS = 2048 };     // the most workgroups of a measuring launch = partial rows the handle owns (8 per CU)

// the whole configuration, as create sees it: nullptr or what is wrong
static inline const char *rfcal_check(const mcrx_hip_rfcal_config *c)
{
    if (c->struct_size != sizeof(mcrx_hip_rfcal_config)) return "mcrx_hip_rfcal_config: wrong struct_size";
    if (c->stages & ~(MCRX_RFCAL_DC | MCRX_RFCAL_IQ)) return "unknown stage bits";
    if (c->input_format > 1u) return "input format must be 0 (cf32) or 1 (sc16)";
    if (c->output_format > 1u) return "output format must be 0 (cf32) or 1 (sc16)";
    if (c->period_log2 != 0u && (c->period_log2 < 6u || c->period_log2 > 30u)) return "period_log2 must be 0 (manual updates) or 6 .. 30";
    if (c->forget_log2 > 30u) return "forget_log2 must be 0 .. 30";
    if (!std::isfinite(c->gain)) return "gain must be finite";
    return nullptr;
}

// the weight of the block means in update j (j earlier updates): the cumulative mean until it meets the exponential floor
RFCAL_HD static inline double rfcal_mu(uint64_t j, uint32_t forget_log2)
{
    const double cumulative = 1.0 / ((double)j + 1.0), floor_ = 1.0 / (double)((uint64_t)1 << forget_log2);
    return cumulative > floor_ ? cumulative : floor_;
}

// The segment that begins at absolute index pos with `left` >= 1 samples of the call to go: its length, and whether it ends a block
// (period_log2 = k != 0: block j is [j 2^k, (j + 1) 2^k) of the index, which wraps with the 64-bit position; k = 0: one segment).
static inline uint64_t rfcal_segment(uint64_t pos, uint64_t left, uint32_t period_log2, bool *ends_block)
{
    if (period_log2 == 0u) { *ends_block = false; return left; }
    const uint64_t B = (uint64_t)1 << period_log2, to_boundary = B - (pos & (B - 1));
    *ends_block = left >= to_boundary;
    return *ends_block ? to_boundary : left;
}
// segments of the call (pos, n)
static inline uint64_t rfcal_segments(uint64_t pos, uint64_t n, uint32_t period_log2)
{
    if (n == 0) return 0;
    if (period_log2 == 0u) return 1;
    const uint64_t B = (uint64_t)1 << period_log2, first = B - (pos & (B - 1));
    return n <= first ? 1 : 1 + ((n - first) + B - 1) / B;
}

// lane pairs of a launch over (pos, n), n >= 1: the index-aligned pairs (2k, 2k + 1) its samples touch
static inline uint64_t rfcal_pairs(uint64_t pos, uint64_t n) { return ((pos & 1u) + n + 1) >> 1; }
// The workgroups of a launch: a function of (pos, n) and of whether the launch measures, nothing else.  A measuring launch writes
// one partial row per workgroup, so its grid is capped and a lane loops over pairs grid * 256 apart; the others take a lane a pair.
static inline uint32_t rfcal_grid(uint64_t pos, uint64_t n, bool measure)
{
    const uint64_t wgs = (rfcal_pairs(pos, n) + RFCAL_WG - 1) / RFCAL_WG;
    return (uint32_t)(measure && wgs > RFCAL_MAX_ROWS ? (uint64_t)RFCAL_MAX_ROWS : wgs);
}

// sc16 input: a sample adds at most 2^31 to an int64 moment, so at most 2^31 samples may be measured between two updates.
// `since` = samples measured since the last update, `first_segment` = what this call measures before its first update (or in all).
static inline bool rfcal_guard_ok(uint64_t since, uint64_t first_segment)
{
    const uint64_t most = (uint64_t)1 << 31;
    return since <= most && first_segment <= most - since;
}

}  // namespace mcrx
