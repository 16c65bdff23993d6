// pamem_plan.hpp -- the host side of the amplifier with memory (pamem.hip: mcrx_hip_pamem_*) that needs no
// device: the configuration check, and what a launch uses of a checked configuration -- lead, the flattened tap list, r_b, the AM/PM in
// turns, the LDS bytes, the rounds of a workgroup and the grid for n outputs.  Plain host code: selftest, create and execute all call
// it; host/pamem_plan_test.cc compiles it with a main of its own.
#pragma once
#include <cmath>
#include <stdint.h>
#include "../../include/mcrx_hip.h"
#include "pd_plan.hpp"
#include "rapp_plan.hpp"

namespace mcrx {

enum { PAMEM_WG = PD_WG,                                    // lanes of a workgroup; a lane owns index-aligned pairs of outputs
       PAMEM_ROUND = 2 * PD_WG,                             // outputs of a round
       PAMEM_MAX_BRANCHES = MCRX_PAMEM_MAX_BRANCHES, PAMEM_MAX_TAPS = MCRX_PAMEM_MAX_TAPS, PAMEM_MAX_DELAY = MCRX_PAMEM_MAX_DELAY,
       PAMEM_MAX_FLAT = MCRX_PAMEM_MAX_BRANCHES * MCRX_PAMEM_MAX_TAPS };

// the whole configuration, as create sees it: nullptr or what is wrong.  Branches at index >= branches are not looked at.
static inline const char *pamem_check(const mcrx_hip_pamem_config *c)
{
    if (c->struct_size != sizeof(mcrx_hip_pamem_config)) return "mcrx_hip_pamem_config: wrong struct_size";
    if (c->branches < 1u || c->branches > (uint32_t)PAMEM_MAX_BRANCHES) return "branches must be 1 .. 4";
    if (c->input_format > 1u) return "input format must be 0 (cf32) or 1 (sc16)";
    if (c->output_format > 1u) return "output format must be 0 (cf32) or 1 (sc16)";
    if (!std::isfinite(c->gain)) return "gain must be finite";
    for (uint32_t b = 0; b < c->branches; b++) {
        const mcrx_hip_pamem_branch &br = c->branch[b];
        if (const char *bad = rapp_check(br.sat, br.smooth, br.amp_gain, br.ampm)) return bad;
        if (br.taps < 1u || br.taps > (uint32_t)PAMEM_MAX_TAPS) return "taps must be 1 .. 8";
        for (uint32_t k = 0; k < br.taps; k++) {
            if (br.delay[k] > (uint32_t)PAMEM_MAX_DELAY) return "a delay must be at most 16";
            if (k && br.delay[k] <= br.delay[k - 1]) return "the delays of a branch must increase strictly";
            if (!std::isfinite(br.h_re[k]) || !std::isfinite(br.h_im[k])) return "the weights must be finite";
        }
    }
    return nullptr;
}

// What a launch uses of a (checked) configuration.  The taps lie flat in the order the sum runs: branch ascending, then tap ascending;
// branch b's are first[b] .. first[b] + taps[b] - 1.  r[b] = fp32(1 / A_b^2) (rapp_plan.hpp); ampm[b] in turns, as the field holds it.
struct PamemConsts {
    uint32_t B, lead, total, first[PAMEM_MAX_BRANCHES], taps[PAMEM_MAX_BRANCHES], smooth[PAMEM_MAX_BRANCHES];
    float r[PAMEM_MAX_BRANCHES], amp_gain[PAMEM_MAX_BRANCHES], ampm[PAMEM_MAX_BRANCHES], gain;
    uint32_t tap_branch[PAMEM_MAX_FLAT], tap_delay[PAMEM_MAX_FLAT];
    float tap_re[PAMEM_MAX_FLAT], tap_im[PAMEM_MAX_FLAT];
};

static inline PamemConsts pamem_consts(const mcrx_hip_pamem_config *c)
{
    PamemConsts k = {};
    k.B = c->branches; k.gain = c->gain;
    for (uint32_t b = 0; b < k.B; b++) {
        const mcrx_hip_pamem_branch &br = c->branch[b];
        k.first[b] = k.total; k.taps[b] = br.taps; k.smooth[b] = br.smooth;
        k.r[b] = rapp_inv_sat2(br.sat); k.amp_gain[b] = br.amp_gain; k.ampm[b] = br.ampm;
        for (uint32_t t = 0; t < br.taps; t++, k.total++) {
            k.tap_branch[k.total] = b; k.tap_delay[k.total] = br.delay[t]; k.tap_re[k.total] = br.h_re[t]; k.tap_im[k.total] = br.h_im[t];
            if (br.delay[t] > k.lead) k.lead = br.delay[t];
        }
    }
    return k;
}

// samples of one branch's plane in LDS: the round's 512 + lead staged samples, made even so that every plane begins on 16 bytes
static inline uint32_t pamem_plane(uint32_t lead) { return ((uint32_t)PAMEM_ROUND + lead + 1u) & ~1u; }
// LDS of a launch: B planes of float2; at most 528 * 4 * 8 = 16896 bytes
static inline uint32_t pamem_lds(uint32_t B, uint32_t lead) { return B * pamem_plane(lead) * 8u; }
// rounds of 256 pairs a workgroup takes: pd_plan.hpp's for a streaming launch with no table to amortise
static inline uint32_t pamem_rounds() { return (uint32_t)PD_UNROLL; }
// outputs one workgroup spans
static inline uint32_t pamem_span() { return pamem_rounds() * (uint32_t)PAMEM_ROUND; }
// (address of the sample of output 0 / bytes a sample) & 1: which half of an index-aligned pair output 0 is
static inline uint64_t pamem_parity(uint64_t addr0, uint32_t bytes_in) { return (addr0 / bytes_in) & 1u; }
// the workgroups of a launch on n >= 1 outputs (at most 2^32: (2^31 + 1) pairs in 1024-pair workgroups)
static inline uint32_t pamem_grid(uint64_t parity, uint64_t n) { return pd_stream_grid(parity, n, pamem_rounds()); }
// nullptr, or why n outputs behind lead samples of history are too many for a call
static inline const char *pamem_size_check(uint64_t n, uint32_t lead)
{
    return n > ((uint64_t)1 << 32) - lead ? "n + lead must not exceed 2^32 samples" : nullptr;
}

}  // namespace mcrx
