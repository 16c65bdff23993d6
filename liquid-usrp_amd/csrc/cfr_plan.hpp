// cfr_plan.hpp -- the host side of the crest-factor reduction (cfr.hip: mcrx_hip_cfr_*) that needs no device: the
// configuration check, A2, the passes of a call (what each of them covers, counts and launches) and the low-pass design.  Plain host
// code: host/cfr_plan_test.cc compiles it with a main of its own.
#pragma once
#include <cmath>
#include <stdint.h>
#include "../../include/mcrx_hip.h"
#include "design.hpp"

namespace mcrx {

enum { CFR_RUN = 2048 };        // outputs a workgroup takes (cfr.hip: 256 lanes, eight consecutive outputs each)

// fp32(A * A), the product in double
static inline float cfr_threshold2(float a) { return (float)((double)a * (double)a); }

// the whole configuration, as create sees it: nullptr or what is wrong
static inline const char *cfr_check(const mcrx_hip_cfr_config *c)
{
    if (c->struct_size != sizeof(mcrx_hip_cfr_config)) return "mcrx_hip_cfr_config: wrong struct_size";
    if (c->half_len < 1u || c->half_len > (uint32_t)MCRX_CFR_MAX_HALF_LEN) return "half_len must be 1 .. 64";
    if (c->passes < 1u || c->passes > (uint32_t)MCRX_CFR_MAX_PASSES) return "passes must be 1 .. 4";
    if (c->output_format > 1u) return "output format must be 0 (cf32) or 1 (sc16)";
    if (!std::isfinite(c->threshold) || !(c->threshold > 0.f)) return "threshold must be finite and positive";
    const float a2 = cfr_threshold2(c->threshold);
    if (!std::isfinite(a2) || !(a2 > 0.f)) return "threshold^2 is not a finite positive fp32";
    if (!std::isfinite(c->gain)) return "gain must be finite";
    for (uint32_t k = 0; k <= c->half_len; k++)
        if (!std::isfinite(c->taps[k])) return "the taps h[0 .. half_len] must be finite";
    return nullptr;
}

// Where every e within reach is +0 the sum c is a zero, and it is +0 unless EVERY tap h[0 .. H] carries a negative sign (DESIGN.md
// section 4.20): x - (+0) = x for every x, x - (-0) turns -0.0 into +0.0.  Only with c = +0 may a wave skip the filter.
static inline bool cfr_may_skip(const mcrx_hip_cfr_config *c)
{
    for (uint32_t k = 0; k <= c->half_len; k++) if (!std::signbit(c->taps[k])) return true;
    return false;
}

static inline uint32_t cfr_halo(const mcrx_hip_cfr_config *c) { return c->passes * c->half_len; }

// a call of n outputs fits when n + 2 halo <= 2^32
static inline bool cfr_fits(const mcrx_hip_cfr_config *c, uint64_t n)
{
    const uint64_t most = (uint64_t)1 << 32, reach = 2ull * cfr_halo(c);
    return n <= most && n + reach <= most;
}

// Pass p (0 .. P - 1) of a call of n outputs: it writes `outputs` samples -- the caller's n and (P - 1 - p) H on either side -- from
// outputs + 2 H samples of its input; of its outputs the indices [count_lo, count_hi) are the caller's n, whose input samples the
// statistics count; `grid` workgroups.
struct CfrPass { uint64_t outputs, count_lo, count_hi; uint32_t grid; };
static inline CfrPass cfr_pass(const mcrx_hip_cfr_config *c, uint64_t n, uint32_t p)
{
    CfrPass r;
    const uint64_t side = (uint64_t)(c->passes - 1u - p) * c->half_len;
    r.outputs = n + 2 * side;
    r.count_lo = side;
    r.count_hi = side + n;
    r.grid = (uint32_t)((r.outputs + CFR_RUN - 1) / CFR_RUN);
    return r;
}
// samples of the scratch buffer a call of n outputs needs (the output of pass 0); 0 with one pass
static inline uint64_t cfr_scratch_samples(const mcrx_hip_cfr_config *c, uint64_t n)
{
    return c->passes > 1u ? n + 2ull * (c->passes - 1u) * c->half_len : 0;
}

// The low-pass: h[k] = 2 fc sinc(2 fc k) w(k), w the Kaiser window of firdes_kaiser over 2 H + 1 taps, scaled to unit sum; nullptr or
// what is wrong (h untouched then)
static inline const char *cfr_design(uint32_t half_len, double cutoff, double beta, float *h)
{
    if (!h) return "null pointer";
    if (half_len < 1u || half_len > (uint32_t)MCRX_CFR_MAX_HALF_LEN) return "half_len must be 1 .. 64";
    if (!std::isfinite(cutoff) || !(cutoff > 0.0) || !(cutoff < 0.5)) return "cutoff must lie in (0, 0.5) cycles per sample";
    if (!std::isfinite(beta) || beta < 0.0) return "beta must be finite and not negative";
    double d[MCRX_CFR_MAX_HALF_LEN + 1], sum = 0.0;
    const double ib = besseli0(beta), len = 2.0 * (double)half_len + 1.0;
    for (uint32_t k = 0; k <= half_len; k++) {
        const double x = 2.0 * cutoff * (double)k;
        const double s = k == 0 ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
        const double r = 2.0 * (double)k / len;
        d[k] = 2.0 * cutoff * s * besseli0(beta * std::sqrt(1.0 - r * r)) / ib;
        sum += k == 0 ? d[k] : 2.0 * d[k];
    }
    if (!std::isfinite(sum) || !(std::fabs(sum) > 1e-6)) return "the taps do not sum to a usable gain";
    for (uint32_t k = 0; k <= half_len; k++) h[k] = (float)(d[k] / sum);
    return nullptr;
}

}  // namespace mcrx
