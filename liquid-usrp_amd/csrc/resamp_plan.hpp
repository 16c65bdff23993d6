// resamp_plan.hpp -- the host side of the multi-stage resampler (msresamp.hip: msresamp_hip_*) that needs no
// device: the rate check, the rate's decomposition into half-band stages and an arbitrary stage, the phase step and its period, the
// half-band branch taps, the 256 x 14 branch table and the delay.  msresamp_hip_create uploads exactly these values and
// msresamp_hip_selftest returns them.  Plain host code: host/resamp_plan_test.cc compiles it with a main of its own.
#pragma once
#include <algorithm>
#include <cmath>
#include <stdint.h>
#include <vector>
#include "design.hpp"

namespace mcrx {

enum { RSP_M = 7, RSP_TAPS = 2 * RSP_M, RSP_NPFB = 256, RSP_PHASE_BITS = 24 };

// The deepest chain of half-band stages.  Interpolating handles never come near it (rate <= 1024: nine stages).  Decimating, with
// ns stages, the arbitrary stage's rate lies in [1/2, 1], so step = rint(2^24 / rate_arb) lies in [2^24, 2^25], and with
// g = gcd(step, 2^24) one period of the phase is per_in = step / g inputs and per_out = 2^24 / g outputs of the arbitrary stage:
// per_in < 2^25 (step = 2^25 has g = 2^24 and per_in = 2), per_out <= 2^24.  What msresamp.hip forms from them, all in 64 bits:
//   * 1ull << ns and input_position >> ns (msresamp_hip_reset_at):                                         ns <= 63
//   * j * step with j below a period plus a call, and r << 24, lim = aend << 24 on the arbitrary stage's
//     input index (the 2^40 of the header, per call): independent of ns
//   * per_in << (ns - i) (rs_period) and r << (ns - i) with r < per_in (msresamp_hip_reset_at): below 2^(25 + ns), signed:
//                                                                                                          ns <= 38
//   * the sample counters of stage buffer i (StageBuf base, end; the kernels' k, 2 k and 2 (k - 26)): rs_rebase keeps a buffer's
//     base below one period of its stage plus what the buffers hold back -- at most the samples of the calls before, a buffer
//     slides only when it is full -- and a call adds its nin: end < 2^(25 + ns) + 3 nin + 2^(ns + 7).  At ns = 38 the period alone
//     may be 2^63 - 2^38, which leaves no room for any of the rest; at ns = 37 the sum stays below 2^63 for every
//     nin < 2^60:                                                                                          ns <= 37
// The binding term is the last one.  The smallest rate of 37 stages is 2^-38 (2^-38 * 2^37 = 1/2 is not below 1/2).
enum { RSP_MAX_STAGES = 37 };

struct ResampPlan {
    bool interp = false;                // rate > 1: the arbitrary stage first, then half-band interpolators
    unsigned num_stages = 0;            // half-band stages: decimators (rate < 1/2) or interpolators (rate > 2)
    double rate_arb = 1;                // the arbitrary stage's rate: in [1/2, 1], or in (1, 2]
    unsigned long long step = 0;        // rint(2^24 / rate_arb): input samples per output of the arbitrary stage, 24 fractional bits
    long long per_in = 1, per_out = 1;  // one period of the phase: step / g inputs, 2^24 / g outputs, g = gcd(step, 2^24)
    float delay = 0;                    // msresamp_hip_get_delay: in input samples of the handle
    std::vector<float> h1;              // [14] half-band branch filter
    std::vector<float> hpfb;            // [256][14] branch table, unity DC gain per branch up to the prototype's rounding
};

// the decomposition alone (no taps): what the rate check needs
static inline void resamp_stages(float rate, bool *interp, unsigned *num_stages, double *rate_arb)
{
    double r = (double)rate;
    unsigned ns = 0;
    const bool up = rate > 1.0f;
    // (a denormal rate needs 149 doublings at most: the loop ends for every positive finite rate)
    if (up) while (r > 2.0) { ns++; r *= 0.5; }
    else    while (r < 0.5) { ns++; r *= 2.0; }
    *interp = up; *num_stages = ns; *rate_arb = r;
}

// nullptr, or why create refuses the rate
static inline const char *resamp_rate_check(float rate)
{
    if (!(rate > 0.0f) || rate > 1024.0f) return "msresamp: rate must be in [2^-38, 1024]";
    bool up; unsigned ns; double ra;
    resamp_stages(rate, &up, &ns, &ra);
    if (ns > (unsigned)RSP_MAX_STAGES) return "msresamp: rate must be in [2^-38, 1024]: at most 37 half-band stages, a rate below 2^-38 needs more";
    return nullptr;
}

// The delay of a slow tone through the chain, in input samples of the handle.
// Decimating (rate <= 1): the arbitrary stage delays its input by 7 samples; a half-band decimator in front of a chain of delay d
// (in that chain's input samples, its own output samples) delays by 2 d + 13 of its input samples: y[k] centres on x[2k-13].
// Interpolating: the arbitrary stage again delays its input -- the handle's input -- by 7 samples.  Half-band interpolator i passes
// v[2k] = u[k-7], 7 samples at rate_arb * 2^i times the input rate: 7 + (7 / rate_arb) sum_{i < num_stages} 2^-i.
static inline float resamp_delay(bool interp, unsigned num_stages, double rate_arb)
{
    if (!interp) {
        float d = (float)RSP_M;
        for (unsigned i = 0; i < num_stages; i++) d = 2.0f * d + (float)(2 * RSP_M - 1);
        return d;
    }
    double s = 0.0, w = 1.0;
    for (unsigned i = 0; i < num_stages; i++) { s += w; w *= 0.5; }
    return (float)((double)RSP_M + ((double)RSP_M / rate_arb) * s);
}

// the whole plan of an accepted rate (resamp_rate_check first)
static inline ResampPlan resamp_plan(float rate, float As)
{
    ResampPlan p;
    resamp_stages(rate, &p.interp, &p.num_stages, &p.rate_arb);
    // half-band branch filter: odd taps of a 29-tap Kaiser design with fc = 0.25, reversed
    p.h1 = halfband_branch_taps(RSP_M, As);
    // arbitrary resampler bank, unity DC gain per branch
    float fc = 0.515f * (float)p.rate_arb; if (fc > 0.49f) fc = 0.49f;
    const unsigned n = 2 * RSP_M * RSP_NPFB + 1;
    const std::vector<float> hf = firdes_kaiser(n, fc / (float)RSP_NPFB, As);
    double gain = 0; for (float v : hf) gain += v;
    gain = (double)RSP_NPFB / gain;
    p.hpfb.assign((size_t)RSP_NPFB * RSP_TAPS, 0.0f);
    for (unsigned b = 0; b < RSP_NPFB; b++)
        for (unsigned k = 0; k < RSP_TAPS; k++)
            p.hpfb[(size_t)b * RSP_TAPS + (RSP_TAPS - 1 - k)] = (float)((double)hf[b + k * RSP_NPFB] * gain);
    p.step = (unsigned long long)std::llrint((double)(1u << RSP_PHASE_BITS) / p.rate_arb);
    const long long g = (long long)std::min<unsigned long long>(p.step & (~p.step + 1), 1ull << RSP_PHASE_BITS);     // gcd(step, 2^24): step's lowest set bit
    p.per_in = (long long)p.step / g; p.per_out = (1ll << RSP_PHASE_BITS) / g;
    p.delay = resamp_delay(p.interp, p.num_stages, p.rate_arb);
    return p;
}

}  // namespace mcrx
