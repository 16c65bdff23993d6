// rfchain_plan.hpp -- the host side of the RF front end (rfchain.hip: mcrx_hip_rfchain_*) that needs no device:
// the configuration check and the oscillator's integers, made from pn_seed.  Plain host code: host/rfchain_plan_test.cc compiles it
// with a main of its own.
#pragma once
#include <cmath>
#include <stdint.h>
#include "../../include/mcrx_hip.h"
#include "fadegen.hpp"
#include "rapp_plan.hpp"

namespace mcrx {

// the oscillator's fields (looked at with the stage on, and by the selftest): nullptr or what is wrong
static inline const char *rfchain_osc_check(const mcrx_hip_rfchain_config *c)
{
    if (c->pn_sinusoids < 1 || c->pn_sinusoids > MCRX_RFCHAIN_MAX_SINUSOIDS) return "pn_sinusoids must be 1 .. 16";
    if (c->pn_log2_block < 1 || c->pn_log2_block > 24) return "pn_log2_block must be 1 .. 24";
    if (c->pn_table_rows == 1) return "pn_table_rows must be 0 (default) or at least 2";
    if (!std::isfinite(c->pn_rms) || c->pn_rms < 0.f) return "pn_rms must be finite and not negative";
    if (!std::isfinite(c->pn_bandwidth) || c->pn_bandwidth < 0.0) return "pn_bandwidth must be finite and not negative";
    if (c->pn_bandwidth * (double)(1u << c->pn_log2_block) > 0.125) return "pn_bandwidth times the update interval exceeds 1/8: the grid does not sample the angle";
    if ((double)c->pn_rms * std::sqrt(2.0 * (double)c->pn_sinusoids) >= 1.5707963267948966) return "pn_rms * sqrt(2 S) must stay below pi / 2 (|theta| < 1/4 turn)";
    return nullptr;
}

// fp32(1 / A^2), the division in double: rapp_plan.hpp's, which the amplifier with memory shares
static inline float rfchain_inv_sat2(float amp_sat) { return rapp_inv_sat2(amp_sat); }

// the whole configuration, as create sees it: nullptr or what is wrong
static inline const char *rfchain_check(const mcrx_hip_rfchain_config *c)
{
    if (c->struct_size != sizeof(mcrx_hip_rfchain_config)) return "mcrx_hip_rfchain_config: wrong struct_size";
    if (c->order > 1u) return "order must be 0 (tx) or 1 (rx)";
    if (c->stages & ~(MCRX_RFCHAIN_MIXER | MCRX_RFCHAIN_OSCILLATOR | MCRX_RFCHAIN_AMPLIFIER)) return "unknown stage bits";
    if (c->input_format > 1u) return "input format must be 0 (cf32) or 1 (sc16)";
    if (c->output_format > 1u) return "output format must be 0 (cf32) or 1 (sc16)";
    if (!std::isfinite(c->gain)) return "gain must be finite";
    if (c->stages & MCRX_RFCHAIN_MIXER) {
        const float m[6] = { c->alpha_re, c->alpha_im, c->beta_re, c->beta_im, c->dc_re, c->dc_im };
        for (float v : m) if (!std::isfinite(v)) return "the mixer's coefficients must be finite";
    }
    if (c->stages & MCRX_RFCHAIN_OSCILLATOR)
        if (const char *bad = rfchain_osc_check(c)) return bad;
    if (c->stages & MCRX_RFCHAIN_AMPLIFIER) {
        if (const char *bad = rapp_check(c->amp_sat, c->amp_smooth, c->amp_gain, c->amp_ampm)) return bad;
    }
    return nullptr;
}

// The oscillator's sinusoids of a checked configuration: N_k = steps[k] (2^64 * cycles per sample), Phi_k = phases[k], k < pn_sinusoids,
// and c = *coef.  The words of counter (k, 0, 3, 0) under key pn_seed: a stratified draw from a Lorentzian line of half-width pn_bandwidth.
static inline void rfchain_phase_integers(const mcrx_hip_rfchain_config *c, int64_t *steps, uint32_t *phases, float *coef)
{
    const uint32_t S = c->pn_sinusoids;
    const double fmax = 0.125 / (double)(1u << c->pn_log2_block);
    for (uint32_t k = 0; k < S; k++) {
        const Philox4 w = philox4x32_10(k, 0u, 3u, 0u, (uint32_t)c->pn_seed, (uint32_t)(c->pn_seed >> 32));
        const double u = ((double)k + ((double)w.w[0] + 0.5) * 2.3283064365386963e-10) / (double)S;
        double f = c->pn_bandwidth * std::tan(3.14159265358979323846 * (u - 0.5));
        f = f < -fmax ? -fmax : (f > fmax ? fmax : f);
        steps[k] = (int64_t)std::rint(f * 18446744073709551616.0);
        phases[k] = w.w[1];
    }
    *coef = (float)((double)c->pn_rms * std::sqrt(2.0 / (double)S) / (2.0 * 3.14159265358979323846));
}

}  // namespace mcrx
