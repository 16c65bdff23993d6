// rapp_plan.hpp -- the host side of the memoryless amplifier (rapp.hpp) that needs no device, once: r = fp32(1 / A^2) and the check of
// the four amplifier fields.  rfchain_plan.hpp judges mcrx_hip_rfchain_config's amplifier with it and pamem_plan.hpp every branch of
// mcrx_hip_pamem_config, so the two operators refuse the same values with the same words.  Plain host code, any compiler.
#pragma once
#include <cmath>
#include <stdint.h>

namespace mcrx {

// fp32(1 / A^2), the division in double
static inline float rapp_inv_sat2(float sat) { return (float)(1.0 / ((double)sat * (double)sat)); }

// nullptr or what is wrong with an amplifier's saturation amplitude, smoothness, small-signal gain and AM/PM (turns)
static inline const char *rapp_check(float sat, uint32_t smooth, float gain, float ampm)
{
    if (smooth != 1u && smooth != 2u && smooth != 4u) return "amp_smooth must be 1, 2 or 4";
    if (!std::isfinite(sat) || !(sat > 0.f)) return "amp_sat must be finite and positive";
    const float r = rapp_inv_sat2(sat);
    if (!std::isfinite(r) || !(r > 0.f)) return "1 / amp_sat^2 is not a finite positive fp32";
    if (!std::isfinite(gain)) return "amp_gain must be finite";
    if (!std::isfinite(ampm) || std::fabs(ampm) > 0.25f) return "amp_ampm must be finite, at most 1/4 turn";
    return nullptr;
}

}  // namespace mcrx
