// fadegen.hpp -- what the two fading emulators share (chanemu.hip: mcrx_hip_chanfade_*; userchan.hip:
// mcrx_hip_userfade_*, section 4.16): Philox4x32-10 and the integers of one fading ray, made on the host from the fading seed.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>

namespace mcrx {

// Philox4x32-10 (Salmon et al., SC'11), the same code on host and device
struct Philox4 { uint32_t w[4]; };
__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    Philox4 o; o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
    return o;
}

// one fading ray against the update interval of B samples: nullptr, or what is wrong with it
static inline const char *fade_ray_check(double B, double doppler, double los_doppler, float rice_k)
{
    if (!std::isfinite(doppler) || !std::isfinite(los_doppler)) return "a Doppler is not finite";
    if (doppler < 0.0) return "doppler must not be negative";
    if (doppler * B > 0.125 || std::fabs(los_doppler) * B > 0.125) return "a Doppler times the update interval exceeds 1/8: the grid does not sample the gain";
    if (!std::isfinite(rice_k) || rice_k < 0.f) return "rice_k must be finite and not negative";
    return nullptr;
}

// One fading ray's sinusoids: entry 0 the line-of-sight term, then the S scattered ones.  The words of counter (k, ray, c2, c3) under
// key `seed` give the stratified arrival angle alpha_k = 2 pi (k + w0 2^-32) / S and the phase Phi_k = w1; steps are 2^64 * cycles per
// sample, coef = { c_los, c_sc } with E|g|^2 = 1.  c2 / c3 keep the emulators' streams apart: chanemu (1, 0), userchan (2, user id).
static inline void fade_ray_integers(uint64_t seed, uint32_t ray, uint32_t c2, uint32_t c3, uint32_t S, double doppler, double los_doppler,
                              float rice_k, uint32_t los_phase, int64_t *steps, uint32_t *phases, float coef[2])
{
    steps[0] = (int64_t)std::rint(los_doppler * 18446744073709551616.0);
    phases[0] = los_phase;
    for (uint32_t k = 0; k < S; k++) {
        const Philox4 w = philox4x32_10(k, ray, c2, c3, (uint32_t)seed, (uint32_t)(seed >> 32));
        const double alpha = 2.0 * 3.14159265358979323846 * ((double)k + (double)w.w[0] * 2.3283064365386963e-10) / (double)S;
        steps[1 + k] = (int64_t)std::rint(doppler * std::cos(alpha) * 18446744073709551616.0);
        phases[1 + k] = w.w[1];
    }
    const double K = (double)rice_k;
    coef[0] = (float)std::sqrt(K / (K + 1.0));
    coef[1] = (float)std::sqrt(1.0 / ((K + 1.0) * (double)S));
}

}  // namespace mcrx
