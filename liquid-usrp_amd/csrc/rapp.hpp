// rapp.hpp -- the memoryless amplifier of the wideband operators, once on the device: Rapp AM/AM of smoothness 1, 2 or 4 and a
// Saleh-shaped AM/PM through the 32-bit phase word (the definition with every operation: include/mcrx_hip.h, the RF front end's
// amplifier).  rfchain.hip's amplifier stage and every branch of pamem.hip are this function; the phase word and the rotation serve
// rfchain's oscillator too.  The including file switches contraction off: the products that matter are written as fmaf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "devmath.h"

namespace mcrx {

// (uint32_t)(int32_t)rintf(turns * 2^32): the hardware's conversion, as sc16_round's (it saturates and turns NaN into 0, where the C cast
// is undefined -- an infinite input sample reaches this through the amplifier's phi)
__device__ __forceinline__ uint32_t rfchain_phase_word(float turns)
{
    const float r = __builtin_rintf(turns * 4294967296.0f);
    int i;
    asm("v_cvt_i32_f32_e32 %0, %1" : "=v"(i) : "v"(r));
    return (uint32_t)i;
}
// z e(p), chanemu_sample's shape
__device__ __forceinline__ float2 rfchain_rotate(float2 z, uint32_t p)
{
    float sn, cs;
    sincos_u32(p, sn, cs);
    return make_float2(fmaf(z.x, cs, -(z.y * sn)), fmaf(z.x, sn, z.y * cs));
}
// inv_a2 = fp32(1 / A^2) (rapp_plan.hpp); smooth 1, 2 or 4; ampm in turns, 0: no rotation
__device__ __forceinline__ float2 rapp_amplifier(float inv_a2, uint32_t smooth, float amp_gain, float ampm, float2 z)
{
    const float t = fmaf(z.x, z.x, z.y * z.y) * inv_a2;
    float q;
    if (smooth == 1u) q = 1.0f + t;
    else if (smooth == 2u) q = sqrtf(fmaf(t, t, 1.0f));
    else { const float t2 = t * t; q = sqrtf(sqrtf(fmaf(t2, t2, 1.0f))); }
    const float G = amp_gain / sqrtf(q);
    const float2 w = make_float2(G * z.x, G * z.y);
    if (ampm == 0.f) return w;
    return rfchain_rotate(w, rfchain_phase_word(ampm * (t / (1.0f + t))));
}

}  // namespace mcrx
