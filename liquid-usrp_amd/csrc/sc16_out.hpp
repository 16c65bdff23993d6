// sc16_out.hpp -- the transmitter's 16-bit integer output format (mctx_hip_set_output_format(q, 1)), defined once.
//
// Let v be the fp32 value a cf32 transmitter stores for one component (behind the oscillator and the gain).  An sc16 transmitter stores
//   Q(v) = clamp(r, -32768, 32767),  r = rint(v * 32768.0f)      round half to even, in fp32; the multiply is exact
// so Q is a function of the cf32 output alone.  NaN stores 0, infinities saturate.  A SAMPLE is clipped when r lies outside
// [-32768, 32767] for its re or its im (NaN does not count).  Layout: interleaved int16 re, im -- 4 bytes a sample, the receiver's
// input_format = 1 as it stands (a sample means (re, im) * 2^-15).
//
// Five vector instructions a component pair behind the multiplies: v_rndne_f32 x 2, v_cvt_i32_f32 x 2 (which saturates to the int32
// range and turns NaN into 0 -- the hardware's conversion, hence the asm: the C cast is undefined outside the range) and the
// saturating pack v_cvt_pk_i16_i32.  The clip test works on the int32s: r + 32768 as an unsigned number is > 65535 exactly outside the
// range, the saturated infinities included.
#pragma once
#include <stdint.h>

namespace mcrx {

enum { TX_CF32 = 0, TX_SC16 = 1 };      // mctx_hip_set_output_format

__device__ __forceinline__ int sc16_round(float v)
{
    const float r = __builtin_rintf(v * 32768.0f);
    int i;
    asm("v_cvt_i32_f32_e32 %0, %1" : "=v"(i) : "v"(r));
    return i;
}
__device__ __forceinline__ bool sc16_outside(int r) { return (unsigned)(r + 32768) > 65535u; }
// one sample: the packed word (re in the low half), nclip += 1 when it is clipped
__device__ __forceinline__ uint32_t sc16_sample(float re, float im, uint32_t &nclip)
{
    typedef short v2s __attribute__((ext_vector_type(2)));
    const int a = sc16_round(re), b = sc16_round(im);
    nclip += (sc16_outside(a) || sc16_outside(b)) ? 1u : 0u;
    const v2s p = __builtin_amdgcn_cvt_pk_i16(a, b);
    return __builtin_bit_cast(uint32_t, p);
}
// The clip count leaves a kernel once per wave: the lanes' registers summed across the wave (every lane of it must get here), and
// one vector atomic from its first lane -- none at all while nothing clips.
__device__ __forceinline__ void sc16_clip_commit(unsigned long long *counter, uint32_t nclip)
{
    if (__ballot(nclip != 0u) == 0ull) return;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) nclip += (uint32_t)__shfl_xor((int)nclip, o, 64);
    if ((threadIdx.x & 63u) == 0u) atomicAdd(counter, (unsigned long long)nclip);
}

}  // namespace mcrx
