// sc16.hpp -- 16-bit integer IQ (sc16), defined once.  A sample is one 32-bit word: int16 re in the low half, im in the high half.
// Input (sc16_unpack): the word means (re, im) * 2^-15; conversion to fp32 and scaling are both exact for every int16.
// Output (transmitter, resampler, channel emulator):
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
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mcrx {

enum { IQ_CF32 = 0, IQ_SC16 = 1 };      // input or output

__device__ __forceinline__ float2 sc16_unpack(uint32_t w)
{
    return make_float2((float)(int16_t)(w & 0xffffu) * 0x1p-15f, (float)((int32_t)w >> 16) * 0x1p-15f);
}

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

// Host side of the count.  Kernels add to *device(); read() waits for the last mark() only.
struct Sc16ClipCount {
    unsigned long long *d_clip = nullptr, clip_base = 0;        // clip_base: already reported and reset
    hipEvent_t clip_ev = nullptr; bool clip_pending = false;

    unsigned long long *device() const { return d_clip; }
    hipError_t ensure()         // all or nothing; no-op once the counter exists
    {
        if (d_clip) return hipSuccess;
        unsigned long long *d = nullptr; hipEvent_t ev = nullptr;
        hipError_t e = hipMalloc((void **)&d, sizeof(*d));
        if (e == hipSuccess) e = hipMemset(d, 0, sizeof(*d));
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e == hipSuccess) { d_clip = d; clip_ev = ev; } else (void)hipFree(d);
        return e;
    }
    hipError_t mark(hipStream_t st)     // behind the launch that stored sc16
    {
        const hipError_t e = hipEventRecord(clip_ev, st);
        clip_pending = clip_pending || e == hipSuccess;
        return e;
    }
    hipError_t read(uint64_t *n, bool reset)    // 0, device untouched, if ensure() never ran
    {
        unsigned long long seen = clip_base;
        hipError_t e = hipSuccess;
        if (clip_pending && (e = hipEventSynchronize(clip_ev)) == hipSuccess) clip_pending = false;
        if (d_clip && e == hipSuccess) e = hipMemcpy(&seen, d_clip, sizeof(seen), hipMemcpyDeviceToHost);
        *n = seen - clip_base;
        if (reset) clip_base = seen;
        return e;
    }
    void release()
    {
        if (d_clip) (void)hipFree(d_clip);
        if (clip_ev) (void)hipEventDestroy(clip_ev);
        *this = Sc16ClipCount();
    }
};

}  // namespace mcrx
