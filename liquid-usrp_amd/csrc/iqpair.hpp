// iqpair.hpp -- the index-aligned pair of the streaming operators (chanemu_kernel, rfchain_kernel, rfcal_kernel), once on the device.
// Pair g of a launch on samples pos .. pos + n - 1 holds the absolute samples base + 2 g, + 1 with base = pos & ~1: relative to the launch's
// first sample that is m0 = 2 g - (pos & 1), m0 + 1.  At the two ends of the launch one half of a pair may lie outside it (ok0 / ok1).
// A pair is one 16-byte access (sc16: 8) where its address allows -- a uniform choice, all lanes' pairs have the same parity -- and two
// single ones otherwise; the masked half of an edge pair is neither read nor written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sc16.hpp"

namespace mcrx {

// pairs that hold samples pos .. pos + n - 1: the lanes of a launch
__host__ __device__ inline uint64_t iq_pairs(uint64_t pos, uint64_t n) { return ((pos & 1u) + n + 1) >> 1; }
// absolute index of pair g's first sample: even; wraps with the 64-bit position
__device__ __forceinline__ uint64_t iq_pair_index(uint64_t pos, uint64_t g) { return (pos - (pos & 1u)) + 2 * g; }

struct IqPair { long long m0; bool ok0, ok1; };

__device__ __forceinline__ IqPair iq_pair(uint64_t pos, uint64_t n, uint64_t g)
{
    IqPair p;
    p.m0 = (long long)(2 * g) - (long long)(pos & 1u);
    p.ok0 = p.m0 >= 0 && p.m0 < (long long)n;
    p.ok1 = p.m0 + 1 < (long long)n;                                   // (m0 + 1 >= 0 always)
    return p;
}

// the pair's two sc16 words as they lie in memory; a masked half is 0
__device__ __forceinline__ void load_pair_words(const void *in, IqPair p, uint32_t &w0, uint32_t &w1)
{
    const uint32_t *q = reinterpret_cast<const uint32_t *>(in) + p.m0;
    w0 = 0; w1 = 0;
    if (p.ok0 && p.ok1 && (reinterpret_cast<uintptr_t>(q) & 7u) == 0) {       // (one 64-bit word: a load of two the compiler may split again)
        const uint64_t w = *reinterpret_cast<const uint64_t *>(q);
        w0 = (uint32_t)w; w1 = (uint32_t)(w >> 32);
    }
    else { if (p.ok0) w0 = q[0]; if (p.ok1) w1 = q[1]; }
}

// the pair's samples as floats; a masked half is a zero
template <int FMT> __device__ __forceinline__ void load_pair(const void *in, IqPair p, float2 &x0, float2 &x1)
{
    if (FMT == IQ_SC16) {
        uint32_t w0, w1;
        load_pair_words(in, p, w0, w1);
        x0 = sc16_unpack(w0); x1 = sc16_unpack(w1);
    } else {
        const float2 *q = reinterpret_cast<const float2 *>(in) + p.m0;
        x0 = make_float2(0.f, 0.f); x1 = x0;
        if (p.ok0 && p.ok1 && (reinterpret_cast<uintptr_t>(q) & 15u) == 0) {
            const float4 v = *reinterpret_cast<const float4 *>(q);
            x0 = make_float2(v.x, v.y); x1 = make_float2(v.z, v.w);
        } else { if (p.ok0) x0 = q[0]; if (p.ok1) x1 = q[1]; }
    }
}

// stores the pair as cf32, or as sc16 through the shared quantiser; returns how many of its samples inside the launch were clipped
template <int FMT> __device__ __forceinline__ uint32_t store_pair(void *out, IqPair p, float2 v0, float2 v1)
{
    if (FMT == IQ_SC16) {
        uint32_t *o = reinterpret_cast<uint32_t *>(out) + p.m0;
        uint32_t c0 = 0, c1 = 0;
        const uint32_t q0 = sc16_sample(v0.x, v0.y, c0), q1 = sc16_sample(v1.x, v1.y, c1);
        if (p.ok0 && p.ok1 && (reinterpret_cast<uintptr_t>(o) & 7u) == 0) *reinterpret_cast<uint2 *>(o) = make_uint2(q0, q1);
        else { if (p.ok0) o[0] = q0; if (p.ok1) o[1] = q1; }
        return (p.ok0 ? c0 : 0u) + (p.ok1 ? c1 : 0u);
    }
    float2 *o = reinterpret_cast<float2 *>(out) + p.m0;
    if (p.ok0 && p.ok1 && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) *reinterpret_cast<float4 *>(o) = make_float4(v0.x, v0.y, v1.x, v1.y);
    else { if (p.ok0) o[0] = v0; if (p.ok1) o[1] = v1; }
    return 0u;
}

}  // namespace mcrx
