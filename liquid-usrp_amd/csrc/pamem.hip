// pamem.hip -- amplifier with memory on the wideband stream for gfx950: a parallel Hammerstein model, B branches of rfchain's memoryless
// amplifier (rapp.hpp) each behind a sparse complex FIR; cf32 or sc16 in, cf32 or sc16 out (mcrx_hip_pamem_*; DESIGN.md section 4.25;
// the definition with every operation is in include/mcrx_hip.h).
//
// Stateless and time-invariant: n + lead samples in, the history in front, n out; a stream cut anywhere with its lead samples of
// history gives the bits of one call.  The handle owns nothing on the device but the clip counter of an sc16-out handle.
//
// pamem_kernel<B, FIN, FOUT>: mpd_apply_kernel's shape.  A lane owns an index-aligned pair of outputs (iqpair.hpp); a workgroup of 256
// lanes takes pamem_rounds() rounds of 512 outputs.  A round stages its 512 + lead input samples: the lane loads its pair (16 bytes
// where the address allows; sc16: 8), lane t < lead the history sample t, and A_b of every staged sample is evaluated ONCE, at staging,
// and written to LDS as B planes of float2.  Behind the barrier an output is sum T_b LDS reads and complex multiply-adds: a tap whose
// distance to the lane's pair is even reads the pair as one aligned 16-byte word, an odd one as two 8-byte words -- a uniform choice.
// The tap list and the branch parameters are kernel arguments: scalar loads, uniform across the grid.  A sample in front of -lead or
// behind n - 1 is staged as the amplifier's answer to a zero and feeds masked outputs only.
//
// Contraction is switched off for this file, as in rfchain.hip: every build rounds the same way, so the integers of an sc16 handle are
// Q of a cf32 handle's floats, and the products that matter are written as fmaf.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/mcrx_hip.h"
#include "iqpair.hpp"
#include "ophost.hpp"
#include "pamem_plan.hpp"
#include "rapp.hpp"
#include "stream_call.hpp"

namespace mcrx {

struct PamemArgs {
    const void *in; void *out;                              // in: the sample of output 0 (lead samples behind the call's d_in)
    unsigned long long *clip;                               // sc16-out builds: the handle's count of clipped samples
    uint64_t parity, n;                                     // (address of in[0] / bytes a sample) & 1; outputs of this launch
    uint32_t rounds, lead, plane;                           // plane: samples of one branch's plane in LDS (even)
    float gain;
    float r[PAMEM_MAX_BRANCHES], amp_gain[PAMEM_MAX_BRANCHES], ampm[PAMEM_MAX_BRANCHES];
    uint32_t smooth[PAMEM_MAX_BRANCHES], taps[PAMEM_MAX_BRANCHES];
    uint32_t tap_delay[PAMEM_MAX_FLAT]; float tap_re[PAMEM_MAX_FLAT], tap_im[PAMEM_MAX_FLAT];   // flat: branch ascending, tap ascending
};

// sample j of the launch (j >= -lead), as floats
template <int FIN> __device__ __forceinline__ float2 pamem_sample(const void *in, long long j)
{
    if (FIN == IQ_SC16) return sc16_unpack(reinterpret_cast<const uint32_t *>(in)[j]);
    return reinterpret_cast<const float2 *>(in)[j];
}

// the staged pair at `at`, `at` + 1 of a plane: one aligned 16-byte read where `at` is even
__device__ __forceinline__ void pamem_read(const float2 *plane, uint32_t at, bool even, float2 &a0, float2 &a1)
{
    if (even) {
        const float4 v = *reinterpret_cast<const float4 *>(plane + at);
        a0 = make_float2(v.x, v.y); a1 = make_float2(v.z, v.w);
    } else { a0 = plane[at]; a1 = plane[at + 1u]; }
}

// y := h a, the first term of the sum: a product and an fmaf a component
__device__ __forceinline__ float2 pamem_first(float hr, float hi, float2 a)
{
    return make_float2(fmaf(hr, a.x, -(hi * a.y)), fmaf(hr, a.y, hi * a.x));
}
// y := y + h a, every later term: two nested fmaf a component
__device__ __forceinline__ float2 pamem_add(float2 y, float hr, float hi, float2 a)
{
    return make_float2(fmaf(hr, a.x, fmaf(-hi, a.y, y.x)), fmaf(hr, a.y, fmaf(hi, a.x, y.y)));
}

template <int B, int FIN, int FOUT>
__global__ __launch_bounds__(PAMEM_WG) void pamem_kernel(PamemArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float2 pamem_planes[];     // B planes of a.plane samples: plane b holds A_b of the window
    uint32_t nclip = 0;
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * a.rounds * PAMEM_WG;
    // plane[s] is the staged sample wbase + s of the launch, wbase = (the round's first pair's m0) - lead
    const long long lead = (long long)a.lead, n = (long long)a.n;
    const uint32_t mine = a.lead + 2u * t;
    const bool wide = (a.lead & 1u) == 0u;                              // the lane's pair lies on 16 bytes of a plane
    for (uint32_t r = 0; r < a.rounds; r++) {
        const uint64_t g0 = base + (uint64_t)r * PAMEM_WG;              // the round's first pair
        if ((long long)(2 * g0) - (long long)a.parity >= n) break;      // (uniform) nothing of this round or a later one lies in the launch
        const IqPair p = iq_pair(a.parity, a.n, g0 + t);
        // the lane's pair as the window needs it: a half in front of the launch's first output is history, not masked
        float2 x0 = make_float2(0.f, 0.f), x1 = x0;
        const bool in0 = p.m0 >= -lead && p.m0 < n, in1 = p.m0 + 1 >= -lead && p.m0 + 1 < n;
        if (FIN == IQ_SC16) {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(a.in) + p.m0;
            if (in0 && in1 && (reinterpret_cast<uintptr_t>(w) & 7u) == 0) {
                const uint64_t v = *reinterpret_cast<const uint64_t *>(w);
                x0 = sc16_unpack((uint32_t)v); x1 = sc16_unpack((uint32_t)(v >> 32));
            } else { if (in0) x0 = sc16_unpack(w[0]); if (in1) x1 = sc16_unpack(w[1]); }
        } else {
            const float2 *w = reinterpret_cast<const float2 *>(a.in) + p.m0;
            if (in0 && in1 && (reinterpret_cast<uintptr_t>(w) & 15u) == 0) {
                const float4 v = *reinterpret_cast<const float4 *>(w);
                x0 = make_float2(v.x, v.y); x1 = make_float2(v.z, v.w);
            } else { if (in0) x0 = w[0]; if (in1) x1 = w[1]; }
        }
        float2 h = make_float2(0.f, 0.f);
        const long long j = p.m0 - 2ll * t - lead + (long long)t;       // lane t < lead: history sample wbase + t
        if ((long long)t < lead && j >= -lead && j < n) h = pamem_sample<FIN>(a.in, j);
#pragma unroll
        for (int b = 0; b < B; b++) {
            float2 *plane = pamem_planes + (uint32_t)b * a.plane;
            const float2 s0 = rapp_amplifier(a.r[b], a.smooth[b], a.amp_gain[b], a.ampm[b], x0);
            const float2 s1 = rapp_amplifier(a.r[b], a.smooth[b], a.amp_gain[b], a.ampm[b], x1);
            if (wide) *reinterpret_cast<float4 *>(plane + mine) = make_float4(s0.x, s0.y, s1.x, s1.y);
            else { plane[mine] = s0; plane[mine + 1u] = s1; }
            if ((long long)t < lead) plane[t] = rapp_amplifier(a.r[b], a.smooth[b], a.amp_gain[b], a.ampm[b], h);
        }
        __syncthreads();
        float2 a0, a1;
        uint32_t at = 0;                                                // the flat index of the next tap
        pamem_read(pamem_planes, mine - a.tap_delay[0], ((a.lead - a.tap_delay[0]) & 1u) == 0u, a0, a1);
        float2 v0 = pamem_first(a.tap_re[0], a.tap_im[0], a0), v1 = pamem_first(a.tap_re[0], a.tap_im[0], a1);
#pragma unroll
        for (int b = 0; b < B; b++) {
            const float2 *plane = pamem_planes + (uint32_t)b * a.plane;
            const uint32_t end = at + a.taps[b];
            for (uint32_t k = at + (b == 0 ? 1u : 0u); k < end; k++) {
                const uint32_t d = a.tap_delay[k];
                pamem_read(plane, mine - d, ((a.lead - d) & 1u) == 0u, a0, a1);
                v0 = pamem_add(v0, a.tap_re[k], a.tap_im[k], a0);
                v1 = pamem_add(v1, a.tap_re[k], a.tap_im[k], a1);
            }
            at = end;
        }
        if (a.gain != 1.0f) { v0 = make_float2(a.gain * v0.x, a.gain * v0.y); v1 = make_float2(a.gain * v1.x, a.gain * v1.y); }
        nclip += store_pair<FOUT>(a.out, p, v0, v1);
        __syncthreads();                                                // the planes are restaged by the next round
    }
    if (FOUT == IQ_SC16) sc16_clip_commit(a.clip, nclip);               // every lane of every wave gets here
}

}  // namespace mcrx

using namespace mcrx;

static thread_local std::string g_pamem_err;

struct mcrx_hip_pamem_s {
    int device = -1;            // the HIP device the handle was created on: every entry point runs with it current (devscope.hpp)
    mcrx_hip_pamem_config cfg;
    PamemConsts k;
    Sc16ClipCount clip;         // sc16-out handles only (allocated at creation): clipped samples since the handle was made
};

extern "C" const char *mcrx_hip_pamem_last_error(void) { return g_pamem_err.c_str(); }

extern "C" int mcrx_hip_pamem_selftest(const mcrx_hip_pamem_config *cfg, uint32_t *lead, float *inv_a2, uint32_t *num_taps, uint32_t *tap_branch,
                                       uint32_t *tap_delay, float *tap_h)
{
    if (!cfg) { g_pamem_err = "null pointer"; return MCRX_EINVAL; }
    if (const char *bad = pamem_check(cfg)) { g_pamem_err = bad; return MCRX_EINVAL; }
    const PamemConsts k = pamem_consts(cfg);
    if (lead) *lead = k.lead;
    if (num_taps) *num_taps = k.total;
    for (uint32_t b = 0; b < k.B; b++) if (inv_a2) inv_a2[b] = k.r[b];
    for (uint32_t i = 0; i < k.total; i++) {
        if (tap_branch) tap_branch[i] = k.tap_branch[i];
        if (tap_delay) tap_delay[i] = k.tap_delay[i];
        if (tap_h) { tap_h[2 * i] = k.tap_re[i]; tap_h[2 * i + 1] = k.tap_im[i]; }
    }
    return MCRX_OK;
}

extern "C" int mcrx_hip_pamem_create(mcrx_hip_pamem_t *out, const mcrx_hip_pamem_config *cfg)
{
    if (!out) { g_pamem_err = "null pointer"; return MCRX_EINVAL; }
    *out = nullptr;
    if (!cfg) { g_pamem_err = "null configuration"; return MCRX_EINVAL; }
    if (const char *bad = pamem_check(cfg)) { g_pamem_err = bad; return MCRX_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { g_pamem_err = "no HIP device (no CPU fallback)"; return MCRX_EHIP; }
    mcrx_hip_pamem_t q = new mcrx_hip_pamem_s();
    q->device = current_device();
    q->cfg = *cfg;
    q->k = pamem_consts(cfg);
    if (cfg->output_format == IQ_SC16) {
        const hipError_t e = q->clip.ensure();
        if (e != hipSuccess) { g_pamem_err = std::string("clip counter: ") + hipGetErrorString(e); mcrx_hip_pamem_destroy(q); return MCRX_EHIP; }
    }
    *out = q;
    return MCRX_OK;
}

extern "C" int mcrx_hip_pamem_destroy(mcrx_hip_pamem_t q)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) return MCRX_OK;
    (void)hipDeviceSynchronize();
    q->clip.release();
    delete q;
    return MCRX_OK;
}

extern "C" unsigned mcrx_hip_pamem_lead(mcrx_hip_pamem_t q) { return q ? q->k.lead : 0u; }
extern "C" unsigned mcrx_hip_pamem_input_format(mcrx_hip_pamem_t q) { return q ? q->cfg.input_format : 0u; }
extern "C" unsigned mcrx_hip_pamem_output_format(mcrx_hip_pamem_t q) { return q ? q->cfg.output_format : 0u; }

template <int FIN, int FOUT> static void pamem_launch(uint32_t B, dim3 grid, uint32_t lds, hipStream_t st, const PamemArgs &a)
{
    const dim3 wg(PAMEM_WG);
    switch (B) {
    case 1: hipLaunchKernelGGL((pamem_kernel<1, FIN, FOUT>), grid, wg, lds, st, a); break;
    case 2: hipLaunchKernelGGL((pamem_kernel<2, FIN, FOUT>), grid, wg, lds, st, a); break;
    case 3: hipLaunchKernelGGL((pamem_kernel<3, FIN, FOUT>), grid, wg, lds, st, a); break;
    default: hipLaunchKernelGGL((pamem_kernel<4, FIN, FOUT>), grid, wg, lds, st, a); break;
    }
}

extern "C" int mcrx_hip_pamem_execute_device(mcrx_hip_pamem_t q, const void *d_in, size_t n, void *d_out, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_pamem_err = "null handle"; return MCRX_EINVAL; }
    const PamemConsts &k = q->k;
    const bool in16 = q->cfg.input_format == IQ_SC16, out16 = q->cfg.output_format == IQ_SC16;
    const uint32_t si = in16 ? 4u : 8u, so = out16 ? 4u : 8u;
    const char *bad = pamem_size_check(n, k.lead);
    if (!bad) bad = stream_call_check(reinterpret_cast<uintptr_t>(d_in), reinterpret_cast<uintptr_t>(d_out), n, si, so, k.lead, false, false,
                                      "d_in and d_out overlap: a lane reads its neighbours' samples, so no overlap is allowed");
    if (bad) { g_pamem_err = bad; return MCRX_EINVAL; }
    if (n == 0) return MCRX_OK;
    hipStream_t st = (hipStream_t)stream;
    PamemArgs a = {};
    a.in = static_cast<const char *>(d_in) + (size_t)k.lead * si;      // the sample of output 0
    a.out = d_out; a.clip = q->clip.device();
    a.parity = pamem_parity(reinterpret_cast<uintptr_t>(a.in), si); a.n = n;
    a.rounds = pamem_rounds(); a.lead = k.lead; a.plane = pamem_plane(k.lead); a.gain = k.gain;
    for (uint32_t b = 0; b < k.B; b++) { a.r[b] = k.r[b]; a.amp_gain[b] = k.amp_gain[b]; a.ampm[b] = k.ampm[b]; a.smooth[b] = k.smooth[b]; a.taps[b] = k.taps[b]; }
    for (uint32_t i = 0; i < k.total; i++) { a.tap_delay[i] = k.tap_delay[i]; a.tap_re[i] = k.tap_re[i]; a.tap_im[i] = k.tap_im[i]; }
    const dim3 grid(pamem_grid(a.parity, n));
    const uint32_t lds = pamem_lds(k.B, k.lead);
    if (in16) { if (out16) pamem_launch<IQ_SC16, IQ_SC16>(k.B, grid, lds, st, a); else pamem_launch<IQ_SC16, IQ_CF32>(k.B, grid, lds, st, a); }
    else      { if (out16) pamem_launch<IQ_CF32, IQ_SC16>(k.B, grid, lds, st, a); else pamem_launch<IQ_CF32, IQ_CF32>(k.B, grid, lds, st, a); }
    MCRX_OP_CHK(g_pamem_err, hipGetLastError());
    if (out16) MCRX_OP_CHK(g_pamem_err, q->clip.mark(st));
    return MCRX_OK;
}

extern "C" int mcrx_hip_pamem_clipped(mcrx_hip_pamem_t q, uint64_t *samples, int reset)
{
    return op_clipped(q, g_pamem_err, samples, reset);
}
