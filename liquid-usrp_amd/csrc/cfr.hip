// cfr.hip -- crest-factor reduction on the wideband stream for gfx950: clip-and-filter, cf32 in, cf32 or sc16 out (mcrx_hip_cfr_*;
// DESIGN.md section 4.20; the definition with every fmaf is in include/mcrx_hip.h).
//
// Stateless and non-causal: one pass reads m + 2 H samples and writes m, out[i] belongs to in[i + H]; P passes are P launches through
// the handle's scratch buffers, each covering H less on either side than the one before (cfr_plan.hpp).
//   e[n] = s x[n], s = 1 - A / sqrtf(t), where t = |x[n]|^2 > A2, else 0        what exceeds the threshold
//   c[n] = h[0] e[n], then fmaf(h[k], e[n-k] + e[n+k], c[n]) for k = 1 .. H       the same, band-limited
//   y[n] = x[n] - c[n]
//
// cfr_kernel<FOUT, LAST, ODD>: a workgroup of 256 lanes takes a run of 2048 outputs, a lane eight consecutive ones.  A lane loads the eight
// input samples under its outputs (64 bytes, as 16-byte words: all lanes' runs have the same parity, the template's ODD), keeps
// them, and writes their e into LDS; lanes 0 .. 2 H - 1 add the H samples on either side of the run.  LDS holds e only, 8 bytes a
// sample, laid out from the run's own position (so that every offset of the filter is a constant) with one word of padding per eight:
// a lane's stride is 72 bytes and the 8-byte reads of a half-wave fall on different banks.  Each wave then decides by ballot whether
// any sample of its window (its 512 outputs and H on either side, in units of a lane's eight) exceeds the threshold; a wave whose
// window holds none copies (c = +0 there, and x - (+0) = x: no bit changes; with every tap negative c = -0 and no wave skips).  The others compute c from LDS: eight taps at a time,
// 15 + 15 values read for 8 x 8 x 2 operands, the taps scalar loads from the kernel's arguments; per output the order of the definition.
// Statistics leave once per wave through sc16_clip_commit (over[p]: 64 counters a cache line apart, the workgroup picks one) and an
// atomicMax on the bit pattern of peak2 that is issued only where the wave's maximum exceeds what the word already holds.
//
// Contraction is switched off for this file: every build rounds the same way, so the integers of an sc16 handle are Q of a cf32
// handle's floats, and the products that matter are written as fmaf.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>
#include <string>
#include "../../include/mcrx_hip.h"
#include "cfr_plan.hpp"
#include "ophost.hpp"
#include "sc16.hpp"
#include "stream_call.hpp"

namespace mcrx {

enum {
    CFR_PER = 8,                                            // consecutive outputs of a lane
    CFR_HMAX = MCRX_CFR_MAX_HALF_LEN,
    CFR_LOGICAL = CFR_RUN + 2 * CFR_HMAX,                   // positions of the LDS window: the run at CFR_HMAX, whatever H is
    CFR_PHYS = CFR_LOGICAL + CFR_LOGICAL / 8,               // ... with one word of padding per eight
    CFR_SLOTS = 64, CFR_SLOT_WORDS = 16                     // counters of over[p], 128 bytes apart
};
static_assert(CFR_RUN == 256 * CFR_PER, "a lane takes eight outputs");

struct CfrArgs {
    const float2 *in; void *out;
    unsigned long long *over;                               // this pass's CFR_SLOTS counters
    unsigned int *peak2;                                    // LAST builds: the bit pattern of the largest |y|^2
    unsigned long long *clip;                               // sc16-out builds: the handle's count of clipped samples
    uint64_t m;                                             // outputs of this launch; `in` holds m + 2 H samples
    uint64_t count_lo, count_hi;                            // outputs whose input samples the statistics count
    uint32_t H, always;                                     // always: no wave may skip the filter (cfr_plan.hpp: cfr_may_skip)
    float A, A2, gain;
    float h[CFR_HMAX + 1];
};

// e of one sample; over = (t > A2)
__device__ __forceinline__ float2 cfr_excess(float2 x, float A, float A2, bool &over)
{
    const float t = fmaf(x.x, x.x, x.y * x.y);
    over = t > A2;
    if (!over) return make_float2(0.f, 0.f);
    const float s = 1.0f - A / sqrtf(t);
    return make_float2(s * x.x, s * x.y);
}

// eight consecutive samples p[0 .. 7], the first of them sample `first` of `total`: zeros beyond the end.  ODD: p is 8 bytes off a
// 16-byte boundary (known on the host: every lane's run has the parity of the launch), so the 16-byte words begin at p + 1
template <bool ODD>
__device__ __forceinline__ void cfr_load8(const float2 *p, uint64_t first, uint64_t total, float2 (&x)[CFR_PER])
{
    if (first + CFR_PER <= total) {
        if (ODD) {
            const float2 a0 = p[0];
            const float4 v1 = *reinterpret_cast<const float4 *>(p + 1), v3 = *reinterpret_cast<const float4 *>(p + 3), v5 = *reinterpret_cast<const float4 *>(p + 5);
            const float2 a7 = p[7];
            x[0] = a0; x[1] = make_float2(v1.x, v1.y); x[2] = make_float2(v1.z, v1.w); x[3] = make_float2(v3.x, v3.y);
            x[4] = make_float2(v3.z, v3.w); x[5] = make_float2(v5.x, v5.y); x[6] = make_float2(v5.z, v5.w); x[7] = a7;
        } else {
            const float4 v0 = *reinterpret_cast<const float4 *>(p), v2 = *reinterpret_cast<const float4 *>(p + 2);
            const float4 v4 = *reinterpret_cast<const float4 *>(p + 4), v6 = *reinterpret_cast<const float4 *>(p + 6);
            x[0] = make_float2(v0.x, v0.y); x[1] = make_float2(v0.z, v0.w); x[2] = make_float2(v2.x, v2.y); x[3] = make_float2(v2.z, v2.w);
            x[4] = make_float2(v4.x, v4.y); x[5] = make_float2(v4.z, v4.w); x[6] = make_float2(v6.x, v6.y); x[7] = make_float2(v6.z, v6.w);
        }
    } else {
#pragma unroll
        for (int j = 0; j < CFR_PER; j++) x[j] = first + j < total ? p[j] : make_float2(0.f, 0.f);
    }
}

__device__ __forceinline__ void cfr_store8(float2 *o, uint64_t first, uint64_t total, const float2 (&v)[CFR_PER])
{
    if (first + CFR_PER <= total) {
        if ((reinterpret_cast<uintptr_t>(o) & 8u) == 0) {
#pragma unroll
            for (int j = 0; j < CFR_PER; j += 2) *reinterpret_cast<float4 *>(o + j) = make_float4(v[j].x, v[j].y, v[j + 1].x, v[j + 1].y);
        } else {
            o[0] = v[0];
#pragma unroll
            for (int j = 1; j < CFR_PER - 1; j += 2) *reinterpret_cast<float4 *>(o + j) = make_float4(v[j].x, v[j].y, v[j + 1].x, v[j + 1].y);
            o[CFR_PER - 1] = v[CFR_PER - 1];
        }
    } else {
#pragma unroll
        for (int j = 0; j < CFR_PER; j++) if (first + j < total) o[j] = v[j];
    }
}

__device__ __forceinline__ void cfr_store8(uint32_t *o, uint64_t first, uint64_t total, const uint32_t (&w)[CFR_PER])
{
    if (first + CFR_PER <= total && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
        *reinterpret_cast<uint4 *>(o) = make_uint4(w[0], w[1], w[2], w[3]);
        *reinterpret_cast<uint4 *>(o + 4) = make_uint4(w[4], w[5], w[6], w[7]);
    } else if (first + CFR_PER <= total && (reinterpret_cast<uintptr_t>(o) & 7u) == 0) {
#pragma unroll
        for (int j = 0; j < CFR_PER; j += 2) *reinterpret_cast<uint2 *>(o + j) = make_uint2(w[j], w[j + 1]);
    } else {
#pragma unroll
        for (int j = 0; j < CFR_PER; j++) if (first + j < total) o[j] = w[j];
    }
}

__device__ __forceinline__ unsigned long long cfr_low_bits(uint32_t n) { return n >= 64u ? ~0ull : (1ull << n) - 1ull; }

template <int FOUT, bool LAST, bool ODD>
__global__ __launch_bounds__(256) void cfr_kernel(CfrArgs a)
{
    // Position u of the window holds e of the run's sample u - CFR_HMAX (the run's own outputs: 0 .. CFR_RUN - 1) at lds[u + (u >> 3)].
    __shared__ float2 lds[CFR_PHYS];
    __shared__ unsigned long long own_mask[4], halo_mask[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t H = a.H;
    const uint64_t base = (uint64_t)blockIdx.x * CFR_RUN;               // the run's first output
    const uint64_t total = a.m + 2ull * H;                              // input samples
    const uint64_t o0 = base + (uint64_t)CFR_PER * tid;                 // this lane's first output; its input sample is o0 + H

    float2 x[CFR_PER], e[CFR_PER];
    cfr_load8<ODD>(a.in + (o0 + H), o0 + H, total, x);
    bool any = false;
    uint32_t nover = 0;
#pragma unroll
    for (int j = 0; j < CFR_PER; j++) {
        bool over;
        e[j] = cfr_excess(x[j], a.A, a.A2, over);
        any = any || over;
        nover += (over && o0 + j >= a.count_lo && o0 + j < a.count_hi) ? 1u : 0u;
    }
    float2 *mine = lds + 9u * (tid + (uint32_t)CFR_HMAX / 8u);          // position CFR_HMAX + 8 tid
#pragma unroll
    for (int j = 0; j < CFR_PER; j++) mine[j] = e[j];
    // the H samples in front of the run (lanes 0 .. H - 1) and behind it (lanes H .. 2 H - 1): counted by the runs that own them
    bool halo_over = false;
    if (tid < 2u * H) {
        const bool behind = tid >= H;
        const uint32_t i = behind ? tid - H : tid;
        const uint32_t w = behind ? (uint32_t)CFR_RUN + H + i : i;      // sample of the run's window, 0 .. CFR_RUN + 2 H - 1
        const float2 v = base + w < total ? a.in[base + w] : make_float2(0.f, 0.f);
        const uint32_t u = (uint32_t)CFR_HMAX - H + w;
        lds[u + (u >> 3)] = cfr_excess(v, a.A, a.A2, halo_over);
    }
    const unsigned long long own = __ballot(any), halo = __ballot(halo_over);
    if (lane == 0) {
        own_mask[wave] = own;
        if (wave < 2u) halo_mask[wave] = halo;
    }
    __syncthreads();

    // the wave's window: its own lanes, and the lanes of its neighbours (or the halo) within H samples, in units of eight
    const uint32_t reach = (H + 7u) >> 3;
    unsigned long long seen = own;
    if (wave > 0u) seen |= own_mask[wave - 1u] >> (64u - reach);
    else seen |= halo_mask[0] & cfr_low_bits(H);
    if (wave < 3u) seen |= own_mask[wave + 1u] & cfr_low_bits(reach);
    else seen |= (halo_mask[0] & ~cfr_low_bits(H)) | halo_mask[1];
    const bool filter = a.always != 0u || __builtin_amdgcn_readfirstlane((int)(seen != 0ull)) != 0;

    float2 y[CFR_PER];
    if (filter) {
        float2 c[CFR_PER];
        const float h0 = a.h[0];
#pragma unroll
        for (int j = 0; j < CFR_PER; j++) c[j] = make_float2(h0 * e[j].x, h0 * e[j].y);
        for (uint32_t b = 0; b < reach; b++) {                          // taps k = 8 b + 1 .. 8 b + 8
            // l[i] = e at this lane's position + (i - 8) - 8 b, r[i] = e at its position + (i + 1) + 8 b
            const float2 *pl = lds + 9u * (tid + (uint32_t)CFR_HMAX / 8u - b);
            const float2 *pr = lds + 9u * (tid + (uint32_t)CFR_HMAX / 8u + b);
            float2 l[15], r[15];
#pragma unroll
            for (int i = 0; i < 15; i++) {
                l[i] = i < 8 ? *(pl + i - 9) : pl[i - 8];
                r[i] = i < 7 ? pr[i + 1] : pr[i + 2];
            }
#pragma unroll
            for (int kk = 1; kk <= 8; kk++) {
                const uint32_t k = 8u * b + (uint32_t)kk;
                if (k <= H) {
                    const float hk = a.h[k];
#pragma unroll
                    for (int j = 0; j < CFR_PER; j++) {
                        const float2 lo = l[j - kk + 8], hi = r[j + kk - 1];
                        c[j].x = fmaf(hk, lo.x + hi.x, c[j].x);
                        c[j].y = fmaf(hk, lo.y + hi.y, c[j].y);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < CFR_PER; j++) y[j] = make_float2(x[j].x - c[j].x, x[j].y - c[j].y);
    } else {
#pragma unroll
        for (int j = 0; j < CFR_PER; j++) y[j] = x[j];
    }

    uint32_t nclip = 0;
    if (LAST) {
        float pk = 0.f;                                                 // (a NaN fails the comparison and does not count)
#pragma unroll
        for (int j = 0; j < CFR_PER; j++) {
            const float t = fmaf(y[j].x, y[j].x, y[j].y * y[j].y);
            pk = (o0 + j < a.m && t > pk) ? t : pk;
        }
        uint32_t bits = __float_as_uint(pk);                            // not negative: the bit patterns order as the values do
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { const uint32_t other = (uint32_t)__shfl_xor((int)bits, o, 64); bits = other > bits ? other : bits; }
        if (lane == 0 && bits > __hip_atomic_load(a.peak2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(a.peak2, bits);
        if (a.gain != 1.0f) {
#pragma unroll
            for (int j = 0; j < CFR_PER; j++) y[j] = make_float2(a.gain * y[j].x, a.gain * y[j].y);
        }
    }
    if (FOUT == IQ_SC16) {
        uint32_t w[CFR_PER];
#pragma unroll
        for (int j = 0; j < CFR_PER; j++) {
            uint32_t cl = 0;
            w[j] = sc16_sample(y[j].x, y[j].y, cl);
            nclip += o0 + j < a.m ? cl : 0u;
        }
        cfr_store8(reinterpret_cast<uint32_t *>(a.out) + o0, o0, a.m, w);
        sc16_clip_commit(a.clip, nclip);                                // every lane of every wave gets here
    } else {
        cfr_store8(reinterpret_cast<float2 *>(a.out) + o0, o0, a.m, y);
    }
    sc16_clip_commit(a.over + (size_t)(blockIdx.x % CFR_SLOTS) * CFR_SLOT_WORDS, nover);
}

}  // namespace mcrx

using namespace mcrx;

static thread_local std::string g_cfr_err;

// what the kernels add to: over[p][slot] a cache line apart, then peak2
struct CfrStats {
    unsigned long long over[MCRX_CFR_MAX_PASSES][CFR_SLOTS][CFR_SLOT_WORDS];
    unsigned int peak2;
};

struct mcrx_hip_cfr_s {
    int device = -1;            // the HIP device the handle was created on: every entry point runs with it current (devscope.hpp)
    mcrx_hip_cfr_config cfg;
    Sc16ClipCount clip;         // sc16-out handles only (allocated at creation): clipped samples since the handle was made
    CfrStats *stats = nullptr;  // device
    hipEvent_t stats_ev = nullptr; bool stats_pending = false;
    uint64_t over_base[MCRX_CFR_MAX_PASSES] = {};   // already reported and reset
    DevBuffer scratch[2];       // P > 1: between the passes
};

extern "C" const char *mcrx_hip_cfr_last_error(void) { return g_cfr_err.c_str(); }

extern "C" int mcrx_hip_cfr_design(uint32_t half_len, double cutoff, double beta, float *h)
{
    if (const char *bad = cfr_design(half_len, cutoff, beta, h)) { g_cfr_err = bad; return MCRX_EINVAL; }
    return MCRX_OK;
}

extern "C" int mcrx_hip_cfr_create(mcrx_hip_cfr_t *out, const mcrx_hip_cfr_config *cfg)
{
    if (!out) { g_cfr_err = "null pointer"; return MCRX_EINVAL; }
    *out = nullptr;
    if (!cfg) { g_cfr_err = "null configuration"; return MCRX_EINVAL; }
    if (const char *bad = cfr_check(cfg)) { g_cfr_err = bad; return MCRX_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { g_cfr_err = "no HIP device (no CPU fallback)"; return MCRX_EHIP; }
    mcrx_hip_cfr_t q = new mcrx_hip_cfr_s();
    q->device = current_device();
    q->cfg = *cfg;
    hipError_t e = hipMalloc((void **)&q->stats, sizeof(CfrStats));
    if (e == hipSuccess) e = hipMemset(q->stats, 0, sizeof(CfrStats));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipEventCreateWithFlags(&q->stats_ev, hipEventDisableTiming);
    if (e == hipSuccess && cfg->output_format == IQ_SC16) e = q->clip.ensure();
    if (e != hipSuccess) { g_cfr_err = std::string("statistics: ") + hipGetErrorString(e); mcrx_hip_cfr_destroy(q); return MCRX_EHIP; }
    *out = q;
    return MCRX_OK;
}

extern "C" int mcrx_hip_cfr_destroy(mcrx_hip_cfr_t q)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) return MCRX_OK;
    (void)hipDeviceSynchronize();
    for (DevBuffer &s : q->scratch) s.release();
    if (q->stats) (void)hipFree(q->stats);
    if (q->stats_ev) (void)hipEventDestroy(q->stats_ev);
    q->clip.release();
    delete q;
    return MCRX_OK;
}

extern "C" unsigned mcrx_hip_cfr_halo(mcrx_hip_cfr_t q) { return q ? cfr_halo(&q->cfg) : 0u; }
extern "C" unsigned mcrx_hip_cfr_output_format(mcrx_hip_cfr_t q) { return q ? q->cfg.output_format : 0u; }

extern "C" int mcrx_hip_cfr_execute_device(mcrx_hip_cfr_t q, const void *d_in, size_t n, void *d_out, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_cfr_err = "null handle"; return MCRX_EINVAL; }
    const mcrx_hip_cfr_config &c = q->cfg;
    const bool out16 = c.output_format == IQ_SC16;
    if (const char *bad = stream_call_check(reinterpret_cast<uintptr_t>(d_in), reinterpret_cast<uintptr_t>(d_out), n, 8u, out16 ? 4u : 8u, 2ull * cfr_halo(&c),
                                            false, false, "d_in and d_out overlap: the operator reads neighbours, in-place use is refused")) { g_cfr_err = bad; return MCRX_EINVAL; }
    if (n == 0) return MCRX_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t want = (size_t)cfr_scratch_samples(&c, n) * sizeof(float2);
    MCRX_OP_CHK(g_cfr_err, q->scratch[0].ensure(want));
    if (c.passes > 2u) MCRX_OP_CHK(g_cfr_err, q->scratch[1].ensure(want));
    CfrArgs a = {};
    a.peak2 = &q->stats->peak2; a.clip = q->clip.device();
    a.H = c.half_len; a.always = cfr_may_skip(&c) ? 0u : 1u; a.A = c.threshold; a.A2 = cfr_threshold2(c.threshold); a.gain = c.gain;
    for (uint32_t k = 0; k <= c.half_len; k++) a.h[k] = c.taps[k];
    for (uint32_t p = 0; p < c.passes; p++) {
        const CfrPass ps = cfr_pass(&c, n, p);
        const bool last = p + 1u == c.passes;
        a.in = p == 0 ? static_cast<const float2 *>(d_in) : q->scratch[(p - 1u) & 1u].as<float2>();
        a.out = last ? d_out : q->scratch[p & 1u].ptr;
        a.over = &q->stats->over[p][0][0];
        a.m = ps.outputs; a.count_lo = ps.count_lo; a.count_hi = ps.count_hi;
        const bool odd = (((reinterpret_cast<uintptr_t>(a.in) >> 3) + c.half_len) & 1u) != 0;     // the lanes' first samples against 16 bytes
#define CFR_LAUNCH(F, L) do { if (odd) hipLaunchKernelGGL((cfr_kernel<F, L, true>), dim3(ps.grid), dim3(256), 0, st, a); \
                              else hipLaunchKernelGGL((cfr_kernel<F, L, false>), dim3(ps.grid), dim3(256), 0, st, a); } while (0)
        if (!last) CFR_LAUNCH(IQ_CF32, false);
        else if (out16) CFR_LAUNCH(IQ_SC16, true);
        else CFR_LAUNCH(IQ_CF32, true);
#undef CFR_LAUNCH
        MCRX_OP_CHK(g_cfr_err, hipGetLastError());
    }
    MCRX_OP_CHK(g_cfr_err, hipEventRecord(q->stats_ev, st));
    q->stats_pending = true;
    if (out16) MCRX_OP_CHK(g_cfr_err, q->clip.mark(st));
    return MCRX_OK;
}

extern "C" int mcrx_hip_cfr_clipped(mcrx_hip_cfr_t q, uint64_t *samples, int reset)
{
    return op_clipped(q, g_cfr_err, samples, reset);
}

extern "C" int mcrx_hip_cfr_stats(mcrx_hip_cfr_t q, uint64_t over[MCRX_CFR_MAX_PASSES], float *peak2, int reset)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_cfr_err = "null handle"; return MCRX_EINVAL; }
    if (q->stats_pending) { MCRX_OP_CHK(g_cfr_err, hipEventSynchronize(q->stats_ev)); q->stats_pending = false; }
    static thread_local CfrStats host;
    MCRX_OP_CHK(g_cfr_err, hipMemcpy(&host, q->stats, sizeof(host), hipMemcpyDeviceToHost));
    for (uint32_t p = 0; p < (uint32_t)MCRX_CFR_MAX_PASSES; p++) {
        uint64_t sum = 0;
        for (uint32_t s = 0; s < (uint32_t)CFR_SLOTS; s++) sum += host.over[p][s][0];
        if (over) over[p] = sum - q->over_base[p];
        if (reset) q->over_base[p] = sum;
    }
    if (peak2) { float v; memcpy(&v, &host.peak2, sizeof(v)); *peak2 = v; }
    if (reset) {                                                        // (the counts reset by their base; the maximum has none)
        MCRX_OP_CHK(g_cfr_err, hipMemset(&q->stats->peak2, 0, sizeof(host.peak2)));
        MCRX_OP_CHK(g_cfr_err, hipStreamSynchronize(nullptr));
    }
    return MCRX_OK;
}
