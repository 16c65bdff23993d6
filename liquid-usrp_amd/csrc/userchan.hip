// userchan.hip -- per-user channel emulator on the transmitter's channel tiles for gfx950: every channel of the bank gets its own sparse
// multipath, oscillator, timing and level at the channel rate, between mctx_hip_traffic_tiles and mctx_hip_synthesize_tiles
// (mcrx_hip_userchan_*).
//
// Everything is a function of the ABSOLUTE block index b and of the input the caller hands over, never of how the stream is cut into
// calls, of the lead or of the launch geometry.  For local channel c:
//   s_c[b] = sum_{i<T_c} a_ci x_c[b - d_ci]             table order, two explicit fused multiply-adds per ray and component (chanemu.hip's shape)
//   r_c[b] = s_c[b] e^{+j 2 pi th / 2^32}                th = phase0_c + cfo_step_c (uint32_t)(uint64_t)b mod 2^32, sincos_u32, cmul_fx's shape
//   y_c[b] = gain_c r_c[b]                               one multiply per component
// The handle holds the parameter table and nothing else: the samples behind a call are in the caller's buffer (lead_blocks of them).
//
// userchan_kernel<ROT>: streaming, no LDS.  Tiles are granules [tile][channel][8] of cf32, 64 bytes each, so the output is one flat array
// of 16-byte sample pairs: lane g owns pair g -- samples 2 (g & 3), + 1 of granule g >> 2 -- four lanes make a granule, a wave covers 16
// adjacent granules (16 channels of one tile where the channel count allows) and stores one contiguous 1 KB.  A ray with an even delay
// is one 16-byte load per lane (the pair stays inside a granule); one with an odd delay is two 8-byte loads, the second of which may
// lie in the next tile, channels * 64 bytes further on.  The width is chosen per wave and ray: 16 bytes when all of the wave's 16
// channels have an even delay there, else 8 bytes for all of them (left to each lane, a wave of mixed parities issues three load
// instructions a ray and the kernel is bound by those: 0.59 ms against 0.42 ms for three rays on the 512-channel slab).
// A wave spans channels, so the parameters are vector loads: the table is kept
// as planes of 16-byte words indexed by the channel (delays and ray count and gain / rays 0, 1 / rays 2, 3 / step and phase), of which a
// wave reads 256 contiguous bytes each, and the plane of steps and phases is read by the rotating build only.
// Builds without rotation carry none of that code (the template parameter; a handle rotates when any of its channels does).
//
// Contraction is switched off for this file: sincos_u32's polynomials and everything else round the same way in both builds and in every
// inlined copy, and the products that matter are written as fmaf.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/mcrx_hip.h"
#include "devmath.h"
#include "devscope.hpp"

namespace mcrx {

struct UserchanArgs {
    const float2 *in; float4 *out;
    const uint4 *head;              // [C]: x = the four delays, a byte each (ray 0 lowest); y = T; z = the bits of gain
    const float4 *ray01, *ray23;    // [C]: (re, im) of rays 0, 1 / 2, 3
    const uint2 *osc;               // [C]: cfo_step, phase0 (ROT builds only)
    uint32_t C, total;              // channels; sample pairs of the output = lanes with work
    uint32_t lead;                  // blocks the input holds in front of the output's first
    uint32_t first_lo;              // the low word of the output's first absolute block index
};

// the input's sample at block r of its own range (r >= 0), channel c
__device__ __forceinline__ size_t userchan_at(uint32_t r, uint32_t c, uint32_t C) { return ((size_t)(r >> 3) * C + c) * 8u + (r & 7u); }

template <bool ROT>
__global__ __launch_bounds__(256) void userchan_kernel(UserchanArgs a)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.total) return;
    const uint32_t gran = g >> 2, k = (g & 3u) * 2u;
    const uint32_t tile = gran / a.C, c = gran - tile * a.C;
    const uint4 head = a.head[c];
    const float4 t01 = a.ray01[c], t23 = a.ray23[c];
    const uint32_t T = head.y;
    const float are[MCRX_USERCHAN_MAX_RAYS] = { t01.x, t01.z, t23.x, t23.z }, aim[MCRX_USERCHAN_MAX_RAYS] = { t01.y, t01.w, t23.y, t23.w };
    const uint32_t m = tile * 8u + k;                       // the pair's first block, relative to the output's first (even)
    float2 x0[MCRX_USERCHAN_MAX_RAYS], x1[MCRX_USERCHAN_MAX_RAYS];
#pragma unroll
    for (int i = 0; i < MCRX_USERCHAN_MAX_RAYS; i++) {      // every ray's loads first: T pairs in flight
        x0[i] = x1[i] = make_float2(0.f, 0.f);
        const uint32_t d = (head.x >> (8 * i)) & 255u;
        // one choice for the wave: 16-byte loads when every lane's delay is even, else two 8-byte loads for all of them (the same
        // values either way).  Lanes that went their own way cost a mixed wave three load instructions a ray.
        const bool wide = !__any(i < (int)T && (d & 1u));
        if (i < (int)T) {
            const uint32_t r = a.lead + m - d;              // >= 0: lead >= every delay of the handle; r + 1 <= the input's last block
            if (wide) {                                     // r even: the pair lies in one granule, 16-byte aligned
                uint32_t re = r;
                asm("" : "+v"(re));                         // (an index of its own: else the compiler shares a dword with the odd side and splits the rest)
                const float4 v = *reinterpret_cast<const float4 *>(a.in + userchan_at(re, c, a.C));
                x0[i] = make_float2(v.x, v.y); x1[i] = make_float2(v.z, v.w);
            } else { x0[i] = a.in[userchan_at(r, c, a.C)]; x1[i] = a.in[userchan_at(r + 1u, c, a.C)]; }
        }
    }
    float2 s0 = make_float2(0.f, 0.f), s1 = s0;
#pragma unroll
    for (int i = 0; i < MCRX_USERCHAN_MAX_RAYS; i++)
        if (i < (int)T) {
            const float ar = are[i], ai = aim[i];
            s0.x = fmaf(ar, x0[i].x, fmaf(-ai, x0[i].y, s0.x)); s0.y = fmaf(ar, x0[i].y, fmaf(ai, x0[i].x, s0.y));
            s1.x = fmaf(ar, x1[i].x, fmaf(-ai, x1[i].y, s1.x)); s1.y = fmaf(ar, x1[i].y, fmaf(ai, x1[i].x, s1.y));
        }
    if (ROT) {
        const uint2 o = a.osc[c];
        const uint32_t th = o.y + o.x * (a.first_lo + m);   // the low word of b is all the phase needs
        float sn, cs;
        sincos_u32(th, sn, cs);
        s0 = cmul_fx(s0, make_float2(cs, sn));
        sincos_u32(th + o.x, sn, cs);
        s1 = cmul_fx(s1, make_float2(cs, sn));
    }
    const float gain = __uint_as_float(head.z);
    a.out[g] = make_float4(gain * s0.x, gain * s0.y, gain * s1.x, gain * s1.y);
}

}  // namespace mcrx

using namespace mcrx;

static thread_local std::string g_uc_err;
#define UCCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { g_uc_err = std::string(#x) + ": " + hipGetErrorString(e_); return MCRX_EHIP; } } while (0)

struct mcrx_hip_userchan_s {
    int device = -1;            // the HIP device the handle was created on: every entry point runs with it current (devscope.hpp)
    uint32_t C = 0, lead = 0;   // channels; the largest delay rounded up to 8
    bool rot = false;           // any channel with a step or a start phase: the rotating build, for every channel
    void *table = nullptr;      // the four planes, one allocation: head[C] | ray01[C] | ray23[C] | osc[C]
};

static const size_t USERCHAN_MAX_GRANULES = (size_t)1 << 28;       // (lanes of a launch and the kernel's 32-bit block arithmetic)

extern "C" const char *mcrx_hip_userchan_last_error(void) { return g_uc_err.c_str(); }

extern "C" int mcrx_hip_userchan_create(mcrx_hip_userchan_t *out, unsigned num_channels, const mcrx_hip_userchan_channel *ch, size_t struct_size)
{
    if (!out) { g_uc_err = "null pointer"; return MCRX_EINVAL; }
    *out = nullptr;
    if (!ch) { g_uc_err = "null channel table"; return MCRX_EINVAL; }
    if (struct_size != sizeof(mcrx_hip_userchan_channel)) { g_uc_err = "mcrx_hip_userchan_channel: wrong struct_size"; return MCRX_EINVAL; }
    if (num_channels < 1 || num_channels > MCRX_USERCHAN_MAX_CHANNELS) { g_uc_err = "num_channels must be 1 .. 1024"; return MCRX_EINVAL; }
    const uint32_t C = num_channels;
    uint32_t D = 0;
    bool rot = false;
    // the planes on the host: 16 + 16 + 16 + 8 bytes a channel
    std::vector<uint32_t> host((size_t)C * 14u, 0u);
    uint32_t *head = host.data(), *osc = head + (size_t)C * 12u;
    float *r01 = reinterpret_cast<float *>(head + (size_t)C * 4u), *r23 = reinterpret_cast<float *>(head + (size_t)C * 8u);
    for (uint32_t c = 0; c < C; c++) {
        const mcrx_hip_userchan_channel &u = ch[c];
        if (u.num_rays < 1 || u.num_rays > MCRX_USERCHAN_MAX_RAYS) { g_uc_err = "num_rays must be 1 .. 4"; return MCRX_EINVAL; }
        uint32_t delays = 0;
        for (uint32_t i = 0; i < u.num_rays; i++) {
            if (u.delay[i] > MCRX_USERCHAN_MAX_DELAY) { g_uc_err = "a delay exceeds MCRX_USERCHAN_MAX_DELAY"; return MCRX_EINVAL; }
            if (!std::isfinite(u.tap_re[i]) || !std::isfinite(u.tap_im[i])) { g_uc_err = "taps must be finite"; return MCRX_EINVAL; }
            delays |= u.delay[i] << (8u * i);
            D = u.delay[i] > D ? u.delay[i] : D;
            float *r = (i < 2 ? r01 : r23) + (size_t)c * 4u + (i & 1u) * 2u;
            r[0] = u.tap_re[i]; r[1] = u.tap_im[i];
        }
        if (!std::isfinite(u.gain)) { g_uc_err = "gain must be finite"; return MCRX_EINVAL; }
        head[(size_t)c * 4u] = delays; head[(size_t)c * 4u + 1u] = u.num_rays;
        reinterpret_cast<float *>(head)[(size_t)c * 4u + 2u] = u.gain;
        osc[(size_t)c * 2u] = u.cfo_step; osc[(size_t)c * 2u + 1u] = u.phase0;
        rot = rot || u.cfo_step != 0 || u.phase0 != 0;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { g_uc_err = "no HIP device (no CPU fallback)"; return MCRX_EHIP; }
    mcrx_hip_userchan_t q = new mcrx_hip_userchan_s();
    q->device = current_device();
    q->C = C; q->lead = (D + 7u) / 8u * 8u; q->rot = rot;
    hipError_t e = hipMalloc(&q->table, host.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(q->table, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        g_uc_err = std::string("parameter table: ") + hipGetErrorString(e);
        mcrx_hip_userchan_destroy(q);
        return MCRX_EHIP;
    }
    *out = q;
    return MCRX_OK;
}

extern "C" int mcrx_hip_userchan_destroy(mcrx_hip_userchan_t q)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) return MCRX_OK;
    (void)hipDeviceSynchronize();
    if (q->table) (void)hipFree(q->table);
    delete q;
    return MCRX_OK;
}

extern "C" unsigned mcrx_hip_userchan_num_channels(mcrx_hip_userchan_t q) { return q ? q->C : 0u; }
extern "C" unsigned mcrx_hip_userchan_lead_blocks(mcrx_hip_userchan_t q) { return q ? q->lead : 0u; }

extern "C" int mcrx_hip_userchan_apply_tiles(mcrx_hip_userchan_t q, const void *d_in, long long first_block, size_t nblocks,
                                             size_t lead_blocks, void *d_out, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_uc_err = "null handle"; return MCRX_EINVAL; }
    if (!d_in || !d_out) { g_uc_err = "null buffer"; return MCRX_EINVAL; }
    const uintptr_t pi = reinterpret_cast<uintptr_t>(d_in), po = reinterpret_cast<uintptr_t>(d_out);
    if ((pi & 15u) || (po & 15u)) { g_uc_err = "d_in and d_out must be 16-byte aligned"; return MCRX_EINVAL; }
    if ((nblocks % 8) || (lead_blocks % 8) || (first_block % 8)) { g_uc_err = "nblocks, lead_blocks and first_block come in granules of 8 blocks"; return MCRX_EINVAL; }
    if (lead_blocks < q->lead) { g_uc_err = "lead_blocks is below the handle's largest delay rounded up to 8 (mcrx_hip_userchan_lead_blocks)"; return MCRX_EINVAL; }
    if (nblocks / 8 > USERCHAN_MAX_GRANULES / q->C || lead_blocks > ((size_t)1 << 30)) { g_uc_err = "at most 2^28 granules a call (and 2^30 blocks of lead)"; return MCRX_EINVAL; }
    const size_t bi = (lead_blocks + nblocks) * q->C * sizeof(float2), bo = nblocks * q->C * sizeof(float2);
    if (pi < po + bo && po < pi + bi) { g_uc_err = "d_in and d_out overlap: the rays read behind the write front, in-place use is not possible"; return MCRX_EINVAL; }
    if (nblocks == 0) return MCRX_OK;
    UserchanArgs a;
    a.in = static_cast<const float2 *>(d_in); a.out = static_cast<float4 *>(d_out);
    const uint32_t *t = static_cast<const uint32_t *>(q->table);
    a.head = reinterpret_cast<const uint4 *>(t);
    a.ray01 = reinterpret_cast<const float4 *>(t + (size_t)q->C * 4u);
    a.ray23 = reinterpret_cast<const float4 *>(t + (size_t)q->C * 8u);
    a.osc = reinterpret_cast<const uint2 *>(t + (size_t)q->C * 12u);
    a.C = q->C; a.total = (uint32_t)(nblocks / 8 * q->C * 4u);
    a.lead = (uint32_t)lead_blocks;
    a.first_lo = (uint32_t)(uint64_t)first_block;
    const dim3 grid((a.total + 255u) / 256u);
    hipStream_t st = (hipStream_t)stream;
    if (q->rot) hipLaunchKernelGGL(userchan_kernel<true>, grid, dim3(256), 0, st, a);
    else        hipLaunchKernelGGL(userchan_kernel<false>, grid, dim3(256), 0, st, a);
    UCCHK(hipGetLastError());
    return MCRX_OK;
}
