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
// With fading on (mcrx_hip_userfade_*) the constant a_ci becomes g_ci(b) a_ci, a sum of sinusoids sampled on the
// grid b = row 2^L and interpolated linearly between its rows -- chanemu.hip's definition at the channel rate, per user:
//   G_ci[row] = c_los e((psi << 32) + Lambda n_r) + c_sc sum_{k<S} e((Phi_k << 32) + N_k n_r)       n_r = row << L, phases mod 2^64
//   g_ci(b)   = fmaf(f, G_ci[row+1] - G_ci[row], G_ci[row])     row = b >> L, f = (b & (2^L - 1)) 2^-L (exact), per component
//   s_c[b]    = sum_i (g_ci(b) a_ci) x_c[b - d_ci]              the product in cmul_fx's shape, then the two fmaf per component as above
// userchan_gain_kernel writes the rows a span needs into the handle's table, float2 [row][channel][4]: a lane per (channel, ray) holds
// that ray's 1 + S phases and steps in registers and walks a chunk of rows, so a wave loads 64 adjacent integers of every plane
// ([term][channel * 4 + ray]) and stores 512 contiguous bytes a row.  userchan_kernel<ROT, FADE = true> reads two rows per granule
// (L >= 3: a granule never straddles a row), one 16-byte word for rays 0, 1 and one for rays 2, 3 of each.
//
// With a clock on (mcrx_hip_userclock_*) the user transmits z_c[b] = x_c(b - tau_c(b)) instead of x_c[b], in front
// of all of the above: tau_fp(b) = delay_fp + floor(sco (b - origin) / 2^16) in Q32 samples (int64), n = tau_fp >> 32, mu its low word,
//   z_c[b]  = sum_{j<32} h_j(mu) x_c[b - n + 15 - j]          j = 0 .. 31 from zero, one fmaf per tap and component; z is fp32
//   h_j(mu) = fmaf(f, W[r+1][j] - W[r][j], W[r][j])           r = mu >> 26, f = ((mu >> 2) & 0xffffff) 2^-24
// userclock_kernel writes z of a span into the handle's scratch buffer, in the tiles' layout, and userchan_kernel runs on that.  A
// workgroup takes 16 adjacent channels x 128 output blocks: it stages the 21 tile rows each of its channels needs (its own window: n is
// per channel) and W in LDS, then a wave walks four tiles with userchan_kernel's lane layout -- lane = (channel, sample pair) -- and
// stores 1 KB a tile.
//
// Contraction is switched off for this file: sincos_u32's polynomials and everything else round the same way in both builds and in every
// inlined copy, and the products that matter are written as fmaf.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/mcrx_hip.h"
#include "devmath.h"
#include "fadegen.hpp"
#include "design.hpp"
#include "interp_table.hpp"
#include "ophost.hpp"
#include "span_plan.hpp"

namespace mcrx {

struct UserchanArgs {
    const float2 *in; float4 *out;
    const uint4 *head;              // [C]: x = the four delays, a byte each (ray 0 lowest); y = T; z = the bits of gain
    const float4 *ray01, *ray23;    // [C]: (re, im) of rays 0, 1 / 2, 3
    const uint2 *osc;               // [C]: cfo_step, phase0 (ROT builds only)
    uint32_t C, total;              // channels; sample pairs of the output = lanes with work
    uint32_t lead;                  // blocks the input holds in front of the output's first
    uint32_t first_lo;              // the low word of the output's first absolute block index
    // FADE builds only: the gain table of this span, its row 0 = the grid row of the output's first block
    const float4 *gtab;             // [row][C][2]: (G of rays 0, 1) / (rays 2, 3)
    uint32_t frac0, L;              // first block & (2^L - 1); log2 of the update interval
    float finv;                     // 2^-L
};

#define USERFADE_TERMS (MCRX_CHANEMU_MAX_SINUSOIDS + 1)     // the line-of-sight term and up to 16 scattered ones
#define USERFADE_CHUNK 8u                                   // rows a lane of the gain kernel walks

struct UserfadeGainArgs {
    const uint64_t *step;           // [1 + S][lanes]: 2^64 * cycles per channel-rate sample, entry 0 the line-of-sight term
    const uint32_t *phase;          // [1 + S][lanes]
    const float2 *coef;             // [lanes]: c_los, c_sc
    float2 *table;                  // [rows][lanes]
    long long row0;                 // the grid row of the table's first
    uint32_t rows, lanes, L, S;     // lanes = channels * 4
};

// table[r][lane] = G_lane[row0 + r], r < rows: blockIdx.x is a chunk of rows, blockIdx.y * 256 + threadIdx.x the lane = channel * 4 + ray
__global__ __launch_bounds__(256) void userchan_gain_kernel(UserfadeGainArgs a)
{
    const uint32_t lane = blockIdx.y * 256u + threadIdx.x;
    if (lane >= a.lanes) return;
    const uint32_t r0 = blockIdx.x * USERFADE_CHUNK;                    // < rows (the grid)
    const uint32_t nr = a.rows - r0 < USERFADE_CHUNK ? a.rows - r0 : USERFADE_CHUNK;
    const uint64_t nb = (uint64_t)(a.row0 + (long long)r0) << a.L;      // the grid index wraps with the 64-bit position
    uint64_t p[USERFADE_TERMS], dp[USERFADE_TERMS];
#pragma unroll
    for (uint32_t j = 0; j < USERFADE_TERMS; j++) {
        p[j] = dp[j] = 0;
        if (j <= a.S) {
            const uint64_t st = a.step[(size_t)j * a.lanes + lane];
            p[j] = ((uint64_t)a.phase[(size_t)j * a.lanes + lane] << 32) + st * nb;
            dp[j] = st << a.L;                                          // one row further: st * (nb + 2^L) mod 2^64
        }
    }
    const float2 co = a.coef[lane];
    float2 *out = a.table + (size_t)r0 * a.lanes + lane;
    for (uint32_t r = 0; r < nr; r++) {
        float sn, cs;
        sincos_u32((uint32_t)(p[0] >> 32), sn, cs);
        float2 G = make_float2(co.x * cs, co.x * sn);
        p[0] += dp[0];
#pragma unroll
        for (uint32_t k = 1; k < USERFADE_TERMS; k++)
            if (k <= a.S) {
                sincos_u32((uint32_t)(p[k] >> 32), sn, cs);
                G.x = fmaf(co.y, cs, G.x); G.y = fmaf(co.y, sn, G.y);
                p[k] += dp[k];
            }
        out[(size_t)r * a.lanes] = G;
    }
}

// the input's sample at block r of its own range (r >= 0), channel c
__device__ __forceinline__ size_t userchan_at(uint32_t r, uint32_t c, uint32_t C) { return ((size_t)(r >> 3) * C + c) * 8u + (r & 7u); }

template <bool ROT, bool FADE>
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
    // FADE: the granule's grid row relative to the table's first, the pair's two fractions, and the two rows' words
    float4 ga01 = make_float4(0.f, 0.f, 0.f, 0.f), ga23 = ga01, gb01 = ga01, gb23 = ga01;
    float f0 = 0.f, f1 = 0.f;
    if (FADE) {
        const uint32_t pm = a.frac0 + m;                    // < 2^32: frac0 < 2^20, m < 2^31
        const uint32_t frac = pm & ((1u << a.L) - 1u);      // even, frac + 1 < 2^L
        f0 = (float)frac * a.finv; f1 = (float)(frac + 1u) * a.finv;
        const float4 *ra = a.gtab + ((size_t)(pm >> a.L) * a.C + c) * 2u, *rb = ra + (size_t)a.C * 2u;
        ga01 = ra[0]; gb01 = rb[0];
        if (T > 2u) { ga23 = ra[1]; gb23 = rb[1]; }
    }
#pragma unroll
    for (int i = 0; i < MCRX_USERCHAN_MAX_RAYS; i++)
        if (i < (int)T && FADE) {
            const float4 wa = i < 2 ? ga01 : ga23, wb = i < 2 ? gb01 : gb23;
            const float2 G0 = (i & 1) ? make_float2(wa.z, wa.w) : make_float2(wa.x, wa.y);
            const float2 G1 = (i & 1) ? make_float2(wb.z, wb.w) : make_float2(wb.x, wb.y);
            const float dx = G1.x - G0.x, dy = G1.y - G0.y;
            const float2 av = make_float2(are[i], aim[i]);
            const float2 h0 = cmul_fx(make_float2(fmaf(f0, dx, G0.x), fmaf(f0, dy, G0.y)), av);
            const float2 h1 = cmul_fx(make_float2(fmaf(f1, dx, G0.x), fmaf(f1, dy, G0.y)), av);
            s0.x = fmaf(h0.x, x0[i].x, fmaf(-h0.y, x0[i].y, s0.x)); s0.y = fmaf(h0.x, x0[i].y, fmaf(h0.y, x0[i].x, s0.y));
            s1.x = fmaf(h1.x, x1[i].x, fmaf(-h1.y, x1[i].y, s1.x)); s1.y = fmaf(h1.x, x1[i].y, fmaf(h1.y, x1[i].x, s1.y));
        } else if (i < (int)T) {
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

#define UCLK_BLOCKS 128u                    // output blocks a workgroup takes
#define UCLK_CH     16u                     // adjacent channels a workgroup takes: a wave is 16 channels x 4 sample pairs, as in userchan_kernel
#define UCLK_ROWS   21u                     // tile rows staged per channel: 128 + 31 samples, one step of n and 7 of alignment are 167 <= 168
#define UCLK_XS     (UCLK_ROWS * 8u + 2u)   // samples a channel's window takes in LDS (16-byte aligned rows, off the power of two)
#define UCLK_WS     (MCRX_USERCLOCK_TAPS + 1u)      // a row of W in LDS: lanes of different phases r read different banks

struct UserclockArgs {
    const float2 *in; float4 *out;
    const uint4 *par;               // [C][2]: delay_fp, sco / origin, enabled (a user without a clock: 15 << 32, 0 / 0, 0)
    const float *W;                 // [65][32]
    long long first;                // the output's first absolute block index
    uint32_t C, tiles;              // channels; tiles of the output
    uint32_t lead;                  // blocks the input holds in front of the output's first
    uint32_t in_rows;               // tile rows the input holds: lead / 8 + tiles
    uint32_t skip;                  // output blocks below this one are written as zeros and read nothing
};

// h_j(mu) from the two rows of W around the fraction: userclock_coef (interp_table.hpp)
// tau_fp(b): the product wraps where the host has not checked it (blocks below `skip` never get here)
__host__ __device__ __forceinline__ int64_t userclock_tau(int64_t delay_fp, int64_t sco, int64_t origin, int64_t b)
{
    return delay_fp + ((int64_t)((uint64_t)sco * (uint64_t)(b - origin)) >> 16);
}

// blockIdx.x: 128 output blocks; blockIdx.y: 16 channels
__global__ __launch_bounds__(256) void userclock_kernel(UserclockArgs a)
{
    __shared__ float sW[(MCRX_USERCLOCK_PHASES + 1) * UCLK_WS];
    __shared__ __attribute__((aligned(16))) float2 sX[UCLK_CH * UCLK_XS];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    for (uint32_t i = t; i < (MCRX_USERCLOCK_PHASES + 1) * MCRX_USERCLOCK_TAPS; i += 256u) sW[(i >> 5) * UCLK_WS + (i & 31u)] = a.W[i];
    const uint32_t cl = lane >> 2, q = lane & 3u, c = blockIdx.y * UCLK_CH + cl;
    const uint32_t m0 = blockIdx.x * UCLK_BLOCKS, left = a.tiles * 8u - m0;        // (the grid: m0 < tiles * 8 <= 2^31)
    const uint32_t nb = left < UCLK_BLOCKS ? left : UCLK_BLOCKS;
    const uint32_t ma = m0 > a.skip ? m0 : a.skip, mb = m0 + nb - 1u;               // the blocks computed here: [ma, mb], none when ma > mb
    const bool live = c < a.C && ma <= mb;
    int64_t dfp = 0, sco = 0, org = 0, base = 0;                                    // base: the input block (of its own range) at sX[.][0]
    bool on = false;
    if (live) {
        const uint4 p0 = a.par[2u * c], p1 = a.par[2u * c + 1u];
        dfp = (int64_t)(((uint64_t)p0.y << 32) | p0.x); sco = (int64_t)(((uint64_t)p0.w << 32) | p0.z);
        org = (int64_t)(((uint64_t)p1.y << 32) | p1.x); on = p1.z != 0u;
        // tau is a straight line: the largest n of the workgroup's blocks is at one of its ends, and the smallest at most one below
        const int64_t na = userclock_tau(dfp, sco, org, a.first + ma) >> 32, nz = userclock_tau(dfp, sco, org, a.first + mb) >> 32;
        const int64_t lo = (int64_t)a.lead + ma - (na > nz ? na : nz) - 16;         // the first sample any of them reads
        base = (lo >> 3) * 8;                                                       // (floor: rows in front of the input are not loaded)
    }
    // the window: tile rows base / 8 .. + 20 of this lane's channel, 16 bytes a lane -- four lanes a granule, as the output's
    for (uint32_t row = wave; row < UCLK_ROWS; row += 4u) {
        const int64_t gr = (base >> 3) + row;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live && gr >= 0 && gr < (int64_t)a.in_rows) v = *reinterpret_cast<const float4 *>(a.in + ((size_t)gr * a.C + c) * 8u + q * 2u);
        *reinterpret_cast<float4 *>(&sX[cl * UCLK_XS + row * 8u + q * 2u]) = v;
    }
    __syncthreads();
    if (c >= a.C) return;
    const float2 *xw = sX + cl * UCLK_XS;
    for (uint32_t i = 0; i < 4u; i++) {
        const uint32_t m = m0 + (wave * 4u + i) * 8u + q * 2u;                      // the pair's first block
        if (m > mb) break;
        float2 z[2];
#pragma unroll
        for (uint32_t s = 0; s < 2u; s++) {
            const uint32_t ms = m + s;
            z[s] = make_float2(0.f, 0.f);
            if (ms < a.skip) continue;
            if (!on) { z[s] = xw[(int64_t)a.lead + ms - base]; continue; }           // z = x, bit for bit (the window lies as for n = 15)
            const int64_t tau = userclock_tau(dfp, sco, org, a.first + ms);
            const uint32_t mu = (uint32_t)(uint64_t)tau, r = mu >> 26;
            const float f = (float)((mu >> 2) & 0xffffffu) * 0x1p-24f;
            int64_t p = (int64_t)a.lead + ms - (tau >> 32) + 15 - base;             // tap 0's sample; 31 <= p < 168 by the choice of base
            p = p < 31 ? 31 : (p > (int64_t)UCLK_XS - 1 ? (int64_t)UCLK_XS - 1 : p);   // (held there whatever the integers are)
            const float *w0 = sW + r * UCLK_WS, *w1 = w0 + UCLK_WS;
            const float2 *x = xw + p;
            float zr = 0.f, zi = 0.f;
#pragma unroll
            for (int j = 0; j < MCRX_USERCLOCK_TAPS; j++) {
                const float h = userclock_coef(w0[j], w1[j], f);
                const float2 v = x[-j];
                zr = fmaf(h, v.x, zr); zi = fmaf(h, v.y, zi);
            }
            z[s] = make_float2(zr, zi);
        }
        a.out[((size_t)(m >> 3) * a.C + c) * 4u + q] = make_float4(z[0].x, z[0].y, z[1].x, z[1].y);
    }
}

}  // namespace mcrx

using namespace mcrx;

static thread_local std::string g_uc_err;

struct mcrx_hip_userchan_s {
    int device = -1;            // the HIP device the handle was created on: every entry point runs with it current (devscope.hpp)
    uint32_t C = 0, lead = 0;   // channels; the largest delay rounded up to 8
    uint32_t D = 0;             // the largest delay itself
    bool rot = false;           // any channel with a step or a start phase: the rotating build, for every channel
    void *table = nullptr;      // the four planes, one allocation: head[C] | ray01[C] | ray23[C] | osc[C]
    std::vector<uint8_t> T;     // rays per channel (what mcrx_hip_userfade_set checks a user's entries against)
    bool fade = false;          // fading on: fplanes holds the sinusoids of every (channel, ray)
    uint32_t fade_L = 0, fade_S = 0;
    uint64_t fade_cap = 0;      // the most rows of the gain table a span may use
    void *fplanes = nullptr;    // one allocation: step[1 + S][4 C] (64-bit) | phase[1 + S][4 C] | coef[4 C]
    DevBuffer gtab;             // the gain table, float4 [row][channel][2]
    bool clock = false;         // a clock on: cplanes holds every user's integers and W
    uint32_t clk_max = 0;       // the configured max_delay
    uint64_t clk_span = 0;      // the most blocks of z a span computes (a multiple of 8)
    std::vector<mcrx_hip_userclock_user> clk_users;     // what a call's two ends are checked against
    void *cplanes = nullptr;    // one allocation: par[C][2] (16-byte words) | W[65][32]
    DevBuffer zbuf;             // z of a span, in the tiles' layout
};

static const size_t USERCHAN_MAX_GRANULES = (size_t)1 << 28;       // (lanes of a launch and the kernel's 32-bit block arithmetic)
static const size_t USERFADE_TABLE_BYTES = (size_t)64 << 20;       // the default cap of the gain table: 32 bytes a channel and row
static const size_t USERCLOCK_SPAN_BYTES = (size_t)64 << 20;       // the default cap of a span's z: 8 bytes a channel and block
static inline uint32_t round_up8(uint32_t v) { return (v + 7u) / 8u * 8u; }

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
    q->C = C; q->D = D; q->lead = round_up8(D); q->rot = rot;
    q->T.resize(C);
    for (uint32_t c = 0; c < C; c++) q->T[c] = (uint8_t)ch[c].num_rays;
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
    if (q->fplanes) (void)hipFree(q->fplanes);
    q->gtab.release();
    if (q->cplanes) (void)hipFree(q->cplanes);
    q->zbuf.release();
    delete q;
    return MCRX_OK;
}

extern "C" unsigned mcrx_hip_userchan_num_channels(mcrx_hip_userchan_t q) { return q ? q->C : 0u; }
extern "C" unsigned mcrx_hip_userclock_lead_blocks(mcrx_hip_userchan_t q) { return q && q->clock ? round_up8(q->clk_max + 16u) : 0u; }
extern "C" unsigned mcrx_hip_userchan_lead_blocks(mcrx_hip_userchan_t q)
{
    if (!q) return 0u;
    return q->clock ? round_up8(q->D + q->clk_max + 16u) : q->lead;
}

// table[r][channel][4] = G[first_row + r], r < rows (rows >= 1), on `st`
static void userfade_launch_gains(mcrx_hip_userchan_t q, long long first_row, uint32_t rows, float2 *table, hipStream_t st)
{
    UserfadeGainArgs g;
    const size_t lanes = (size_t)q->C * MCRX_USERCHAN_MAX_RAYS, terms = q->fade_S + 1;
    g.step = static_cast<const uint64_t *>(q->fplanes);
    g.phase = reinterpret_cast<const uint32_t *>(g.step + lanes * terms);
    g.coef = reinterpret_cast<const float2 *>(g.phase + lanes * terms);
    g.table = table; g.row0 = first_row; g.rows = rows; g.lanes = (uint32_t)lanes; g.L = q->fade_L; g.S = q->fade_S;
    hipLaunchKernelGGL(userchan_gain_kernel, dim3((unsigned)(((uint64_t)rows + USERFADE_CHUNK - 1u) / USERFADE_CHUNK), (unsigned)((lanes + 255) / 256)), dim3(256), 0, st, g);
}

// what every call on tiles is checked for (q not null); need_lead / lead_what: the least lead and the message below it
static const char *userchan_check_call(mcrx_hip_userchan_t q, const void *d_in, long long first_block, size_t nblocks, size_t lead_blocks,
                                       const void *d_out, size_t need_lead, const char *lead_what)
{
    if (!d_in || !d_out) return "null buffer";
    const uintptr_t pi = reinterpret_cast<uintptr_t>(d_in), po = reinterpret_cast<uintptr_t>(d_out);
    if ((pi & 15u) || (po & 15u)) return "d_in and d_out must be 16-byte aligned";
    if ((nblocks % 8) || (lead_blocks % 8) || (first_block % 8)) return "nblocks, lead_blocks and first_block come in granules of 8 blocks";
    if (lead_blocks < need_lead) return lead_what;
    if (nblocks / 8 > USERCHAN_MAX_GRANULES / q->C || lead_blocks > ((size_t)1 << 30)) return "at most 2^28 granules a call (and 2^30 blocks of lead)";
    const size_t bi = (lead_blocks + nblocks) * q->C * sizeof(float2), bo = nblocks * q->C * sizeof(float2);
    if (pi < po + bo && po < pi + bi) return "d_in and d_out overlap: the rays read behind the write front, in-place use is not possible";
    return nullptr;
}

// the operator of rays, gains, rotation and level on checked arguments (nblocks > 0): the kernels of a handle without a clock
static int userchan_run(mcrx_hip_userchan_t q, const void *d_in, long long first_block, size_t nblocks, size_t lead_blocks, void *d_out, hipStream_t st)
{
    UserchanArgs a = {};
    const uint32_t *t = static_cast<const uint32_t *>(q->table);
    a.head = reinterpret_cast<const uint4 *>(t);
    a.ray01 = reinterpret_cast<const float4 *>(t + (size_t)q->C * 4u);
    a.ray23 = reinterpret_cast<const float4 *>(t + (size_t)q->C * 8u);
    a.osc = reinterpret_cast<const uint2 *>(t + (size_t)q->C * 12u);
    a.C = q->C;
    a.lead = (uint32_t)lead_blocks;
    if (!q->fade) {
        a.in = static_cast<const float2 *>(d_in); a.out = static_cast<float4 *>(d_out);
        a.total = (uint32_t)(nblocks / 8 * q->C * 4u);
        a.first_lo = (uint32_t)(uint64_t)first_block;
        const dim3 grid((a.total + 255u) / 256u);
        if (q->rot) hipLaunchKernelGGL((userchan_kernel<true, false>), grid, dim3(256), 0, st, a);
        else        hipLaunchKernelGGL((userchan_kernel<false, false>), grid, dim3(256), 0, st, a);
        MCRX_OP_CHK(g_uc_err, hipGetLastError());
        return MCRX_OK;
    }
    // fading: spans of at most cap - 1 grid intervals (span_plan.hpp, on the signed block index), gain kernel -> main kernel each.  The
    // operator is a function of the absolute block index, so the spans are invisible in the output; a span ends on a grid row or with
    // the call, both multiples of 8 blocks.
    const uint32_t L = q->fade_L;
    const size_t row_bytes = (size_t)q->C * 2u * sizeof(float4);
    const uint64_t cap = span_cap(span_rows(span_frac(first_block, L), nblocks, L), q->fade_cap), have = q->gtab.bytes / row_bytes;
    if (cap > have) MCRX_OP_CHK(g_uc_err, q->gtab.ensure((size_t)span_grow(have, q->fade_cap, cap) * row_bytes));
    a.gtab = q->gtab.as<float4>(); a.L = L; a.finv = std::ldexp(1.0f, -(int)L);
    for (size_t off = 0; off < nblocks; ) {
        const long long pos = first_block + (long long)off;
        const Span<long long> s = span_next(pos, nblocks - off, L, cap);
        const size_t m = (size_t)s.m;
        userfade_launch_gains(q, s.row0, (uint32_t)s.rows, q->gtab.as<float2>(), st);
        MCRX_OP_CHK(g_uc_err, hipGetLastError());
        a.in = static_cast<const float2 *>(d_in) + off * q->C; a.out = static_cast<float4 *>(d_out) + off * q->C / 2u;
        a.total = (uint32_t)(m / 8 * q->C * 4u);
        a.first_lo = (uint32_t)(uint64_t)pos; a.frac0 = (uint32_t)s.frac;
        const dim3 grid((a.total + 255u) / 256u);
        if (q->rot) hipLaunchKernelGGL((userchan_kernel<true, true>), grid, dim3(256), 0, st, a);
        else        hipLaunchKernelGGL((userchan_kernel<false, true>), grid, dim3(256), 0, st, a);
        MCRX_OP_CHK(g_uc_err, hipGetLastError());
        off += m;
    }
    return MCRX_OK;
}

static bool userclock_check_range(mcrx_hip_userchan_t q, long long first_block, size_t nblocks, uint32_t D);
static int userclock_launch(mcrx_hip_userchan_t q, const float2 *in, long long first_block, size_t nblocks, size_t lead_blocks, uint32_t skip,
                            float2 *out, hipStream_t st);

extern "C" int mcrx_hip_userchan_apply_tiles(mcrx_hip_userchan_t q, const void *d_in, long long first_block, size_t nblocks,
                                             size_t lead_blocks, void *d_out, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_uc_err = "null handle"; return MCRX_EINVAL; }
    const char *bad = userchan_check_call(q, d_in, first_block, nblocks, lead_blocks, d_out, mcrx_hip_userchan_lead_blocks(q),
                                          q->clock ? "lead_blocks is below the largest delay + max_delay + 16 rounded up to 8 (mcrx_hip_userchan_lead_blocks)"
                                                   : "lead_blocks is below the handle's largest delay rounded up to 8 (mcrx_hip_userchan_lead_blocks)");
    if (bad) { g_uc_err = bad; return MCRX_EINVAL; }
    if (nblocks == 0) return MCRX_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!q->clock) return userchan_run(q, d_in, first_block, nblocks, lead_blocks, d_out, st);
    // a clock on: spans of at most clk_span blocks, clock kernel -> z (with the rays' lead in front) -> the operator on z.  Both are
    // functions of the absolute block index, so the spans are invisible in the output.  z in front of block first - D is not read.
    if (!userclock_check_range(q, first_block, nblocks, q->D)) return MCRX_EINVAL;
    const size_t lz = q->lead, lead_in = lead_blocks - lz;                 // (lead_blocks >= D + max_delay + 16: z of block first - D has its window)
    const uint64_t span = nblocks < q->clk_span ? nblocks : q->clk_span;
    MCRX_OP_CHK(g_uc_err, q->zbuf.ensure((size_t)(lz + span) * q->C * sizeof(float2)));
    for (size_t off = 0; off < nblocks; ) {
        const size_t m = nblocks - off < span ? nblocks - off : (size_t)span;
        const long long pos = first_block + (long long)off;
        int rc = userclock_launch(q, static_cast<const float2 *>(d_in) + off * q->C, pos - (long long)lz, lz + m, lead_in, (uint32_t)lz - q->D, q->zbuf.as<float2>(), st);
        if (rc == MCRX_OK) rc = userchan_run(q, q->zbuf.ptr, pos, m, lz, static_cast<float2 *>(d_out) + off * q->C, st);
        if (rc != MCRX_OK) return rc;
        off += m;
    }
    return MCRX_OK;
}

// ---- fading rays per user (mcrx_hip_userfade_*) ----
static const char *userfade_check_config(const mcrx_hip_userfade_config *f)
{
    if (f->struct_size != sizeof(mcrx_hip_userfade_config)) return "mcrx_hip_userfade_config: wrong struct_size";
    if (f->user_struct_size != sizeof(mcrx_hip_userfade_user)) return "mcrx_hip_userfade_user: wrong user_struct_size";
    if (f->log2_block < MCRX_USERFADE_MIN_LOG2_BLOCK || f->log2_block > MCRX_USERFADE_MAX_LOG2_BLOCK) return "log2_block must be 3 .. 20";
    if (f->num_sinusoids < 1 || f->num_sinusoids > MCRX_CHANEMU_MAX_SINUSOIDS) return "num_sinusoids must be 1 .. 16";
    if (f->table_rows == 1) return "table_rows must be 0 (default) or at least 2";
    return nullptr;
}

// rays [ray0, ray1) of one user against the update interval (users who do not fade are not looked at)
static const char *userfade_check_user(const mcrx_hip_userfade_config *f, const mcrx_hip_userfade_user *u, unsigned ray0, unsigned ray1)
{
    if (!u->enabled) return nullptr;
    const double B = (double)(1u << f->log2_block);
    for (unsigned i = ray0; i < ray1; i++)
        if (const char *bad = fade_ray_check(B, u->doppler[i], u->los_doppler[i], u->rice_k[i])) return bad;
    return nullptr;
}

// the integers and coefficients of one ray of a checked user: entry 0 the line-of-sight term, then the S scattered sinusoids
static void userfade_ray(const mcrx_hip_userfade_config *f, const mcrx_hip_userfade_user *u, unsigned i, int64_t *steps, uint32_t *phases, float coef[2])
{
    if (!u->enabled) {                                                  // G = (1, 0): the ray as it is without fading
        for (uint32_t k = 0; k <= f->num_sinusoids; k++) { steps[k] = 0; phases[k] = 0; }
        coef[0] = 1.f; coef[1] = 0.f;
        return;
    }
    fade_ray_integers(f->seed, i, 2u, u->id, f->num_sinusoids, u->doppler[i], u->los_doppler[i], u->rice_k[i], u->los_phase[i], steps, phases, coef);
}

extern "C" int mcrx_hip_userfade_selftest(const mcrx_hip_userfade_config *f, const mcrx_hip_userfade_user *u, unsigned ray, int64_t *steps,
                                          uint32_t *phases, float coef[2])
{
    if (!f || !u || !steps || !phases || !coef) { g_uc_err = "null pointer"; return MCRX_EINVAL; }
    if (ray >= MCRX_USERCHAN_MAX_RAYS) { g_uc_err = "ray must be 0 .. 3"; return MCRX_EINVAL; }
    const char *bad = userfade_check_config(f);
    if (!bad) bad = userfade_check_user(f, u, ray, ray + 1);
    if (bad) { g_uc_err = bad; return MCRX_EINVAL; }
    userfade_ray(f, u, ray, steps, phases, coef);
    return MCRX_OK;
}

extern "C" int mcrx_hip_userfade_on(mcrx_hip_userchan_t q) { return q && q->fade ? 1 : 0; }

extern "C" int mcrx_hip_userfade_set(mcrx_hip_userchan_t q, const mcrx_hip_userfade_config *f, const mcrx_hip_userfade_user *users)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_uc_err = "null handle"; return MCRX_EINVAL; }
    if (!f) {                                                           // off: the planes and the table go with the handle
        MCRX_OP_CHK(g_uc_err, hipDeviceSynchronize());
        q->fade = false;
        return MCRX_OK;
    }
    if (!users) { g_uc_err = "null user table"; return MCRX_EINVAL; }
    const char *bad = userfade_check_config(f);
    for (uint32_t c = 0; c < q->C && !bad; c++) bad = userfade_check_user(f, &users[c], 0, q->T[c]);
    if (bad) { g_uc_err = bad; return MCRX_EINVAL; }
    // the planes on the host: [term][lane], lane = channel * 4 + ray; rays a channel does not have are static ones
    const uint32_t S = f->num_sinusoids, terms = S + 1;
    const size_t lanes = (size_t)q->C * MCRX_USERCHAN_MAX_RAYS;
    const size_t bytes = lanes * terms * (sizeof(uint64_t) + sizeof(uint32_t)) + lanes * sizeof(float2);
    std::vector<uint64_t> host((bytes + 7) / 8, 0);
    uint64_t *step = host.data();
    uint32_t *phase = reinterpret_cast<uint32_t *>(step + lanes * terms);
    float *coef = reinterpret_cast<float *>(phase + lanes * terms);
    mcrx_hip_userfade_user none = {};
    for (uint32_t c = 0; c < q->C; c++)
        for (uint32_t i = 0; i < MCRX_USERCHAN_MAX_RAYS; i++) {
            int64_t st[USERFADE_TERMS]; uint32_t ph[USERFADE_TERMS]; float co[2];
            userfade_ray(f, i < q->T[c] ? &users[c] : &none, i, st, ph, co);
            const size_t lane = (size_t)c * MCRX_USERCHAN_MAX_RAYS + i;
            for (uint32_t k = 0; k < terms; k++) { step[k * lanes + lane] = (uint64_t)st[k]; phase[k * lanes + lane] = ph[k]; }
            coef[lane * 2] = co[0]; coef[lane * 2 + 1] = co[1];
        }
    MCRX_OP_CHK(g_uc_err, hipDeviceSynchronize());                                      // calls in flight read the planes about to go
    void *planes = nullptr;
    MCRX_OP_CHK(g_uc_err, hipMalloc(&planes, bytes));
    hipError_t e = hipMemcpy(planes, host.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(planes); g_uc_err = std::string("fading planes: ") + hipGetErrorString(e); return MCRX_EHIP; }
    if (q->fplanes) (void)hipFree(q->fplanes);
    q->fplanes = planes;
    q->fade_L = f->log2_block; q->fade_S = S;
    const uint64_t fit = USERFADE_TABLE_BYTES / ((size_t)q->C * 2u * sizeof(float4));
    q->fade_cap = f->table_rows ? f->table_rows : fit;
    q->fade = true;
    return MCRX_OK;
}

// the gain kernel on its own, into the caller's buffer: what apply_tiles computes for itself, for tests and measurements
extern "C" int mcrx_hip_userfade_gains(mcrx_hip_userchan_t q, long long first_row, uint32_t rows, void *d_table, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_uc_err = "null handle"; return MCRX_EINVAL; }
    if (!q->fade) { g_uc_err = "fading is off"; return MCRX_EINVAL; }
    if (!d_table || (reinterpret_cast<uintptr_t>(d_table) & 15u)) { g_uc_err = "d_table must be a 16-byte aligned device buffer"; return MCRX_EINVAL; }
    if (rows == 0) return MCRX_OK;
    userfade_launch_gains(q, first_row, rows, static_cast<float2 *>(d_table), (hipStream_t)stream);
    MCRX_OP_CHK(g_uc_err, hipGetLastError());
    return MCRX_OK;
}

// ---- each user's own sample clock and fractional timing (mcrx_hip_userclock_*) ----
static const char *userclock_check_config(const mcrx_hip_userclock_config *f)
{
    if (f->struct_size != sizeof(mcrx_hip_userclock_config)) return "mcrx_hip_userclock_config: wrong struct_size";
    if (f->user_struct_size != sizeof(mcrx_hip_userclock_user)) return "mcrx_hip_userclock_user: wrong user_struct_size";
    if (f->max_delay < MCRX_USERCLOCK_MIN_DELAY || f->max_delay > MCRX_USERCLOCK_MAX_DELAY) return "max_delay must be 15 .. 255";
    if (f->span_blocks % 8u) return "span_blocks must be 0 (default) or a multiple of 8";
    return nullptr;
}

static const char *userclock_check_user(uint32_t max_delay, const mcrx_hip_userclock_user *u)
{
    if (!u->enabled) return nullptr;
    if (u->sco > ((int64_t)1 << 38) || u->sco < -((int64_t)1 << 38)) return "|sco| exceeds 2^38";
    const uint64_t n = u->delay_fp >> 32;
    if (n < MCRX_USERCLOCK_MIN_DELAY || n > max_delay) return "delay_fp: the whole samples of the delay lie outside [15, max_delay]";
    return nullptr;
}

// tau_fp of a checked, enabled user at block b: nullptr, or what is wrong there
static const char *userclock_at(uint32_t max_delay, const mcrx_hip_userclock_user *u, long long b, int64_t *tau_fp)
{
    long long d, p;
    if (__builtin_sub_overflow(b, (long long)u->origin, &d) || __builtin_mul_overflow((long long)u->sco, d, &p)) return "sco * (block - origin) leaves int64";
    const int64_t tau = (int64_t)u->delay_fp + ((int64_t)p >> 16);      // (delay_fp < 2^40, the shifted product < 2^47)
    const int64_t n = tau >> 32;
    if (n < MCRX_USERCLOCK_MIN_DELAY || n > (int64_t)max_delay) return "the whole samples of the delay leave [15, max_delay]";
    *tau_fp = tau;
    return nullptr;
}

// the two ends of a call -- blocks first_block - D and first_block + nblocks - 1 (nblocks > 0) -- for every user with a clock
static bool userclock_check_range(mcrx_hip_userchan_t q, long long first_block, size_t nblocks, uint32_t D)
{
    long long ends[2];
    if (__builtin_sub_overflow(first_block, (long long)D, &ends[0]) || __builtin_add_overflow(first_block, (long long)(nblocks - 1), &ends[1])) {
        g_uc_err = "the call's blocks leave int64";
        return false;
    }
    for (uint32_t c = 0; c < q->C; c++) {
        if (!q->clk_users[c].enabled) continue;
        for (int e = 0; e < 2; e++) {
            int64_t tau;
            const char *bad = userclock_at(q->clk_max, &q->clk_users[c], ends[e], &tau);
            if (bad) { g_uc_err = "channel " + std::to_string(c) + ", block " + std::to_string(ends[e]) + ": " + bad; return false; }
        }
    }
    return true;
}

// z of blocks [first_block, first_block + nblocks) into out (the tiles' layout), blocks below `skip` of them as zeros
static int userclock_launch(mcrx_hip_userchan_t q, const float2 *in, long long first_block, size_t nblocks, size_t lead_blocks, uint32_t skip,
                            float2 *out, hipStream_t st)
{
    UserclockArgs a;
    a.in = in; a.out = reinterpret_cast<float4 *>(out);
    a.par = static_cast<const uint4 *>(q->cplanes);
    a.W = reinterpret_cast<const float *>(a.par + (size_t)q->C * 2u);
    a.first = first_block; a.C = q->C; a.tiles = (uint32_t)(nblocks / 8);
    a.lead = (uint32_t)lead_blocks; a.in_rows = (uint32_t)((lead_blocks + nblocks) / 8); a.skip = skip;
    const dim3 grid((unsigned)((nblocks + UCLK_BLOCKS - 1u) / UCLK_BLOCKS), (q->C + UCLK_CH - 1u) / UCLK_CH);
    hipLaunchKernelGGL(userclock_kernel, grid, dim3(256), 0, st, a);
    MCRX_OP_CHK(g_uc_err, hipGetLastError());
    return MCRX_OK;
}

extern "C" int mcrx_hip_userclock_on(mcrx_hip_userchan_t q) { return q && q->clock ? 1 : 0; }

extern "C" int mcrx_hip_userclock_table(float *W)
{
    if (!W) { g_uc_err = "null pointer"; return MCRX_EINVAL; }
    const float *t = userclock_table();
    for (int i = 0; i < (MCRX_USERCLOCK_PHASES + 1) * MCRX_USERCLOCK_TAPS; i++) W[i] = t[i];
    return MCRX_OK;
}

extern "C" int mcrx_hip_userclock_selftest(const mcrx_hip_userclock_config *f, const mcrx_hip_userclock_user *u, long long block, int64_t *tau_fp, float *h)
{
    if (!f || !u || !tau_fp || !h) { g_uc_err = "null pointer"; return MCRX_EINVAL; }
    const char *bad = userclock_check_config(f);
    if (!bad) bad = userclock_check_user(f->max_delay, u);
    int64_t tau = 0;
    if (!bad && u->enabled) bad = userclock_at(f->max_delay, u, block, &tau);
    if (bad) { g_uc_err = bad; return MCRX_EINVAL; }
    *tau_fp = tau;
    if (!u->enabled) {                                                  // z = x: n = 0 in the definition's indexing
        for (int j = 0; j < MCRX_USERCLOCK_TAPS; j++) h[j] = j == 15 ? 1.f : 0.f;
        return MCRX_OK;
    }
    const uint32_t mu = (uint32_t)(uint64_t)tau, r = mu >> 26;
    const float fr = (float)((mu >> 2) & 0xffffffu) * 0x1p-24f;
    const float *w0 = userclock_table() + r * MCRX_USERCLOCK_TAPS, *w1 = w0 + MCRX_USERCLOCK_TAPS;
    for (int j = 0; j < MCRX_USERCLOCK_TAPS; j++) h[j] = userclock_coef(w0[j], w1[j], fr);
    return MCRX_OK;
}

extern "C" int mcrx_hip_userclock_set(mcrx_hip_userchan_t q, const mcrx_hip_userclock_config *f, const mcrx_hip_userclock_user *users)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_uc_err = "null handle"; return MCRX_EINVAL; }
    if (!f) {                                                           // off: the planes and the buffer go with the handle
        MCRX_OP_CHK(g_uc_err, hipDeviceSynchronize());
        q->clock = false;
        return MCRX_OK;
    }
    if (!users) { g_uc_err = "null user table"; return MCRX_EINVAL; }
    const char *bad = userclock_check_config(f);
    for (uint32_t c = 0; c < q->C && !bad; c++) {
        bad = userclock_check_user(f->max_delay, &users[c]);
        if (bad) { g_uc_err = "channel " + std::to_string(c) + ": " + bad; return MCRX_EINVAL; }
    }
    if (bad) { g_uc_err = bad; return MCRX_EINVAL; }
    // the planes on the host: 32 bytes a channel, then W.  A user without a clock keeps the window of n = 15 (the kernel copies x)
    const size_t words = (size_t)q->C * 4u, wn = (size_t)(MCRX_USERCLOCK_PHASES + 1) * MCRX_USERCLOCK_TAPS;
    const size_t bytes = words * sizeof(uint64_t) + wn * sizeof(float);
    std::vector<uint64_t> host((bytes + 7) / 8, 0);
    for (uint32_t c = 0; c < q->C; c++) {
        const mcrx_hip_userclock_user &u = users[c];
        uint64_t *w = host.data() + (size_t)c * 4u;
        if (u.enabled) { w[0] = u.delay_fp; w[1] = (uint64_t)u.sco; w[2] = (uint64_t)u.origin; w[3] = 1u; }
        else           { w[0] = (uint64_t)MCRX_USERCLOCK_MIN_DELAY << 32; w[1] = w[2] = w[3] = 0; }
    }
    std::memcpy(host.data() + words, userclock_table(), wn * sizeof(float));
    MCRX_OP_CHK(g_uc_err, hipDeviceSynchronize());                                      // calls in flight read the planes about to go
    void *planes = nullptr;
    MCRX_OP_CHK(g_uc_err, hipMalloc(&planes, bytes));
    hipError_t e = hipMemcpy(planes, host.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(planes); g_uc_err = std::string("clock planes: ") + hipGetErrorString(e); return MCRX_EHIP; }
    if (q->cplanes) (void)hipFree(q->cplanes);
    q->cplanes = planes;
    q->clk_users.assign(users, users + q->C);
    q->clk_max = f->max_delay;
    const uint64_t fit = USERCLOCK_SPAN_BYTES / ((size_t)q->C * sizeof(float2)) / UCLK_BLOCKS * UCLK_BLOCKS;
    q->clk_span = f->span_blocks ? f->span_blocks : fit;
    q->clock = true;
    return MCRX_OK;
}

// the clock kernel on its own, into the caller's buffer: what apply_tiles computes for itself, for tests and measurements
extern "C" int mcrx_hip_userclock_apply_tiles(mcrx_hip_userchan_t q, const void *d_in, long long first_block, size_t nblocks,
                                              size_t lead_blocks, void *d_out, void *stream)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_uc_err = "null handle"; return MCRX_EINVAL; }
    if (!q->clock) { g_uc_err = "the clock is off"; return MCRX_EINVAL; }
    const char *bad = userchan_check_call(q, d_in, first_block, nblocks, lead_blocks, d_out, mcrx_hip_userclock_lead_blocks(q),
                                          "lead_blocks is below max_delay + 16 rounded up to 8 (mcrx_hip_userclock_lead_blocks)");
    if (bad) { g_uc_err = bad; return MCRX_EINVAL; }
    if (nblocks == 0) return MCRX_OK;
    if (!userclock_check_range(q, first_block, nblocks, 0u)) return MCRX_EINVAL;
    return userclock_launch(q, static_cast<const float2 *>(d_in), first_block, nblocks, lead_blocks, 0u, static_cast<float2 *>(d_out), (hipStream_t)stream);
}
