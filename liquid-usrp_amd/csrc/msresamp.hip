// msresamp.hip -- multi-stage arbitrary resampler (decimating front end, rate <= 1; interpolating, rate > 1) for gfx950.
//
// Replaces liquid's msresamp_crcf as the reference applications use it in front of a
// synchronizer (pattern: src/flexframe_rx.cc:179 `msresamp_crcf_create(rate, 60.0f)`,
// :240 `msresamp_crcf_execute(q, in, nin, out, &nout)`; rate computed like
// src/multichannel_rx.cc:129-138).  Structure (liquid msresamp / resamp2 / resamp):
//   * half-band decimators while rate < 0.5 (4m+1 = 29-tap Kaiser half-band, m = 7):
//       y[k] = 0.5 * ( x[2k-13] + sum_{i<14} h1[i] * x[2(k-13+i)] )
//   * a 256-branch polyphase arbitrary resampler (14 taps per branch, fc = min(0.515 r, 0.49))
//     stepped by a 24-bit fixed-point phase: output j comes from input n_j = (j*step) >> 24 with
//     branch b_j = ((j*step) mod 2^24) >> 16:   y[j] = sum_{k<14} H[b_j][k] * x[n_j-13+k]
// Interpolating (rate > 1, the transmit applications' msresamp_crcf_create(2.0, 60), src/flexframe_tx.cc:170): the
// arbitrary stage first (rate in (1, 2]: same closed form, step < 2^24), then half-band interpolators while rate > 2:
//       v[2k] = u[k-7],   v[2k+1] = sum_{i<14} h1[i] * u[k-13+i]
// Every output is a closed form of its index, so each stage is one embarrassingly parallel
// kernel (64-bit integer phase, exact); overlapping 14/27-sample windows are served by L1/L2.
// Streaming state = sample counters on the host + retained tails of each stage buffer.  The counters are NOT absolute for ever:
// the phase j * step is a 64-bit product with 24 fractional bits, so it wraps once the arbitrary stage's input index reaches 2^40
// (three hours of a 100 Msample/s stream).  The phase repeats exactly every step / g inputs = 2^24 / g outputs of that stage
// (g = gcd(step, 2^24)); before every call the host takes whole periods off every counter (rs_rebase), which changes no bit of
// any output and keeps the kernels' indices below a period plus the samples the stage buffers still hold.
#include "../../include/mcrx_hip.h"
#include "design.hpp"
#include "devscope.hpp"
#include "resamp_plan.hpp"
#include "sc16.hpp"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace mcrx;

#define RS_M 7
#define RS_TAPS (2 * RS_M)          // taps per polyphase branch / half-band filter branch
#define RS_NPFB 256
#define RS_PHASE_BITS 24
#define RS_KEEP 64                  // samples of history retained per stage (>= 27; >= 54 where the last half-band stage is folded into the arbitrary one)

#define RS_OB 1024                  // outputs per workgroup (256 threads x 4)
#define RS_HROW 16                  // floats per row of the padded branch table (14 taps + 2): one row = 4 x 16-B loads
static_assert(RS_M == RSP_M && RS_TAPS == RSP_TAPS && RS_NPFB == RSP_NPFB && RS_PHASE_BITS == RSP_PHASE_BITS, "resamp_plan.hpp plans for these kernels");

// Input formats of the caller's buffer (template parameter FMT of the kernels that can be a first stage; msresamp_hip_set_input_format):
// IQ_CF32 / IQ_SC16, an sc16 sample as sc16.hpp defines it.  The word stays packed from the load to the store
// into the LDS span (rs_cvt), half the bytes and half the registers of a cf32 sample in flight; behind that store the source is the
// cf32 build's, so that the two formats share every later rounding.  Only the caller's buffer and its retained tail (in[0]) are in
// the handle's format: every later stage buffer is cf32.
// Output formats of the caller's buffer (msresamp_hip_set_output_format), in the kernels that can be a last stage.
// Let y be the fp32 value the stage computes for one component.  The store to the caller's buffer is v = y * gain (one multiply of its
// own; gain = 1 stores y) as cf32, or Q(v) as sc16: the shared quantiser and clip count (sc16.hpp), one packed 4-byte word
// a sample.  Only that store knows the format: stage buffers between the kernels are cf32 and are written with gain = 1.
// In the builds that can store sc16 (template parameter SC16) the format is a run-time choice at the store (clip != NULL: sc16), inside
// one body that keeps the cf32 store, as in txgen.hip's txfir_column and for its reason: a build that ended in the 4-byte store alone
// contracted the multiply-adds of the tap sums differently from its cf32 twin (more than half of them left as a multiply and an add),
// and Q is a function of the cf32 value only if that value is the same.  With both stores in the body the sums compile to the cf32
// build's fused multiply-adds.  The builds without SC16 are the cf32 handles': no branch, no clip count, the parent's registers.
template <int FMT> struct RsElem { typedef float2 type; };
template <> struct RsElem<IQ_SC16> { typedef uint32_t type; };

// A stage input: samples [tail_base, cur_base) in `tail` (the retained end of the previous call's input, may be NULL),
// [cur_base, end) in `cur`; everything before sample 0 is zero.
template <int FMT> struct RsInT { const typename RsElem<FMT>::type *tail; long long tail_base; const typename RsElem<FMT>::type *cur; long long cur_base, end; };
typedef RsInT<IQ_CF32> RsIn;

__device__ __forceinline__ float2 rs_cvt(float2 v) { return v; }
__device__ __forceinline__ float2 rs_cvt(uint32_t w) { return sc16_unpack(w); }
template <int FMT> __device__ __forceinline__ typename RsElem<FMT>::type rs_zero()
{
    if constexpr (FMT == IQ_SC16) return 0u; else return make_float2(0.f, 0.f);
}

// sample t as it lies in memory (sc16: the packed word; the zero word is the zero sample)
template <int FMT> __device__ __forceinline__ typename RsElem<FMT>::type rs_fetch(const RsInT<FMT> &s, long long t)
{
    if (t >= s.cur_base) return t < s.end ? s.cur[t - s.cur_base] : rs_zero<FMT>();
    if (s.tail && t >= s.tail_base && t >= 0) return s.tail[t - s.tail_base];
    return rs_zero<FMT>();
}

// Half-band decimator, outputs k in [k0, k1) -> out[k - k0].  A workgroup stages the 2 x (1024 + 13) input samples of
// its 1024 outputs in LDS, de-interleaved (the filter branch reads even samples, the delay branch odd ones), with
// coalesced loads; every thread then makes 4 outputs from conflict-free LDS reads.  HBM: 8 B in + 4 B out per input sample
// (4 B in where it is the first stage of an sc16 handle: FMT, converted on the way into LDS).
template <int FMT>
__global__ __launch_bounds__(256) void halfband_kernel(RsInT<FMT> in, float2 *out, long long k0, long long k1, const float *h1)
{
    __shared__ float2 ev[RS_OB + RS_TAPS], od[RS_OB + RS_TAPS];
    const long long kb = k0 + (long long)blockIdx.x * RS_OB;
    const int tid = threadIdx.x;
    const long long tb = 2 * (kb - (RS_TAPS - 1));          // sample behind ev[0]
    const int np = (int)min((long long)RS_OB, k1 - kb) + RS_TAPS - 1;
    for (int p = tid; p < np; p += 256) {
        ev[p] = rs_cvt(rs_fetch(in, tb + 2 * p));
        od[p] = rs_cvt(rs_fetch(in, tb + 2 * p + 1));
    }
    __syncthreads();
    float h[RS_TAPS];
#pragma unroll
    for (int i = 0; i < RS_TAPS; i++) h[i] = h1[i];
#pragma unroll
    for (int r = 0; r < RS_OB / 256; r++) {
        const int o = tid + 256 * r;
        const long long k = kb + o;
        if (k >= k1) break;
        float2 acc = make_float2(0.f, 0.f);
#pragma unroll
        for (int i = 0; i < RS_TAPS; i++) { const float2 v = ev[o + i]; acc.x += h[i] * v.x; acc.y += h[i] * v.y; }
        const float2 d = od[o + RS_M - 1];                  // x[2k-13]
        out[k - k0] = make_float2(0.5f * (d.x + acc.x), 0.5f * (d.y + acc.y));
    }
}

// Half-band interpolator: inputs k in [k0, k1) -> outputs 2k, 2k+1 at out[2 (k - k0)]
// SC16 and clip != NULL, sc16 (only where `out` is the caller's buffer): the pair is two packed words, stored as one 8-byte word where `out` is 8-byte
// aligned and as two 4-byte stores where it is not -- pair p lies at out + 8 p bytes, so the choice is the same for every lane of a
// launch.  The clip count stays in a lane register and leaves once per wave, behind the loop and its per-lane break.
template <bool SC16>
__global__ __launch_bounds__(256) void halfband_interp_kernel(RsIn in, float2 *out, long long k0, long long k1, const float *h1, float gain,
                                                              unsigned long long *clip)
{
    __shared__ float2 x[RS_OB + RS_TAPS];
    const long long kb = k0 + (long long)blockIdx.x * RS_OB;
    const int tid = threadIdx.x;
    const int np = (int)min((long long)RS_OB, k1 - kb) + RS_TAPS - 1;
    for (int p = tid; p < np; p += 256) x[p] = rs_fetch(in, kb - (RS_TAPS - 1) + p);
    __syncthreads();
    float h[RS_TAPS];
#pragma unroll
    for (int i = 0; i < RS_TAPS; i++) h[i] = h1[i];
    uint32_t nclip = 0;
    const bool pair8 = (reinterpret_cast<size_t>(out) & 7) == 0;
#pragma unroll
    for (int r = 0; r < RS_OB / 256; r++) {
        const int o = tid + 256 * r;
        const long long k = kb + o;
        if (k >= k1) break;
        float2 acc = make_float2(0.f, 0.f);
#pragma unroll
        for (int i = 0; i < RS_TAPS; i++) { const float2 v = x[o + i]; acc.x += h[i] * v.x; acc.y += h[i] * v.y; }
        const float2 d = x[o + RS_TAPS - 1 - RS_M];         // u[k-7]
        const float4 v = make_float4(d.x * gain, d.y * gain, acc.x * gain, acc.y * gain);
        if (SC16 && clip) {
            uint32_t *o32 = reinterpret_cast<uint32_t *>(out) + 2 * (k - k0);
            const uint32_t w0 = sc16_sample(v.x, v.y, nclip), w1 = sc16_sample(v.z, v.w, nclip);
            if (pair8) *reinterpret_cast<uint2 *>(o32) = make_uint2(w0, w1);
            else { o32[0] = w0; o32[1] = w1; }
        } else reinterpret_cast<float4 *>(out)[k - k0] = v;
    }
    if (SC16 && clip) sc16_clip_commit(clip, nclip);
}

// Arbitrary stage, outputs j in [j0, j1): input index and branch are closed forms of j (64-bit phase).  The input span
// of 1024 outputs (<= 2048 + 14 samples: step <= 2 samples per output) is staged in LDS; so is the branch table, TRANSPOSED
// (round 6): lane l's branch is b_0 + l * db mod 256 -- at any rate but 1/2, 1 and 2 every lane has a row of its own, and the
// four 16-byte loads per output that fetched it from the (cache-resident) table were 64 different lines per instruction: the
// stage ran at 28-32 % of HBM for r = 0.37, 0.8, 2.0 against 54 % at r = 0.5, where all lanes share a row
// (profiles/r2_resamp_roofline.csv).  With tap k of all 256 branches side by side in LDS (a pad word per 32 branches, so that
// the strides rational rates produce -- r = 0.8: branches 0, 64, 128, 192 -- do not pile onto one bank) a lane's 14 taps are 14
// four-byte LDS reads at lane-dependent addresses, conflict-free or nearly, and equal addresses broadcast.  A workgroup stages
// the table once and works through RS_CHUNKS chunks of 1024 outputs.
// FIXED (round 6): rates whose 24-bit step has no low 16 bits -- 1/2, 1, 2, 0.8, 1.25 ...: every rate k / 2^8 samples per output (the float
// nearest 0.64 is not one: its step is 26214401) --
// walk the branches with a period that divides 256, so a thread's outputs (1024 n + tid + 256 r) all use ONE branch: its 14 taps sit in
// registers for the whole workgroup and the table is not staged at all.
// Both builds request the next chunk's input span (global loads into registers) before they work on the current one.
// HB (round 6, rates below 1/2): the LAST half-band decimator is folded in -- `in` is THAT stage's input, and the samples the arbitrary
// stage reads, y[k] = 0.5 (u[2k-13] + sum_i h1[i] u[2(k-13+i)]), are formed in LDS from the staged raw span (even and odd samples apart,
// as in halfband_kernel) instead of travelling through HBM: at r = 0.37 the two kernels moved 8 + 4 + 4 + 3 = 19 bytes per input sample
// for 11 algorithmic ones.  Chunks of 512 outputs there (the raw span is twice the half-band span), 40 KB of LDS.
#define RS_CHUNKS 8
#define RS_HT_ROW (RS_NPFB + RS_NPFB / 32)
// SC16 and clip != NULL, sc16 (only where `out` is the caller's buffer): one packed 4-byte store per lane and output; the clip count stays in a lane
// register through all chunks and leaves once per wave at the end, behind the output loop's per-lane break (the exits in front of it,
// a workgroup without a chunk, are taken by whole workgroups).
template <bool FIXED, bool HB, int FMT, bool SC16>
__global__ __launch_bounds__(256) void arbitrary_kernel(RsInT<FMT> in, float2 *out, long long j0, long long j1,
                                                        unsigned long long step, const float *hpfb, const float *h1, float gain,
                                                        unsigned long long *clip)
{
    constexpr int RS_OBK = HB ? RS_OB / 2 : RS_OB;          // outputs per chunk
    constexpr int RS_SPAN = 2 * RS_OBK + RS_TAPS + 2;       // samples of the arbitrary stage's input behind a chunk (step <= 2 per output)
    constexpr int RS_SPANR = RS_SPAN + RS_TAPS;             // HB: (even, odd) pairs of raw samples behind those
    constexpr int RS_PER = ((HB ? RS_SPANR : RS_SPAN) + 255) / 256;
    constexpr int RS_PERY = (RS_SPAN + 255) / 256;
    __shared__ float2 x[RS_SPAN];
    __shared__ float2 ev[HB ? RS_SPANR : 1], od[HB ? RS_SPANR : 1];
    __shared__ float2 ht[FIXED ? 1 : (RS_TAPS / 2) * RS_HT_ROW];      // taps (2 k, 2 k + 1) of branch b at ht[k][b + b / 32]
    const int tid = threadIdx.x;
    float hh[HB ? RS_TAPS : 1];
    if constexpr (HB) {
#pragma unroll
        for (int i = 0; i < RS_TAPS; i++) hh[i] = h1[i];
    }
    float hfix[RS_TAPS];
    if constexpr (FIXED) {
        const unsigned long long P = (unsigned long long)(j0 + tid) * step;
        const unsigned bq = (unsigned)((P & ((1ull << RS_PHASE_BITS) - 1)) >> (RS_PHASE_BITS - 8));
        const float4 *hp = reinterpret_cast<const float4 *>(hpfb + (size_t)bq * RS_HROW);
        const float4 ha = hp[0], hb = hp[1], hc = hp[2], hd = hp[3];
        const float h[RS_HROW] = { ha.x, ha.y, ha.z, ha.w, hb.x, hb.y, hb.z, hb.w, hc.x, hc.y, hc.z, hc.w, hd.x, hd.y, hd.z, hd.w };
#pragma unroll
        for (int k = 0; k < RS_TAPS; k++) hfix[k] = h[k];
    } else {   // branch tid's row (16 floats, 14 used) -> column tid of the transposed table
        const float4 *hp = reinterpret_cast<const float4 *>(hpfb + (size_t)tid * RS_HROW);
        const float4 ha = hp[0], hb = hp[1], hc = hp[2], hd = hp[3];
        const float h[RS_HROW] = { ha.x, ha.y, ha.z, ha.w, hb.x, hb.y, hb.z, hb.w, hc.x, hc.y, hc.z, hc.w, hd.x, hd.y, hd.z, hd.w };
        const int bp = tid + (tid >> 5);
#pragma unroll
        for (int k = 0; k < RS_TAPS / 2; k++) ht[k * RS_HT_ROW + bp] = make_float2(h[2 * k], h[2 * k + 1]);
    }
    // chunk geometry: first input sample and span length of chunk c
    auto geom = [&](int c, long long &jb, long long &je, long long &nf, int &np) -> bool {
        jb = j0 + ((long long)blockIdx.x * RS_CHUNKS + c) * RS_OBK;
        if (c >= RS_CHUNKS || jb >= j1) return false;
        je = min(jb + (long long)RS_OBK, j1);
        nf = (long long)(((unsigned long long)jb * step) >> RS_PHASE_BITS);
        const long long nl = (long long)(((unsigned long long)(je - 1) * step) >> RS_PHASE_BITS);
        np = (int)(nl - nf) + RS_TAPS;
        return true;
    };
    typedef typename RsElem<FMT>::type elem_t;              // a sample as fetched: it waits in registers in the caller's format
    elem_t pre[RS_PER], pro[HB ? RS_PER : 1];
    auto fetch = [&](long long nf, int np) {
        if constexpr (HB) {     // y[nf - 13 + p], p < np, read raw pairs q < np + 13 from sample tb = 2 (nf - 26) on
            const long long tb = 2 * (nf - 2 * (RS_TAPS - 1));
            const int nq = np + RS_TAPS - 1;
            // inside the new samples, on a 16-byte boundary (all chunks but a call's first and last, while calls are even-sized): one
            // 16-byte load per (even, odd) pair, whole lines per instruction
            // (sc16: a pair is 8 bytes, and what has to line up is the pair's own address -- a buffer that is only 4-byte aligned takes
            //  this path whenever tb falls on an odd sample of it)
            bool whole = tb >= in.cur_base && tb + 2 * (long long)nq <= in.end;
            if constexpr (FMT == IQ_SC16) whole = whole && ((reinterpret_cast<size_t>(in.cur + (tb - in.cur_base)) & 7) == 0);
            else whole = whole && (((tb - in.cur_base) & 1) == 0) && ((reinterpret_cast<size_t>(in.cur) & 15) == 0);
            if (whole) {
                if constexpr (FMT == IQ_SC16) {
                    const uint2 *src = reinterpret_cast<const uint2 *>(in.cur + (tb - in.cur_base));
#pragma unroll
                    for (int i = 0; i < RS_PER; i++) {
                        const int q = tid + 256 * i;
                        const uint2 v = src[q < nq ? q : 0];
                        pre[i] = v.x; pro[i] = v.y;
                    }
                } else {
                    const float4 *src = reinterpret_cast<const float4 *>(in.cur + (tb - in.cur_base));
#pragma unroll
                    for (int i = 0; i < RS_PER; i++) {
                        const int q = tid + 256 * i;
                        const float4 v = src[q < nq ? q : 0];
                        pre[i] = make_float2(v.x, v.y); pro[i] = make_float2(v.z, v.w);
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < RS_PER; i++) {
                    const int q = tid + 256 * i;
                    const bool on = q < nq;
                    pre[i] = on ? rs_fetch(in, tb + 2 * q) : rs_zero<FMT>();
                    pro[i] = on ? rs_fetch(in, tb + 2 * q + 1) : rs_zero<FMT>();
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < RS_PER; i++) { const int p = tid + 256 * i; pre[i] = p < np ? rs_fetch(in, nf - (RS_TAPS - 1) + p) : rs_zero<FMT>(); }
        }
    };
    long long jb, je, nf; int np;
    uint32_t nclip = 0;
    if (!geom(0, jb, je, nf, np)) return;
    fetch(nf, np);
    for (int c = 0; c < RS_CHUNKS; c++) {
        __syncthreads();                                     // (the previous chunk's reads of x; the table's writes)
        if constexpr (HB) {
#pragma unroll
            for (int i = 0; i < RS_PER; i++) { const int q = tid + 256 * i; if (q < np + RS_TAPS - 1) { ev[q] = rs_cvt(pre[i]); od[q] = rs_cvt(pro[i]); } }
        } else {
#pragma unroll
            for (int i = 0; i < RS_PER; i++) { const int p = tid + 256 * i; if (p < np) x[p] = rs_cvt(pre[i]); }
        }
        __syncthreads();
        const long long cjb = jb, cje = je, cnf = nf;
        const int cnp = np;
        const bool more = geom(c + 1, jb, je, nf, np);
        if (more) fetch(nf, np);                             // in flight while this chunk is worked on
        if constexpr (HB) {     // the half-band stage's outputs behind this chunk (same arithmetic as halfband_kernel)
#pragma unroll
            for (int r = 0; r < RS_PERY; r++) {
                const int p = tid + 256 * r;
                if (p < cnp) {
                    float2 acc = make_float2(0.f, 0.f);
#pragma unroll
                    for (int i = 0; i < RS_TAPS; i++) { const float2 v = ev[p + i]; acc.x += hh[i] * v.x; acc.y += hh[i] * v.y; }
                    const float2 d = od[p + RS_M - 1];
                    x[p] = make_float2(0.5f * (d.x + acc.x), 0.5f * (d.y + acc.y));
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < RS_OBK / 256; r++) {
            const long long j = cjb + tid + 256 * r;
            if (j >= cje) break;
            const unsigned long long P = (unsigned long long)j * step;
            const int o = (int)((long long)(P >> RS_PHASE_BITS) - cnf);
            float2 acc = make_float2(0.f, 0.f);
            if constexpr (FIXED) {
#pragma unroll
                for (int k = 0; k < RS_TAPS; k++) { const float2 v = x[o + k]; acc.x += hfix[k] * v.x; acc.y += hfix[k] * v.y; }
            } else {
                const unsigned bq = (unsigned)((P & ((1ull << RS_PHASE_BITS) - 1)) >> (RS_PHASE_BITS - 8));
                const float2 *hcol = ht + bq + (bq >> 5);
#pragma unroll
                for (int k = 0; k < RS_TAPS / 2; k++) {
                    const float2 h = hcol[k * RS_HT_ROW];
                    const float2 v0 = x[o + 2 * k], v1 = x[o + 2 * k + 1];
                    acc.x += h.x * v0.x; acc.y += h.x * v0.y;
                    acc.x += h.y * v1.x; acc.y += h.y * v1.y;
                }
            }
            const float2 v = make_float2(acc.x * gain, acc.y * gain);
            if (SC16 && clip) reinterpret_cast<uint32_t *>(out)[j - j0] = sc16_sample(v.x, v.y, nclip);
            else out[j - j0] = v;
        }
        if (!more) break;
    }
    if (SC16 && clip) sc16_clip_commit(clip, nclip);
}
// (FIXED needs the branch of output j to depend on j mod 256 only, and a thread's outputs to share it: the step's low 16 bits clear)
static inline bool rs_fixed_rate(unsigned long long step) { return (step & 0xFFFFull) == 0; }
// How a launch stores its outputs: into a stage buffer (the default: cf32, gain 1) or into the caller's buffer (rs_caller_out)
struct RsOut { void *d; float gain; unsigned long long *clip; };       // clip != NULL: sc16, and where the clipped samples are counted
static inline RsOut rs_stage_out(float2 *d) { return RsOut{ d, 1.0f, nullptr }; }
// h1 != nullptr: `in` is the input of the last half-band decimator, folded into the launch (arbitrary_kernel, HB)
template <int FMT, bool SC16>
static inline void rs_launch_arbitrary_out(const RsInT<FMT> &in, const RsOut &o, long long j0, long long j1, unsigned long long step, const float *hpfb, hipStream_t st,
                                           const float *h1)
{
    const unsigned n = (unsigned)(j1 - j0), ob = h1 ? RS_OB / 2 : RS_OB, grid = (n + ob * RS_CHUNKS - 1) / (ob * RS_CHUNKS);
    float2 *out = (float2 *)o.d;
    if (h1) {
        if (rs_fixed_rate(step)) hipLaunchKernelGGL((arbitrary_kernel<true, true, FMT, SC16>), dim3(grid), dim3(256), 0, st, in, out, j0, j1, step, hpfb, h1, o.gain, o.clip);
        else hipLaunchKernelGGL((arbitrary_kernel<false, true, FMT, SC16>), dim3(grid), dim3(256), 0, st, in, out, j0, j1, step, hpfb, h1, o.gain, o.clip);
    } else {
        if (rs_fixed_rate(step)) hipLaunchKernelGGL((arbitrary_kernel<true, false, FMT, SC16>), dim3(grid), dim3(256), 0, st, in, out, j0, j1, step, hpfb, h1, o.gain, o.clip);
        else hipLaunchKernelGGL((arbitrary_kernel<false, false, FMT, SC16>), dim3(grid), dim3(256), 0, st, in, out, j0, j1, step, hpfb, h1, o.gain, o.clip);
    }
}
template <int FMT>
static inline void rs_launch_arbitrary(const RsInT<FMT> &in, const RsOut &o, long long j0, long long j1, unsigned long long step, const float *hpfb, hipStream_t st,
                                       const float *h1 = nullptr)
{
    if (o.clip) rs_launch_arbitrary_out<FMT, true>(in, o, j0, j1, step, hpfb, st, h1);
    else rs_launch_arbitrary_out<FMT, false>(in, o, j0, j1, step, hpfb, st, h1);
}

// the last RS_KEEP samples of a two-segment input become the next call's tail (one workgroup, staged through registers
// because source and destination may overlap).  The tail stays in the format of the input: sc16 words are copied as they are.
template <int FMT>
__global__ void tail_save_kernel(RsInT<FMT> in, typename RsElem<FMT>::type *tail, long long new_base)
{
    const int i = threadIdx.x;
    const typename RsElem<FMT>::type v = rs_fetch(in, new_base + i);
    __syncthreads();
    if (new_base + i < in.end) tail[i] = v;
}

static thread_local std::string g_rs_err;
#define RSCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { g_rs_err = hipGetErrorString(e_); return MCRX_EHIP; } } while (0)

struct StageBuf {                   // device buffer holding samples [base, end) of one stage input
    float2 *d = nullptr; size_t cap = 0; long long base = 0, end = 0;
};

struct msresamp_hip_s {
    int device = -1;            // the HIP device the handle was created on: every entry point runs with it current (devscope.hpp)
    float rate = 1, As = 60;
    bool interp = false;
    unsigned num_stages = 0;
    double rate_arb = 1;
    float delay = 0;            // msresamp_hip_get_delay
    unsigned long long step = 0;
    float *d_h1 = nullptr, *d_hpfb = nullptr;
    std::vector<StageBuf> in;       // decimating: in[0] = resampler input, in[s] = input of half-band s / arbitrary stage;
                                    // interpolating: in[0] = input of the arbitrary stage, in[1 + s] = input of half-band interpolator s
    long long out_count = 0;        // outputs of the arbitrary stage produced so far (j), less the whole periods taken off by rs_rebase
    long long per_in = 1, per_out = 1;      // one period of the phase: step / g inputs, 2^24 / g outputs of the arbitrary stage
    hipStream_t stream = nullptr;
    unsigned in_fmt = IQ_CF32;   // format of the caller's samples and of in[0], their retained tail (msresamp_hip_set_input_format)
    // The caller's output (msresamp_hip_set_output_format, _set_output_gain): read at every call and nowhere retained -- no stage buffer
    // is an output buffer -- so both may change between any two calls.
    unsigned out_fmt = IQ_CF32;
    float out_gain = 1.0f;
    Sc16ClipCount clip;         // allocated when sc16 output is first selected; marked behind the last sc16-output call's kernels
    hipEvent_t ev_first[2] = { nullptr, nullptr };      // msresamp_hip_time_first_stage: around the launch that reads the caller's samples
    bool time_first = false, timed_first = false;
};

// events around the first stage's launch (the kernel that reads the caller's buffer), when the handle is asked to time it
struct FirstStageTimer {
    msresamp_hip_s *q; hipStream_t st;
    FirstStageTimer(msresamp_hip_s *q_, hipStream_t st_) : q(q_), st(st_) { if (q->time_first) (void)hipEventRecord(q->ev_first[0], st); }
    ~FirstStageTimer() { if (q->time_first) { (void)hipEventRecord(q->ev_first[1], st); q->timed_first = true; } }
};

static int stage_reserve(msresamp_hip_t q, StageBuf &b, size_t extra, hipStream_t st)
{
    // make room for `extra` more samples, keeping the last RS_KEEP samples
    size_t have = (size_t)(b.end - b.base);
    if (have + extra <= b.cap) return MCRX_OK;
    size_t keep = std::min(have, (size_t)RS_KEEP);
    if (keep + extra <= b.cap) {                        // slide the tail to the front (stream ordered, no allocation)
        if (keep) {
            const RsIn me = { nullptr, 0, b.d, b.base, b.end };
            hipLaunchKernelGGL(tail_save_kernel<IQ_CF32>, dim3(1), dim3(RS_KEEP), 0, st, me, b.d, b.end - (long long)keep);
            RSCHK(hipGetLastError());
        }
        b.base = b.end - (long long)keep;
        return MCRX_OK;
    }
    size_t ncap = std::max(b.cap, 2 * (keep + extra) + 64);
    float2 *nd = nullptr;
    RSCHK(hipMalloc((void **)&nd, ncap * sizeof(float2)));
    if (keep) RSCHK(hipMemcpyAsync(nd, b.d + (have - keep), keep * sizeof(float2), hipMemcpyDeviceToDevice, st));
    RSCHK(hipStreamSynchronize(st));
    if (b.d) (void)hipFree(b.d);
    b.d = nd; b.cap = ncap; b.base = b.end - (long long)keep;
    (void)q;
    return MCRX_OK;
}

// Sample positions of stage buffer i per input sample of the arbitrary stage (decimating: in[i] runs 2^(num_stages - i) times as
// fast), or per output of it (interpolating, i >= 1: in[i] is the input of half-band interpolator i - 1); whole periods of those.
static inline long long rs_period(const msresamp_hip_s *q, unsigned i)
{
    if (q->interp) return i ? q->per_out << (i - 1) : q->per_in;
    return q->per_in << (q->num_stages - i);
}
// Take as many whole periods of the phase off every counter as all of them allow (a buffer's base must stay >= 0: samples
// before 0 read as zeros).  Output j - m * per_out reads input n_j - m * per_in with the fraction of output j: nothing changes.
static void rs_rebase(msresamp_hip_s *q)
{
    const unsigned ns = q->num_stages;
    long long m = q->out_count / q->per_out;
    for (unsigned i = 0; i <= ns && m > 0; i++) {
        const bool counted = !q->interp && ns && i == ns;       // the folded half-band stage's output: counted, never stored
        m = std::min(m, (counted ? q->in[i].end : q->in[i].base) / rs_period(q, i));
    }
    if (m <= 0) return;
    for (unsigned i = 0; i <= ns; i++) {
        const bool counted = !q->interp && ns && i == ns;
        const long long d = m * rs_period(q, i);
        q->in[i].end -= d;
        q->in[i].base = counted ? q->in[i].end : q->in[i].base - d;
    }
    q->out_count -= m * q->per_out;
}

// in[0] only ever holds the retained tail of the caller's input: the stages read the new samples where they lie
static inline RsIn stage_in(const StageBuf &b) { return RsIn{ nullptr, 0, b.d, b.base, b.end }; }

// The plan of a rate, without a device: the integers, the taps and the table a handle of that rate uploads (resamp_plan.hpp)
extern "C" int msresamp_hip_selftest(float rate, float As, msresamp_hip_plan *plan)
{
    if (!plan) { g_rs_err = "null pointer"; return MCRX_EINVAL; }
    if (plan->struct_size != sizeof(msresamp_hip_plan)) { g_rs_err = "msresamp_hip_plan: wrong struct_size"; return MCRX_EINVAL; }
    if (const char *bad = resamp_rate_check(rate)) { g_rs_err = bad; return MCRX_EINVAL; }
    const ResampPlan p = resamp_plan(rate, As);
    plan->interp = p.interp ? 1u : 0u; plan->num_stages = p.num_stages; plan->reserved = 0;
    plan->step = p.step; plan->per_in = (uint64_t)p.per_in; plan->per_out = (uint64_t)p.per_out;
    plan->rate_arb = p.rate_arb; plan->delay = p.delay;
    std::memcpy(plan->h1, p.h1.data(), sizeof(plan->h1));
    std::memcpy(plan->hpfb, p.hpfb.data(), sizeof(plan->hpfb));
    return MCRX_OK;
}

extern "C" int msresamp_hip_create(msresamp_hip_t *out, float rate, float As)
{
    if (!out) { g_rs_err = "null pointer"; return MCRX_EINVAL; }
    if (const char *bad = resamp_rate_check(rate)) { g_rs_err = bad; return MCRX_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { g_rs_err = "no HIP device (no CPU fallback)"; return MCRX_EHIP; }
    const ResampPlan p = resamp_plan(rate, As);
    msresamp_hip_t q = new msresamp_hip_s();
    q->device = current_device();
    q->rate = rate; q->As = As; q->rate_arb = p.rate_arb;
    q->interp = p.interp; q->num_stages = p.num_stages;
    q->step = p.step; q->per_in = p.per_in; q->per_out = p.per_out; q->delay = p.delay;
    const std::vector<float> &h1 = p.h1;
    std::vector<float> hp((size_t)RS_NPFB * RS_HROW, 0.0f);              // the table's rows padded to 16 floats
    for (unsigned b = 0; b < RS_NPFB; b++) std::memcpy(&hp[(size_t)b * RS_HROW], &p.hpfb[(size_t)b * RS_TAPS], RS_TAPS * sizeof(float));
    if (hipMalloc((void **)&q->d_h1, h1.size() * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&q->d_hpfb, hp.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(q->d_h1, h1.data(), h1.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(q->d_hpfb, hp.data(), hp.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipStreamCreate(&q->stream) != hipSuccess) { g_rs_err = "device allocation failed"; delete q; return MCRX_EHIP; }
    q->in.resize(q->num_stages + 1);     // (interpolating: in[1 .. num_stages] feed the half-band interpolators)
    *out = q;
    return MCRX_OK;
}

extern "C" int msresamp_hip_destroy(msresamp_hip_t q)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) return MCRX_OK;
    (void)hipDeviceSynchronize();
    for (auto &b : q->in) if (b.d) (void)hipFree(b.d);
    (void)hipFree(q->d_h1); (void)hipFree(q->d_hpfb);
    if (q->stream) (void)hipStreamDestroy(q->stream);
    for (hipEvent_t e : q->ev_first) if (e) (void)hipEventDestroy(e);
    q->clip.release();
    delete q;
    return MCRX_OK;
}

extern "C" int msresamp_hip_reset(msresamp_hip_t q) { return msresamp_hip_reset_at(q, 0); }

// msresamp_hip_reset, but the stream goes on from input sample `input_position` with zero history: as if that many zeros had been
// consumed and their outputs discarded.  Only the position within a period of the phase matters (rs_rebase).
extern "C" int msresamp_hip_reset_at(msresamp_hip_t q, uint64_t input_position)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) return MCRX_EINVAL;
    const unsigned ns = q->num_stages;
    if (input_position & ((1ull << ns) - 1)) { g_rs_err = "msresamp: a position must be a multiple of 2^num_stages"; return MCRX_EINVAL; }
    // the arbitrary stage's input index within its period, and the first output that reads a sample from there on
    const long long r = (long long)((q->interp ? input_position : input_position >> ns) % (uint64_t)q->per_in);
    const long long j = (long long)((((unsigned long long)r << RS_PHASE_BITS) + q->step - 1) / q->step);
    for (unsigned i = 0; i <= ns; i++) {
        StageBuf &b = q->in[i];
        b.base = b.end = q->interp ? (i ? j << (i - 1) : r) : r << (ns - i);
    }
    q->out_count = j;
    return MCRX_OK;
}

// in input samples of the handle (resamp_plan.hpp: resamp_delay)
extern "C" float msresamp_hip_get_delay(msresamp_hip_t q) { return q ? q->delay : 0.f; }

extern "C" size_t msresamp_hip_max_output(msresamp_hip_t q, size_t nin)
{ return q ? (size_t)((double)nin * q->rate * 1.0001) + (q->interp ? (4u << q->num_stages) : 4) : 0; }

// The format of the caller's samples belongs to the handle.  It may change only while in[0] is empty -- a new handle, or directly after
// a reset -- because the retained tail is in the old format otherwise.
extern "C" int msresamp_hip_set_input_format(msresamp_hip_t q, unsigned format)
{
    if (!q) { g_rs_err = "null argument"; return MCRX_EINVAL; }
    if (format != IQ_CF32 && format != IQ_SC16) { g_rs_err = "msresamp: input format must be 0 (cf32) or 1 (sc16)"; return MCRX_EINVAL; }
    if (q->in[0].end > q->in[0].base) { g_rs_err = "msresamp: the input format cannot change while the handle holds input history (reset first)"; return MCRX_EBUSY; }
    q->in_fmt = format;
    return MCRX_OK;
}

extern "C" unsigned msresamp_hip_input_format(msresamp_hip_t q) { return q ? q->in_fmt : 0; }

// The output format and gain belong to the handle too, but no state is kept in them: every stage buffer is an INPUT buffer and stays
// cf32, so either may change between any two calls, in mid-stream as well (no MCRX_EBUSY case).  The clip counter and its event are
// allocated when sc16 output is first selected; a handle that never selects it allocates nothing.
extern "C" int msresamp_hip_set_output_format(msresamp_hip_t q, unsigned format)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_rs_err = "null argument"; return MCRX_EINVAL; }
    if (format != IQ_CF32 && format != IQ_SC16) { g_rs_err = "msresamp: output format must be 0 (cf32) or 1 (sc16)"; return MCRX_EINVAL; }
    if (format == IQ_SC16) RSCHK(q->clip.ensure());
    q->out_fmt = format;
    return MCRX_OK;
}

extern "C" unsigned msresamp_hip_output_format(msresamp_hip_t q) { return q ? q->out_fmt : 0u; }

extern "C" int msresamp_hip_set_output_gain(msresamp_hip_t q, float gain)
{
    if (!q) { g_rs_err = "null argument"; return MCRX_EINVAL; }
    if (!std::isfinite(gain)) { g_rs_err = "msresamp: the output gain must be finite"; return MCRX_EINVAL; }
    q->out_gain = gain;
    return MCRX_OK;
}

extern "C" float msresamp_hip_output_gain(msresamp_hip_t q) { return q ? q->out_gain : 0.0f; }

// Samples clipped by sc16-output calls since the last reset of the count (mctx_hip_clipped's semantics): waits for the event behind the
// last such call only, not for the stream.  0 on a handle that never selected sc16 output.
extern "C" int msresamp_hip_clipped(msresamp_hip_t q, uint64_t *samples, int reset)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_rs_err = "null argument"; return MCRX_EINVAL; }
    uint64_t n = 0;
    RSCHK(q->clip.read(&n, reset != 0));        // (whatever the format is now)
    if (samples) *samples = n;
    return MCRX_OK;
}

// Measurement aid (bench_resamp_sc16.py): HIP events around the first stage's launch of every following execute call.
extern "C" int msresamp_hip_time_first_stage(msresamp_hip_t q, int enable)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q) { g_rs_err = "null argument"; return MCRX_EINVAL; }
    if (enable) for (hipEvent_t &e : q->ev_first) if (!e) RSCHK(hipEventCreate(&e));
    q->time_first = enable != 0; q->timed_first = false;
    return MCRX_OK;
}

// ... and the time between them for the last such call (waits for it).  MCRX_EINVAL when no first stage has been timed.
extern "C" int msresamp_hip_first_stage_ms(msresamp_hip_t q, float *ms)
{
    DevScope dev_scope_(q ? q->device : -1);
    if (!q || !ms) { g_rs_err = "null argument"; return MCRX_EINVAL; }
    if (!q->timed_first) { g_rs_err = "msresamp: no first stage has been timed (msresamp_hip_time_first_stage)"; return MCRX_EINVAL; }
    RSCHK(hipEventSynchronize(q->ev_first[1]));
    RSCHK(hipEventElapsedTime(ms, q->ev_first[0], q->ev_first[1]));
    return MCRX_OK;
}

// d_in: nin new input samples in device memory, in format FMT; d_out receives *nout <= out_cap samples in the handle's output format
template <int FMT>
static int rs_execute(msresamp_hip_t q, const void *d_in, size_t nin, void *d_out, size_t out_cap, size_t *nout, void *stream)
{
    typedef typename RsElem<FMT>::type elem_t;
    DevScope dev_scope_(q ? q->device : -1);
    if (!q || !nout || (!d_in && nin) || !d_out) { g_rs_err = "null argument"; return MCRX_EINVAL; }
    if (q->in_fmt != (unsigned)FMT) {       // (before anything is counted: the call consumes nothing)
        g_rs_err = FMT == IQ_SC16 ? "msresamp: input format mismatch, an sc16 call on a cf32 handle (msresamp_hip_set_input_format)"
                                     : "msresamp: input format mismatch, a cf32 call on an sc16 handle (msresamp_hip_execute_device_sc16)";
        return MCRX_EINVAL;
    }
    // NULL = the legacy default stream, like the other stage operators: what a caller enqueues next -- on that stream or on a
    // receiver handle's own (blocking) streams -- is ordered behind the resampler's kernels.  (A private stream here left
    // msresamp -> multichannelrx chains on the default stream unordered: the bank could read samples not yet written.)
    hipStream_t st = (hipStream_t)stream;
    *nout = 0;
    // the last stage's store: the handle's format and gain as they are now (sc16: any 4-byte-aligned d_out)
    const bool sc16_out = q->out_fmt == IQ_SC16;
    if (sc16_out && (reinterpret_cast<uintptr_t>(d_out) & 3u)) { g_rs_err = "sc16 output must be 4-byte aligned"; return MCRX_EINVAL; }
    const RsOut caller = { d_out, q->out_gain, sc16_out ? q->clip.device() : nullptr };
    auto clip_mark = [&]() -> int {         // behind the launch that wrote the caller's sc16 samples: what msresamp_hip_clipped waits for
        if (sc16_out) RSCHK(q->clip.mark(st));
        return MCRX_OK;
    };
    rs_rebase(q);
    // the first stage reads [retained tail | the caller's new samples]; nothing is copied
    StageBuf &b0 = q->in[0];
    int rc;
    if (!b0.d) { RSCHK(hipMalloc((void **)&b0.d, RS_KEEP * sizeof(float2))); b0.cap = RS_KEEP; }    // (room for either format)
    const long long end0 = b0.end + (long long)nin;
    const RsInT<FMT> src0 = { b0.end > b0.base ? (const elem_t *)b0.d : nullptr, b0.base, (const elem_t *)d_in, b0.end, end0 };
    auto keep_tail = [&]() -> int {
        const long long nb = std::max(b0.base, end0 - (long long)RS_KEEP);
        if (end0 > nb) {
            hipLaunchKernelGGL(tail_save_kernel<FMT>, dim3(1), dim3(RS_KEEP), 0, st, src0, (elem_t *)b0.d, nb);
            RSCHK(hipGetLastError());
        }
        b0.base = nb; b0.end = end0;
        return MCRX_OK;
    };
    const unsigned OB = RS_OB;
    if (q->interp) {
        // arbitrary stage over the input: outputs j with n_j < end go to the first half-band interpolator's input (or out)
        const long long j0 = q->out_count;
        const unsigned long long lim = (unsigned long long)end0 << RS_PHASE_BITS;
        long long j1 = (long long)((lim + q->step - 1) / q->step);
        if (j1 < j0) j1 = j0;
        const size_t total_out = (size_t)(j1 - j0) << q->num_stages;
        if (total_out > out_cap) { g_rs_err = "output buffer too small"; return MCRX_EINVAL; }
        RsOut dst = caller;
        if (q->num_stages) {
            StageBuf &b1 = q->in[1];
            if ((rc = stage_reserve(q, b1, (size_t)(j1 - j0), st))) return rc;
            dst = rs_stage_out(b1.d + (b1.end - b1.base));
            b1.end += j1 - j0;
        }
        if (j1 > j0) {
            {
                FirstStageTimer timer(q, st);
                rs_launch_arbitrary(src0, dst, j0, j1, q->step, q->d_hpfb, st);
            }
            RSCHK(hipGetLastError());
            if (!q->num_stages && (rc = clip_mark())) return rc;
        }
        q->out_count = j1;
        if ((rc = keep_tail())) return rc;
        // half-band interpolators: stage s consumes the new samples of in[1 + s] (all of them: no look-ahead needed)
        long long k0 = j0;
        for (unsigned s = 0; s < q->num_stages; s++) {
            StageBuf &bi = q->in[1 + s];
            const long long k1 = bi.end;
            const bool last = s + 1 == q->num_stages;
            RsOut o = caller;
            if (!last) {
                StageBuf &bo = q->in[2 + s];
                if ((rc = stage_reserve(q, bo, (size_t)(2 * (k1 - k0)), st))) return rc;
                o = rs_stage_out(bo.d + (bo.end - bo.base));
                bo.end += 2 * (k1 - k0);
            }
            if (k1 > k0) {
                const unsigned n = (unsigned)(k1 - k0);
                const dim3 grid((n + OB - 1) / OB);
                if (o.clip) hipLaunchKernelGGL(halfband_interp_kernel<true>, grid, dim3(256), 0, st, stage_in(bi), (float2 *)o.d, k0, k1, q->d_h1, o.gain, o.clip);
                else hipLaunchKernelGGL(halfband_interp_kernel<false>, grid, dim3(256), 0, st, stage_in(bi), (float2 *)o.d, k0, k1, q->d_h1, o.gain, o.clip);
                RSCHK(hipGetLastError());
                if (last && (rc = clip_mark())) return rc;
            }
            k0 *= 2;
        }
        *nout = total_out;
        return MCRX_OK;
    }
    // half-band stages: stage s consumes in[s] (s = 0: the caller's samples), appends to in[s+1]
    for (unsigned s = 0; s < q->num_stages; s++) {
        StageBuf &bo = q->in[s + 1];
        const long long iend = s ? q->in[s].end : end0;
        const long long k0 = bo.end, k1 = iend / 2;         // output k exists once x[2k+1] has arrived
        if (s + 1 == q->num_stages) {                       // the last one runs inside the arbitrary stage's kernel: its samples are counted, not stored
            if (k1 > k0) bo.end = k1;
            break;
        }
        if (k1 > k0) {
            if ((rc = stage_reserve(q, bo, (size_t)(k1 - k0), st))) return rc;
            const unsigned n = (unsigned)(k1 - k0);
            float2 *o = bo.d + (bo.end - bo.base);
            if (s) hipLaunchKernelGGL(halfband_kernel<IQ_CF32>, dim3((n + OB - 1) / OB), dim3(256), 0, st, stage_in(q->in[s]), o, k0, k1, q->d_h1);
            else { FirstStageTimer timer(q, st); hipLaunchKernelGGL(halfband_kernel<FMT>, dim3((n + OB - 1) / OB), dim3(256), 0, st, src0, o, k0, k1, q->d_h1); }
            RSCHK(hipGetLastError());
            bo.end = k1;
        }
    }
    // arbitrary stage over in[num_stages]: outputs j with n_j < end
    const long long aend = q->num_stages ? q->in[q->num_stages].end : end0;
    const long long j0 = q->out_count;
    // largest j with (j*step >> 24) < end  <=>  j*step < end << 24
    const unsigned long long lim = (unsigned long long)aend << RS_PHASE_BITS;
    long long j1 = (long long)((lim + q->step - 1) / q->step);          // first j with j*step >= lim
    if (j1 < j0) j1 = j0;
    if ((size_t)(j1 - j0) > out_cap) { g_rs_err = "output buffer too small"; return MCRX_EINVAL; }
    if (j1 > j0) {
        const unsigned ns = q->num_stages;
        if (ns > 1) rs_launch_arbitrary(stage_in(q->in[ns - 1]), caller, j0, j1, q->step, q->d_hpfb, st, q->d_h1);
        else {
            FirstStageTimer timer(q, st);
            if (ns) rs_launch_arbitrary(src0, caller, j0, j1, q->step, q->d_hpfb, st, q->d_h1);
            else rs_launch_arbitrary(src0, caller, j0, j1, q->step, q->d_hpfb, st);
        }
        RSCHK(hipGetLastError());
        if ((rc = clip_mark())) return rc;
    }
    q->out_count = j1;
    if ((rc = keep_tail())) return rc;
    *nout = (size_t)(j1 - j0);
    return MCRX_OK;
}

extern "C" int msresamp_hip_execute_device(msresamp_hip_t q, const void *d_in, size_t nin, void *d_out,
                                           size_t out_cap, size_t *nout, void *stream)
{ return rs_execute<IQ_CF32>(q, d_in, nin, d_out, out_cap, nout, stream); }

// the same for a handle whose input format is sc16: nin samples = 2 * nin int16 (any 4-byte-aligned d_in)
extern "C" int msresamp_hip_execute_device_sc16(msresamp_hip_t q, const void *d_in, size_t nin, void *d_out,
                                                size_t out_cap, size_t *nout, void *stream)
{ return rs_execute<IQ_SC16>(q, d_in, nin, d_out, out_cap, nout, stream); }

extern "C" const char *msresamp_hip_last_error(void) { return g_rs_err.c_str(); }
